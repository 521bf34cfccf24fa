// equirect.h -- the records of the launches that build cubes from equirectangular panoramas (equirect.hip,
// r3n_texture_cubes_write_sources).  The rule and the launch plan: equirect_rule.h; cube_plan.h fills the records.  Plain C++17, no
// HIP, no context.
//
// Everything is indexed in 32-bit words of the call's scratch block ("dense": decoded sources, then the dense faces of every level,
// laid out as cube_plan.h lays them out for every entry: a level's six faces back to back, n * n * 4 words each), except an
// RGBE8 source, which is read where it lies in the staged payload (a 64-bit byte offset).
#pragma once
#include <stdint.h>

#include "equirect_rule.h"

#define R3N_EQUIRECT_TAIL_DEFAULT 64u  // R3N_TUNE equirect_tail (profiles/equirect.md)

namespace equirect {

enum SourceMode : uint32_t {
    SOURCE_RGBE8 = 0,       // one RGBE word per texel in the staged payload, decoded inline
    SOURCE_F32 = 1,         // four f32 per texel in the scratch block (a float-decoded format)
    SOURCE_RGBA8 = 2,       // one RGBA8 word per texel in the scratch block, byte / 255
    SOURCE_RGBA8_SRGB = 3,  // the same, colour through the sRGB decode table
};

// k_equirect_faces: one record per (cube, face), 16 words so that a wave reads it as scalar loads.  A wave slot takes 64 consecutive
// texels of ONE face, row-major (records | wave_first | wave_instance, vertex_block.h).
struct FaceRec {
    uint32_t n, face;         // the face's extent, the face
    uint32_t mode;            // SourceMode
    uint32_t W, H;            // the panorama's extent
    uint32_t src_lo, src_hi;  // SOURCE_RGBE8: byte offset in the staged payload; else src_lo = first word in the scratch block
    uint32_t dst;             // first word of this dense level-0 face
    uint32_t units;           // n * n
    uint32_t pad[7];
};
static_assert(sizeof(FaceRec) == 64, "a face record is 16 words");

// the chain launches: one record per (cube, face), 8 words.
//     level launch: texel unit of the face at `dst` (extent d) from the face at `src` (extent s); units = d * d; wave map as above
//     tail launch:  workgroup b takes record b: `src` = first word of the six faces of the level of extent s (<= TAIL_CAP), and the
//                   `levels` levels behind it follow in the scratch block level by level
struct ChainRec {
    uint32_t s, d;
    uint32_t src, dst;
    uint32_t units;
    uint32_t face, levels;
    uint32_t pad;
};
static_assert(sizeof(ChainRec) == 32, "a chain record is 8 words");
constexpr uint32_t FACE_REC_WORDS = sizeof(FaceRec) / 4u, CHAIN_REC_WORDS = sizeof(ChainRec) / 4u, UNITS_PER_WAVE = 64u;
// texels of the levels a tail workgroup keeps in LDS: extents TAIL_CAP / 2, TAIL_CAP / 4, ..., 1
constexpr uint32_t TAIL_LDS_TEXELS = 32u * 32u + 16u * 16u + 8u * 8u + 4u * 4u + 2u * 2u + 1u;

}  // namespace equirect
