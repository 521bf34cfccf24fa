// ibl.h -- argument block and launcher of the passes that prefilter an environment cube (ibl.hip, r3n_environment_prefilter).  The
// rule: ibl_rule.h.  Plain C++17 besides the stream type.
//
// The call's scratch block (ibl_scratch below lays it out; a block of the call's own, freed before the call returns), every part
// on a 256-byte boundary:
//     records | dense | SH row sums | SH sums | assemble table
// records: one IblRecord (32 bytes: u.xyz, w, sanitised c.rgb, pad) per texel of every source level the call reads -- levels
// 1 .. L - 1 for the pair kernel, and level 0 as well when the SH source is level 0.  dense: the result's dense f32 faces, level by
// level (cube_faces.h), which k_cube_assemble turns into the bordered faces of the new cube.
// Launches of one call: records, mirror (result level 0), pairs (all levels 1 .. L - 1), SH rows, SH combine, k_cube_assemble.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/r3n.h"
#include "ibl_rule.h"

#define R3N_IBL_TILE_DEFAULT 256u   // R3N_TUNE ibl_tile: source records per LDS tile, 0 = no LDS (wave-uniform loads: 20.2 against 16.6 ms, profiles/ibl.md)
#define R3N_IBL_TILE_MAX 512u       // 16 KiB of LDS
#define R3N_IBL_BLOCK_DEFAULT 256u  // R3N_TUNE ibl_block: outputs (threads) per workgroup of the pair kernel: 64 | 128 | 256

struct IblRecord {
    float ux, uy, uz, w;
    float r, g, b, pad;
};
static_assert(sizeof(IblRecord) == 32, "a record is two 16-byte words");

struct IblLevel {
    uint32_t n;            // extent of source / result level k
    uint32_t src_word;     // first pool word of the source level's six bordered faces
    uint32_t rec_base;     // its first record (levels with records only)
    uint32_t dense_word;   // first word of result level k's dense faces in `dense`
    uint32_t first_block;  // pair kernel: the level's first workgroup (k >= 1)
    float a2, oma;         // ibl_rule::roughness(k, L)
    uint32_t pad;
};
struct IblArgs {
    const uint32_t *pool;   // the cube pool
    const float *decode;    // 256 entries: the decode table of the source cube's class (RGBA8 classes only)
    uint32_t f32_class;     // the source texels are four f32 words
    uint32_t L;             // levels
    uint32_t rec_from;      // first level with records: 0 (the SH source is level 0) or 1
    uint32_t rec_total;     // records of the call
    uint32_t sh_k;          // the SH source level
    uint32_t tile, block;   // the pair kernel's plan
    uint32_t pair_blocks;   // its grid
    IblRecord *records;
    uint32_t *dense;
    float *sh_rows;         // 6 n rows of 27 sums (3 m + ch)
    float *sh_out;          // 27 sums
    IblLevel lv[ibl_rule::MAX_LEVELS];
};
// byte offsets of the parts of the scratch block, and its size.  dense_words, assemble_words: of cube_plan::plan_append; sh_n: the
// extent of the SH source level
struct IblScratch {
    uint64_t records, dense, sh_rows, sh_out, assemble, bytes;
};
inline IblScratch ibl_scratch(uint32_t rec_total, uint64_t dense_words, uint32_t sh_n, uint64_t assemble_words) {
    const auto up = [](uint64_t b) { return (b + 255u) & ~255ull; };
    IblScratch s{};
    s.dense = up((uint64_t)rec_total * sizeof(IblRecord));
    s.sh_rows = up(s.dense + dense_words * 4u);
    s.sh_out = up(s.sh_rows + (uint64_t)6u * sh_n * 27u * 4u);
    s.assemble = up(s.sh_out + 27u * 4u);
    s.bytes = s.assemble + assemble_words * 4u;
    return s;
}
inline bool ibl_block_valid(uint32_t b) { return b == 64u || b == 128u || b == 256u; }

// Enqueues every pass but the assemble.  taps (may be null): taps[0 .. 3] are recorded in front of the record pass, behind the mirror
// pass, behind the pair kernel and behind the SH passes.  Returns the hipError_t of the first failure; *launches
// counts kernels.
extern "C" int r3n_internal_ibl(const IblArgs *a, hipEvent_t *taps, hipStream_t stream, uint64_t *launches);
