// cube_faces.h -- the bordered faces of the cube-texture pool (skybox.h): which texel a border position holds, where a level of a
// cube lies in the pool, and the table of the launch that assembles the faces of every cube upload (cube_faces.hip; cube_plan.h
// fills the table for r3n_texture_cubes_write, _encoded and _sources alike).  Plain C++17, no HIP, no context, shared by host and
// kernel: tests/cube_faces_check.cpp compiles it alone.
//
// A face of extent n is stored WITH A ONE-TEXEL BORDER: (n + 2) x (n + 2) texels, row-major, interior texel (i, j) at bordered
// position (i + 1, j + 1).  A border position of an edge holds the adjacent face's texel across that edge, OF THE SAME LEVEL: the
// texel the centre of the missing texel, extended on the face's plane and re-projected, falls into (tests/skybox_reference.py
// resolve_texel finds it geometrically; the table below is that function's result, checked against it for every n the tests name,
// and the library's only statement of the rule: no entry builds a border on the host).
// The four corner positions have no texel: they are written as zero and never read (the sampler forms a corner from three texels).
//
// Pool layout of ONE cube of extent N with `mips` levels, in words (per_texel = 1: an RGBA8 word, 4: four f32):
//     level 0's six bordered faces (+X, -X, +Y, -Y, +Z, -Z), then level 1's, ...; every level starts on a 4-word boundary
//     level k: n_k = max(1, N >> k), a face is (n_k + 2)^2 * per_texel words, the level 6 faces, padded to a multiple of 4 words
// Every cube starts on a 4-word boundary as well.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CUBE_FACES_HD __host__ __device__ inline
#else
#define CUBE_FACES_HD inline
#endif

namespace cube_faces {

// ---- the pool layout
CUBE_FACES_HD uint32_t level_extent(uint32_t n0, uint32_t k) {
    const uint32_t n = k < 32u ? n0 >> k : 0u;
    return n ? n : 1u;
}
CUBE_FACES_HD uint64_t face_words(uint32_t n, uint32_t per_texel) { return (uint64_t)(n + 2u) * (n + 2u) * per_texel; }
CUBE_FACES_HD uint64_t level_words(uint32_t n, uint32_t per_texel) { return (6u * face_words(n, per_texel) + 3u) & ~(uint64_t)3u; }
// first word of level k, relative to the cube's first word
CUBE_FACES_HD uint64_t level_start(uint32_t n0, uint32_t k, uint32_t per_texel) {
    uint64_t at = 0;
    for (uint32_t l = 0; l < k; ++l) at += level_words(level_extent(n0, l), per_texel);
    return at;
}
CUBE_FACES_HD uint64_t cube_words(uint32_t n0, uint32_t mips, uint32_t per_texel) { return level_start(n0, mips, per_texel); }

// ---- the edge table.  Edges of a face: 0 = the column left of i = 0, 1 = the column right of i = n - 1, 2 = the row above j = 0,
// 3 = the row below j = n - 1.  Position k along an edge is the j (edges 0, 1) or the i (edges 2, 3) of the missing texel.  Across
// edge e of face f lies face `face`, whose texels along ITS edge `edge` (the outermost column or row on that side) are the
// neighbours, in the same order or reversed.
struct Edge {
    uint8_t face, edge, flip;
};
// one entry as 6 bits, a face's four entries as one word: constants in the instruction stream, the kernel reads no table
constexpr uint32_t edge_bits(uint32_t face, uint32_t edge, uint32_t flip) { return face | edge << 3 | flip << 5; }
constexpr uint32_t edge_row(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) { return e0 | e1 << 6 | e2 << 12 | e3 << 18; }
CUBE_FACES_HD Edge edge_of(uint32_t f, uint32_t e) {
    //                               edge 0               edge 1               edge 2               edge 3
    constexpr uint32_t PX = edge_row(edge_bits(4, 1, 0), edge_bits(5, 0, 0), edge_bits(2, 1, 1), edge_bits(3, 1, 0));
    constexpr uint32_t NX = edge_row(edge_bits(5, 1, 0), edge_bits(4, 0, 0), edge_bits(2, 0, 0), edge_bits(3, 0, 1));
    constexpr uint32_t PY = edge_row(edge_bits(1, 2, 0), edge_bits(0, 2, 1), edge_bits(5, 2, 1), edge_bits(4, 2, 0));
    constexpr uint32_t NY = edge_row(edge_bits(1, 3, 1), edge_bits(0, 3, 0), edge_bits(4, 3, 0), edge_bits(5, 3, 1));
    constexpr uint32_t PZ = edge_row(edge_bits(1, 1, 0), edge_bits(0, 0, 0), edge_bits(2, 3, 0), edge_bits(3, 2, 0));
    constexpr uint32_t NZ = edge_row(edge_bits(0, 1, 0), edge_bits(1, 0, 0), edge_bits(2, 2, 1), edge_bits(3, 3, 1));
    const uint32_t row = f == 0u ? PX : f == 1u ? NX : f == 2u ? PY : f == 3u ? NY : f == 4u ? PZ : NZ;
    const uint32_t b = (row >> (6u * e)) & 63u;
    return Edge{(uint8_t)(b & 7u), (uint8_t)((b >> 3) & 3u), (uint8_t)(b >> 5)};
}

// the texel a position of a bordered face holds
struct Source {
    uint32_t face, i, j;
    bool corner;  // no texel: written as zero
};
// (bx, by) in [0, n + 1]^2 of face f of a level of extent n
CUBE_FACES_HD Source source_of(uint32_t f, uint32_t bx, uint32_t by, uint32_t n) {
    const bool out_x = bx == 0u || bx == n + 1u, out_y = by == 0u || by == n + 1u;
    if (out_x && out_y) return Source{f, 0u, 0u, true};
    if (!out_x && !out_y) return Source{f, bx - 1u, by - 1u, false};
    const uint32_t e = out_x ? (bx == 0u ? 0u : 1u) : (by == 0u ? 2u : 3u);
    const uint32_t k = out_x ? by - 1u : bx - 1u;
    const Edge ed = edge_of(f, e);
    const uint32_t a = ed.flip ? n - 1u - k : k;
    switch (ed.edge) {
        case 0: return Source{ed.face, 0u, a, false};
        case 1: return Source{ed.face, n - 1u, a, false};
        case 2: return Source{ed.face, a, 0u, false};
        default: return Source{ed.face, a, n - 1u, false};
    }
}

// ---- the assemble launch: one record per (cube, level, face), 8 words so that a wave reads it as one scalar load.  A wave slot
// takes 64 consecutive positions of ONE bordered face (records | wave_first | wave_instance, vertex_block.h).
struct Record {
    uint32_t n, face;       // the level's extent, the face
    uint32_t per_texel;     // 1 | 4
    uint32_t units;         // (n + 2)^2
    uint32_t src;           // first word of the LEVEL's six dense faces in the scratch block (face f at src + f * src_stride)
    uint32_t src_stride;    // words from one dense face to the next
    uint32_t dst;           // first pool word of this bordered face
    uint32_t pad;
};
static_assert(sizeof(Record) == 32, "an assemble record is 8 words");
constexpr uint32_t REC_WORDS = sizeof(Record) / 4u, UNITS_PER_WAVE = 64u;
// words from one dense face of a level to the next: every dense face starts on a 4-word boundary (the decoders store float4s)
CUBE_FACES_HD uint64_t dense_face_words(uint32_t n, uint32_t per_texel) { return ((uint64_t)n * n * per_texel + 3u) & ~(uint64_t)3u; }

// One position of a bordered face over plain arrays: what the kernel does per lane, for one word class.  T = uint32_t (per_texel 1)
// or a 16-byte texel (per_texel 4); `dense` = the level's six dense faces, `stride` texels apart; `dst` = the bordered face.
template <class T>
CUBE_FACES_HD void assemble_at(const T *dense, size_t stride, T *dst, uint32_t f, uint32_t n, uint32_t unit, T zero) {
    const uint32_t pitch = n + 2u, by = unit / pitch, bx = unit - by * pitch;
    const Source s = source_of(f, bx, by, n);
    if (s.corner) dst[unit] = zero;
    else dst[unit] = dense[(size_t)s.face * stride + (size_t)s.j * n + s.i];
}

}  // namespace cube_faces
