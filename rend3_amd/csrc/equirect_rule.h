// equirect_rule.h -- the rule that turns an equirectangular (latitude / longitude) panorama into the six dense faces of a cube and
// each face into its mip chain (DESIGN.md section 2 "Cubes from panoramas"), and the launch plan of the call that does it
// (r3n_texture_cubes_write_sources).  Plain C++17, no HIP, no context: shared by the kernels (equirect.hip), the host (r3n.hip)
// and the stand-alone check program (tests/equirect_rule_check.cpp); tests/equirect_reference.py restates it in numpy float32.
//
// Everything is PINNED: f32 in the order written, one rounding per operation (the units are built with -ffp-contract=off), IEEE
// division and square root, comparisons, selects and integer operations.  No libm call: the angle comes from atan2_turns below,
// floor from a conversion and a compare.
//
// The error of atan2_turns.  For a reduced argument t = lo / hi in [0, 1] the polynomial p(t) = t q(t^2) (7 terms, degree 13) is
// evaluated by Horner's rule.  Over EVERY f32 t in [0, 1] the f32 evaluation differs from atan(t) / 2 pi by at most 2^-24.1 turns
// (an exhaustive sweep of the 1 065 353 217 arguments: 5.52e-8 at t = 0.90943426; tests/equirect_rule_check.cpp repeats a dense
// part of it, 2^22 + 1 evenly spaced arguments and both f32 neighbours of each).  The division rounds t by at most 2^-24 relative
// and atan has slope <= 1, so it adds at most 2^-24 rad = 2^-26.6 turns; the octant steps (0.25 - p, 0.5 - p) are one rounding
// each of a value <= 0.25 and <= 0.5: 2^-26 and 2^-25 turns.  The sum, 1.15e-7, is below 2^-23 turns, and the bound this header
// states is
//     E = 2^-22 turns
// which leaves room for the f32 direction and the f32 square root in front of the latitude (a few 2^-24 relative on the arguments:
// below 2^-26 turns) and for the latitude entering v twice (v = 0.5 - 2 theta; its x is a square root, so it never takes the
// 0.5 - p step: 2 * 8.6e-8 < E).  At the widest source the entry accepts (65 535 texels) E is 1 / 64 of a source texel.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EQUIRECT_HD __host__ __device__ inline
#else
#define EQUIRECT_HD inline
#endif

namespace equirect_rule {

constexpr float ATAN2_TURNS_E = 0x1p-22f;  // E: the stated bound on |atan2_turns(y, x) - atan2(y, x) / 2 pi|
constexpr uint32_t MAX_SOURCE_EXTENT = 65535u, MAX_FACE_EXTENT = 16384u, TAIL_CAP = 64u;

struct vec4 {
    float x, y, z, w;
};

EQUIRECT_HD float bits_to_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- RGBE8 (Ward's rgbe.c): bytes (r, g, b, e) in one little-endian word.  e == 0 is black; otherwise a channel is
// (float)byte * 2^(e - 136), exact in f32 for every e (e < 10 gives subnormal scales: byte * 2^(e - 136) is a multiple of 2^-149).
EQUIRECT_HD float rgbe_scale(uint32_t e) { return bits_to_f32(e >= 10u ? (e - 9u) << 23 : 1u << (e + 13u)); }
EQUIRECT_HD vec4 rgbe_decode(uint32_t word) {
    const uint32_t e = word >> 24;
    if (e == 0u) return vec4{0.0f, 0.0f, 0.0f, 1.0f};
    const float s = rgbe_scale(e);
    return vec4{(float)(word & 255u) * s, (float)((word >> 8) & 255u) * s, (float)((word >> 16) & 255u) * s, 1.0f};
}

// ---- the direction through the centre of texel (i, j) of face f at extent n: the unnormalised point of the cube table of
// skybox.hip (sky_project read backwards; tests/skybox_reference.py _face_point).  sc = (2 i + 1 - n) / n: the numerator is an
// exact integer, so the grid is exactly antisymmetric about the face's centre and the centre of an odd face is exactly 0.
struct vec3 {
    float x, y, z;
};
EQUIRECT_HD vec3 face_direction(uint32_t f, uint32_t i, uint32_t j, uint32_t n) {
    const float fn = (float)n;
    const float sc = (float)((int32_t)(2u * i + 1u) - (int32_t)n) / fn;
    const float tc = (float)((int32_t)(2u * j + 1u) - (int32_t)n) / fn;
    switch (f) {
        case 0: return vec3{1.0f, -tc, -sc};   // +X: (sc, tc) = (-z, -y)
        case 1: return vec3{-1.0f, -tc, sc};   // -X: (z, -y)
        case 2: return vec3{sc, 1.0f, tc};     // +Y: (x, z)
        case 3: return vec3{sc, -1.0f, -tc};   // -Y: (x, -z)
        case 4: return vec3{sc, -tc, 1.0f};    // +Z: (x, -y)
        default: return vec3{-sc, -tc, -1.0f}; // -Z: (-x, -y)
    }
}

// ---- atan2(y, x) / 2 pi in [-0.5, 0.5]: octant reduction by swaps and negations, ONE division of the smaller by the larger
// magnitude, an odd polynomial.  atan2_turns(0, 0) = 0 (either sign of either zero); a zero counts as positive.
EQUIRECT_HD float atan_turns_poly(float t) {
    const float s = t * t;
    float q = 0x1.1c32aep-10f;
    q = q * s + -0x1.5e8124p-8f;
    q = q * s + 0x1.9f409ap-7f;
    q = q * s + -0x1.591266p-6f;
    q = q * s + 0x1.0240f6p-5f;
    q = q * s + -0x1.b26414p-5f;
    q = q * s + 0x1.45f2b4p-3f;
    return q * t;
}
EQUIRECT_HD float atan2_turns(float y, float x) {
    const float ax = x < 0.0f ? -x : x, ay = y < 0.0f ? -y : y;
    const bool swap = ay > ax;
    const float hi = swap ? ay : ax, lo = swap ? ax : ay;
    if (!(hi > 0.0f)) return 0.0f;
    float p = atan_turns_poly(lo / hi);
    if (swap) p = 0.25f - p;
    if (x < 0.0f) p = 0.5f - p;
    return y < 0.0f ? -p : p;
}

// ---- panorama coordinates of a direction: u = 0.5 + phi / 2 pi, v = 0.5 - theta / pi, row 0 is +Y
struct vec2 {
    float x, y;
};
EQUIRECT_HD vec2 panorama_uv(const vec3 &d) {
    const float phi = atan2_turns(d.z, d.x);
    const float theta = atan2_turns(d.y, sqrtf(d.x * d.x + d.z * d.z));
    return vec2{0.5f + phi, 0.5f - (theta + theta)};
}

// ---- the four taps: x = u W - 0.5, y = v H - 0.5, floor and fraction; columns wrap modulo W, rows clamp to [0, H - 1]
struct Taps {
    uint32_t c0, c1, r0, r1;
    float fx, fy;
};
EQUIRECT_HD int32_t floor_i(float x) {  // x in [-1, 65536)
    const int32_t i = (int32_t)x;
    return (float)i > x ? i - 1 : i;
}
EQUIRECT_HD Taps taps_of(const vec2 &uv, uint32_t W, uint32_t H) {
    const float x = uv.x * (float)W - 0.5f, y = uv.y * (float)H - 0.5f;
    const int32_t ix = floor_i(x), iy = floor_i(y);
    Taps t;
    t.fx = x - (float)ix;
    t.fy = y - (float)iy;
    // u, v lie in [0, 1]: ix in [-1, W - 1], iy in [-1, H - 1].  The second select of c0 only keeps the index inside the
    // source whatever the arithmetic above it was given.
    const int32_t w = (int32_t)W, h = (int32_t)H;
    int32_t c0 = ix < 0 ? ix + w : (ix >= w ? ix - w : ix);
    c0 = c0 < 0 ? 0 : (c0 > w - 1 ? w - 1 : c0);
    const int32_t c1 = c0 + 1 >= w ? 0 : c0 + 1;
    const int32_t r0 = iy < 0 ? 0 : (iy > h - 1 ? h - 1 : iy), r1 = iy + 1 < 0 ? 0 : (iy + 1 > h - 1 ? h - 1 : iy + 1);
    t.c0 = (uint32_t)c0; t.c1 = (uint32_t)c1; t.r0 = (uint32_t)r0; t.r1 = (uint32_t)r1;
    return t;
}
EQUIRECT_HD Taps face_taps(uint32_t f, uint32_t i, uint32_t j, uint32_t n, uint32_t W, uint32_t H) {
    return taps_of(panorama_uv(face_direction(f, i, j, n)), W, H);
}

// the bilinear filter of the faces: top = a + (b - a) fx, bottom = c + (d - c) fx, out = top + (bottom - top) fy; a = (c0, r0),
// b = (c1, r0), c = (c0, r1), d = (c1, r1).  Equal taps give that value exactly.
EQUIRECT_HD float lerp1(float a, float b, float f) { return a + (b - a) * f; }
EQUIRECT_HD vec4 bilinear(const vec4 &a, const vec4 &b, const vec4 &c, const vec4 &d, float fx, float fy) {
    return vec4{lerp1(lerp1(a.x, b.x, fx), lerp1(c.x, d.x, fx), fy), lerp1(lerp1(a.y, b.y, fx), lerp1(c.y, d.y, fx), fy),
                lerp1(lerp1(a.z, b.z, fx), lerp1(c.z, d.z, fx), fy), lerp1(lerp1(a.w, b.w, fx), lerp1(c.w, d.w, fx), fy)};
}

// ---- the chain: level k + 1 of a face (extent d = max(1, s >> 1)) from level k (extent s): the Linear / ClampToEdge blit of
// k_generate_mip_f32 (texture_decode.hip) on float texels, all four channels, without a render-target rounding.  Per face: nothing
// is filtered across an edge.
EQUIRECT_HD uint32_t half_extent(uint32_t s) { return s > 1u ? s >> 1 : 1u; }
struct ChainTaps {
    uint32_t x0, x1;
    float f;
};
EQUIRECT_HD ChainTaps chain_taps(uint32_t x, uint32_t s, uint32_t d) {
    const float u = ((float)x + 0.5f) / (float)d;
    const float t = u * (float)s - 0.5f;
    const int32_t i = floor_i(t), hi = (int32_t)s - 1;
    ChainTaps c;
    c.f = t - (float)i;
    c.x0 = (uint32_t)(i < 0 ? 0 : (i > hi ? hi : i));
    c.x1 = (uint32_t)(i + 1 < 0 ? 0 : (i + 1 > hi ? hi : i + 1));
    return c;
}
EQUIRECT_HD float blit1(float q0, float q1, float q2, float q3, float fx, float fy) {
    const float top = q0 * (1.0f - fx) + q1 * fx;
    const float bot = q2 * (1.0f - fx) + q3 * fx;
    return top * (1.0f - fy) + bot * fy;
}
EQUIRECT_HD vec4 blit(const vec4 &a, const vec4 &b, const vec4 &c, const vec4 &d, float fx, float fy) {
    return vec4{blit1(a.x, b.x, c.x, d.x, fx, fy), blit1(a.y, b.y, c.y, d.y, fx, fy), blit1(a.z, b.z, c.z, d.z, fx, fy),
                blit1(a.w, b.w, c.w, d.w, fx, fy)};
}
// texel (x, y) of the next level of ONE face held as s * s texels at `src`
template <class Fetch>
EQUIRECT_HD vec4 chain_texel(Fetch fetch, uint32_t x, uint32_t y, uint32_t s, uint32_t d) {
    const ChainTaps cx = chain_taps(x, s, d), cy = chain_taps(y, s, d);
    return blit(fetch(cy.x0 * s + cx.x0), fetch(cy.x0 * s + cx.x1), fetch(cy.x1 * s + cx.x0), fetch(cy.x1 * s + cx.x1), cx.f, cy.f);
}

// ---- the launch plan of the equirect sources of one call, a function of (face extents, mips, tail threshold T):
//     1 launch of k_equirect_faces (level 0 of every such cube);
//     level launch k = 1, 2, ...: level k of every cube with k <= tail_from(cube), across all its faces;
//     1 tail launch when some cube has levels behind tail_from: one workgroup per (cube, face) builds them all through LDS.
// tail_from = the first level whose extent is at most T (T = 0: never), the last level when there is none.  Every plan gives the
// same words: a level is the same function of the level above whichever kernel evaluates it.
EQUIRECT_HD uint32_t level_extent(uint32_t n0, uint32_t k) {
    const uint32_t n = k < 32u ? n0 >> k : 0u;
    return n ? n : 1u;
}
EQUIRECT_HD uint32_t max_mips(uint32_t n0) {
    uint32_t m = 0;
    for (uint32_t n = n0; n; n >>= 1) ++m;
    return m;
}
EQUIRECT_HD uint32_t tail_from(uint32_t n0, uint32_t mips, uint32_t T) {
    for (uint32_t k = 0; k + 1u < mips; ++k)
        if (T && level_extent(n0, k) <= T) return k;
    return mips - 1u;
}
struct Plan {
    uint32_t faces;   // 0 | 1: the k_equirect_faces launch
    uint32_t levels;  // level launches
    uint32_t tail;    // 0 | 1: the tail launch
};
EQUIRECT_HD Plan plan(const uint32_t *extents, const uint32_t *mips, uint32_t n_cubes, uint32_t T) {
    Plan p{n_cubes ? 1u : 0u, 0u, 0u};
    for (uint32_t c = 0; c < n_cubes; ++c) {
        const uint32_t from = tail_from(extents[c], mips[c], T);
        if (from > p.levels) p.levels = from;
        if (from + 1u < mips[c]) p.tail = 1u;
    }
    return p;
}
EQUIRECT_HD uint32_t plan_launches(const Plan &p) { return p.faces + p.levels + p.tail; }

}  // namespace equirect_rule
