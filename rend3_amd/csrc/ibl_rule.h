// ibl_rule.h -- the rule that prefilters an environment cube: a chain of GGX-prefiltered specular levels and nine SH coefficients of
// its radiance (DESIGN.md section 2 "Environment prefilter"; include/r3n.h r3n_environment_prefilter).  Plain C++17, no HIP, no
// context: shared by the kernels (ibl.hip), the lookup (ibl_lookup.h), the host (r3n.hip) and the stand-alone check program
// (tests/ibl_rule_check.cpp), which runs `prefilter` and `sh9` below serially; tests/ibl_reference.py restates both in numpy f32.
//
// Everything is PINNED: f32 in the order written, one rounding per operation (the units are built with -ffp-contract=off), IEEE
// division and square root, comparisons, selects, integers.  No libm call.
//
// 1. Inputs.  A cube, a base level of extent S <= MAX_EXTENT and L levels, 2 <= L <= min(stored levels from the base,
//    floor(log2 S) + 1, MAX_LEVELS).  Source level k is the stored level base + k (extent n_k = max(1, S >> k)): chains are never
//    generated here.  The radiance of a texel is its decoded interior texel, each channel through envlight_rule::sanitise (NaN,
//    +-inf, negative and zero count as 0); its unit direction u and solid angle w are envlight_rule::geometry's.
// 2. Result level 0 is source level 0, decoded, alpha 1, NOT sanitised: the mirror level.
// 3. Result level k in 1 .. L - 1, output texel o of extent n_k with N = geometry(o).u integrates SOURCE LEVEL k, which has the
//    same direction grid, so o's own texel always contributes (q = 0, weight w / a2^2 > 0) and the denominator is never 0:
//        r = (float)k / (float)(L - 1), a = r r, a2 = a a, oma = 1 - a2                         (`roughness`)
//        per source texel t:  dx = N.x - u.x ..., q = (dx dx + dy dy) + dz dz                    chord^2 = 2 (1 - N.u)
//                             q < 2, else the term is skipped                                    N.u <= 0
//                             cs = 1 - q 0.5;  d = a2 + (q 0.25) oma;  wt = (cs w) / (d d)       (`weight`)
//                             num[ch] += wt c[ch];  den += wt
//        out[ch] = num[ch] / den, alpha 1.
//    This is D(h) (N.L) dw of the GGX lobe with N = V = R, (N.H)^2 = 1 - q / 4, up to the constant a2 / pi, which cancels.  The
//    chord form is deliberate: with cs = dot(N, u) and d = h2 (a2 - 1) + 1 the f32 result is up to 5e-5 off a float64 evaluation
//    at a = 0.04 (cancellation at the lobe's centre, where the weight is largest); the chord form has no cancellation there.
//    A skipped term and a term of weight 0 give the same words: every term is >= +0, and x + (+0) = x for every x >= +0.
// 4. The summation tree.  Every sum (num[3], den; the 27 sums of 5.) is taken per source ROW in ascending i, the row sums per FACE
//    in ascending j, the six face sums in face order; all f32, every accumulator starting at +0 (`Tree`).  A thread that walks the
//    source in linear order (f n + j) n + i implements it with three accumulators per sum, whatever the launch plan.
// 5. SH9.  Source: the first source level k >= 0 of extent <= SH_EXTENT, else level L - 1 (`sh_level`).  With (x, y, z) = u:
//        Y[0] = 0.282095                      Y[1] = 0.488603 y            Y[2] = 0.488603 z          Y[3] = 0.488603 x
//        Y[4] = (1.092548 x) y                Y[5] = (1.092548 y) z        Y[6] = 0.315392 (((3 z) z) - 1)
//        Y[7] = (1.092548 x) z                Y[8] = 0.546274 (x x - y y)
//    L[m][ch] = sum c[ch] (w Y[m]) under the tree.  The ambient radiance in direction n is E(n) / pi, E(n) = sum A_l L[m] Y[m](n),
//    A = (pi, 2 pi / 3, pi / 4): `irradiance` adds (K[m] L[m][ch]) Y[m](n) for m = 0 .. 8 in that order from +0, with
//    K = A / pi: 1 for m = 0, 2/3 (the f32 literal 0.6666667) for m = 1 .. 3, 1/4 for m = 4 .. 8.
//
// ERROR against a float64 evaluation of the same formulas FROM THE SAME f32 inputs (u, w, c, N, a2, oma).  A term wt c takes twelve
// roundings (3 differences, 3 squares and 2 sums for q; cs: 2; d: 3 of which the sum dominates; cs w, d d, the division, the
// product with c -- d enters squared, so its three count twice; the term is within 12 * 2^-24 relative to first order, all factors
// being positive and none formed by cancellation: q is a sum of squares, cs > 0 is scaled by its own rounding only where q is near
// 2, where the weight itself vanishes).  A sum of positive terms through the tree passes at most n + n + 6 additions, each
// (1 + e), |e| <= 2^-24: relative (2 n + 6) * 2^-24.  Numerator and denominator each carry tree + term, the quotient one more
// rounding, so per channel
//        |out - out64| <= (2 (2 n + 6) + 24 + 1) * 2^-24 * out64                                   (`prefilter_bound`)
// to first order (the +1 is the final division; tests hold the reference to this with n the level's extent).  The SH sums are
// signed, so the same form holds relative to sum |term|: (2 n + 6 + 5) * 2^-24 * sum |c w Y| (`sh_bound`: Y takes at most four
// roundings, w Y one).
#pragma once
#include <stdint.h>

#include "envlight_rule.h"

#if defined(__HIPCC__)
#define IBL_HD __host__ __device__ inline
#else
#define IBL_HD inline
#endif

namespace ibl_rule {

using envlight_rule::vec3;

constexpr uint32_t MAX_EXTENT = 256u, MAX_LEVELS = 16u, SH_EXTENT = 32u;

IBL_HD uint32_t level_extent(uint32_t S, uint32_t k) {
    const uint32_t n = k < 32u ? S >> k : 0u;
    return n ? n : 1u;
}
// floor(log2 S) + 1, S >= 1
IBL_HD uint32_t levels_of(uint32_t S) {
    uint32_t l = 0;
    while (S) { ++l; S >>= 1; }
    return l;
}
// the most levels a call may ask for from a base level of extent S with `stored` levels from the base on
IBL_HD uint32_t max_levels(uint32_t S, uint32_t stored) {
    uint32_t m = levels_of(S);
    if (m > stored) m = stored;
    return m > MAX_LEVELS ? MAX_LEVELS : m;
}
IBL_HD uint32_t sh_level(uint32_t S, uint32_t L) {
    for (uint32_t k = 0; k < L; ++k)
        if (level_extent(S, k) <= SH_EXTENT) return k;
    return L - 1u;
}

// ---- 3. the lobe of level k
struct Roughness {
    float a2, oma;
};
IBL_HD Roughness roughness(uint32_t k, uint32_t L) {
    const float r = (float)k / (float)(L - 1u);
    const float a = r * r;
    Roughness o;
    o.a2 = a * a;
    o.oma = 1.0f - o.a2;
    return o;
}
// the weight of a source texel (unit direction u, solid angle w) for the output direction N; 0 for a skipped term
IBL_HD float weight(const vec3 &N, const vec3 &u, float w, const Roughness &r) {
    const float dx = N.x - u.x, dy = N.y - u.y, dz = N.z - u.z;
    const float q = (dx * dx + dy * dy) + dz * dz;
    if (!(q < 2.0f)) return 0.0f;
    const float cs = 1.0f - q * 0.5f;
    const float d = r.a2 + (q * 0.25f) * r.oma;
    return (cs * w) / (d * d);
}

// ---- 4. the tree: NV sums side by side
template <int NV>
struct Tree {
    float row[NV], face[NV], total[NV];
};
template <int NV>
IBL_HD void tree_clear(Tree<NV> &t) {
    for (int v = 0; v < NV; ++v) t.row[v] = t.face[v] = t.total[v] = 0.0f;
}
template <int NV>
IBL_HD void tree_end_row(Tree<NV> &t) {
    for (int v = 0; v < NV; ++v) {
        t.face[v] = t.face[v] + t.row[v];
        t.row[v] = 0.0f;
    }
}
template <int NV>
IBL_HD void tree_end_face(Tree<NV> &t) {
    for (int v = 0; v < NV; ++v) {
        t.total[v] = t.total[v] + t.face[v];
        t.face[v] = 0.0f;
    }
}

// ---- 5. the basis
constexpr float Y00 = 0.282095f, Y1 = 0.488603f, Y2A = 1.092548f, Y20 = 0.315392f, Y22 = 0.546274f;
IBL_HD void basis(const vec3 &u, float Y[9]) {
    Y[0] = Y00;
    Y[1] = Y1 * u.y;
    Y[2] = Y1 * u.z;
    Y[3] = Y1 * u.x;
    Y[4] = (Y2A * u.x) * u.y;
    Y[5] = (Y2A * u.y) * u.z;
    Y[6] = Y20 * (((3.0f * u.z) * u.z) - 1.0f);
    Y[7] = (Y2A * u.x) * u.z;
    Y[8] = Y22 * (u.x * u.x - u.y * u.y);
}
// K[m] = A_l / pi
IBL_HD float band_scale(int m) { return m == 0 ? 1.0f : (m < 4 ? 0.6666667f : 0.25f); }
// E(n) / pi from the nine coefficients (sh[m][ch], ch < 3)
IBL_HD void irradiance(const float sh[9][4], const vec3 &n, float out[3]) {
    float Y[9];
    basis(n, Y);
    for (int ch = 0; ch < 3; ++ch) {
        float e = 0.0f;
        for (int m = 0; m < 9; ++m) e = e + (band_scale(m) * sh[m][ch]) * Y[m];
        out[ch] = e;
    }
}

// ---- the bounds of the header's error paragraph, relative
inline double prefilter_bound(uint32_t n) { return (double)(2u * (2u * n + 6u) + 25u) * 5.9604644775390625e-8; }
inline double sh_bound(uint32_t n) { return (double)(2u * n + 6u + 5u) * 5.9604644775390625e-8; }

// ---- the serial definitions the kernels are held to.  rgb: the 6 n n texels of ONE source level, three f32 each, in linear-index
// order, decoded, NOT sanitised.
// result level k >= 1 from source level k of extent n: out = 6 n n texels of four f32
inline void prefilter_level(const float *rgb, uint32_t n, uint32_t k, uint32_t L, float *out) {
    const Roughness r = roughness(k, L);
    const uint32_t count = 6u * n * n;
    for (uint32_t o = 0; o < count; ++o) {
        const vec3 N = envlight_rule::geometry_at(o, n).u;
        Tree<4> t;
        tree_clear(t);
        uint32_t s = 0;
        for (uint32_t f = 0; f < 6u; ++f) {
            for (uint32_t j = 0; j < n; ++j) {
                for (uint32_t i = 0; i < n; ++i, ++s) {
                    const envlight_rule::Geometry g = envlight_rule::geometry(f, i, j, n);
                    const float wt = weight(N, g.u, g.w, r);
                    for (int ch = 0; ch < 3; ++ch) t.row[ch] = t.row[ch] + wt * envlight_rule::sanitise(rgb[3u * s + ch]);
                    t.row[3] = t.row[3] + wt;
                }
                tree_end_row(t);
            }
            tree_end_face(t);
        }
        for (int ch = 0; ch < 3; ++ch) out[4u * o + ch] = t.total[ch] / t.total[3];
        out[4u * o + 3u] = 1.0f;
    }
}
// levels_rgb[k]: source level k (k = 0 .. L - 1); out[k]: result level k, 6 n_k n_k texels of four f32
inline void prefilter(const float *const *levels_rgb, uint32_t S, uint32_t L, float *const *out) {
    const uint32_t count0 = 6u * S * S;
    for (uint32_t t = 0; t < count0; ++t) {
        for (int ch = 0; ch < 3; ++ch) out[0][4u * t + ch] = levels_rgb[0][3u * t + ch];
        out[0][4u * t + 3u] = 1.0f;
    }
    for (uint32_t k = 1; k < L; ++k) prefilter_level(levels_rgb[k], level_extent(S, k), k, L, out[k]);
}
// the nine coefficients of one level of extent n
inline void sh9(const float *rgb, uint32_t n, float sh[9][4]) {
    Tree<27> t;
    tree_clear(t);
    uint32_t s = 0;
    for (uint32_t f = 0; f < 6u; ++f) {
        for (uint32_t j = 0; j < n; ++j) {
            for (uint32_t i = 0; i < n; ++i, ++s) {
                const envlight_rule::Geometry g = envlight_rule::geometry(f, i, j, n);
                float Y[9];
                basis(g.u, Y);
                for (int m = 0; m < 9; ++m) {
                    const float wy = g.w * Y[m];
                    for (int ch = 0; ch < 3; ++ch) t.row[3 * m + ch] = t.row[3 * m + ch] + envlight_rule::sanitise(rgb[3u * s + ch]) * wy;
                }
            }
            tree_end_row(t);
        }
        tree_end_face(t);
    }
    for (int m = 0; m < 9; ++m) {
        for (int ch = 0; ch < 3; ++ch) sh[m][ch] = t.total[3 * m + ch];
        sh[m][3] = 0.0f;
    }
}

}  // namespace ibl_rule
