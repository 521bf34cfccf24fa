// bloom_rule.h -- the bloom rule (DESIGN.md section 2 "Bloom"): bright pass, 4x4 tent down-sample, 2x tent up-sample with scatter,
// composite.  Shared by the kernels (bloom.hip, exposure.hip), the host side of r3n_bloom_set (r3n.hip) and the stand-alone check
// program (tests/bloom_rule_check.cpp).  Hangs on rend3-routine/src/tonemapping.rs:1-10 like the operators; nothing here restates
// reference code.
//
// Everything is f32 in the order written, one rounding per operation (the units are built with -ffp-contract=off), IEEE division;
// what is stored is a half, rounded to nearest even.  Weights are small integers and the two normalisations (1/64, 1/16) powers
// of two, so a constant image keeps a constant pyramid exactly.
#pragma once
#include <stdint.h>
#include <string.h>

#include "exposure_rule.h"

#ifndef R3N_BLOOM_MAX_LEVELS
#define R3N_BLOOM_MAX_LEVELS 16u  // (include/r3n.h; the stand-alone check program sees this header alone)
#endif

namespace bloom_rule {

// what r3n_bloom_set validated, with the constants of the bright pass computed once on the host in f32
struct Params {
    float intensity, threshold, knee, scatter;
    float lo, k2, inv;  // threshold - knee, 2 * knee, knee > 0 ? 0.25 / knee : 0
    uint32_t max_levels;
};
R3N_EXP_HD Params make_params(float intensity, float threshold, float knee, float scatter, uint32_t max_levels) {
    Params p;
    p.intensity = intensity; p.threshold = threshold; p.knee = knee; p.scatter = scatter;
    p.lo = threshold - knee;
    p.k2 = 2.0f * knee;
    p.inv = knee > 0.0f ? 0.25f / knee : 0.0f;
    p.max_levels = max_levels;
    return p;
}

// the level sizes: level 0 is ((W + 1) / 2, (H + 1) / 2), each further one halves again (rounding up); the chain ends with the
// first level whose larger side is 1, or at max_levels
struct Levels {
    uint32_t n;
    uint32_t w[R3N_BLOOM_MAX_LEVELS], h[R3N_BLOOM_MAX_LEVELS];
};
R3N_EXP_HD Levels levels(uint32_t W, uint32_t H, uint32_t max_levels) {
    Levels l;
    l.n = 0;
    uint32_t w = W, h = H;
    while (l.n < max_levels && l.n < (uint32_t)R3N_BLOOM_MAX_LEVELS) {
        w = (w + 1u) / 2u; h = (h + 1u) / 2u;
        l.w[l.n] = w; l.h[l.n] = h;
        ++l.n;
        if ((w > h ? w : h) == 1u) break;
    }
    for (uint32_t k = l.n; k < (uint32_t)R3N_BLOOM_MAX_LEVELS; ++k) l.w[k] = l.h[k] = 0u;
    return l;
}

R3N_EXP_HD float half_to_f32(uint16_t h) {
    _Float16 x;
    memcpy(&x, &h, 2);
    return (float)x;
}
// The value is rounded to f32 FIRST and to half second (two roundings, as the contract and numpy's astype do).  On the device the
// compiler would otherwise fold a product and its conversion into one mixed-precision instruction that rounds the exact product
// to half once -- a different half where the f32 result is a tie (16004.0003 -> f32 16004 -> half 16000, but -> half 16008
// directly).  The empty asm makes the f32 value opaque to that fold.
R3N_EXP_HD uint16_t half_rne(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__("" : "+v"(v));
#endif
    const _Float16 x = (_Float16)v;
    uint16_t h;
    memcpy(&h, &x, 2);
    return h;
}
R3N_EXP_HD float max2(float a, float b) { return a > b ? a : b; }
R3N_EXP_HD float min2(float a, float b) { return a < b ? a : b; }
R3N_EXP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bright pass of one pixel: the three stored halves of the HDR target, exposed, weighted by the soft-knee curve of their maximum
R3N_EXP_HD void bright(const uint16_t rgb[3], float scale, const Params &p, uint16_t out[3]) {
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = exposure_rule::exposed(half_to_f32(rgb[c]), scale);
    const float m = max2(v[0], max2(v[1], v[2]));
    const float s = min2(max2(m - p.lo, 0.0f), p.k2);
    const float q = (s * s) * p.inv;
    const float e = max2(q, m - p.threshold);
    const float w = e / max2(m, 6.103515625e-05f);  // 2^-14
    for (int c = 0; c < 3; ++c) out[c] = half_rne(v[c] * w);
}

// 4x4 tent, separable: a row of four taps, then four rows
R3N_EXP_HD float down_row(float s0, float s1, float s2, float s3) { return (s0 + 3.0f * s1) + (3.0f * s2 + s3); }
R3N_EXP_HD float down_col(float r0, float r1, float r2, float r3) { return ((r0 + 3.0f * r1) + (3.0f * r2 + r3)) * 0.015625f; }
// the source column (or row) of tap i = 0..3 of destination x
R3N_EXP_HD int down_tap(int x, int i, int n) { return clampi(2 * x - 1 + i, 0, n - 1); }

// 2x tent up-sample: the nearer and the farther coarse column (or row) of destination x
R3N_EXP_HD int up_near(int x) { return x >> 1; }
R3N_EXP_HD int up_far(int x, int n) { return clampi((x >> 1) + ((x & 1) ? 1 : -1), 0, n - 1); }
R3N_EXP_HD float up_row(float near, float far) { return 3.0f * near + far; }
R3N_EXP_HD float up_col(float hrow_near, float hrow_far) { return (3.0f * hrow_near + hrow_far) * 0.0625f; }
R3N_EXP_HD uint16_t up_store(float d, float u, float scatter) { return half_rne(d + scatter * u); }
R3N_EXP_HD float composite(float v, float b, float intensity) { return min2(v + intensity * b, R3N_EXP_MAX_HALF); }

// One texel of a down step / of an up-sample from a source given as `texel(x, y, rgb)`, which writes the f32 values of the three
// stored halves.  The serial forms: the tiled kernels compute the same row sums once per source row and share them.
template <class F>
R3N_EXP_HD void down_at(F texel, int sw, int sh, int x, int y, uint16_t out[3]) {
    float r[4][3];
    for (int j = 0; j < 4; ++j) {
        const int sy = down_tap(y, j, sh);
        float s[4][3];
        for (int i = 0; i < 4; ++i) texel(down_tap(x, i, sw), sy, s[i]);
        for (int c = 0; c < 3; ++c) r[j][c] = down_row(s[0][c], s[1][c], s[2][c], s[3][c]);
    }
    for (int c = 0; c < 3; ++c) out[c] = half_rne(down_col(r[0][c], r[1][c], r[2][c], r[3][c]));
}
template <class F>
R3N_EXP_HD void up_at(F texel, int cw, int ch, int x, int y, float u[3]) {
    const int xn = up_near(x), xf = up_far(x, cw), yn = up_near(y), yf = up_far(y, ch);
    float nn[3], fn[3], nf[3], ff[3];  // [column][row]: near / far
    texel(xn, yn, nn); texel(xf, yn, fn); texel(xn, yf, nf); texel(xf, yf, ff);
    for (int c = 0; c < 3; ++c) u[c] = up_col(up_row(nn[c], fn[c]), up_row(nf[c], ff[c]));
}

}  // namespace bloom_rule
