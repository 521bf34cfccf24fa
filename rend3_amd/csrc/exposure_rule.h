// exposure_rule.h -- the auto-exposure and tonemapping-operator rule (DESIGN.md section 2 "Exposure and tonemapping operators"),
// shared by the kernels (exposure.hip), the host side of r3n_tonemap_set (r3n.hip) and the stand-alone check program
// (tests/exposure_rule_check.cpp).  Completes rend3-routine/src/tonemapping.rs:1-10 ("no tonemapping applied as we don't have
// auto-exposure yet"); nothing here restates reference code.
//
// Everything is f32 in the order written, one rounding per operation (the units are built with -ffp-contract=off), IEEE division;
// floorf / ldexpf are exact.  No transcendental is evaluated at run time: the two tables (bin values, 2^(k/256)) are built once on
// the host in double.  The metering is integer arithmetic, so it does not depend on the order in which pixels were counted.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define R3N_EXP_HD __host__ __device__ inline
#else
#define R3N_EXP_HD inline
#endif

#define R3N_EXP_BINS 256         // 8 per octave over [2^-16, 2^16)
#define R3N_EXP_E_ENTRIES 257    // E[k] = (float)exp2(k / 256.0), k = 0..256
#define R3N_EXP_MAX_HALF 65504.0f

namespace exposure_rule {

// what r3n_tonemap_set validated, as the kernels take it
struct Params {
    uint32_t op, exposure_mode;
    float exposure_ev, white_sq, key_log2, min_ev, max_ev, adapt;
    uint32_t low_permille, high_permille;
};
// the state words of r3n_exposure_state behind its histogram
struct Step {
    uint32_t valid;
    float mean_log2, target_ev, current_ev, scale;
};

R3N_EXP_HD uint32_t f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// l = (0.2126 r + 0.7152 g) + 0.0722 b of the stored halves widened to f32
R3N_EXP_HD float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// bin of a luminance, -1: excluded (NaN, zero, negative).  Exponent and top three mantissa bits: (bits >> 20) - 888 is 8 * (e - 127 +
// 16) + the mantissa's top three bits, clamped (below 2^-16 -> 0; 2^16 and above, +inf included -> 255)
R3N_EXP_HD int bin_of(float l) {
    if (!(l > 0.0f)) return -1;
    const int b = (int)(f32_bits(l) >> 20) - 888;
    return b < 0 ? 0 : (b > R3N_EXP_BINS - 1 ? R3N_EXP_BINS - 1 : b);
}

// Lq[j]: log2 of the bin's middle in 1/65536 steps; E[k]: 2^(k/256).  Host tables, uploaded once.
inline void build_tables(int32_t lq[R3N_EXP_BINS], float e[R3N_EXP_E_ENTRIES]) {
    for (int j = 0; j < R3N_EXP_BINS; ++j)
        lq[j] = (int32_t)llround(((double)((j >> 3) - 16) + log2(1.0 + ((double)(j & 7) + 0.5) / 8.0)) * 65536.0);
    for (int k = 0; k < R3N_EXP_E_ENTRIES; ++k) e[k] = (float)exp2((double)k / 256.0);
}

// scale = 2^e by linear interpolation in the 256-step table: an integer stop is exactly a power of two
R3N_EXP_HD float exp2_lin(float e, const float *E) {
    const float i = floorf(e);
    const float f = e - i;
    const float t = f * 256.0f;
    const int k = (int)t;
    const float w = t - (float)k;
    const float m = E[k] + (E[k < 256 ? k + 1 : 256] - E[k]) * w;  // (k == 256: f rounded up to 1, w == 0; the table ends at E[256])
    return ldexpf(m, (int)i);
}

R3N_EXP_HD float clamp_ev(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ranks [lo, hi) of the sorted luminances: T = sum of the histogram, floor division in u64
R3N_EXP_HD void rank_window(uint64_t total, const Params &p, uint64_t &lo, uint64_t &hi) {
    lo = total * (uint64_t)p.low_permille / 1000u;
    hi = total * (uint64_t)p.high_permille / 1000u;
}
// the share of bin j (exclusive prefix c0, inclusive c1) that lies inside [lo, hi)
R3N_EXP_HD uint64_t bin_share(uint64_t c0, uint64_t c1, uint64_t lo, uint64_t hi) {
    const uint64_t a = c0 > lo ? c0 : lo, b = c1 < hi ? c1 : hi;
    return b > a ? b - a : 0u;
}
// S = sum n_j Lq[j], N = hi - lo -- the serial form (the kernel computes the same integers with a wave-wide prefix)
R3N_EXP_HD void meter_serial(const uint32_t hist[R3N_EXP_BINS], const int32_t *lq, const Params &p, int64_t &S, uint64_t &N) {
    uint64_t total = 0;
    for (int j = 0; j < R3N_EXP_BINS; ++j) total += hist[j];
    uint64_t lo, hi;
    rank_window(total, p, lo, hi);
    N = hi - lo;
    S = 0;
    uint64_t c = 0;
    for (int j = 0; j < R3N_EXP_BINS; ++j) {
        S += (int64_t)bin_share(c, c + hist[j], lo, hi) * (int64_t)lq[j];
        c += hist[j];
    }
}

// One step of the adaptation from the state the previous frame committed.  prev_valid == 0: nothing metered yet (or the options
// changed): the first metered frame adapts instantly.  N == 0 (nothing to meter): the state is carried over; while it is still
// invalid the exposure is clamp(exposure_ev).
R3N_EXP_HD Step step(const Step &prev, int64_t S, uint64_t N, const Params &p, const float *E) {
    Step s;
    if (N == 0u) {
        if (prev.valid) return prev;
        s.valid = 0u;
        s.mean_log2 = 0.0f;
        s.target_ev = clamp_ev(p.exposure_ev, p.min_ev, p.max_ev);
        s.current_ev = s.target_ev;
        s.scale = exp2_lin(s.current_ev, E);
        return s;
    }
    s.valid = 1u;
    s.mean_log2 = (float)((double)S / ((double)N * 65536.0));
    s.target_ev = clamp_ev((p.key_log2 - s.mean_log2) + p.exposure_ev, p.min_ev, p.max_ev);
    if (!prev.valid || p.adapt == 1.0f) s.current_ev = s.target_ev;
    else s.current_ev = prev.current_ev + (s.target_ev - prev.current_ev) * p.adapt;
    s.scale = exp2_lin(s.current_ev, E);
    return s;
}

// one colour channel: exposure, clamp to the half range, operator.  (Alpha is not passed through here.)
R3N_EXP_HD float exposed(float h, float scale) {
    const float v = h * scale;
    return !(v > 0.0f) ? 0.0f : (v >= R3N_EXP_MAX_HALF ? R3N_EXP_MAX_HALF : v);
}
R3N_EXP_HD float op_reinhard(float v, float white_sq) { return (v * (1.0f + v / white_sq)) / (1.0f + v); }
R3N_EXP_HD float op_aces(float v) { return (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f); }

}  // namespace exposure_rule
