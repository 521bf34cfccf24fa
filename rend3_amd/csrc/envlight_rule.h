// envlight_rule.h -- the rule that reads directional lights and an ambient term out of one level of a cube (DESIGN.md section 2
// "Environment lights"; include/r3n.h r3n_environment_lights).  Plain C++17, no HIP, no context: shared by the kernels
// (envlight.hip), the host (r3n.hip) and the stand-alone check program (tests/envlight_rule_check.cpp), which runs the whole
// extraction serially through `extract` below; tests/envlight_reference.py restates it in numpy with Python integers.
//
// Everything is PINNED: f32 in the order written, one rounding per operation (the units are built with -ffp-contract=off), IEEE
// division and square root, comparisons, selects and integer operations; the few f64 operations (a conversion of an integer, a
// product with a power of two, a sum, a division, a square root) are IEEE too.  No libm call: a power of two is built from its
// bits, a quantisation is a shift of the mantissa, the rounding of a direction component is a sum and a truncation.
//
// 1. Texel quantities.  Texel (f, i, j) of a level of extent n has the direction d = equirect_rule::face_direction(f, i, j, n)
//    (one component is +-1, the others are sc and tc up to sign), r2 = (1 + sc^2) + tc^2, r = sqrt(r2), the unit direction u = d / r
//    and the solid angle w = 4 / ((n n) (r2 r)).  Its radiance is the decoded texel; a channel that is NaN, +-inf, negative or zero
//    counts as 0 (`sanitise`): an environment with a corrupt texel must not produce a NaN light, and an infinite texel has no
//    finite share to hand to a light.  Its luminance is exposure_rule::luminance of the sanitised channels.
// 2. Order-free sums.  Everything that is summed over texels is an integer, so every launch plan gives the same bits.  e = c w
//    (one f32 product) per channel; e_max = the largest e of the level, found by comparing the bits of the non-negative floats as
//    integers.  With X(e) = max(1, exponent field of e) the scale is S = 2^scale_exp, scale_exp = 166 - X(e_max), which puts e_max
//    into [2^39, 2^40) (below 2^17 when e_max is subnormal), and q = floor(e S) is the mantissa of e shifted by
//    16 + X(e) - X(e_max) <= 16 places: exact, below 2^40, no floating-point operation.  The energy of a texel is
//    qY = (13933 q_r + 46871 q_g + 4732 q_b) >> 16 (the weights sum to 65 536).  The solid angle is quantised the same way at the
//    fixed scale 2^44: qw = floor(w 2^44), exact for n <= 1024 (w >= 4 / (2^20 3^1.5) > 2^-21, so its last mantissa bit is worth
//    at least 2^-44).  A direction is weighted as dq = trunc(u 32767 + 0.5) (minus the same of -u for a negative component), per
//    component, |dq| <= 32767.  Sum qY dq is kept as two sums, of (qY >> 20) dq and of (qY & 0xFFFFF) dq.
//
//    OVERFLOW, for the 6 * 1024^2 < 2^22.6 texels of the largest level the entry takes (MAX_EXTENT):
//      13933 q_r + 46871 q_g + 4732 q_b < 65536 * 2^40 = 2^56                                     (u64)
//      sum q_c, sum qY                  < 2^22.6 * 2^40 = 2^62.6                                  (u64)
//      sum qw                           = 2^44 * (6 sum w) < 2^44 * 4 pi * 1.3 < 2^49             (u64; 6 sum w <= 1.3 * 4 pi for n >= 2,
//                                                                                                  and n = 1 gives 24)
//      each half of sum qY dq           < 2^22.6 * 2^20 * 2^15 = 2^57.6 in magnitude              (i64)
//      cone qY * 2^32 against floor(min_share 2^32) * total qY: both below 2^95                   (u128)
// 3. Peaks, at most max_lights times.  (a) The seed is the live texel of greatest luminance, the f32 bits compared as u32; ties go
//    to the lowest linear index (f n + j) n + i: the u64 key (bits << 32) | ~index under an integer max is order-free.  A texel is
//    DEAD when it lies in the cone of a light already emitted (dot(u, direction) >= cone_cos), live otherwise.  No live texel of
//    luminance above 0: the loop stops.  (b) Gather the live texels with dot(u, centre) >= cone_cos around the seed's u (the dot as
//    (u.x c.x + u.y c.y) + u.z c.z); the new centre is the f32 rounding of the f64 normalisation of their sum qY dq (`shifted`).
//    This is a mean-shift step, and it is taken SHIFT_STEPS = 2 times: without it the cone sits on the rim of a sun disc, because
//    ties break to the disc's first texel, and from the rim of a disc wider than the cone's radius one step covers only part of
//    the disc (a 4 degree disc under a 6 degree cone at n = 32: 1.29 degrees off its axis after one step, 0.57 after two).
//    (c) Gather again around the last centre: this cone is the light.  (d) If its sum qY is 0, or
//    sum qY * 2^32 < floor(min_share * 2^32) * (sum qY of the level), the loop stops: no light is emitted, nothing is consumed.
//    (e) Otherwise the light is emitted and its texels are dead.
// 4. Outputs.  Per light: direction = the centre of (c); irradiance[c] = (float)((double)sum q_c * 2^-scale_exp), at most FLT_MAX;
//    solid_angle = (float)((double)sum qw * 2^-44); texels; the seed's index.  ambient[c] = (float)(((double)sum q_c of what no
//    light took * 2^-scale_exp) / 4 pi), ambient[3] = 1: the solid-angle mean radiance of the remainder, which is the level's sums
//    minus the lights' (the cones are disjoint), so no pass computes it.  A level without energy (e_max == 0) gives no light and
//    ambient 0 with scale_exp 0.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "equirect_rule.h"
#include "exposure_rule.h"

#if defined(__HIPCC__)
#define ENVLIGHT_HD __host__ __device__ inline
#else
#define ENVLIGHT_HD inline
#endif

namespace envlight_rule {

constexpr uint32_t MAX_LIGHTS = 16u, MAX_EXTENT = 1024u, SHIFT_STEPS = 2u;
constexpr int32_t W_SCALE_EXP = 44;
constexpr uint64_t WEIGHT_R = 13933u, WEIGHT_G = 46871u, WEIGHT_B = 4732u;  // 65536 * (0.2126, 0.7152, 0.0722), rounded so that they sum to 65536
constexpr float DIR_SCALE = 32767.0f, COS_MIN = 0.5f;
constexpr double FOUR_PI = 12.566370614359172;  // the f64 nearest 4 pi
constexpr float F32_MAX = 3.4028234663852886e38f;

struct vec3 {
    float x, y, z;
};

ENVLIGHT_HD uint32_t f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
ENVLIGHT_HD double pow2(int32_t e) {  // e in [-1022, 1023]
    const uint64_t u = (uint64_t)(1023 + e) << 52;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// ---- 1. texel quantities
ENVLIGHT_HD float sanitise(float c) { return (c > 0.0f && c <= F32_MAX) ? c : 0.0f; }
struct Geometry {
    vec3 u;
    float w;
};
ENVLIGHT_HD Geometry geometry(uint32_t f, uint32_t i, uint32_t j, uint32_t n) {
    const equirect_rule::vec3 d = equirect_rule::face_direction(f, i, j, n);
    const float fn = (float)n;
    const float sc = (float)((int32_t)(2u * i + 1u) - (int32_t)n) / fn;
    const float tc = (float)((int32_t)(2u * j + 1u) - (int32_t)n) / fn;
    const float r2 = (1.0f + sc * sc) + tc * tc;
    const float r = sqrtf(r2);
    Geometry g;
    g.u = vec3{d.x / r, d.y / r, d.z / r};
    g.w = 4.0f / ((fn * fn) * (r2 * r));
    return g;
}
// linear index (f n + j) n + i of a level of extent n <= MAX_EXTENT
ENVLIGHT_HD void texel_of(uint32_t index, uint32_t n, uint32_t &f, uint32_t &i, uint32_t &j) {
    const uint32_t row = index / n;
    i = index - row * n;
    f = row / n;
    j = row - f * n;
}
ENVLIGHT_HD Geometry geometry_at(uint32_t index, uint32_t n) {
    uint32_t f, i, j;
    texel_of(index, n, f, i, j);
    return geometry(f, i, j, n);
}

// ---- 2. order-free sums
ENVLIGHT_HD uint32_t energy_bits(float c, float w) { return f32_bits(c * w); }  // c sanitised, w > 0: a non-negative float
ENVLIGHT_HD uint32_t exp_field(uint32_t bits) {
    const uint32_t x = (bits >> 23) & 255u;
    return x ? x : 1u;
}
ENVLIGHT_HD int32_t scale_exp_of(uint32_t emax_bits) { return emax_bits ? 166 - (int32_t)exp_field(emax_bits) : 0; }
// floor(m 2^places) for the mantissa m < 2^24 of a non-negative finite float (its value is m 2^(X - 150)); a shift of 64 or more
// places to the right gives 0
ENVLIGHT_HD uint64_t shifted_mantissa(uint32_t bits, int32_t places) {
    const uint32_t x = (bits >> 23) & 255u;
    const uint64_t m = (uint64_t)(bits & 0x7FFFFFu) | (x ? 0x800000u : 0u);
    if (places >= 0) return m << places;  // places <= 16 (quantise: below 2^40) or <= 23 (quantise_w, w <= 4: below 2^47)
    return places > -64 ? m >> -places : 0u;
}
ENVLIGHT_HD uint64_t quantise(uint32_t e_bits, uint32_t emax_bits) {  // floor(e * 2^scale_exp), e <= e_max
    return shifted_mantissa(e_bits, 16 + (int32_t)exp_field(e_bits) - (int32_t)exp_field(emax_bits));
}
ENVLIGHT_HD uint64_t quantise_w(float w) {  // floor(w * 2^44), 0 < w <= 4
    const uint32_t b = f32_bits(w);
    return shifted_mantissa(b, (int32_t)exp_field(b) - 150 + W_SCALE_EXP);
}
ENVLIGHT_HD uint64_t energy(uint64_t qr, uint64_t qg, uint64_t qb) { return (WEIGHT_R * qr + WEIGHT_G * qg + WEIGHT_B * qb) >> 16; }
ENVLIGHT_HD int32_t dir_q(float u) {
    const float x = u * DIR_SCALE;
    return x < 0.0f ? -(int32_t)(0.5f - x) : (int32_t)(x + 0.5f);
}
// what a texel adds to the sums
struct Texel {
    uint64_t q[3], qy, qw;
    float lum;
};
ENVLIGHT_HD float luminance_of(const float rgb[3]) { return exposure_rule::luminance(rgb[0], rgb[1], rgb[2]); }
ENVLIGHT_HD uint32_t texel_emax(const float rgb[3], float w) {  // rgb sanitised
    const uint32_t a = energy_bits(rgb[0], w), b = energy_bits(rgb[1], w), c = energy_bits(rgb[2], w);
    const uint32_t ab = a > b ? a : b;
    return ab > c ? ab : c;
}
ENVLIGHT_HD Texel texel(const float rgb[3], float w, uint32_t emax_bits) {  // rgb sanitised
    Texel t;
    for (int c = 0; c < 3; ++c) t.q[c] = quantise(energy_bits(rgb[c], w), emax_bits);
    t.qy = energy(t.q[0], t.q[1], t.q[2]);
    t.qw = quantise_w(w);
    t.lum = luminance_of(rgb);
    return t;
}

// ---- 3. peaks
ENVLIGHT_HD uint64_t seed_key(float lum, uint32_t index) { return (uint64_t)f32_bits(lum) << 32 | (uint64_t)(~index); }
ENVLIGHT_HD bool seed_valid(uint64_t key) { return (key >> 32) != 0u; }  // a live texel of luminance above 0 was seen
ENVLIGHT_HD uint32_t seed_index(uint64_t key) { return ~(uint32_t)key; }
ENVLIGHT_HD float dot3(const vec3 &u, const vec3 &c) { return (u.x * c.x + u.y * c.y) + u.z * c.z; }
ENVLIGHT_HD bool in_cone(const vec3 &u, const vec3 &centre, float cone_cos) { return dot3(u, centre) >= cone_cos; }
// the six sums of one gather: component c at [c] (of qY >> 20) and [3 + c] (of qY & 0xFFFFF)
ENVLIGHT_HD void shift_terms(uint64_t qy, const vec3 &u, int64_t t[6]) {
    const int64_t hi = (int64_t)(qy >> 20), lo = (int64_t)(qy & 0xFFFFFu);
    const int64_t d[3] = {dir_q(u.x), dir_q(u.y), dir_q(u.z)};
    for (int c = 0; c < 3; ++c) {
        t[c] = hi * d[c];
        t[3 + c] = lo * d[c];
    }
}
// the centre after the mean-shift step; sums of zero length keep the old one
ENVLIGHT_HD vec3 shifted(const vec3 &old, const int64_t s[6]) {
    double v[3];
    for (int c = 0; c < 3; ++c) v[c] = (double)s[c] * 1048576.0 + (double)s[3 + c];
    const double len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(len2 > 0.0)) return old;
    const double len = sqrt(len2);
    return vec3{(float)(v[0] / len), (float)(v[1] / len), (float)(v[2] / len)};
}
ENVLIGHT_HD uint64_t share_floor(float min_share) { return (uint64_t)((double)min_share * 4294967296.0); }  // min_share in [0, 1): exact, below 2^32
ENVLIGHT_HD bool emits(uint64_t cone_qy, uint64_t total_qy, uint64_t share) {
    if (cone_qy == 0u) return false;
    return !(((unsigned __int128)cone_qy << 32) < (unsigned __int128)share * total_qy);
}

// ---- 4. outputs
ENVLIGHT_HD float scaled(uint64_t sum, int32_t scale_exp) {
    const double v = (double)sum * pow2(-scale_exp);
    return v > (double)F32_MAX ? F32_MAX : (float)v;
}
ENVLIGHT_HD float ambient_of(uint64_t sum, int32_t scale_exp) {
    const double v = ((double)sum * pow2(-scale_exp)) / FOUR_PI;
    return v > (double)F32_MAX ? F32_MAX : (float)v;
}

// The raw sums of a set of texels: q per channel, qY, qw, the number of texels.
struct Sums {
    uint64_t q[3], qy, qw, texels;
};
ENVLIGHT_HD void add(Sums &s, const Texel &t) {
    for (int c = 0; c < 3; ++c) s.q[c] += t.q[c];
    s.qy += t.qy;
    s.qw += t.qw;
    s.texels += 1u;
}
ENVLIGHT_HD Sums minus(const Sums &a, const Sums &b) {
    return Sums{{a.q[0] - b.q[0], a.q[1] - b.q[1], a.q[2] - b.q[2]}, a.qy - b.qy, a.qw - b.qw, a.texels - b.texels};
}

// What the passes leave behind, and all the kernels hand to each other (envlight.hip keeps it in device memory, zeroed in front
// of the first pass; every slot is written by ONE pass, with integer atomics, and read only by later ones).  Light k is described
// by seed[k] (a), shift[k][step] (b) and light[k] (c); seed[k + 1] is searched among the texels (c) left alive.
struct State {
    uint32_t emax_bits, pad;
    Sums total;
    uint64_t seed[MAX_LIGHTS + 1u];
    int64_t shift[MAX_LIGHTS][SHIFT_STEPS][6];
    Sums light[MAX_LIGHTS];
};
struct Params {
    uint32_t n, max_lights;
    float cone_cos;
    uint64_t share;  // share_floor(min_share)
};
// the centre of light k's cone once `steps` of its gathers (b) have run: the seed's direction, shifted `steps` times
ENVLIGHT_HD vec3 centre_after(const State &s, uint32_t k, uint32_t n, uint32_t steps) {
    vec3 c = geometry_at(seed_index(s.seed[k]), n).u;
    for (uint32_t t = 0; t < steps; ++t) c = shifted(c, s.shift[k][t]);
    return c;
}
// the direction of light k, once every gather (b) has run
ENVLIGHT_HD vec3 light_centre(const State &s, uint32_t k, uint32_t n) { return centre_after(s, k, n, SHIFT_STEPS); }
// was light k emitted, once its gather (c) has run (lights before it are the caller's concern)
ENVLIGHT_HD bool light_emitted(const State &s, uint32_t k, const Params &p) {
    return s.emax_bits != 0u && k < p.max_lights && seed_valid(s.seed[k]) && emits(s.light[k].qy, s.total.qy, p.share);
}
// the lights of a finished state: those in front of the first that was not emitted
ENVLIGHT_HD uint32_t lights_emitted(const State &s, const Params &p) {
    uint32_t k = 0;
    while (k < p.max_lights && light_emitted(s, k, p)) ++k;
    return k;
}

// ---- what the caller gets, from a finished state
struct LightOut {
    vec3 direction;
    float solid_angle, irradiance[3];
    uint32_t texels;
};
struct Outputs {
    uint32_t n_lights;   // emitted
    uint32_t ran;        // lights whose passes ran: n_lights, plus one for a candidate that was refused by (d)
    int32_t scale_exp;
    float ambient[4];
    Sums remainder;
    LightOut lights[MAX_LIGHTS];  // [0, n_lights)
};
inline Outputs outputs(const State &s, const Params &p) {
    Outputs o;
    memset(&o, 0, sizeof o);
    o.scale_exp = scale_exp_of(s.emax_bits);
    o.n_lights = lights_emitted(s, p);
    o.ran = o.n_lights + ((s.emax_bits != 0u && o.n_lights < p.max_lights && seed_valid(s.seed[o.n_lights])) ? 1u : 0u);
    o.remainder = s.total;
    for (uint32_t k = 0; k < o.n_lights; ++k) {
        LightOut &l = o.lights[k];
        l.direction = light_centre(s, k, p.n);
        l.solid_angle = scaled(s.light[k].qw, W_SCALE_EXP);
        for (int c = 0; c < 3; ++c) l.irradiance[c] = scaled(s.light[k].q[c], o.scale_exp);
        l.texels = (uint32_t)s.light[k].texels;
        o.remainder = minus(o.remainder, s.light[k]);
    }
    for (int c = 0; c < 3; ++c) o.ambient[c] = s.emax_bits ? ambient_of(o.remainder.q[c], o.scale_exp) : 0.0f;
    o.ambient[3] = 1.0f;
    return o;
}

// ---- the whole extraction over host arrays, serially: the definition the kernels are held to.  rgb: 6 n n texels of three f32 in
// linear-index order, already decoded, NOT sanitised.
inline void extract(const float *rgb, const Params &p, State &s) {
    memset(&s, 0, sizeof s);
    const uint32_t n = p.n, count = 6u * n * n;
    for (uint32_t t = 0; t < count; ++t) {
        const float c[3] = {sanitise(rgb[3u * t]), sanitise(rgb[3u * t + 1u]), sanitise(rgb[3u * t + 2u])};
        const uint32_t e = texel_emax(c, geometry_at(t, n).w);
        if (e > s.emax_bits) s.emax_bits = e;
    }
    if (s.emax_bits == 0u) return;
    const auto at = [&](uint32_t t, const Geometry &g) {
        const float c[3] = {sanitise(rgb[3u * t]), sanitise(rgb[3u * t + 1u]), sanitise(rgb[3u * t + 2u])};
        return texel(c, g.w, s.emax_bits);
    };
    vec3 dirs[MAX_LIGHTS];
    const auto live = [&](const vec3 &u, uint32_t k) {
        for (uint32_t l = 0; l < k; ++l)
            if (in_cone(u, dirs[l], p.cone_cos)) return false;
        return true;
    };
    for (uint32_t t = 0; t < count; ++t) {
        const Geometry g = geometry_at(t, n);
        const Texel x = at(t, g);
        add(s.total, x);
        const uint64_t key = seed_key(x.lum, t);
        if (key > s.seed[0]) s.seed[0] = key;
    }
    for (uint32_t k = 0; k < p.max_lights; ++k) {
        if (!seed_valid(s.seed[k])) return;
        for (uint32_t step = 0; step < SHIFT_STEPS; ++step) {
            const vec3 c0 = centre_after(s, k, n, step);
            for (uint32_t t = 0; t < count; ++t) {
                const Geometry g = geometry_at(t, n);
                if (!live(g.u, k) || !in_cone(g.u, c0, p.cone_cos)) continue;
                int64_t terms[6];
                shift_terms(at(t, g).qy, g.u, terms);
                for (int a = 0; a < 6; ++a) s.shift[k][step][a] += terms[a];
            }
        }
        dirs[k] = light_centre(s, k, n);
        for (uint32_t t = 0; t < count; ++t) {
            const Geometry g = geometry_at(t, n);
            if (!live(g.u, k)) continue;
            const Texel x = at(t, g);
            if (in_cone(g.u, dirs[k], p.cone_cos)) {
                add(s.light[k], x);
            } else {
                const uint64_t key = seed_key(x.lum, t);
                if (key > s.seed[k + 1u]) s.seed[k + 1u] = key;
            }
        }
        if (!light_emitted(s, k, p)) return;
    }
}

}  // namespace envlight_rule
