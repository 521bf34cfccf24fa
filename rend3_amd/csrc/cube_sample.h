// cube_sample.h -- the lookup of a cube of the pool (skybox.h) by direction: face selection, the seamless bilinear footprint on the
// bordered faces, and the mix of two levels.  Shared by the skybox node (skybox.hip), which derives the level from the direction's
// screen-space differences, and by the environment lookups (ibl_lookup.h), which are given it.  Arithmetic contract: DESIGN.md
// section 2, restated in tests/skybox_reference.py: f32, one rounding per operation, IEEE division.
#pragma once
#include <hip/hip_runtime.h>

#include "cube_faces.h"
#include "device_math.h"

// A texel of a bordered face (skybox.h), decoded BEFORE filtering.
R3N_DEV void sky_decode(const float *__restrict__ tab, uint32_t w, float o[3]) {
    o[0] = tab[w & 0xFFu]; o[1] = tab[(w >> 8) & 0xFFu]; o[2] = tab[(w >> 16) & 0xFFu];
}
// floor(coordinate) of the footprint's first texel -> its index in the bordered face.  s in [0, 1] gives a floor in [-1, N - 1];
// anything else (a NaN direction) is clamped, so no fetch can leave the face's (N + 2)^2 words.
R3N_DEV uint32_t sky_border_index(float f0, uint32_t n) {
    int i = (f0 == f0) ? (int)fminf(fmaxf(f0, -1.0f), (float)n) : -1;
    i = i < -1 ? -1 : (i > (int)n - 1 ? (int)n - 1 : i);
    return (uint32_t)(i + 1);
}
// face and coordinates of direction d (Vulkan / WebGPU cube table; ties: z over y over x; a component that is not negative selects
// the positive face): (sc, tc) and the major component's magnitude ma
R3N_DEV void sky_select_face(const float d[3], uint32_t &face, float &sc, float &tc, float &ma) {
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    if (az >= ax && az >= ay) {
        const bool neg = d[2] < 0.0f;
        face = neg ? 5u : 4u; sc = neg ? -d[0] : d[0]; tc = -d[1]; ma = az;
    } else if (ay >= ax) {
        const bool neg = d[1] < 0.0f;
        face = neg ? 3u : 2u; sc = d[0]; tc = neg ? -d[2] : d[2]; ma = ay;
    } else {
        const bool neg = d[0] < 0.0f;
        face = neg ? 1u : 0u; sc = neg ? d[2] : -d[2]; tc = -d[1]; ma = ax;
    }
}
// a row of the cube table: (sc, tc) and the signed major component m of direction e ON FACE `face` -- the face is given, not
// selected from e
R3N_DEV void sky_project(uint32_t face, const float e[3], float &sc, float &tc, float &m) {
    const bool neg = (face & 1u) != 0u;
    if (face >= 4u) { sc = neg ? -e[0] : e[0]; tc = -e[1]; m = neg ? -e[2] : e[2]; }
    else if (face >= 2u) { sc = e[0]; tc = neg ? -e[2] : e[2]; m = neg ? -e[1] : e[1]; }
    else { sc = neg ? e[2] : -e[2]; tc = -e[1]; m = neg ? -e[0] : e[0]; }
}
template <bool F32>
R3N_DEV void sky_fetch(const uint32_t *__restrict__ face, const float *__restrict__ tab, size_t at, float o[3]) {
    if (F32) {
        const float4 v = reinterpret_cast<const float4 *>(face)[at];
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    } else {
        sky_decode(tab, face[at], o);
    }
}
// (bx, by) in [0, N + 1]^2.  The four corner positions of the bordered face have no texel: there the value is ((a + b) + c) / 3 per
// channel of the in-face corner texel a, its neighbour b across the s edge and its neighbour c across the t edge -- both are
// border texels of this very face.
template <bool F32>
R3N_DEV void sky_texel_any(const uint32_t *__restrict__ face, const float *__restrict__ tab, uint32_t n, uint32_t bx, uint32_t by, float o[3]) {
    const uint32_t pitch = n + 2u;
    const bool edge_x = bx == 0u || bx == n + 1u, edge_y = by == 0u || by == n + 1u;
    if (edge_x && edge_y) {
        const uint32_t ix = bx == 0u ? 1u : n, iy = by == 0u ? 1u : n;
        float a[3], b[3], c[3];
        sky_fetch<F32>(face, tab, (size_t)iy * pitch + ix, a);
        sky_fetch<F32>(face, tab, (size_t)iy * pitch + bx, b);
        sky_fetch<F32>(face, tab, (size_t)by * pitch + ix, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = ((a[k] + b[k]) + c[k]) / 3.0f;
        return;
    }
    sky_fetch<F32>(face, tab, (size_t)by * pitch + bx, o);
}
// the seamless bilinear on the bordered face `face_texels` of extent n: the 2D sampler's footprint (texture.h tex_level_footprint /
// tex_bilinear) through the border
template <bool F32>
R3N_DEV void sky_bilinear(const uint32_t *__restrict__ face_texels, const float *__restrict__ tab, uint32_t n, float s, float t, float v[3]) {
    const float tx = s * (float)n - 0.5f, ty = t * (float)n - 0.5f;
    const float fx0 = floorf(tx), fy0 = floorf(ty);
    float fx = tx - fx0, fy = ty - fy0;
    if (!(fx == fx)) fx = 0.0f;
    if (!(fy == fy)) fy = 0.0f;
    const uint32_t x0 = sky_border_index(fx0, n), y0 = sky_border_index(fy0, n);
    float c00[3], c10[3], c01[3], c11[3];
    sky_texel_any<F32>(face_texels, tab, n, x0, y0, c00);
    sky_texel_any<F32>(face_texels, tab, n, x0 + 1u, y0, c10);
    sky_texel_any<F32>(face_texels, tab, n, x0, y0 + 1u, c01);
    sky_texel_any<F32>(face_texels, tab, n, x0 + 1u, y0 + 1u, c11);
    const float omx = 1.0f - fx, omy = 1.0f - fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = c00[k] * omx + c10[k] * fx, bot = c01[k] * omx + c11[k] * fx;
        v[k] = top * omy + bot * fy;
    }
}
// The lookup with the level GIVEN: the seamless bilinear on `level` of the cube at `texels` (extent n0, `mips` levels; tab: the
// decode table of its class, RGBA8 classes only), and on level + 1 when frac > 0, mixed as the skybox mixes them:
// v (1 - frac) + hi frac.  The caller keeps level <= mips - 1, and frac = 0 on the last level.
template <bool F32>
R3N_DEV void cube_sample_level(const uint32_t *__restrict__ texels, const float *__restrict__ tab, uint32_t n0, uint32_t mips, const float dir[3], uint32_t level, float frac,
                               float v[3]) {
    uint32_t face;
    float sc, tc, ma;
    sky_select_face(dir, face, sc, tc, ma);
    const float s = 0.5f * (sc / ma) + 0.5f, t = 0.5f * (tc / ma) + 0.5f;
    constexpr uint32_t per_texel = F32 ? 4u : 1u;
    const uint32_t n = cube_faces::level_extent(n0, level);
    const uint32_t *lvl = texels + cube_faces::level_start(n0, level, per_texel);
    sky_bilinear<F32>(lvl + (size_t)face * cube_faces::face_words(n, per_texel), tab, n, s, t, v);
    if (frac > 0.0f && level + 1u < mips) {
        const uint32_t n1 = cube_faces::level_extent(n0, level + 1u);
        const uint32_t *lvl1 = lvl + cube_faces::level_words(n, per_texel);
        float hi[3];
        sky_bilinear<F32>(lvl1 + (size_t)face * cube_faces::face_words(n1, per_texel), tab, n1, s, t, hi);
        const float omf = 1.0f - frac;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] * omf + hi[k] * frac;
    }
}
