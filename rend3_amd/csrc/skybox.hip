// skybox.hip -- the skybox node: rend3-routine/src/skybox.rs (a full-screen triangle at depth 0.0, depth compare GreaterEqual,
// no depth write, drawn between the opaque and the transparent pass, base.rs:175) + skybox.wgsl (fs_main: clip position ->
// world direction through inv_origin_view_proj -> one sample of the cube texture, alpha 1).
//
// One thread per pixel of the row range.  Cubes with levels and cubes of f32 texels (r3n_texture_cubes_write_encoded) take
// instantiations of their own (sky_fragment_levels); a one-level RGBA8 cube runs sky_fragment, unchanged.  Arithmetic contract (restated in tests/skybox_reference.py): f32,
// one rounding per operation (the unit is built with -ffp-contract=off), IEEE division and square root.
#include <hip/hip_runtime.h>

#include "kernels_shade.h"
#include "cube_faces.h"
#include "cube_sample.h"
#include "exact_math.h"
#include "skybox.h"

namespace {

// A texel of a bordered face of RGBA8 words, corners included: cube_sample.h's sky_texel_any for the one-level RGBA8 kernel.
R3N_DEV void sky_texel(const uint32_t *__restrict__ face, const float *__restrict__ tab, uint32_t n, uint32_t bx, uint32_t by, float o[3]) {
    const uint32_t pitch = n + 2u;
    const bool edge_x = bx == 0u || bx == n + 1u, edge_y = by == 0u || by == n + 1u;
    if (edge_x && edge_y) {
        const uint32_t ix = bx == 0u ? 1u : n, iy = by == 0u ? 1u : n;
        float a[3], b[3], c[3];
        sky_decode(tab, face[(size_t)iy * pitch + ix], a);
        sky_decode(tab, face[(size_t)iy * pitch + bx], b);
        sky_decode(tab, face[(size_t)by * pitch + ix], c);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = ((a[k] + b[k]) + c[k]) / 3.0f;
        return;
    }
    sky_decode(tab, face[(size_t)by * pitch + bx], o);
}
// skybox.wgsl fs_main at the centre of pixel (x, y), rounded to half.
R3N_DEV ushort4 sky_fragment(const SkyboxArgs &a, uint32_t x, uint32_t y) {
    // 1. clip position of the pixel centre
    const float cx = (((float)x + 0.5f) * 2.0f) / (float)a.width - 1.0f;
    const float cy = 1.0f - (((float)y + 0.5f) * 2.0f) / (float)a.height;
    // 2. / 3. world direction
    float wu[4];
    mul_vec4(a.fu->inv_origin_view_proj, cx, cy, 1.0f, 1.0f, wu);
    float d[3] = {wu[0] / wu[3], wu[1] / wu[3], wu[2] / wu[3]};
    normalize3(d);  // d * (1 / sqrt(dot3(d, d)))
    // 4. face and coordinates (Vulkan / WebGPU cube table; ties: z over y over x; a component that is not negative selects the
    // positive face)
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    uint32_t face;
    float sc, tc, ma;
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
    const float s = 0.5f * (sc / ma) + 0.5f, t = 0.5f * (tc / ma) + 0.5f;
    // 5. bilinear on level 0 with the 2D sampler's footprint (texture.h tex_level_footprint / tex_bilinear), seamless through the border
    const uint32_t n = a.n;
    const float tx = s * (float)n - 0.5f, ty = t * (float)n - 0.5f;
    const float fx0 = floorf(tx), fy0 = floorf(ty);
    float fx = tx - fx0, fy = ty - fy0;
    if (!(fx == fx)) fx = 0.0f;
    if (!(fy == fy)) fy = 0.0f;
    const uint32_t x0 = sky_border_index(fx0, n), y0 = sky_border_index(fy0, n);
    const uint32_t *face_texels = a.texels + (size_t)face * (n + 2u) * (n + 2u);
    const float *tab = a.decode + (a.srgb ? 256 : 0);
    float c00[3], c10[3], c01[3], c11[3];
    sky_texel(face_texels, tab, n, x0, y0, c00);
    sky_texel(face_texels, tab, n, x0 + 1u, y0, c10);
    sky_texel(face_texels, tab, n, x0, y0 + 1u, c01);
    sky_texel(face_texels, tab, n, x0 + 1u, y0 + 1u, c11);
    const float omx = 1.0f - fx, omy = 1.0f - fy;
    float v[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = c00[k] * omx + c10[k] * fx, bot = c01[k] * omx + c11[k] * fx;
        v[k] = top * omy + bot * fy;
    }
    v[3] = 1.0f;  // 6.
    return pack_half4(v);
}

// ---- cubes with levels and cubes of the f32 class (r3n_texture_cubes_write_encoded).  sky_fragment above stays what a one-level
// RGBA8 cube runs; what follows restates steps 1-4 for three pixel centres and adds level selection.

// steps 1-3 for the centre of pixel (x, y) -- which may lie outside the target
R3N_DEV void sky_direction(const SkyboxArgs &a, uint32_t x, uint32_t y, float d[3]) {
    const float cx = (((float)x + 0.5f) * 2.0f) / (float)a.width - 1.0f;
    const float cy = 1.0f - (((float)y + 0.5f) * 2.0f) / (float)a.height;
    float wu[4];
    mul_vec4(a.fu->inv_origin_view_proj, cx, cy, 1.0f, 1.0f, wu);
    d[0] = wu[0] / wu[3]; d[1] = wu[1] / wu[3]; d[2] = wu[2] / wu[3];
    normalize3(d);
}
template <bool F32, bool LOD>
R3N_DEV ushort4 sky_fragment_levels(const SkyboxArgs &a, uint32_t x, uint32_t y) {
    float d[3];
    sky_direction(a, x, y, d);
    // 4. face and coordinates, as sky_fragment
    uint32_t face;
    float sc, tc, ma;
    sky_select_face(d, face, sc, tc, ma);
    const float s = 0.5f * (sc / ma) + 0.5f, t = 0.5f * (tc / ma) + 0.5f;
    // the level: the gradients are the differences to the pixels (x + 1, y) and (x, y + 1), projected onto THIS face; then
    // tex_footprint's rule (texture.h) with W = H = N.  A one-level cube pays for none of it.
    uint32_t level = 0;
    float frac = 0.0f;
    if (LOD && a.mips > 1u) {
        float e[3], g[2][2];
        bool unbounded = false;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            sky_direction(a, x + (k == 0 ? 1u : 0u), y + (k == 1 ? 1u : 0u), e);
            float sce, tce, me;
            sky_project(face, e, sce, tce, me);
            if (!(me > 0.0f)) unbounded = true;  // at or behind the face's horizon (or NaN): the footprint has no bound
            g[k][0] = (0.5f * (sce / me) + 0.5f) - s;
            g[k][1] = (0.5f * (tce / me) + 0.5f) - t;
        }
        if (unbounded) {
            level = a.mips - 1u;
        } else {
            const float N = (float)a.n;
            const float gax = g[0][0] * N, gay = g[0][1] * N, gbx = g[1][0] * N, gby = g[1][1] * N;
            const float rho = exact_math::sqrt(fmaxf(gax * gax + gay * gay, gbx * gbx + gby * gby));
            if (rho > 1.0f && rho < INFINITY) {
                const uint32_t bits = __float_as_uint(rho);
                level = (bits >> 23) - 127u;
                frac = (float)(bits & 0x7FFFFFu) / 8388608.0f;
            } else if (rho == INFINITY) {
                level = a.mips;  // clamped below
            }
            if (level >= a.mips - 1u) { level = a.mips - 1u; frac = 0.0f; }
        }
    }
    // 5. the seamless bilinear on `level`, and on level + 1 when the fraction asks for it
    constexpr uint32_t per_texel = F32 ? 4u : 1u;
    const float *tab = a.decode + (a.srgb ? 256 : 0);
    const uint32_t n = cube_faces::level_extent(a.n, level);
    const uint32_t *lvl = a.texels + cube_faces::level_start(a.n, level, per_texel);
    float v[4];
    sky_bilinear<F32>(lvl + (size_t)face * cube_faces::face_words(n, per_texel), tab, n, s, t, v);
    if (LOD && frac > 0.0f) {  // level + 1 <= mips - 1 here
        const uint32_t n1 = cube_faces::level_extent(a.n, level + 1u);
        const uint32_t *lvl1 = lvl + cube_faces::level_words(n, per_texel);
        float hi[3];
        sky_bilinear<F32>(lvl1 + (size_t)face * cube_faces::face_words(n1, per_texel), tab, n1, s, t, hi);
        const float omf = 1.0f - frac;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] * omf + hi[k] * frac;
    }
    v[3] = 1.0f;  // 6.
    return pack_half4(v);
}
// a cube with levels drawn at a GIVEN level (r3n_skybox_set_level): steps 1-4, then step 5 with the level and fraction of the
// argument block instead of the footprint's
template <bool F32>
R3N_DEV ushort4 sky_fragment_fixed(const SkyboxArgs &a, uint32_t x, uint32_t y) {
    float d[3];
    sky_direction(a, x, y, d);
    float v[4];
    cube_sample_level<F32>(a.texels, a.decode + (a.srgb ? 256 : 0), a.n, a.mips, d, a.fixed_level, a.fixed_frac, v);
    v[3] = 1.0f;
    return pack_half4(v);
}
template <bool F32, bool LOD, bool FIXED>
R3N_DEV ushort4 sky_fragment_of(const SkyboxArgs &a, uint32_t x, uint32_t y) {
    if (FIXED) return sky_fragment_fixed<F32>(a, x, y);
    if (!F32 && !LOD) return sky_fragment(a, x, y);
    return sky_fragment_levels<F32, LOD>(a, x, y);
}

// The reference's depth test for the sky's fragment at depth 0.0: GreaterEqual against the stored depth (skybox.rs: depth
// compare of the pipeline).  A cleared sample (depth 0.0) always passes.  A sample that holds a TRIANGLE at depth exactly 0.0
// (or -0.0) passes too: the sky is drawn after the opaque passes and wins, as in the reference; tests/skybox_reference.py
// (takes_sky) states the same rule.
R3N_DEV bool sky_passes(unsigned long long key) { return 0.0f >= __uint_as_float((uint32_t)(key >> 32)); }

R3N_DEV void half4_to_float(ushort4 h, float o[4]) {
    o[0] = (float)__builtin_bit_cast(_Float16, h.x); o[1] = (float)__builtin_bit_cast(_Float16, h.y);
    o[2] = (float)__builtin_bit_cast(_Float16, h.z); o[3] = (float)__builtin_bit_cast(_Float16, h.w);
}

// F32: the cube's texels are four f32 words; LOD: the cube has more than one level.  <S, false, false> is the kernel of the
// one-level RGBA8 cubes.  FIXED (with LOD): the level is the argument block's, not the footprint's.
template <int S, bool F32, bool LOD, bool FIXED = false>
__global__ __launch_bounds__(256) void k_skybox(SkyboxArgs a) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t first = (size_t)a.row_begin * a.width, count = (size_t)(a.row_end - a.row_begin) * a.width;
    if (i >= count) return;
    const size_t pix = first + i;
    const uint32_t y = (uint32_t)pix / a.width, x = (uint32_t)pix - y * a.width;  // (a target holds fewer than 2^29 samples: r3n_frame_begin)
    if (S == 1) {
        if (!sky_passes(a.vis[pix])) return;
        const ushort4 h = sky_fragment_of<F32, LOD, FIXED>(a, x, y);
        a.hdr_out[pix] = h;
        a.ldr_out[pix] = tonemap_half4(a.srgb_lut, h, a.out_bgr != 0u);
        return;
    }
    // four samples: the full-screen triangle covers every sample, so the fragment is evaluated once, at the pixel centre, and
    // written to the samples that pass
    unsigned long long keys[4];
    {
        const ulonglong2 k01 = *reinterpret_cast<const ulonglong2 *>(a.vis + pix * 4u);
        const ulonglong2 k23 = *reinterpret_cast<const ulonglong2 *>(a.vis + pix * 4u + 2u);
        keys[0] = k01.x; keys[1] = k01.y; keys[2] = k23.x; keys[3] = k23.y;
    }
    uint32_t mask = 0;
#pragma unroll
    for (int sm = 0; sm < 4; ++sm) mask |= sky_passes(keys[sm]) ? 1u << sm : 0u;
    if (mask == 0u) return;
    const ushort4 h = sky_fragment_of<F32, LOD, FIXED>(a, x, y);
    const bool keep_samples = a.samples_form == R3N_SKY_SAMPLES_ALL;
    float col[4][4];
    half4_to_float(h, col[0]);
    if (mask == 0xFu) {
#pragma unroll
        for (int sm = 1; sm < 4; ++sm)
#pragma unroll
            for (int c = 0; c < 4; ++c) col[sm][c] = col[0][c];
    } else {
        // the other samples keep what the resolve gave them
        const uint32_t id0 = (uint32_t)keys[0];
        const bool uniform = (uint32_t)keys[1] == id0 && (uint32_t)keys[2] == id0 && (uint32_t)keys[3] == id0;
        float sky[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) sky[c] = col[0][c];
        if (!keep_samples && uniform) {  // split resolve, one triangle in the pixel: four equal samples, nothing parked
            float same[4];
            half4_to_float(a.hdr_out[pix], same);
#pragma unroll
            for (int sm = 0; sm < 4; ++sm)
#pragma unroll
                for (int c = 0; c < 4; ++c) col[sm][c] = ((mask >> sm) & 1u) ? sky[c] : same[c];
        } else {
#pragma unroll
            for (int sm = 0; sm < 4; ++sm) {
                if ((mask >> sm) & 1u) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) col[sm][c] = sky[c];
                } else {
                    half4_to_float(a.samples[pix * 4u + (size_t)sm], col[sm]);
                }
            }
        }
    }
    if (keep_samples) {
#pragma unroll
        for (int sm = 0; sm < 4; ++sm)
            if ((mask >> sm) & 1u) a.samples[pix * 4u + (size_t)sm] = h;
    }
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = ((col[0][c] + col[1][c]) + (col[2][c] + col[3][c])) * 0.25f;  // the box resolve, as everywhere
    const ushort4 ho = pack_half4(out);
    a.hdr_out[pix] = ho;
    a.ldr_out[pix] = tonemap_half4(a.srgb_lut, ho, a.out_bgr != 0u);
}

}  // namespace

template <int S>
static void launch_skybox(const SkyboxArgs &a, bool f32, bool lod, dim3 grid, hipStream_t stream) {
    if (lod && a.fixed != 0u) {  // a one-level cube ignores the fixed level
        if (f32) hipLaunchKernelGGL((k_skybox<S, true, true, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((k_skybox<S, false, true, true>), grid, dim3(256), 0, stream, a);
        return;
    }
    if (f32 && lod) hipLaunchKernelGGL((k_skybox<S, true, true>), grid, dim3(256), 0, stream, a);
    else if (f32) hipLaunchKernelGGL((k_skybox<S, true, false>), grid, dim3(256), 0, stream, a);
    else if (lod) hipLaunchKernelGGL((k_skybox<S, false, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((k_skybox<S, false, false>), grid, dim3(256), 0, stream, a);
}

extern "C" int r3n_internal_skybox(const SkyboxArgs *ap, uint32_t samples, uint32_t f32_class, hipStream_t stream) {
    const SkyboxArgs &a = *ap;
    const size_t count = (size_t)(a.row_end - a.row_begin) * a.width;
    const dim3 grid((unsigned)((count + 255u) / 256u));
    if (samples == 4) launch_skybox<4>(a, f32_class != 0u, a.mips > 1u, grid, stream);
    else launch_skybox<1>(a, f32_class != 0u, a.mips > 1u, grid, stream);
    return (int)hipGetLastError();
}
