// exposure.hip -- what rend3-routine/src/tonemapping.rs:1-10 leaves open ("no tonemapping applied as we don't have auto-exposure
// yet"): a luminance histogram of the HDR target, the metering / adaptation step, and the blit with an exposure and an operator in
// front of its transfer.  Opt-in (r3n_tonemap_set); the default frame launches none of this.  Arithmetic contract: DESIGN.md
// section 2 "Exposure and tonemapping operators", restated in tests/tonemap_reference.py; the rule is exposure_rule.h.
#include <hip/hip_runtime.h>

#include "kernels_shade.h"
#include "exposure.h"
#include "bloom_rule.h"

namespace {

using exposure_rule::Params;
using exposure_rule::Step;

R3N_DEV float half_f32(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }

// Two pixels of the HDR target as k_tonemap reads them: one 16-byte load where the pair is whole and starts at an even pixel, the
// scalar form at an odd first pixel and at the tail.
R3N_DEV void load_pair(const ushort4 *__restrict__ hdr, size_t i0, bool two, ushort4 h[2]) {
    if (two && (i0 & 1u) == 0u) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(hdr + i0);
        h[0] = make_ushort4(raw.x & 0xFFFFu, raw.x >> 16, raw.y & 0xFFFFu, raw.y >> 16);
        h[1] = make_ushort4(raw.z & 0xFFFFu, raw.z >> 16, raw.w & 0xFFFFu, raw.w >> 16);
    } else {
        h[0] = hdr[i0];
        h[1] = two ? hdr[i0 + 1u] : make_ushort4(0, 0, 0, 0);
    }
}

// Per-wave private histograms in LDS (no-return ds_add), summed per workgroup at the end; one global atomic per non-zero bin.
// A wave whose active lanes all hold the same bin (sky, a cleared background) issues ONE add of the lane count instead of 64 adds
// to one LDS word, which the LDS serialises: 16 instead of 23 us on a 3840 x 2160 target of one bin, nothing on a lit frame
// (profiles/tonemap.md).
__global__ __launch_bounds__(256) void k_luminance_histogram(const ushort4 *__restrict__ hdr, size_t first_pixel, size_t n_pixels,
                                                             uint32_t *__restrict__ counters) {
    __shared__ uint32_t lh[4][R3N_EXP_BINS + 1];
    for (uint32_t i = threadIdx.x; i < 4u * (R3N_EXP_BINS + 1); i += 256u) (&lh[0][0])[i] = 0u;
    __syncthreads();
    uint32_t *mine = lh[threadIdx.x >> 6];
    const size_t pairs = (n_pixels + 1u) / 2u;
    for (size_t pair = (size_t)blockIdx.x * 256u + threadIdx.x; pair < pairs; pair += (size_t)gridDim.x * 256u) {
        const size_t i0 = first_pixel + pair * 2u;
        const bool two = pair * 2u + 1u < n_pixels;
        ushort4 h[2];
        load_pair(hdr, i0, two, h);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 1 && !two) continue;
            const int b = exposure_rule::bin_of(exposure_rule::luminance(half_f32(h[k].x), half_f32(h[k].y), half_f32(h[k].z)));
            const uint32_t idx = b < 0 ? (uint32_t)R3N_EXP_BINS : (uint32_t)b;
            const unsigned long long active = __ballot(1);
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            if (__ballot(idx == first) == active) {
                if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(active)) atomicAdd(&mine[first], (uint32_t)__popcll(active));
            } else {
                atomicAdd(&mine[idx], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t bin = threadIdx.x; bin < R3N_EXP_BINS + 1u; bin += 256u) {
        const uint32_t n = (lh[0][bin] + lh[1][bin]) + (lh[2][bin] + lh[3][bin]);
        if (n != 0u) atomicAdd(&counters[bin], n);
    }
}

// One wave: lane l owns bins 4l..4l+3.  Exclusive prefix over the 256 bins, the clipped sum S, then lane 0 takes the step.
__global__ __launch_bounds__(64) void k_exposure_update(ExposureBlock *__restrict__ blk, int prev_i, int cur_i, Params p, int prev_invalid) {
    __shared__ unsigned long long scan[64];
    __shared__ long long part[64];
    const uint32_t lane = threadIdx.x;
    uint32_t n[4];
    unsigned long long own = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        n[k] = blk->counters[lane * 4u + k];
        own += n[k];
    }
    scan[lane] = own;
    __syncthreads();
    for (uint32_t d = 1; d < 64u; d <<= 1) {  // inclusive scan of the lanes' totals
        const unsigned long long add = lane >= d ? scan[lane - d] : 0ull;
        __syncthreads();
        scan[lane] += add;
        __syncthreads();
    }
    const unsigned long long total = scan[63];
    unsigned long long c = scan[lane] - own;  // exclusive prefix of bin 4l
    uint64_t lo, hi;
    exposure_rule::rank_window(total, p, lo, hi);
    long long s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s += (long long)exposure_rule::bin_share(c, c + n[k], lo, hi) * (long long)blk->lq[lane * 4u + k];
        c += n[k];
    }
    part[lane] = s;
    __syncthreads();
    for (uint32_t d = 32; d > 0u; d >>= 1) {
        if (lane < d) part[lane] += part[lane + d];
        __syncthreads();
    }
    r3n_exposure_state *cur = &blk->state[cur_i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cur->histogram[lane * 4u + k] = n[k];  // the snapshot r3n_readback_exposure returns
        blk->counters[lane * 4u + k] = 0u;     // ready for the next frame's histogram
    }
    if (lane == 0u) {
        const r3n_exposure_state *pv = &blk->state[prev_i];
        Step prev;
        prev.valid = prev_invalid ? 0u : pv->valid;
        prev.mean_log2 = pv->mean_log2; prev.target_ev = pv->target_ev; prev.current_ev = pv->current_ev; prev.scale = pv->scale;
        const Step st = exposure_rule::step(prev, (int64_t)part[0], hi - lo, p, blk->e);
        cur->excluded = blk->counters[R3N_EXP_BINS];
        blk->counters[R3N_EXP_BINS] = 0u;
        cur->valid = st.valid; cur->mean_log2 = st.mean_log2; cur->target_ev = st.target_ev; cur->current_ev = st.current_ev;
        cur->scale = st.scale;
        cur->_pad[0] = 0u; cur->_pad[1] = 0u;
    }
}

// k_tonemap's shape (two pixels per thread) with exposure and operator in front of the transfer.  The exposed, operated value is
// rounded to half and then takes exactly the blit's path: tonemap_half4 for the bytes, the float view's formulas for the tap.
// BLOOM (r3n_bloom_set, DESIGN.md section 2 "Bloom"): the 2x tent up-sample of the pyramid's level 0 is added to the exposed value
// in front of the operator.  Four taps per pixel; a thread whose two pixels lie side by side in one row (the first at an even x)
// shares the two taps of their common nearer column.
R3N_DEV float bloom_chan(ushort4 t, int c) { return half_f32(c == 0 ? t.x : (c == 1 ? t.y : t.z)); }

template <uint32_t OP, bool BLOOM = false>
__global__ __launch_bounds__(256) void k_tonemap_op(const ushort4 *__restrict__ hdr, uchar4 *__restrict__ out, float4 *__restrict__ out_f32,
                                                    size_t first_pixel, size_t n_pixels, const unsigned char *__restrict__ srgb_lut,
                                                    uint32_t output_format, const float *__restrict__ scale_ptr, float scale_arg, float white_sq,
                                                    R3nBloomComposite bloom) {
    const bool bgr = (output_format & 1u) != 0u, manual = (output_format & 2u) != 0u;
    const size_t pair = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t i0 = first_pixel + pair * 2u;
    if (pair * 2u >= n_pixels) return;
    const bool two = pair * 2u + 1u < n_pixels;
    const float scale = scale_ptr != nullptr ? *scale_ptr : scale_arg;  // uniform
    ushort4 h[2];
    load_pair(hdr, i0, two, h);
    float glow[2][3] = {};
    if (BLOOM) {
        const ushort4 *__restrict__ a0 = bloom.a0;
        const int bw = (int)bloom.bw, bh = (int)bloom.bh;
        const uint32_t y0 = (uint32_t)i0 / bloom.width, x0 = (uint32_t)i0 - y0 * bloom.width;
        if (two && (x0 & 1u) == 0u && x0 + 1u < bloom.width) {
            const int X = (int)(x0 >> 1), yn = bloom_rule::up_near((int)y0), yf = bloom_rule::up_far((int)y0, bh);
            const int xl = bloom_rule::clampi(X - 1, 0, bw - 1), xr = bloom_rule::clampi(X + 1, 0, bw - 1);
            const ushort4 mn = a0[(size_t)yn * bw + X], mf = a0[(size_t)yf * bw + X];
            const ushort4 ln = a0[(size_t)yn * bw + xl], lf = a0[(size_t)yf * bw + xl], rn = a0[(size_t)yn * bw + xr], rf = a0[(size_t)yf * bw + xr];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float n = bloom_chan(mn, j), f = bloom_chan(mf, j);
                glow[0][j] = bloom_rule::up_col(bloom_rule::up_row(n, bloom_chan(ln, j)), bloom_rule::up_row(f, bloom_chan(lf, j)));
                glow[1][j] = bloom_rule::up_col(bloom_rule::up_row(n, bloom_chan(rn, j)), bloom_rule::up_row(f, bloom_chan(rf, j)));
            }
        } else {
            const auto texel = [&](int sx, int sy, float rgb[3]) {
                const ushort4 t = a0[(size_t)sy * bw + sx];
                rgb[0] = half_f32(t.x); rgb[1] = half_f32(t.y); rgb[2] = half_f32(t.z);
            };
            bloom_rule::up_at(texel, bw, bh, (int)x0, (int)y0, glow[0]);
            if (two) {
                const uint32_t y1 = ((uint32_t)i0 + 1u) / bloom.width, x1 = (uint32_t)i0 + 1u - y1 * bloom.width;
                bloom_rule::up_at(texel, bw, bh, (int)x1, (int)y1, glow[1]);
            }
        }
    }
    uchar4 o8[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned short in[3] = {h[k].x, h[k].y, h[k].z};
        unsigned short ch[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float v = exposure_rule::exposed(half_f32(in[j]), scale);
            if (BLOOM) v = bloom_rule::composite(v, glow[k][j], bloom.intensity);
            const float y = OP == R3N_TONEMAP_OP_REINHARD ? exposure_rule::op_reinhard(v, white_sq)
                          : OP == R3N_TONEMAP_OP_ACES   ? exposure_rule::op_aces(v) : v;
            ch[j] = __builtin_bit_cast(unsigned short, (_Float16)y);
        }
        const ushort4 t = make_ushort4(ch[0], ch[1], ch[2], h[k].w);
        o8[k] = tonemap_half4(srgb_lut, t, bgr);
        if (out_f32 != nullptr && (k == 0 || two)) {  // float view of the same target (readback tap only)
            const float r = half_f32(t.x), g = half_f32(t.y), b = half_f32(t.z), al = half_f32(t.w);
            out_f32[i0 + (size_t)k] = make_float4(manual ? srgb_scene_to_display(r) : srgb_oetf(r), manual ? srgb_scene_to_display(g) : srgb_oetf(g),
                                                  manual ? srgb_scene_to_display(b) : srgb_oetf(b),
                                                  (!(al > 0.0f)) ? 0.0f : (al >= 1.0f ? 1.0f : al));
        }
    }
    out[i0] = o8[0];
    if (two) out[i0 + 1u] = o8[1];
}

int launch_status() { return (int)hipGetLastError(); }

}  // namespace

extern "C" {

int r3n_internal_luminance_histogram(const ushort4 *hdr, size_t first_pixel, size_t n_pixels, uint32_t *counters, hipStream_t stream) {
    if (n_pixels == 0) return (int)hipSuccess;
    const size_t pairs = (n_pixels + 1) / 2, blocks = (pairs + 255) / 256;
    const dim3 grid((unsigned)(blocks < R3N_EXP_HIST_GRID ? blocks : R3N_EXP_HIST_GRID));
    hipLaunchKernelGGL(k_luminance_histogram, grid, dim3(256), 0, stream, hdr, first_pixel, n_pixels, counters);
    return launch_status();
}

int r3n_internal_exposure_update(ExposureBlock *block, int prev, int cur, const Params *p, int prev_invalid, hipStream_t stream) {
    hipLaunchKernelGGL(k_exposure_update, dim3(1), dim3(64), 0, stream, block, prev, cur, *p, prev_invalid);
    return launch_status();
}

int r3n_internal_tonemap_op(const ushort4 *hdr, uchar4 *out, float4 *out_f32, size_t first_pixel, size_t n_pixels, const unsigned char *srgb_lut,
                            uint32_t output_format, uint32_t op, const float *scale_ptr, float scale, float white_sq, const R3nBloomComposite *bloom,
                            hipStream_t stream) {
    const size_t pairs = (n_pixels + 1) / 2;
    const dim3 grid((unsigned)((pairs + 255) / 256));
    const R3nBloomComposite b = bloom ? *bloom : R3nBloomComposite{};
#define R3N_LAUNCH_OP(OP, BLOOM)                                                                                                       \
    hipLaunchKernelGGL((k_tonemap_op<OP, BLOOM>), grid, dim3(256), 0, stream, hdr, out, out_f32, first_pixel, n_pixels, srgb_lut, output_format, \
                       scale_ptr, scale, white_sq, b)
    if (bloom) {
        if (op == R3N_TONEMAP_OP_REINHARD) R3N_LAUNCH_OP(R3N_TONEMAP_OP_REINHARD, true);
        else if (op == R3N_TONEMAP_OP_ACES) R3N_LAUNCH_OP(R3N_TONEMAP_OP_ACES, true);
        else R3N_LAUNCH_OP(R3N_TONEMAP_OP_BLIT, true);
    } else {
        if (op == R3N_TONEMAP_OP_REINHARD) R3N_LAUNCH_OP(R3N_TONEMAP_OP_REINHARD, false);
        else if (op == R3N_TONEMAP_OP_ACES) R3N_LAUNCH_OP(R3N_TONEMAP_OP_ACES, false);
        else R3N_LAUNCH_OP(R3N_TONEMAP_OP_BLIT, false);
    }
#undef R3N_LAUNCH_OP
    return launch_status();
}

}  // extern "C"
