// bloom.hip -- the bloom chain in front of the tonemapping node's operator: a pyramid of the bright-passed HDR target, built down
// with a 4x4 tent and back up with a 2x tent and a scatter factor.  Not in the reference (rend3-routine/src/tonemapping.rs:1-10 is
// where it hangs); opt-in (r3n_bloom_set), the default frame launches none of this.  Arithmetic contract: DESIGN.md section 2
// "Bloom", restated in tests/bloom_reference.py; the rule is bloom_rule.h.  The composite is k_tonemap_op's (exposure.hip).
#include <hip/hip_runtime.h>

#include "bloom.h"

namespace {

using bloom_rule::Params;

#define BLOOM_DEV __device__ __forceinline__

constexpr uint32_t TX = R3N_BLOOM_TILE_X, TY = R3N_BLOOM_TILE_Y;
constexpr uint32_t SW = 2u * TX + 2u, SH = 2u * TY + 2u;  // the source tile with its halo
constexpr uint32_t PAIRS = SW / 2u + 1u;                  // aligned source pairs that cover a row of it

BLOOM_DEV ushort4 bright_texel(ushort4 h, float scale, const Params &p) {
    const uint16_t in[3] = {h.x, h.y, h.z};
    uint16_t out[3];
    bloom_rule::bright(in, scale, p, out);
    return make_ushort4(out[0], out[1], out[2], 0);
}
BLOOM_DEV float chan(ushort4 t, int c) { return bloom_rule::half_to_f32(c == 0 ? t.x : (c == 1 ? t.y : t.z)); }
BLOOM_DEV void chans(ushort4 t, float rgb[3]) {
    rgb[0] = bloom_rule::half_to_f32(t.x); rgb[1] = bloom_rule::half_to_f32(t.y); rgb[2] = bloom_rule::half_to_f32(t.z);
}

// One workgroup owns a TX x TY destination tile.  It stages the (2 TX + 2) x (2 TY + 2) source texels it needs -- clamped at the
// source's edges, bright-passed and rounded to half where the source is the HDR target -- in LDS, computes the row sums of the
// separable tent once per (source row, destination column), then combines four of them per destination texel.  Every global read
// goes through a clamped coordinate, so a tile that hangs over the level's edge (or a level smaller than a tile) reads in bounds.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_bloom_down(const ushort4 *__restrict__ src, uint32_t sw, uint32_t sh, ushort4 *__restrict__ dst,
                                                    uint32_t dw, uint32_t dh, Params p, const float *__restrict__ scale_ptr, float scale_arg) {
    __shared__ ushort4 tile[SH][SW];
    __shared__ float rows[3][SH][TX];
    const float scale = scale_ptr != nullptr ? *scale_ptr : scale_arg;  // uniform
    const int x0 = (int)(blockIdx.x * TX), y0 = (int)(blockIdx.y * TY);
    for (uint32_t idx = threadIdx.x; idx < SH * PAIRS; idx += 256u) {
        const uint32_t row = idx / PAIRS, i = idx - row * PAIRS;
        const int sy = bloom_rule::clampi(2 * y0 - 1 + (int)row, 0, (int)sh - 1);
        const int c0 = 2 * x0 - 2 + 2 * (int)i;  // even
        ushort4 t[2];
        if (c0 >= 0 && c0 + 1 < (int)sw) {
            const size_t at = (size_t)sy * sw + (size_t)c0;
            if ((at & 1u) == 0u) {  // one 16-byte load
                const uint4 raw = *reinterpret_cast<const uint4 *>(src + at);
                t[0] = make_ushort4(raw.x & 0xFFFFu, raw.x >> 16, raw.y & 0xFFFFu, raw.y >> 16);
                t[1] = make_ushort4(raw.z & 0xFFFFu, raw.z >> 16, raw.w & 0xFFFFu, raw.w >> 16);
            } else {
                t[0] = src[at];
                t[1] = src[at + 1u];
            }
        } else {
            t[0] = src[(size_t)sy * sw + (size_t)bloom_rule::clampi(c0, 0, (int)sw - 1)];
            t[1] = src[(size_t)sy * sw + (size_t)bloom_rule::clampi(c0 + 1, 0, (int)sw - 1)];
        }
        if (FIRST) {
            t[0] = bright_texel(t[0], scale, p);
            t[1] = bright_texel(t[1], scale, p);
        }
        if (i > 0u) tile[row][2u * i - 1u] = t[0];
        if (2u * i < SW) tile[row][2u * i] = t[1];
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < SH * TX; idx += 256u) {
        const uint32_t row = idx / TX, x = idx - row * TX;
        const ushort4 s0 = tile[row][2u * x], s1 = tile[row][2u * x + 1u], s2 = tile[row][2u * x + 2u], s3 = tile[row][2u * x + 3u];
#pragma unroll
        for (int c = 0; c < 3; ++c) rows[c][row][x] = bloom_rule::down_row(chan(s0, c), chan(s1, c), chan(s2, c), chan(s3, c));
    }
    __syncthreads();
    const uint32_t x = threadIdx.x % TX;
#pragma unroll
    for (uint32_t y = threadIdx.x / TX; y < TY; y += 256u / TX) {
        const uint32_t gx = (uint32_t)x0 + x, gy = (uint32_t)y0 + y;
        if (gx >= dw || gy >= dh) continue;
        uint16_t o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[c] = bloom_rule::half_rne(bloom_rule::down_col(rows[c][2u * y][x], rows[c][2u * y + 1u][x], rows[c][2u * y + 2u][x], rows[c][2u * y + 3u][x]));
        dst[(size_t)gy * dw + gx] = make_ushort4(o[0], o[1], o[2], 0);
    }
}

// One thread per texel (X, Y) of the coarser level: the 2x2 texels of the finer level above it take their taps from the same 3x3
// neighbourhood, so the six row terms (3 near + left, 3 near + right, per coarse row) are computed once.  In place over d: a
// thread reads and writes its own four texels and reads the coarser level only.
__global__ __launch_bounds__(256) void k_bloom_up(const ushort4 *__restrict__ coarse, uint32_t cw, uint32_t ch, const ushort4 *d, ushort4 *a,
                                                  uint32_t w, uint32_t h, float scatter) {
    const uint32_t X = blockIdx.x * 32u + (threadIdx.x & 31u), Y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (X >= cw || Y >= ch) return;
    const int xs[3] = {bloom_rule::clampi((int)X - 1, 0, (int)cw - 1), (int)X, bloom_rule::clampi((int)X + 1, 0, (int)cw - 1)};
    const int ys[3] = {bloom_rule::clampi((int)Y - 1, 0, (int)ch - 1), (int)Y, bloom_rule::clampi((int)Y + 1, 0, (int)ch - 1)};
    float hl[3][3], hr[3][3];  // [coarse row][channel]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const ushort4 l = coarse[(size_t)ys[r] * cw + xs[0]], m = coarse[(size_t)ys[r] * cw + xs[1]], q = coarse[(size_t)ys[r] * cw + xs[2]];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hl[r][c] = bloom_rule::up_row(chan(m, c), chan(l, c));
            hr[r][c] = bloom_rule::up_row(chan(m, c), chan(q, c));
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t x = 2u * X + i, y = 2u * Y + j;
            if (x >= w || y >= h) continue;
            const int far = j == 0 ? 0 : 2;  // an even row's farther coarse row lies above
            const size_t at = (size_t)y * w + x;
            const ushort4 dt = d[at];
            uint16_t o[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float u = i == 0 ? bloom_rule::up_col(hl[1][c], hl[far][c]) : bloom_rule::up_col(hr[1][c], hr[far][c]);
                o[c] = bloom_rule::up_store(chan(dt, c), u, scatter);
            }
            a[at] = make_ushort4(o[0], o[1], o[2], 0);
        }
    }
}

// The small levels in ONE workgroup: every level from plan.tail on goes down through LDS and back up without leaving the CU.
// The first of them is taken from the level above it in global memory (or, where the tail starts at level 0, from the bright
// pass of the HDR target); each finished a_k (and d_k, where the down chain is kept) is written out for the up kernels, the
// composite and r3n_readback_bloom.  The serial forms of the rule (bloom_rule::down_at / up_at): no row sums are shared here.
template <bool FIRST>
__global__ __launch_bounds__(1024) void k_bloom_tail(const ushort4 *__restrict__ src, uint32_t sw, uint32_t sh, ushort4 *d, ushort4 *a, BloomPlan plan,
                                                     Params p, const float *__restrict__ scale_ptr, float scale_arg) {
    extern __shared__ ushort4 lds[];
    const float scale = scale_ptr != nullptr ? *scale_ptr : scale_arg;  // uniform
    const uint32_t T = plan.tail, L = plan.lv.n;
    uint32_t base = 0, prev_base = 0;
    for (uint32_t k = T; k < L; ++k) {
        const uint32_t w = plan.lv.w[k], h = plan.lv.h[k];
        for (uint32_t i = threadIdx.x; i < w * h; i += 1024u) {
            const int y = (int)(i / w), x = (int)(i - (uint32_t)y * w);
            uint16_t o[3];
            if (k == T) {
                bloom_rule::down_at([&](int sx, int sy, float rgb[3]) {
                    const ushort4 t = src[(size_t)sy * sw + (size_t)sx];
                    chans(FIRST ? bright_texel(t, scale, p) : t, rgb);
                }, (int)sw, (int)sh, x, y, o);
            } else {
                const uint32_t pw = plan.lv.w[k - 1u];
                bloom_rule::down_at([&](int sx, int sy, float rgb[3]) { chans(lds[prev_base + (uint32_t)sy * pw + (uint32_t)sx], rgb); },
                                    (int)pw, (int)plan.lv.h[k - 1u], x, y, o);
            }
            const ushort4 t = make_ushort4(o[0], o[1], o[2], 0);
            lds[base + i] = t;
            if (d != a || k + 1u == L) d[plan.off[k] + i] = t;
            if (d != a && k + 1u == L) a[plan.off[k] + i] = t;  // a_{L-1} = d_{L-1}
        }
        __syncthreads();
        prev_base = base;
        base += w * h;
    }
    base = prev_base;  // of level L - 1
    for (uint32_t k = L - 1u; k-- > T;) {
        const uint32_t w = plan.lv.w[k], h = plan.lv.h[k], cw = plan.lv.w[k + 1u], chh = plan.lv.h[k + 1u];
        const uint32_t coarse = base;
        base -= w * h;
        for (uint32_t i = threadIdx.x; i < w * h; i += 1024u) {
            const int y = (int)(i / w), x = (int)(i - (uint32_t)y * w);
            float u[3];
            bloom_rule::up_at([&](int sx, int sy, float rgb[3]) { chans(lds[coarse + (uint32_t)sy * cw + (uint32_t)sx], rgb); }, (int)cw, (int)chh, x, y, u);
            const ushort4 dt = lds[base + i];
            const ushort4 t = make_ushort4(bloom_rule::up_store(chan(dt, 0), u[0], p.scatter), bloom_rule::up_store(chan(dt, 1), u[1], p.scatter),
                                           bloom_rule::up_store(chan(dt, 2), u[2], p.scatter), 0);
            lds[base + i] = t;
            a[plan.off[k] + i] = t;
        }
        __syncthreads();
    }
}

int launch_status() { return (int)hipGetLastError(); }

}  // namespace

extern "C" {

int r3n_internal_bloom_down(const ushort4 *hdr, uint32_t W, uint32_t H, ushort4 *d, const BloomPlan *plan, uint32_t k, const Params *p,
                            const float *scale_ptr, float scale, hipStream_t stream) {
    const uint32_t dw = plan->lv.w[k], dh = plan->lv.h[k];
    const dim3 grid((dw + TX - 1u) / TX, (dh + TY - 1u) / TY);
    if (k == 0u)
        hipLaunchKernelGGL(k_bloom_down<true>, grid, dim3(256), 0, stream, hdr, W, H, d + plan->off[0], dw, dh, *p, scale_ptr, scale);
    else
        hipLaunchKernelGGL(k_bloom_down<false>, grid, dim3(256), 0, stream, d + plan->off[k - 1u], plan->lv.w[k - 1u], plan->lv.h[k - 1u],
                           d + plan->off[k], dw, dh, *p, nullptr, 1.0f);
    return launch_status();
}

int r3n_internal_bloom_up(const ushort4 *d, ushort4 *a, const BloomPlan *plan, uint32_t k, const Params *p, hipStream_t stream) {
    const uint32_t cw = plan->lv.w[k + 1u], ch = plan->lv.h[k + 1u];
    const dim3 grid((cw + 31u) / 32u, (ch + 7u) / 8u);
    hipLaunchKernelGGL(k_bloom_up, grid, dim3(256), 0, stream, a + plan->off[k + 1u], cw, ch, d + plan->off[k], a + plan->off[k], plan->lv.w[k],
                       plan->lv.h[k], p->scatter);
    return launch_status();
}

int r3n_internal_bloom_tail(const ushort4 *hdr, uint32_t W, uint32_t H, ushort4 *d, ushort4 *a, const BloomPlan *plan, const Params *p,
                            const float *scale_ptr, float scale, hipStream_t stream) {
    uint32_t texels = 0;
    for (uint32_t k = plan->tail; k < plan->lv.n; ++k) texels += plan->lv.w[k] * plan->lv.h[k];
    const uint32_t lds = texels * 8u;
    if (plan->tail >= plan->lv.n || lds > R3N_BLOOM_TAIL_LDS) return (int)hipErrorInvalidValue;
    // more than 64 KiB of dynamic LDS needs the attribute (per device, so it is set with every launch that needs it)
    if (lds > 65536u) {
        const void *fn = plan->tail == 0u ? reinterpret_cast<const void *>(&k_bloom_tail<true>) : reinterpret_cast<const void *>(&k_bloom_tail<false>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R3N_BLOOM_TAIL_LDS);
        if (e != hipSuccess) return (int)e;
    }
    if (plan->tail == 0u)
        hipLaunchKernelGGL(k_bloom_tail<true>, dim3(1), dim3(1024), lds, stream, hdr, W, H, d, a, *plan, *p, scale_ptr, scale);
    else
        hipLaunchKernelGGL(k_bloom_tail<false>, dim3(1), dim3(1024), lds, stream, d + plan->off[plan->tail - 1u], plan->lv.w[plan->tail - 1u],
                           plan->lv.h[plan->tail - 1u], d, a, *plan, *p, nullptr, 1.0f);
    return launch_status();
}

}  // extern "C"
