// envlight.hip -- dominant-light extraction from one level of a cube (r3n_environment_lights): the passes of envlight_rule.h over
// the interior texels of the level's bordered faces.  Not in the reference (rend3-routine/src/skybox.rs only draws the cube);
// opt-in: no frame launches any of this.
//
// Every pass is a grid-stride loop of 256-thread blocks that sums in registers, then across the wave (shuffles), then across the
// block's four waves through LDS, and issues ONE 64-bit integer atomic per accumulator per block into the state block.  Integer
// sums and maxima do not depend on the order of arrival, so every grid size and both plans give the same words.  What a pass
// needs from the passes before it (the scale, the emitted lights' cones, the centre of its own cone) it derives from the raw
// sums in the state with the rule's own functions, once per block: nothing but atomics ever writes the state.
#include <hip/hip_runtime.h>

#include "envlight.h"

namespace {

using namespace envlight_rule;

constexpr uint32_t BLOCK = 256u, WAVES = BLOCK / 64u;

// ---- a texel of the level, decoded exactly as skybox.hip's sky_fetch decodes it, then sanitised
template <bool F32>
__device__ inline void fetch(const EnvlightArgs &a, uint32_t index, float rgb[3]) {
    uint32_t f, i, j;
    texel_of(index, a.n, f, i, j);
    const uint32_t pitch = a.n + 2u;
    const size_t at = (size_t)f * pitch * pitch + (size_t)(j + 1u) * pitch + (i + 1u);  // interior texel (i, j) of bordered face f
    if (F32) {
        const float4 v = reinterpret_cast<const float4 *>(a.level)[at];
        rgb[0] = v.x; rgb[1] = v.y; rgb[2] = v.z;
    } else {
        const uint32_t w = a.level[at];
        rgb[0] = a.decode[w & 0xFFu]; rgb[1] = a.decode[(w >> 8) & 0xFFu]; rgb[2] = a.decode[(w >> 16) & 0xFFu];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = sanitise(rgb[c]);
}

enum Source { SRC_RGBA8 = 0, SRC_F32 = 1, SRC_PLANE = 2 };
// the texel's quantities for a gather: from the plane (one 16-byte load, and the luminance where it is used), or decoded again
template <int SRC>
__device__ inline Texel texel_for(const EnvlightArgs &a, uint32_t index, float w, uint32_t emax_bits) {
    if (SRC == SRC_PLANE) {
        const uint4 v = a.plane_q[index];
        Texel t;
        t.q[0] = (uint64_t)v.x | (uint64_t)(v.w & 0xFFu) << 32;
        t.q[1] = (uint64_t)v.y | (uint64_t)((v.w >> 8) & 0xFFu) << 32;
        t.q[2] = (uint64_t)v.z | (uint64_t)((v.w >> 16) & 0xFFu) << 32;
        t.qy = energy(t.q[0], t.q[1], t.q[2]);
        t.qw = quantise_w(w);
        t.lum = a.plane_lum[index];
        return t;
    }
    float rgb[3];
    fetch<SRC == SRC_F32>(a, index, rgb);
    return texel(rgb, w, emax_bits);
}

// ---- reductions: registers -> wave -> block -> one atomic per accumulator.  `max_from`: accumulators [max_from, NV) are maxima.
template <int NV>
__device__ inline void reduce_and_commit(uint64_t (&v)[NV], int max_from, uint64_t *const (&dst)[NV]) {
    __shared__ uint64_t part[WAVES][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v[k], off);
            v[k] = k >= max_from ? (o > v[k] ? o : v[k]) : v[k] + o;
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < NV; ++k) part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)NV) {
        const int k = (int)threadIdx.x;
        uint64_t r = part[0][k];
        for (uint32_t wv = 1; wv < WAVES; ++wv) r = k >= max_from ? (part[wv][k] > r ? part[wv][k] : r) : r + part[wv][k];
        if (k >= max_from) {
            if (r != 0u) atomicMax(reinterpret_cast<unsigned long long *>(dst[k]), (unsigned long long)r);
        } else if (r != 0u) {
            atomicAdd(reinterpret_cast<unsigned long long *>(dst[k]), (unsigned long long)r);
        }
    }
}

// ---- what a light pass derives from the state, once per block
struct Cones {
    uint32_t active;           // the pass has work: every light before k was emitted and light k has a seed
    vec3 centre;               // of this pass's cone
    vec3 dead[MAX_LIGHTS];     // the directions of the lights before k
    uint32_t emitted[MAX_LIGHTS];
};
// the cone of the pass sits where `steps` mean-shift steps of light k left it: gather (b) number `steps`, or gather (c) at SHIFT_STEPS
__device__ inline void derive(const EnvlightArgs &a, uint32_t k, uint32_t steps, Cones &s) {
    const State &st = *a.state;
    if (threadIdx.x < k) {
        s.dead[threadIdx.x] = light_centre(st, threadIdx.x, a.n);
        s.emitted[threadIdx.x] = light_emitted(st, threadIdx.x, a.rule) ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        bool on = st.emax_bits != 0u && seed_valid(st.seed[k]);
        for (uint32_t l = 0; l < k; ++l) on = on && s.emitted[l] != 0u;
        s.active = on ? 1u : 0u;
        if (on) s.centre = centre_after(st, k, a.n, steps);
    }
    __syncthreads();
}
__device__ inline bool live(const Cones &s, uint32_t k, const vec3 &u, float cone_cos) {
    bool alive = true;
    for (uint32_t l = 0; l < k; ++l) alive = alive && !in_cone(u, s.dead[l], cone_cos);
    return alive;
}

// ---- pass 0: e_max.  A non-negative f32 compared as u32 is exact.
template <bool F32>
__global__ __launch_bounds__(BLOCK) void k_envlight_emax(EnvlightArgs a) {
    __shared__ uint32_t part[WAVES];
    const uint32_t count = 6u * a.n * a.n, stride = gridDim.x * BLOCK;
    uint32_t best = 0u;
    for (uint32_t t = blockIdx.x * BLOCK + threadIdx.x; t < count; t += stride) {
        float rgb[3];
        fetch<F32>(a, t, rgb);
        const uint32_t e = texel_emax(rgb, geometry_at(t, a.n).w);
        best = e > best ? e : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t wv = 1; wv < WAVES; ++wv) best = part[wv] > best ? part[wv] : best;
        if (best != 0u) atomicMax(&a.state->emax_bits, best);
    }
}

// ---- pass 1: quantise (into the plane under plan 1), the level's totals, the seed of light 0
template <bool F32, bool PLANE>
__global__ __launch_bounds__(BLOCK) void k_envlight_quantise(EnvlightArgs a) {
    const uint32_t emax_bits = a.state->emax_bits;
    if (emax_bits == 0u) return;  // a level without energy: no light, ambient 0
    const uint32_t count = 6u * a.n * a.n, stride = gridDim.x * BLOCK;
    uint64_t acc[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = blockIdx.x * BLOCK + threadIdx.x; t < count; t += stride) {
        float rgb[3];
        fetch<F32>(a, t, rgb);
        const Texel x = texel(rgb, geometry_at(t, a.n).w, emax_bits);
        if (PLANE) {
            a.plane_q[t] = make_uint4((uint32_t)x.q[0], (uint32_t)x.q[1], (uint32_t)x.q[2],
                                      (uint32_t)(x.q[0] >> 32) | (uint32_t)(x.q[1] >> 32) << 8 | (uint32_t)(x.q[2] >> 32) << 16);
            a.plane_lum[t] = x.lum;
        }
        acc[0] += x.q[0]; acc[1] += x.q[1]; acc[2] += x.q[2]; acc[3] += x.qy; acc[4] += x.qw; acc[5] += 1u;
        const uint64_t key = seed_key(x.lum, t);
        acc[6] = key > acc[6] ? key : acc[6];
    }
    Sums &tot = a.state->total;
    uint64_t *const dst[7] = {&tot.q[0], &tot.q[1], &tot.q[2], &tot.qy, &tot.qw, &tot.texels, &a.state->seed[0]};
    reduce_and_commit<7>(acc, 6, dst);
}

// ---- gather (b) number `step` of light k: the six sums of qY dq over the live texels of the cone
template <int SRC>
__global__ __launch_bounds__(BLOCK) void k_envlight_shift(EnvlightArgs a, uint32_t k, uint32_t step) {
    __shared__ Cones s;
    derive(a, k, step, s);
    if (!s.active) return;
    const uint32_t emax_bits = a.state->emax_bits;
    const uint32_t count = 6u * a.n * a.n, stride = gridDim.x * BLOCK;
    uint64_t acc[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = blockIdx.x * BLOCK + threadIdx.x; t < count; t += stride) {
        const Geometry g = geometry_at(t, a.n);
        if (!in_cone(g.u, s.centre, a.rule.cone_cos) || !live(s, k, g.u, a.rule.cone_cos)) continue;
        int64_t terms[6];
        shift_terms(texel_for<SRC>(a, t, g.w, emax_bits).qy, g.u, terms);
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += (uint64_t)terms[c];  // two's complement: the sum of the words is the word of the sum
    }
    int64_t *sh = a.state->shift[k][step];
    uint64_t *const dst[6] = {reinterpret_cast<uint64_t *>(sh), reinterpret_cast<uint64_t *>(sh + 1), reinterpret_cast<uint64_t *>(sh + 2),
                              reinterpret_cast<uint64_t *>(sh + 3), reinterpret_cast<uint64_t *>(sh + 4), reinterpret_cast<uint64_t *>(sh + 5)};
    reduce_and_commit<6>(acc, 6, dst);
}

// ---- gather (c) of light k, and the seed of light k + 1 among the live texels outside its cone (a texel knows in this pass whether
// it survives light k; were light k not emitted the loop stops and the seed is never read)
template <int SRC>
__global__ __launch_bounds__(BLOCK) void k_envlight_light(EnvlightArgs a, uint32_t k) {
    __shared__ Cones s;
    derive(a, k, SHIFT_STEPS, s);
    if (!s.active) return;
    const uint32_t emax_bits = a.state->emax_bits;
    const uint32_t count = 6u * a.n * a.n, stride = gridDim.x * BLOCK;
    uint64_t acc[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = blockIdx.x * BLOCK + threadIdx.x; t < count; t += stride) {
        const Geometry g = geometry_at(t, a.n);
        if (!live(s, k, g.u, a.rule.cone_cos)) continue;
        const Texel x = texel_for<SRC>(a, t, g.w, emax_bits);
        if (in_cone(g.u, s.centre, a.rule.cone_cos)) {
            acc[0] += x.q[0]; acc[1] += x.q[1]; acc[2] += x.q[2]; acc[3] += x.qy; acc[4] += x.qw; acc[5] += 1u;
        } else {
            const uint64_t key = seed_key(x.lum, t);
            acc[6] = key > acc[6] ? key : acc[6];
        }
    }
    Sums &l = a.state->light[k];
    uint64_t *const dst[7] = {&l.q[0], &l.q[1], &l.q[2], &l.qy, &l.qw, &l.texels, &a.state->seed[k + 1u]};
    reduce_and_commit<7>(acc, 6, dst);
}

template <int SRC>
void enqueue_lights(const EnvlightArgs &a, dim3 grid, hipStream_t stream, uint64_t &launches) {
    for (uint32_t k = 0; k < a.rule.max_lights; ++k) {
        for (uint32_t step = 0; step < SHIFT_STEPS; ++step) hipLaunchKernelGGL((k_envlight_shift<SRC>), grid, dim3(BLOCK), 0, stream, a, k, step);
        hipLaunchKernelGGL((k_envlight_light<SRC>), grid, dim3(BLOCK), 0, stream, a, k);
        launches += SHIFT_STEPS + 1u;
    }
}

}  // namespace

extern "C" int r3n_internal_envlight(const EnvlightArgs *ap, hipEvent_t *taps, hipStream_t stream, uint64_t *launches) {
    const EnvlightArgs &a = *ap;
    if (a.n == 0u || a.n > MAX_EXTENT || a.rule.max_lights > MAX_LIGHTS || a.blocks == 0u || a.blocks > R3N_ENVLIGHT_BLOCKS_MAX) return (int)hipErrorInvalidValue;
    const bool plane = a.plane_q != nullptr, f32 = a.f32_class != 0u;
    const dim3 grid(a.blocks);
    uint64_t count = 0;
    const auto tap = [&](int i) { return taps ? hipEventRecord(taps[i], stream) : hipSuccess; };
    hipError_t e = hipMemsetAsync(a.state, 0, sizeof(State), stream);
    if (e != hipSuccess) return (int)e;
    if ((e = tap(0)) != hipSuccess) return (int)e;
    if (f32) hipLaunchKernelGGL((k_envlight_emax<true>), grid, dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((k_envlight_emax<false>), grid, dim3(BLOCK), 0, stream, a);
    if ((e = tap(1)) != hipSuccess) return (int)e;
    if (f32 && plane) hipLaunchKernelGGL((k_envlight_quantise<true, true>), grid, dim3(BLOCK), 0, stream, a);
    else if (f32) hipLaunchKernelGGL((k_envlight_quantise<true, false>), grid, dim3(BLOCK), 0, stream, a);
    else if (plane) hipLaunchKernelGGL((k_envlight_quantise<false, true>), grid, dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((k_envlight_quantise<false, false>), grid, dim3(BLOCK), 0, stream, a);
    count += 2u;
    if ((e = tap(2)) != hipSuccess) return (int)e;
    if (plane) enqueue_lights<SRC_PLANE>(a, grid, stream, count);
    else if (f32) enqueue_lights<SRC_F32>(a, grid, stream, count);
    else enqueue_lights<SRC_RGBA8>(a, grid, stream, count);
    if ((e = tap(3)) != hipSuccess) return (int)e;
    if (launches) *launches = count;
    return (int)hipGetLastError();
}
