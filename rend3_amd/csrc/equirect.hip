// equirect.hip -- cubes from equirectangular panoramas on the device (r3n_texture_cubes_write_sources).  The rule: equirect_rule.h;
// the records: equirect.h.
//
// k_equirect_faces: ONE launch resamples every panorama of the call into its six dense level-0 faces.  Wave slot -> (cube, face)
// through the wave map of the vertex stages (vertex_block.h / vertex_gather.h), as k_cube_assemble: the record is wave-uniform and
// comes through scalar registers; a wave takes 64 consecutive texels of a face row-major, so neighbouring lanes read neighbouring
// source texels.  Four source fetches per texel (RGBE words decoded inline, or texels the decode jobs left in the scratch block),
// one 16-byte store.
// k_equirect_level: one launch builds one level of every face that has it from the level above (16-byte loads and stores).
// k_equirect_tail: one workgroup per (cube, face) builds every remaining level: the first from the scratch block, the others from
// LDS (at most 32^2 + 16^2 + ... + 1 texels, 21.3 KiB).  The chain's faces are independent: nothing crosses a workgroup.
// All launched as (total_waves + 3) / 4 blocks of 256, the tail as one block of 256 per record.
#include <hip/hip_runtime.h>

#include "equirect.h"
#include "vertex_gather.h"

namespace {

using equirect::ChainRec;
using equirect::FaceRec;
using equirect_rule::vec4;

struct FacesArgs {
    const FaceRec *recs;
    const uint32_t *wave_rec, *wave_first;
    uint32_t total_waves;
    const uint8_t *staged;  // the call's payload
    uint32_t *dense;        // the call's scratch block
    const float *srgb_decode;
};
struct ChainArgs {
    const ChainRec *recs;
    const uint32_t *wave_rec, *wave_first;
    uint32_t total_waves;  // level launch: wave slots; tail launch: records
    uint32_t *dense;
};

__device__ __forceinline__ vec4 load4(const vec4 *p) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    return vec4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void store4(vec4 *p, const vec4 &v) { *reinterpret_cast<float4 *>(p) = make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ vec4 rgba8_texel(uint32_t w, const float *__restrict__ table) {
    const float a = (float)(w >> 24) / 255.0f;
    if (table) return vec4{table[w & 255u], table[(w >> 8) & 255u], table[(w >> 16) & 255u], a};
    return vec4{(float)(w & 255u) / 255.0f, (float)((w >> 8) & 255u) / 255.0f, (float)((w >> 16) & 255u) / 255.0f, a};
}

__global__ __launch_bounds__(256) void k_equirect_faces(FacesArgs a) {
    const uint32_t wv = vertex_gather::wave_index();
    if (wv >= a.total_waves) return;
    uint32_t unit;
    const FaceRec r = vertex_gather::wave_record(wv, a.recs, a.wave_rec, a.wave_first, equirect::UNITS_PER_WAVE, unit);
    if (unit >= r.units) return;
    const uint32_t j = unit / r.n, i = unit - j * r.n;
    const equirect_rule::Taps t = equirect_rule::face_taps(r.face, i, j, r.n, r.W, r.H);
    const size_t W = r.W;
    const size_t at[4] = {t.r0 * W + t.c0, t.r0 * W + t.c1, t.r1 * W + t.c0, t.r1 * W + t.c1};
    vec4 q[4];
    if (r.mode == equirect::SOURCE_RGBE8) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.staged + (((uint64_t)r.src_hi << 32) | r.src_lo));
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = src[at[k]];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = equirect_rule::rgbe_decode(w[k]);
    } else if (r.mode == equirect::SOURCE_F32) {
        const vec4 *src = reinterpret_cast<const vec4 *>(a.dense + r.src_lo);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = load4(src + at[k]);
    } else {
        const uint32_t *src = a.dense + r.src_lo;
        const float *table = r.mode == equirect::SOURCE_RGBA8_SRGB ? a.srgb_decode : nullptr;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = src[at[k]];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = rgba8_texel(w[k], table);
    }
    store4(reinterpret_cast<vec4 *>(a.dense + r.dst) + unit, equirect_rule::bilinear(q[0], q[1], q[2], q[3], t.fx, t.fy));
}

__global__ __launch_bounds__(256) void k_equirect_level(ChainArgs a) {
    const uint32_t wv = vertex_gather::wave_index();
    if (wv >= a.total_waves) return;
    uint32_t unit;
    const ChainRec r = vertex_gather::wave_record(wv, a.recs, a.wave_rec, a.wave_first, equirect::UNITS_PER_WAVE, unit);
    if (unit >= r.units) return;
    const uint32_t y = unit / r.d, x = unit - y * r.d;
    const vec4 *src = reinterpret_cast<const vec4 *>(a.dense + r.src);
    store4(reinterpret_cast<vec4 *>(a.dense + r.dst) + unit,
           equirect_rule::chain_texel([&](uint32_t k) { return load4(src + k); }, x, y, r.s, r.d));
}

__global__ __launch_bounds__(256) void k_equirect_tail(ChainArgs a) {
    __shared__ vec4 lds[equirect::TAIL_LDS_TEXELS];
    if (blockIdx.x >= a.total_waves) return;
    const ChainRec r = a.recs[blockIdx.x];  // (block-uniform)
    if (r.s > equirect_rule::TAIL_CAP) return;  // the levels behind it would not fit the LDS block; the host plans none
    uint32_t s = r.s, level_at = r.src, lds_src = 0u, lds_dst = 0u;
    for (uint32_t l = 0; l < r.levels; ++l) {
        const uint32_t d = equirect_rule::half_extent(s);
        const vec4 *src = reinterpret_cast<const vec4 *>(a.dense + level_at) + (size_t)r.face * s * s;
        level_at += 6u * s * s * 4u;
        vec4 *dst = reinterpret_cast<vec4 *>(a.dense + level_at) + (size_t)r.face * d * d;
        for (uint32_t unit = threadIdx.x; unit < d * d; unit += 256u) {
            const uint32_t y = unit / d, x = unit - y * d;
            const vec4 v = l == 0u ? equirect_rule::chain_texel([&](uint32_t k) { return load4(src + k); }, x, y, s, d)
                                   : equirect_rule::chain_texel([&](uint32_t k) { return lds[lds_src + k]; }, x, y, s, d);
            lds[lds_dst + unit] = v;
            store4(dst + unit, v);
        }
        __syncthreads();
        lds_src = lds_dst;
        lds_dst += d * d;
        s = d;
    }
}

}  // namespace

// `block` = the device copy of a table (records | wave_first | wave_instance at the layout's word offsets)
extern "C" int r3n_internal_equirect_faces(const uint32_t *block, uint64_t o_first, uint64_t o_inst, uint32_t total_waves, const void *staged,
                                           uint32_t *dense, const float *srgb_decode, hipStream_t stream) {
    if (!total_waves) return (int)hipSuccess;
    FacesArgs a;
    a.recs = reinterpret_cast<const FaceRec *>(block);
    a.wave_first = block + o_first;
    a.wave_rec = block + o_inst;
    a.total_waves = total_waves;
    a.staged = static_cast<const uint8_t *>(staged);
    a.dense = dense;
    a.srgb_decode = srgb_decode;
    hipLaunchKernelGGL(k_equirect_faces, dim3((total_waves + 3u) / 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
extern "C" int r3n_internal_equirect_level(const uint32_t *block, uint64_t o_first, uint64_t o_inst, uint32_t total_waves, uint32_t *dense,
                                           hipStream_t stream) {
    if (!total_waves) return (int)hipSuccess;
    ChainArgs a;
    a.recs = reinterpret_cast<const ChainRec *>(block);
    a.wave_first = block + o_first;
    a.wave_rec = block + o_inst;
    a.total_waves = total_waves;
    a.dense = dense;
    hipLaunchKernelGGL(k_equirect_level, dim3((total_waves + 3u) / 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
// `recs` = n_recs chain records on the device, one workgroup each
extern "C" int r3n_internal_equirect_tail(const uint32_t *recs, uint32_t n_recs, uint32_t *dense, hipStream_t stream) {
    if (!n_recs) return (int)hipSuccess;
    ChainArgs a;
    a.recs = reinterpret_cast<const ChainRec *>(recs);
    a.wave_first = a.wave_rec = nullptr;
    a.total_waves = n_recs;
    a.dense = dense;
    hipLaunchKernelGGL(k_equirect_tail, dim3(n_recs), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
