// ibl.hip -- the environment prefilter (r3n_environment_prefilter): the passes of ibl_rule.h over the stored levels of a cube, and
// the probe of the lookups a later resolve will call (r3n_environment_probe, ibl_lookup.h).  Not in the reference
// (rend3-routine/src/skybox.rs only draws the cube); opt-in: no frame launches any of this.
//
// The pair kernel is an N-body loop: a thread owns ONE output texel of one level and walks that level's source records in linear
// order, so the summation tree of ibl_rule.h is three accumulators per sum in its registers and no launch plan can change a word.
// The workgroup stages the records in an LDS tile; every lane reads the same record, which is a broadcast.  With ibl_tile = 0 the
// records come through wave-uniform loads instead (profiles/ibl.md has both).
#include <hip/hip_runtime.h>

#include "cube_sample.h"
#include "ibl.h"
#include "ibl_lookup.h"

namespace {

using namespace ibl_rule;
using envlight_rule::geometry_at;
using envlight_rule::sanitise;

// ---- a texel of a source level, decoded exactly as skybox.hip's sky_fetch decodes it (NOT sanitised)
template <bool F32>
__device__ inline void fetch(const IblArgs &a, const IblLevel &lv, uint32_t index, float rgb[3]) {
    uint32_t f, i, j;
    envlight_rule::texel_of(index, lv.n, f, i, j);
    const uint32_t pitch = lv.n + 2u;
    const size_t at = (size_t)f * pitch * pitch + (size_t)(j + 1u) * pitch + (i + 1u);  // interior texel (i, j) of bordered face f
    const uint32_t *level = a.pool + lv.src_word;
    if (F32) {
        const float4 v = reinterpret_cast<const float4 *>(level)[at];
        rgb[0] = v.x; rgb[1] = v.y; rgb[2] = v.z;
    } else {
        const uint32_t w = level[at];
        rgb[0] = a.decode[w & 0xFFu]; rgb[1] = a.decode[(w >> 8) & 0xFFu]; rgb[2] = a.decode[(w >> 16) & 0xFFu];
    }
}

// ---- (a) the records of every source level the call reads: one thread per record
template <bool F32>
__global__ __launch_bounds__(256) void k_ibl_records(IblArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.rec_total) return;
    uint32_t k = a.rec_from;
    while (k + 1u < a.L && t >= a.lv[k + 1u].rec_base) ++k;
    const IblLevel &lv = a.lv[k];
    const uint32_t index = t - lv.rec_base;
    float rgb[3];
    fetch<F32>(a, lv, index, rgb);
    const envlight_rule::Geometry g = geometry_at(index, lv.n);
    float4 *dst = reinterpret_cast<float4 *>(a.records + t);
    dst[0] = make_float4(g.u.x, g.u.y, g.u.z, g.w);
    dst[1] = make_float4(sanitise(rgb[0]), sanitise(rgb[1]), sanitise(rgb[2]), 0.0f);
}

// ---- (d) result level 0: the source's level 0, decoded, alpha 1, not sanitised
template <bool F32>
__global__ __launch_bounds__(256) void k_ibl_mirror(IblArgs a) {
    const IblLevel &lv = a.lv[0];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 6u * lv.n * lv.n) return;
    float rgb[3];
    fetch<F32>(a, lv, t, rgb);
    reinterpret_cast<float4 *>(a.dense + lv.dense_word)[t] = make_float4(rgb[0], rgb[1], rgb[2], 1.0f);
}

// ---- (b) the pair kernel
__device__ inline void pair_term(const vec3 &N, const Roughness &r, const float4 &ru, const float4 &rc, Tree<4> &t) {
    const float wt = weight(N, vec3{ru.x, ru.y, ru.z}, ru.w, r);
    t.row[0] = t.row[0] + wt * rc.x;
    t.row[1] = t.row[1] + wt * rc.y;
    t.row[2] = t.row[2] + wt * rc.z;
    t.row[3] = t.row[3] + wt;
}
// BLOCK outputs of ONE level per workgroup; LDS: the records come through a tile of a.tile records, else straight from memory at a
// wave-uniform address
template <uint32_t BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void k_ibl_pairs(IblArgs a) {
    __shared__ float4 tile[LDS ? 2u * R3N_IBL_TILE_MAX : 1u];
    uint32_t k = 1u;
    while (k + 1u < a.L && blockIdx.x >= a.lv[k + 1u].first_block) ++k;  // (wave-uniform)
    const IblLevel &lv = a.lv[k];
    const uint32_t n = lv.n, count = 6u * n * n;
    const uint32_t o = (blockIdx.x - lv.first_block) * BLOCK + threadIdx.x;
    const bool owns = o < count;
    const vec3 N = geometry_at(owns ? o : count - 1u, n).u;
    const Roughness r{lv.a2, lv.oma};
    const float4 *recs = reinterpret_cast<const float4 *>(a.records + lv.rec_base);
    Tree<4> t;
    tree_clear(t);
    uint32_t col = 0, row = 0;  // of the next source texel: wave-uniform
    const auto advance = [&]() {
        if (++col == n) {
            col = 0;
            tree_end_row(t);
            if (++row == n) {
                row = 0;
                tree_end_face(t);
            }
        }
    };
    if (LDS) {
        for (uint32_t base = 0; base < count; base += a.tile) {
            const uint32_t cnt = count - base < a.tile ? count - base : a.tile;  // <= R3N_IBL_TILE_MAX: the launcher checks the plan
            __syncthreads();                                                    // the tile of the round before has been read
            for (uint32_t x = threadIdx.x; x < 2u * cnt; x += BLOCK) tile[x] = recs[2u * (size_t)base + x];
            __syncthreads();
            for (uint32_t s = 0; s < cnt; ++s) {
                pair_term(N, r, tile[2u * s], tile[2u * s + 1u], t);
                advance();
            }
        }
    } else {
        for (uint32_t s = 0; s < count; ++s) {
            pair_term(N, r, recs[2u * (size_t)s], recs[2u * (size_t)s + 1u], t);
            advance();
        }
    }
    if (!owns) return;
    reinterpret_cast<float4 *>(a.dense + lv.dense_word)[o] = make_float4(t.total[0] / t.total[3], t.total[1] / t.total[3], t.total[2] / t.total[3], 1.0f);
}

// ---- (c) SH: one workgroup per face row; thread 3 m + ch sums its row in ascending i
__global__ __launch_bounds__(64) void k_ibl_sh_rows(IblArgs a) {
    if (threadIdx.x >= 27u) return;
    const IblLevel &lv = a.lv[a.sh_k];
    const uint32_t m = threadIdx.x / 3u, ch = threadIdx.x - 3u * m;
    const IblRecord *row = a.records + lv.rec_base + (size_t)blockIdx.x * lv.n;
    float sum = 0.0f;
    for (uint32_t i = 0; i < lv.n; ++i) {
        const IblRecord rec = row[i];
        float Y[9];
        basis(vec3{rec.ux, rec.uy, rec.uz}, Y);
        const float wy = rec.w * Y[m];
        const float c = ch == 0u ? rec.r : (ch == 1u ? rec.g : rec.b);
        sum = sum + c * wy;
    }
    a.sh_rows[(size_t)blockIdx.x * 27u + threadIdx.x] = sum;
}
// the rows of a face in ascending j, the faces in face order: the tree's order, not the order of arrival
__global__ __launch_bounds__(64) void k_ibl_sh_combine(IblArgs a) {
    if (threadIdx.x >= 27u) return;
    const uint32_t n = a.lv[a.sh_k].n;
    float total = 0.0f;
    for (uint32_t f = 0; f < 6u; ++f) {
        float face = 0.0f;
        for (uint32_t j = 0; j < n; ++j) face = face + a.sh_rows[(size_t)(f * n + j) * 27u + threadIdx.x];
        total = total + face;
    }
    a.sh_out[threadIdx.x] = total;
}

template <uint32_t BLOCK>
void launch_pairs(const IblArgs &a, hipStream_t stream) {
    if (a.tile) hipLaunchKernelGGL((k_ibl_pairs<BLOCK, true>), dim3(a.pair_blocks), dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((k_ibl_pairs<BLOCK, false>), dim3(a.pair_blocks), dim3(BLOCK), 0, stream, a);
}

// ---- the probe: one thread per query
template <bool F32>
__global__ __launch_bounds__(64) void k_ibl_probe(IblCube cube, IblSh sh, const r3n_env_query32 *queries, uint32_t n, r3n_env_sample32 *out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const r3n_env_query32 q = queries[i];
    r3n_env_sample32 s;
    ibl_specular<F32>(cube, q.dir, q.roughness, s.specular, s.level, s.fraction);
    ibl_irradiance(sh, q.n, s.irradiance);
    out[i] = s;
}

}  // namespace

extern "C" int r3n_internal_ibl(const IblArgs *ap, hipEvent_t *taps, hipStream_t stream, uint64_t *launches) {
    const IblArgs &a = *ap;
    if (a.L < 2u || a.L > MAX_LEVELS || a.lv[0].n > MAX_EXTENT || a.lv[0].n < 2u || a.tile > R3N_IBL_TILE_MAX || !ibl_block_valid(a.block) || a.rec_from > 1u ||
        a.sh_k >= a.L || a.sh_k < a.rec_from || !a.pair_blocks || !a.rec_total)
        return (int)hipErrorInvalidValue;
    const bool f32 = a.f32_class != 0u;
    const auto tap = [&](int i) { return taps ? hipEventRecord(taps[i], stream) : hipSuccess; };
    hipError_t e;
    if ((e = tap(0)) != hipSuccess) return (int)e;
    const dim3 rec_grid((a.rec_total + 255u) / 256u), mirror_grid((6u * a.lv[0].n * a.lv[0].n + 255u) / 256u);
    if (f32) {
        hipLaunchKernelGGL((k_ibl_records<true>), rec_grid, dim3(256), 0, stream, a);
        hipLaunchKernelGGL((k_ibl_mirror<true>), mirror_grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((k_ibl_records<false>), rec_grid, dim3(256), 0, stream, a);
        hipLaunchKernelGGL((k_ibl_mirror<false>), mirror_grid, dim3(256), 0, stream, a);
    }
    if ((e = tap(1)) != hipSuccess) return (int)e;
    if (a.block == 64u) launch_pairs<64u>(a, stream);
    else if (a.block == 128u) launch_pairs<128u>(a, stream);
    else launch_pairs<256u>(a, stream);
    if ((e = tap(2)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ibl_sh_rows, dim3(6u * a.lv[a.sh_k].n), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(k_ibl_sh_combine, dim3(1), dim3(64), 0, stream, a);
    if ((e = tap(3)) != hipSuccess) return (int)e;
    if (launches) *launches = 5u;
    return (int)hipGetLastError();
}

extern "C" int r3n_internal_ibl_probe(const IblCube *cube, const IblSh *sh, uint32_t f32_class, const r3n_env_query32 *queries, uint32_t n,
                                      r3n_env_sample32 *out, hipStream_t stream) {
    const dim3 grid((n + 63u) / 64u);
    if (f32_class) hipLaunchKernelGGL((k_ibl_probe<true>), grid, dim3(64), 0, stream, *cube, *sh, queries, n, out);
    else hipLaunchKernelGGL((k_ibl_probe<false>), grid, dim3(64), 0, stream, *cube, *sh, queries, n, out);
    return (int)hipGetLastError();
}
