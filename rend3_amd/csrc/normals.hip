// normals.hip -- vertex normals of every instance of one r3n_vertex_normals call, recomputed from the instance's (morphed) positions
// in ONE launch.  Contract, adjacency layout and terms: normals.h.
//
// One thread per vertex: wave slot w belongs to instance wave_instance[w] (the map k_morph and k_skinning use) and covers vertices
// [64 * (w - wave_first[instance]), +64).  The 32-byte record is wave-uniform and comes through scalar registers.  A thread walks
// its adjacency row -- triangle number -> three indices -> three positions -> face term -> add -- in the row's order, which is
// ascending triangle number: a deterministic gather that reproduces the serial loop's additions word for word.  No atomics, no LDS,
// no scratch buffer.  Every face term is recomputed by each of its (up to three) vertices; the terms of one triangle are the same
// words wherever they are computed (origin p[i0], one rounding per operation).
//
// The row is walked four entries at a time: the four triangle numbers, then their twelve indices, then their thirty-six position
// words are each requested together, and the four terms are added in row order.  The dependent chain of a row of valence 6 is two
// rounds of three loads instead of six.  Rows longer than any unrolling take the same loop; its trip count differs per lane.
//
// Defence in depth: a row bound past the list, a triangle number >= T or an index >= vertex_count read from device memory is never
// used as an address (the entry is skipped); r3n_host_vertex_adjacency writes none.
//
// Gather-latency bound; the positions, indices and adjacency of a mesh that many instances share come from the caches
// (profiles/normals.md).
// -Rpass-analysis=kernel-resource-usage (gfx950): 66 VGPRs, 0 AGPRs, 37 SGPRs, 0 B scratch, 0 B LDS, occupancy 7 waves per SIMD
// (the thirty-six position words of a batch are what passes 64 VGPRs).
#include <hip/hip_runtime.h>

#include "exact_math.h"
#include "normals.h"

namespace {

#define NORMALS_DEV __device__ __forceinline__
#define NORMALS_BATCH 4

struct vec3 {
    float x, y, z;
};

NORMALS_DEV vec3 sub(const vec3 &a, const vec3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// (-ffp-contract=off: every product and every difference rounds on its own)
NORMALS_DEV vec3 cross(const vec3 &a, const vec3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

struct corners {
    vec3 p0, p1, p2;
    bool ok;
};

NORMALS_DEV vec3 load_vec3(const float *__restrict__ pos, uint32_t i) { return {pos[3u * i], pos[3u * i + 1u], pos[3u * i + 2u]}; }

NORMALS_DEV void add_face(vec3 &acc, const corners &c, bool left_handed) {
    if (!c.ok) return;
    const vec3 e1 = sub(c.p1, c.p0), e2 = sub(c.p2, c.p0);
    const vec3 n = left_handed ? cross(e1, e2) : cross(e2, e1);
    acc.x = acc.x + n.x;
    acc.y = acc.y + n.y;
    acc.z = acc.z + n.z;
}

// entries [k, k + N) of the row: N triangle numbers, then their indices, then their corners, each level requested together
template <int N>
NORMALS_DEV void add_entries(vec3 &acc, const uint32_t *__restrict__ list, uint32_t k, const uint32_t *__restrict__ idx, uint32_t n_tris,
                             const float *__restrict__ pos, uint32_t vertex_count, bool left_handed) {
    uint32_t t[N], i0[N], i1[N], i2[N];
    corners c[N];
#pragma unroll
    for (int u = 0; u < N; ++u) t[u] = list[k + u];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        c[u].ok = t[u] < n_tris;
        i0[u] = i1[u] = i2[u] = 0xFFFFFFFFu;
        if (c[u].ok) {
            i0[u] = idx[3u * t[u]];
            i1[u] = idx[3u * t[u] + 1u];
            i2[u] = idx[3u * t[u] + 2u];
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        c[u].ok = c[u].ok && i0[u] < vertex_count && i1[u] < vertex_count && i2[u] < vertex_count;
        c[u].p0 = c[u].p1 = c[u].p2 = vec3{0.0f, 0.0f, 0.0f};
        if (c[u].ok) {
            c[u].p0 = load_vec3(pos, i0[u]);
            c[u].p1 = load_vec3(pos, i1[u]);
            c[u].p2 = load_vec3(pos, i2[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) add_face(acc, c[u], left_handed);  // in row order: ascending triangle number
}

__global__ __launch_bounds__(256) void k_vertex_normals(uint32_t *__restrict__ mesh, const r3n_normals_input32 *__restrict__ recs,
                                                        const uint32_t *__restrict__ wave_instance, const uint32_t *__restrict__ wave_first,
                                                        uint32_t total_waves) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (w >= total_waves) return;
    const uint32_t inst = __builtin_amdgcn_readfirstlane(wave_instance[w]);
    const r3n_normals_input32 rec = recs[inst];
    const uint32_t v = (w - __builtin_amdgcn_readfirstlane(wave_first[inst])) * R3N_NORMALS_WAVE_VERTICES + lane;
    if (v >= rec.vertex_count) return;
    const float *pos = reinterpret_cast<const float *>(mesh + rec.position_offset / 4u);
    const uint32_t *idx = mesh + rec.index_offset / 4u;
    const uint32_t *rows = mesh + rec.adjacency_offset / 4u;
    const uint32_t *list = rows + rec.vertex_count + 1u;
    const uint32_t n_tris = rec.index_count / 3u;
    const bool left_handed = rec.left_handed != 0u;
    const uint32_t end = min(rows[v + 1u], 3u * n_tris);
    uint32_t k = min(rows[v], end);
    vec3 acc{0.0f, 0.0f, 0.0f};  // +0, not the first term: -0 + -0 would differ
    for (; k + NORMALS_BATCH <= end; k += NORMALS_BATCH) add_entries<NORMALS_BATCH>(acc, list, k, idx, n_tris, pos, rec.vertex_count, left_handed);
    for (; k < end; ++k) add_entries<1>(acc, list, k, idx, n_tris, pos, rec.vertex_count, left_handed);
    // glam normalize_or_zero
    const float rcp = exact_math::rsqrt((acc.x * acc.x + acc.y * acc.y) + acc.z * acc.z);
    vec3 out{0.0f, 0.0f, 0.0f};
    if (__builtin_isfinite(rcp) && rcp > 0.0f) out = vec3{acc.x * rcp, acc.y * rcp, acc.z * rcp};
    float *dst = reinterpret_cast<float *>(mesh + rec.normal_offset / 4u) + 3u * v;
    dst[0] = out.x;
    dst[1] = out.y;
    dst[2] = out.z;
}

}  // namespace

extern "C" int r3n_internal_vertex_normals(const NormalsArgs *a, hipStream_t stream) {
    if (a->total_waves == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_vertex_normals, dim3((a->total_waves + 3u) / 4u), dim3(256), 0, stream, a->mesh, a->recs, a->wave_instance,
                       a->wave_first, a->total_waves);
    return (int)hipGetLastError();
}
