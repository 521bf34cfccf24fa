// tangents.hip -- vertex tangents of every instance of one r3n_vertex_tangents call, generated from the instance's (morphed)
// positions and normals and the mesh's uv0 in ONE launch.  Contract and terms: tangents.h.
//
// The shape of normals.hip: one thread per vertex, wave slot w belongs to instance wave_instance[w] and covers vertices
// [64 * (w - wave_first[instance]), +64); the 32-byte record is wave-uniform and comes through scalar registers.  A thread walks its
// adjacency row -- triangle number -> three indices -> three positions and three uvs -> g_t -> add -- in the row's order, which is
// ascending triangle number: a deterministic gather that reproduces the serial loop's additions word for word.  Then it reads its
// own normal, projects and normalises, and writes 12 bytes.  No atomics, no LDS, no scratch buffer.  Every g_t is recomputed by
// each of its (up to three) vertices; the terms of one triangle are the same words wherever they are computed.
//
// The row is walked TANGENTS_BATCH entries at a time: the triangle numbers, then their indices, then their position and uv words are
// each requested together, and the terms are added in row order.  Rows longer than any unrolling take the same loop.
//
// Defence in depth: a row bound past the list, a triangle number >= T or an index >= vertex_count read from device memory is never
// used as an address (the entry is skipped); r3n_host_vertex_adjacency writes none.
//
// Gather-latency bound, like the normals kernel, with 60 instead of 36 gathered bytes behind every row entry: 1.3 times its time
// (profiles/tangents.md).
// -Rpass-analysis=kernel-resource-usage (gfx950): 60 VGPRs, 0 AGPRs, 31 SGPRs, 0 B scratch, 0 B LDS, occupancy 8 waves per SIMD.
#include <hip/hip_runtime.h>

#include "exact_math.h"
#include "tangents.h"

namespace {

#define TANGENTS_DEV __device__ __forceinline__
#define TANGENTS_BATCH 2

struct vec3 {
    float x, y, z;
};
struct vec2 {
    float x, y;
};

struct corners {
    vec3 p0, p1, p2;
    vec2 t0, t1, t2;
    bool ok;
};

TANGENTS_DEV vec3 load_vec3(const float *__restrict__ a, uint32_t i) { return {a[3u * i], a[3u * i + 1u], a[3u * i + 2u]}; }
TANGENTS_DEV vec2 load_vec2(const float *__restrict__ a, uint32_t i) { return {a[2u * i], a[2u * i + 1u]}; }

// (-ffp-contract=off: every product, difference and sum rounds on its own)
TANGENTS_DEV void add_term(vec3 &acc, const corners &c) {
    if (!c.ok) return;
    const vec3 e1{c.p1.x - c.p0.x, c.p1.y - c.p0.y, c.p1.z - c.p0.z}, e2{c.p2.x - c.p0.x, c.p2.y - c.p0.y, c.p2.z - c.p0.z};
    const vec2 a{c.t1.x - c.t0.x, c.t1.y - c.t0.y}, b{c.t2.x - c.t0.x, c.t2.y - c.t0.y};
    const float r = 1.0f / (a.x * b.y - a.y * b.x);  // any sign, zero, subnormal: the compiler's correctly rounded division
    // lib.rs:825: (edge1 * uv2.y) - (edge2 * uv1.y) * r
    acc.x = acc.x + (e1.x * b.y - (e2.x * a.y) * r);
    acc.y = acc.y + (e1.y * b.y - (e2.y * a.y) * r);
    acc.z = acc.z + (e1.z * b.y - (e2.z * a.y) * r);
}

// entries [k, k + N) of the row: N triangle numbers, then their indices, then their corners, each level requested together
template <int N>
TANGENTS_DEV void add_entries(vec3 &acc, const uint32_t *__restrict__ list, uint32_t k, const uint32_t *__restrict__ idx, uint32_t n_tris,
                              const float *__restrict__ pos, const float *__restrict__ uv, uint32_t vertex_count) {
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
        c[u].t0 = c[u].t1 = c[u].t2 = vec2{0.0f, 0.0f};
        if (c[u].ok) {
            c[u].p0 = load_vec3(pos, i0[u]);
            c[u].p1 = load_vec3(pos, i1[u]);
            c[u].p2 = load_vec3(pos, i2[u]);
            c[u].t0 = load_vec2(uv, i0[u]);
            c[u].t1 = load_vec2(uv, i1[u]);
            c[u].t2 = load_vec2(uv, i2[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) add_term(acc, c[u]);  // in row order: ascending triangle number
}

__global__ __launch_bounds__(256) void k_vertex_tangents(uint32_t *__restrict__ mesh, const r3n_tangents_input32 *__restrict__ recs,
                                                         const uint32_t *__restrict__ wave_instance, const uint32_t *__restrict__ wave_first,
                                                         uint32_t total_waves) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (w >= total_waves) return;
    const uint32_t inst = __builtin_amdgcn_readfirstlane(wave_instance[w]);
    const r3n_tangents_input32 rec = recs[inst];
    const uint32_t v = (w - __builtin_amdgcn_readfirstlane(wave_first[inst])) * R3N_TANGENTS_WAVE_VERTICES + lane;
    if (v >= rec.vertex_count) return;
    const float *pos = reinterpret_cast<const float *>(mesh + rec.position_offset / 4u);
    const float *nrm = reinterpret_cast<const float *>(mesh + rec.normal_offset / 4u);
    const float *uv = reinterpret_cast<const float *>(mesh + rec.uv_offset / 4u);
    const uint32_t *idx = mesh + rec.index_offset / 4u;
    const uint32_t *rows = mesh + rec.adjacency_offset / 4u;
    const uint32_t *list = rows + rec.vertex_count + 1u;
    const uint32_t n_tris = rec.index_count / 3u;
    const uint32_t end = min(rows[v + 1u], 3u * n_tris);
    uint32_t k = min(rows[v], end);
    const vec3 n = load_vec3(nrm, v);  // (requested in front of the walk; used behind it)
    vec3 acc{0.0f, 0.0f, 0.0f};        // +0, not the first term: -0 + -0 would differ
    for (; k + TANGENTS_BATCH <= end; k += TANGENTS_BATCH) add_entries<TANGENTS_BATCH>(acc, list, k, idx, n_tris, pos, uv, rec.vertex_count);
    for (; k < end; ++k) add_entries<1>(acc, list, k, idx, n_tris, pos, uv, rec.vertex_count);
    // lib.rs:834-835: t = tan - norm * norm.dot(tan), then glam normalize_or_zero
    const float d = (n.x * acc.x + n.y * acc.y) + n.z * acc.z;
    const vec3 q{acc.x - n.x * d, acc.y - n.y * d, acc.z - n.z * d};
    const float rcp = exact_math::rsqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
    vec3 out{0.0f, 0.0f, 0.0f};
    if (__builtin_isfinite(rcp) && rcp > 0.0f) out = vec3{q.x * rcp, q.y * rcp, q.z * rcp};
    float *dst = reinterpret_cast<float *>(mesh + rec.tangent_offset / 4u) + 3u * v;
    dst[0] = out.x;
    dst[1] = out.y;
    dst[2] = out.z;
}

}  // namespace

extern "C" int r3n_internal_vertex_tangents(const TangentsArgs *a, hipStream_t stream) {
    if (a->total_waves == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_vertex_tangents, dim3((a->total_waves + 3u) / 4u), dim3(256), 0, stream, a->mesh, a->recs, a->wave_instance,
                       a->wave_first, a->total_waves);
    return (int)hipGetLastError();
}
