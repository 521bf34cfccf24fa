// vertex_gather.h -- device side of the vertex stages that rewrite runs of the mesh buffer in front of skinning (morph.hip,
// normals.hip, tangents.hip): the argument block, the wave-slot prologue, and the adjacency row walk of the two stages that sum a
// per-triangle term into every vertex.  Host side (the block these pointers point into): vertex_block.h.
//
// Wave map: wave slot w belongs to instance wave_instance[w] (the map k_skinning uses) and is the (w - wave_first[instance])-th of
// that instance.  The record is wave-uniform and comes through scalar registers.
//
// Row walk: a thread walks its vertex's adjacency row (r3n_host_vertex_adjacency: rows[0 .. V], then the triangle numbers; row v =
// entries [rows[v], rows[v + 1]), the triangles naming v, ascending, one entry per occurrence) -- triangle number -> three indices
// -> the term's corners -> term -> add -- in the row's order, starting from +0: a deterministic gather that reproduces the serial
// loop's additions word for word.  No atomics, no LDS, no scratch buffer.  The row is walked BATCH entries at a time: the triangle
// numbers, then their indices, then their corners are each requested together, and the terms are added in row order.  Rows longer
// than any unrolling take the same loop; its trip count differs per lane.
//
// Defence in depth: a row bound past the list, a triangle number >= T or an index >= vertex_count read from device memory is never
// used as an address (the entry is skipped); r3n_host_vertex_adjacency writes none.  Nothing is touched past a run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_math.h"

namespace vertex_gather {

#define VERTEX_DEV __device__ __forceinline__

template <class Rec>
struct Args {
    uint32_t *mesh;
    const Rec *recs;                // one per instance, a power-of-two count of words: one scalar load
    const uint32_t *wave_instance;  // total_waves: the instance of every wave slot
    const uint32_t *wave_first;     // per instance: its first wave slot
    uint32_t total_waves;
};

// Prologue of a kernel launched as (total_waves + 3) / 4 blocks of 256 threads:
//     const uint32_t w = wave_index();  if (w >= total_waves) return;  const Rec rec = wave_record(w, ..., first);  if (first >= count) return;
// The calling wave's slot.  (The exit stays in the kernel: the compiler does not thread a helper's return value through the
// readfirstlanes and keeps a second branch on it.)
VERTEX_DEV uint32_t wave_index() { return __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)); }
// The record of wave slot w's instance, and `first` = the first of this lane's per_wave / 64 elements of that instance, at
// `per_wave` elements per wave slot.
template <class Rec>
VERTEX_DEV Rec wave_record(uint32_t w, const Rec *__restrict__ recs, const uint32_t *__restrict__ wave_instance,
                           const uint32_t *__restrict__ wave_first, uint32_t per_wave, uint32_t &first) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t inst = __builtin_amdgcn_readfirstlane(wave_instance[w]);
    const Rec rec = recs[inst];
    first = (w - __builtin_amdgcn_readfirstlane(wave_first[inst])) * per_wave + lane * (per_wave / 64u);
    return rec;
}

struct vec3 {
    float x, y, z;
};
struct vec2 {
    float x, y;
};
VERTEX_DEV vec3 load_vec3(const float *__restrict__ a, uint32_t i) { return {a[3u * i], a[3u * i + 1u], a[3u * i + 2u]}; }
VERTEX_DEV vec2 load_vec2(const float *__restrict__ a, uint32_t i) { return {a[2u * i], a[2u * i + 1u]}; }

// A Term says what one triangle contributes:
//     struct corners;                                         what it reads of a triangle, every member initialised to +0
//     corners load(uint32_t i0, uint32_t i1, uint32_t i2);    for three indices < vertex_count
//     void add(vec3 &acc, const corners &c);                  acc = fl(acc + term)
// (The zeros are member initialisers on purpose: a value-initialised plain struct is one byte-wise fill, which the compiler does
// not fold into the guarded loads; k_vertex_tangents then takes 638 instead of 562 instructions.)

// entries [k, k + N) of the row: N triangle numbers, then their indices, then their corners, each level requested together
template <int N, class Term>
VERTEX_DEV void add_entries(vec3 &acc, const Term &term, const uint32_t *__restrict__ list, uint32_t k, const uint32_t *__restrict__ idx,
                            uint32_t n_tris, uint32_t vertex_count) {
    uint32_t t[N], i0[N], i1[N], i2[N];
    bool ok[N];
    typename Term::corners c[N];
#pragma unroll
    for (int u = 0; u < N; ++u) t[u] = list[k + u];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        ok[u] = t[u] < n_tris;
        i0[u] = i1[u] = i2[u] = 0xFFFFFFFFu;
        if (ok[u]) {
            i0[u] = idx[3u * t[u]];
            i1[u] = idx[3u * t[u] + 1u];
            i2[u] = idx[3u * t[u] + 2u];
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        ok[u] = ok[u] && i0[u] < vertex_count && i1[u] < vertex_count && i2[u] < vertex_count;
        c[u] = typename Term::corners{};
        if (ok[u]) c[u] = term.load(i0[u], i1[u], i2[u]);
    }
#pragma unroll
    for (int u = 0; u < N; ++u)
        if (ok[u]) term.add(acc, c[u]);  // in row order: ascending triangle number
}

// the sum of vertex v's row: `index_count` index words at `index_offset`, the adjacency words at `adjacency_offset`
template <int BATCH, class Term>
VERTEX_DEV vec3 gather_row(const Term &term, const uint32_t *__restrict__ mesh, uint32_t index_offset, uint32_t index_count,
                           uint32_t adjacency_offset, uint32_t vertex_count, uint32_t v) {
    const uint32_t *idx = mesh + index_offset / 4u;
    const uint32_t *rows = mesh + adjacency_offset / 4u;
    const uint32_t *list = rows + vertex_count + 1u;
    const uint32_t n_tris = index_count / 3u;
    const uint32_t end = min(rows[v + 1u], 3u * n_tris);
    uint32_t k = min(rows[v], end);
    vec3 acc{0.0f, 0.0f, 0.0f};  // +0, not the first term: -0 + -0 would differ
    for (; k + BATCH <= end; k += BATCH) add_entries<BATCH>(acc, term, list, k, idx, n_tris, vertex_count);
    for (; k < end; ++k) add_entries<1>(acc, term, list, k, idx, n_tris, vertex_count);
    return acc;
}

// glam normalize_or_zero of q into vertex v of the f32x3 run at `offset`: 12 bytes
VERTEX_DEV void store_normalized(uint32_t *__restrict__ mesh, uint32_t offset, uint32_t v, const vec3 &q) {
    const float rcp = exact_math::rsqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
    vec3 out{0.0f, 0.0f, 0.0f};
    if (__builtin_isfinite(rcp) && rcp > 0.0f) out = vec3{q.x * rcp, q.y * rcp, q.z * rcp};
    float *dst = reinterpret_cast<float *>(mesh + offset / 4u) + 3u * v;
    dst[0] = out.x;
    dst[1] = out.y;
    dst[2] = out.z;
}

}  // namespace vertex_gather
