// tangents.hip -- vertex tangents of every instance of one r3n_vertex_tangents call, generated from the instance's (morphed)
// positions and normals and the mesh's uv0 in ONE launch.  Contract and terms: tangents.h.
//
// One thread per vertex: wave map, adjacency row walk, its defences and the normalising store are vertex_gather.h's.  Specific here:
// the uv term g_t (three positions and three uvs per triangle), and behind the walk the thread's own normal, the projection and the
// normalisation.  Every g_t is recomputed by each of its (up to three) vertices; the terms of one triangle are the same words
// wherever they are computed.
//
// Gather-latency bound, like the normals kernel, with 60 instead of 36 gathered bytes behind every row entry: 1.3 times its time
// (profiles/tangents.md).
// -Rpass-analysis=kernel-resource-usage (gfx950): 60 VGPRs, 0 AGPRs, 31 SGPRs, 0 B scratch, 0 B LDS, occupancy 8 waves per SIMD.
#include <hip/hip_runtime.h>

#include "tangents.h"

namespace {

using namespace vertex_gather;

#define TANGENTS_BATCH 2

struct uv_term {
    const float *__restrict__ pos, *__restrict__ uv;
    struct corners {
        vec3 p0{0.0f, 0.0f, 0.0f}, p1{0.0f, 0.0f, 0.0f}, p2{0.0f, 0.0f, 0.0f};
        vec2 t0{0.0f, 0.0f}, t1{0.0f, 0.0f}, t2{0.0f, 0.0f};
    };
    VERTEX_DEV corners load(uint32_t i0, uint32_t i1, uint32_t i2) const {
        return {load_vec3(pos, i0), load_vec3(pos, i1), load_vec3(pos, i2), load_vec2(uv, i0), load_vec2(uv, i1), load_vec2(uv, i2)};
    }
    // (-ffp-contract=off: every product, difference and sum rounds on its own)
    VERTEX_DEV void add(vec3 &acc, const corners &c) const {
        const vec3 e1{c.p1.x - c.p0.x, c.p1.y - c.p0.y, c.p1.z - c.p0.z}, e2{c.p2.x - c.p0.x, c.p2.y - c.p0.y, c.p2.z - c.p0.z};
        const vec2 a{c.t1.x - c.t0.x, c.t1.y - c.t0.y}, b{c.t2.x - c.t0.x, c.t2.y - c.t0.y};
        const float r = 1.0f / (a.x * b.y - a.y * b.x);  // any sign, zero, subnormal: the compiler's correctly rounded division
        // lib.rs:825: (edge1 * uv2.y) - (edge2 * uv1.y) * r
        acc.x = acc.x + (e1.x * b.y - (e2.x * a.y) * r);
        acc.y = acc.y + (e1.y * b.y - (e2.y * a.y) * r);
        acc.z = acc.z + (e1.z * b.y - (e2.z * a.y) * r);
    }
};

__global__ __launch_bounds__(256) void k_vertex_tangents(uint32_t *__restrict__ mesh, const r3n_tangents_input32 *__restrict__ recs,
                                                         const uint32_t *__restrict__ wave_instance, const uint32_t *__restrict__ wave_first,
                                                         uint32_t total_waves) {
    const uint32_t w = wave_index();
    if (w >= total_waves) return;
    uint32_t v;
    const r3n_tangents_input32 rec = wave_record(w, recs, wave_instance, wave_first, R3N_TANGENTS_WAVE_VERTICES, v);
    if (v >= rec.vertex_count) return;
    const uv_term term{reinterpret_cast<const float *>(mesh + rec.position_offset / 4u), reinterpret_cast<const float *>(mesh + rec.uv_offset / 4u)};
    const vec3 n = load_vec3(reinterpret_cast<const float *>(mesh + rec.normal_offset / 4u), v);  // (requested in front of the walk; used behind it)
    const vec3 acc = gather_row<TANGENTS_BATCH>(term, mesh, rec.index_offset, rec.index_count, rec.adjacency_offset, rec.vertex_count, v);
    // lib.rs:834-835: t = tan - norm * norm.dot(tan), then glam normalize_or_zero
    const float d = (n.x * acc.x + n.y * acc.y) + n.z * acc.z;
    store_normalized(mesh, rec.tangent_offset, v, vec3{acc.x - n.x * d, acc.y - n.y * d, acc.z - n.z * d});
}

}  // namespace

extern "C" int r3n_internal_vertex_tangents(const TangentsArgs *a, hipStream_t stream) {
    if (a->total_waves == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_vertex_tangents, dim3((a->total_waves + 3u) / 4u), dim3(256), 0, stream, a->mesh, a->recs, a->wave_instance,
                       a->wave_first, a->total_waves);
    return (int)hipGetLastError();
}
