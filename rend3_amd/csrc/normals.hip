// normals.hip -- vertex normals of every instance of one r3n_vertex_normals call, recomputed from the instance's (morphed) positions
// in ONE launch.  Contract, adjacency layout and terms: normals.h.
//
// One thread per vertex: wave map, adjacency row walk, its defences and the normalising store are vertex_gather.h's.  Specific here:
// the face term.  Every face term is recomputed by each of its (up to three) vertices; the terms of one triangle are the same
// words wherever they are computed (origin p[i0], one rounding per operation).
//
// The row is walked four entries at a time: the dependent chain of a row of valence 6 is two rounds of three loads instead of six.
//
// Gather-latency bound; the positions, indices and adjacency of a mesh that many instances share come from the caches
// (profiles/normals.md).
// -Rpass-analysis=kernel-resource-usage (gfx950): 66 VGPRs, 0 AGPRs, 37 SGPRs, 0 B scratch, 0 B LDS, occupancy 7 waves per SIMD
// (the thirty-six position words of a batch are what passes 64 VGPRs).
#include <hip/hip_runtime.h>

#include "normals.h"

namespace {

using namespace vertex_gather;

#define NORMALS_BATCH 4

VERTEX_DEV vec3 sub(const vec3 &a, const vec3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// (-ffp-contract=off: every product and every difference rounds on its own)
VERTEX_DEV vec3 cross(const vec3 &a, const vec3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

struct face_term {
    const float *__restrict__ pos;
    bool left_handed;
    struct corners {
        vec3 p0{0.0f, 0.0f, 0.0f}, p1{0.0f, 0.0f, 0.0f}, p2{0.0f, 0.0f, 0.0f};
    };
    VERTEX_DEV corners load(uint32_t i0, uint32_t i1, uint32_t i2) const { return {load_vec3(pos, i0), load_vec3(pos, i1), load_vec3(pos, i2)}; }
    VERTEX_DEV void add(vec3 &acc, const corners &c) const {
        const vec3 e1 = sub(c.p1, c.p0), e2 = sub(c.p2, c.p0);
        const vec3 n = left_handed ? cross(e1, e2) : cross(e2, e1);
        acc.x = acc.x + n.x;
        acc.y = acc.y + n.y;
        acc.z = acc.z + n.z;
    }
};

__global__ __launch_bounds__(256) void k_vertex_normals(uint32_t *__restrict__ mesh, const r3n_normals_input32 *__restrict__ recs,
                                                        const uint32_t *__restrict__ wave_instance, const uint32_t *__restrict__ wave_first,
                                                        uint32_t total_waves) {
    const uint32_t w = wave_index();
    if (w >= total_waves) return;
    uint32_t v;
    const r3n_normals_input32 rec = wave_record(w, recs, wave_instance, wave_first, R3N_NORMALS_WAVE_VERTICES, v);
    if (v >= rec.vertex_count) return;
    const face_term term{reinterpret_cast<const float *>(mesh + rec.position_offset / 4u), rec.left_handed != 0u};
    const vec3 acc = gather_row<NORMALS_BATCH>(term, mesh, rec.index_offset, rec.index_count, rec.adjacency_offset, rec.vertex_count, v);
    store_normalized(mesh, rec.normal_offset, v, acc);
}

}  // namespace

extern "C" int r3n_internal_vertex_normals(const NormalsArgs *a, hipStream_t stream) {
    if (a->total_waves == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_vertex_normals, dim3((a->total_waves + 3u) / 4u), dim3(256), 0, stream, a->mesh, a->recs, a->wave_instance,
                       a->wave_first, a->total_waves);
    return (int)hipGetLastError();
}
