// cube_faces.hip -- k_cube_assemble: ONE launch builds every bordered face of every level of every cube of an
// r3n_texture_cubes_write_encoded call from the dense faces the decode jobs (texture_decode.hip) left in the call's scratch block.
// Layout, edge table and the per-position function: cube_faces.h (shared with the host and with tests/cube_faces_check.cpp).
//
// Wave slot -> (cube, level, face) through the wave map of the vertex stages (vertex_block.h lays the block out, vertex_gather.h
// reads it): the record is wave-uniform and comes through scalar registers; lane l of a face's k-th wave slot takes position
// 64 k + l of the bordered face: one gather from the dense faces, one store -- 4 bytes for the RGBA8 classes, 16 for the f32 class
// (dense faces, pool levels and cubes all start on 4-word boundaries and an f32 texel is 4 words).  A corner position stores zero.
// Launched as (total_waves + 3) / 4 blocks of 256.
#include <hip/hip_runtime.h>

#include "cube_faces.h"
#include "vertex_gather.h"

namespace {

using cube_faces::Record;
typedef uint32_t texel16 __attribute__((ext_vector_type(4)));  // an f32-class texel: one 16-byte load, one 16-byte store
struct AssembleArgs {
    const Record *recs;
    const uint32_t *wave_rec, *wave_first;
    uint32_t total_waves;
    const uint32_t *dense;  // the call's scratch block: decoded faces without borders
    uint32_t *pool;         // the cube pool
};

__global__ __launch_bounds__(256) void k_cube_assemble(AssembleArgs a) {
    const uint32_t wv = vertex_gather::wave_index();
    if (wv >= a.total_waves) return;
    uint32_t unit;
    const Record r = vertex_gather::wave_record(wv, a.recs, a.wave_rec, a.wave_first, cube_faces::UNITS_PER_WAVE, unit);
    if (unit >= r.units) return;
    if (r.per_texel == 4u) {
        cube_faces::assemble_at(reinterpret_cast<const texel16 *>(a.dense + r.src), (size_t)(r.src_stride / 4u),
                                reinterpret_cast<texel16 *>(a.pool + r.dst), r.face, r.n, unit, (texel16){0u, 0u, 0u, 0u});
    } else {
        cube_faces::assemble_at(a.dense + r.src, (size_t)r.src_stride, a.pool + r.dst, r.face, r.n, unit, 0u);
    }
}

}  // namespace

// `block` = the device copy of the table (records | wave_first | wave_instance at the layout's word offsets), dense = the scratch
// block the records' src index, pool = the cube pool their dst index.
extern "C" int r3n_internal_cube_assemble(const uint32_t *block, uint64_t o_first, uint64_t o_inst, uint32_t total_waves, const uint32_t *dense,
                                          uint32_t *pool, hipStream_t stream) {
    if (!total_waves) return (int)hipSuccess;
    AssembleArgs a;
    a.recs = reinterpret_cast<const Record *>(block);
    a.wave_first = block + o_first;
    a.wave_rec = block + o_inst;
    a.total_waves = total_waves;
    a.dense = dense;
    a.pool = pool;
    hipLaunchKernelGGL(k_cube_assemble, dim3((total_waves + 3u) / 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
