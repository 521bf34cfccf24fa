// Device side of r3n_textures_from_texture: ONE kernel that copies a table of segments (src_word, dst_word, units) inside the texel
// pool -- the levels [start_mip, start_mip + mip_count) of a resident texture into the fresh words of a new one
// (TextureManager::fill_from_texture, rend3/src/managers/texture.rs:198-242: one copy_texture_to_texture per level there, one
// contiguous word range here).  What a launch may copy is decided on the host (texel_tail.h): no word written by a launch is a tail
// word the same launch reads, so no thread waits for another and there is no inter-workgroup ordering of any kind.
//
// The streaming shape of k_move_segments (texture_compact.hip): wave slot -> segment through the wave map of the vertex stages, the
// record wave-uniform through scalar registers; a wave slot takes 256 consecutive 16-byte destination units of ONE segment, lane l
// moves units l, 64 + l, 128 + l, 192 + l, and the lane's four loads are all issued before its first store.  What is new is the
// source's alignment: the destination starts on a 4-word boundary and is written as whole uint4 units, the source starts on ANY
// word, src & 3 uniform per segment.  Unit u is read as the four words src + 4u .. src + 4u + 3 by ONE 16-byte load whose address
// is 4-byte aligned (a vector type declared with 4-byte alignment: global memory takes dword-aligned multi-dword accesses), so the
// aligned and the misaligned segment run the same instructions; a misaligned wave load of 1 KiB touches nine 128-byte lines, not
// eight.  Unit indices are clamped to the segment's last unit as in k_move_segments: no lane reads past last unit + 3 words, which
// is at most 3 words past the tail's end and inside the pool block (16 bytes of slack behind the high-water mark); the up to 3
// padding words of the last unit stored lie inside the destination's own padded range.
// The code object: 25 vector registers, 18 scalar registers, no LDS, no scratch; global_load_dwordx4 x 4, then
// global_store_dwordx4 x 4 behind counted waits.  Launched as (waves + 3) / 4 blocks of 256.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "texel_tail.h"
#include "vertex_gather.h"

namespace {

using texel_tail::Record;
// four pool words at any word boundary
typedef uint32_t words4 __attribute__((ext_vector_type(4), aligned(4)));
struct TailArgs {
    const Record *recs;
    const uint32_t *wave_segment, *wave_first;
    uint32_t waves;
    uint32_t *pool;
};

__global__ __launch_bounds__(256) void k_copy_tails(TailArgs a) {
    const uint32_t w = vertex_gather::wave_index();
    if (w >= a.waves) return;
    const uint32_t seg = __builtin_amdgcn_readfirstlane(a.wave_segment[w]);
    const Record r = a.recs[seg];
    const uint32_t first = (w - __builtin_amdgcn_readfirstlane(a.wave_first[seg])) * texel_tail::UNITS_PER_WAVE + (threadIdx.x & 63u);
    const words4 *src = reinterpret_cast<const words4 *>(a.pool + r.src);  // any word
    uint4 *dst = reinterpret_cast<uint4 *>(a.pool + r.dst);                // a multiple of 4 words from a 16-byte-aligned base
    static_assert(texel_tail::LOADS_PER_LANE == 4u, "four named values below");
    if (first >= r.units) return;
    // unconditional loads, four named values: see k_move_segments
    const uint32_t last = r.units - 1u;
    const uint32_t u0 = first, u1 = first + 64u, u2 = first + 128u, u3 = first + 192u;
    const words4 v0 = src[u0];
    const words4 v1 = src[min(u1, last)];
    const words4 v2 = src[min(u2, last)];
    const words4 v3 = src[min(u3, last)];
    dst[u0] = make_uint4(v0.x, v0.y, v0.z, v0.w);
    if (u1 <= last) dst[u1] = make_uint4(v1.x, v1.y, v1.z, v1.w);
    if (u2 <= last) dst[u2] = make_uint4(v2.x, v2.y, v2.z, v2.w);
    if (u3 <= last) dst[u3] = make_uint4(v3.x, v3.y, v3.z, v3.w);
}

}  // namespace

// The call's table (`block` = its device copy, o_first / o_inst = the layout's word offsets), all `waves` wave slots, inside `pool`.
extern "C" int r3n_internal_copy_tails(const uint32_t *block, uint64_t o_first, uint64_t o_inst, uint32_t waves, uint32_t *pool,
                                       hipStream_t stream) {
    if (!waves) return (int)hipSuccess;
    TailArgs a;
    a.recs = reinterpret_cast<const Record *>(block);
    a.wave_first = block + o_first;
    a.wave_segment = block + o_inst;
    a.waves = waves;
    a.pool = pool;
    hipLaunchKernelGGL(k_copy_tails, dim3((waves + 3u) / 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
