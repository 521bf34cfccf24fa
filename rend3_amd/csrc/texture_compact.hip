// Device side of r3n_textures_compact: ONE kernel that moves a table of segments (src_word, dst_word, words), every value a
// multiple of 4 words, between two word arrays -- pool -> pool (a direct pass), pool -> scratch and scratch -> pool (the two halves
// of a staged pass).  What a launch may move is decided on the host (texel_compact.h): no word written by a launch is read by the
// same launch, so no thread waits for another and there is no inter-workgroup ordering of any kind.
//
// A streaming, HBM-bound copy.  Wave slot -> segment through the wave map of the vertex stages (vertex_block.h lays it out,
// vertex_gather.h reads it): the record is wave-uniform and comes through scalar registers.  A wave slot takes 256 consecutive
// 16-byte units of ONE segment; lane l moves units l, 64 + l, 128 + l, 192 + l of it, so every wave instruction touches 1 KiB of
// consecutive bytes, and the lane's four loads are all issued before its first store: 4 KiB in flight per wave, 32 KiB per CU
// with eight resident waves -- the amount that keeps a CU's HBM loads streaming -- and more at higher occupancy (the code
// object: 25 vector registers, no LDS, no scratch; global_load_dwordx4 x 4, then global_store_dwordx4 x 4 behind counted waits).
// Launched as (waves + 3) / 4 blocks of 256.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "texel_compact.h"
#include "vertex_gather.h"

namespace {

using texel_compact::Record;
struct MoveArgs {
    const Record *recs;
    const uint32_t *wave_segment, *wave_first;  // the plan's whole table; this launch covers slots [first_wave, first_wave + waves)
    uint32_t first_wave, waves;
    const uint32_t *src;
    uint32_t *dst;
};

__global__ __launch_bounds__(256) void k_move_segments(MoveArgs a) {
    const uint32_t local = vertex_gather::wave_index();
    if (local >= a.waves) return;
    const uint32_t w = a.first_wave + local;
    const uint32_t seg = __builtin_amdgcn_readfirstlane(a.wave_segment[w]);
    const Record r = a.recs[seg];
    const uint32_t first = (w - __builtin_amdgcn_readfirstlane(a.wave_first[seg])) * texel_compact::UNITS_PER_WAVE + (threadIdx.x & 63u);
    // (src and dst are multiples of 4 words from 16-byte-aligned bases: whole uint4 accesses)
    const uint4 *src = reinterpret_cast<const uint4 *>(a.src + r.src);
    uint4 *dst = reinterpret_cast<uint4 *>(a.dst + r.dst);
    static_assert(texel_compact::LOADS_PER_LANE == 4u, "four named values below");
    if (first >= r.units) return;
    // the loads are unconditional -- a unit past the segment's end reads its last unit again and stores nothing -- so that the four
    // are requested together (guarded loads are each waited for inside their branch).  Four named values, not an array: an array
    // indexed in an unrolled loop was kept as an alloca and promoted to LDS, a round trip per unit.
    const uint32_t last = r.units - 1u;
    const uint32_t u0 = first, u1 = first + 64u, u2 = first + 128u, u3 = first + 192u;
    const uint4 v0 = src[u0];
    const uint4 v1 = src[min(u1, last)];
    const uint4 v2 = src[min(u2, last)];
    const uint4 v3 = src[min(u3, last)];
    dst[u0] = v0;
    if (u1 <= last) dst[u1] = v1;
    if (u2 <= last) dst[u2] = v2;
    if (u3 <= last) dst[u3] = v3;
}

}  // namespace

// Wave slots [first_wave, first_wave + waves) of the plan's table (`block` = its device copy, o_first / o_inst = the layout's word
// offsets): their segments from `src` to `dst`.
extern "C" int r3n_internal_move_segments(const uint32_t *block, uint64_t o_first, uint64_t o_inst, uint32_t first_wave, uint32_t waves,
                                          const uint32_t *src, uint32_t *dst, hipStream_t stream) {
    if (!waves) return (int)hipSuccess;
    MoveArgs a;
    a.recs = reinterpret_cast<const Record *>(block);
    a.wave_first = block + o_first;
    a.wave_segment = block + o_inst;
    a.first_wave = first_wave;
    a.waves = waves;
    a.src = src;
    a.dst = dst;
    hipLaunchKernelGGL(k_move_segments, dim3((waves + 3u) / 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
