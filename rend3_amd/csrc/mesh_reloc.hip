// Device side of r3n_mesh_compact's relocation: ONE kernel that walks the object buffer and rewrites, in every 128-byte record, the
// seven words that name mesh-buffer addresses (mesh_reloc.h holds the table, the lookup and the patch; the host and
// tests/mesh_reloc_check.cpp compile the same code).  It runs behind the call's full wait -- no frame reads a record while it is
// patched -- and touches every slot below the context's capacity by address alone, enabled or not.
//
// One thread per object slot, 256 per workgroup.  A thread reads words 20..28 of its record (bytes 80..115: two 16-byte loads and
// one 4-byte load inside ONE 128-byte line -- the line is the unit HBM delivers, so the kernel is bound by capacity x 128 B of
// reads, a quarter of what re-sending the records costs the bus) and stores only the words that changed, one dword store each:
// records that name no moved block are not written at all.
//
// Where the table lives.  Up to mesh_reloc::LDS_TABLE_ENTRIES entries (4 KiB): every thread of the workgroup fetches ONE entry
// into LDS, the seven lookups then cost LDS latency instead of up to 8 x 7 dependent L2 round trips.  A longer table stays in global
// memory: 100 000 entries are 1.6 MB, the upper levels of every thread's search are the same few lines and stay in the XCD's L2
// (4 MiB), and copying such a table into LDS per workgroup would cost more than the records.  The hint (the entry that served the
// previous field) saves most searches either way: a plain object names ONE block with all seven fields.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mesh_reloc.h"

namespace {

using mesh_reloc::Entry;

template <class Table>
__device__ __forceinline__ void relocate_record(Table table, uint32_t n, uint32_t *rec) {
    static_assert(mesh_reloc::LOAD_FIRST_WORD == 20u && mesh_reloc::LOAD_WORDS == 9u && mesh_reloc::FIRST_INDEX_WORD == 20u &&
                      mesh_reloc::ATTRIBUTE_WORD == 23u && mesh_reloc::ATTRIBUTES == 6u,
                  "the loads below are words 20..23, 24..27 and 28 of the record");
    // (a record is 128-byte aligned: words 20 and 24 are 16-byte aligned)
    const uint4 a = *reinterpret_cast<const uint4 *>(rec + 20);  // first_index, index_count, material_index, attribute 0
    const uint4 b = *reinterpret_cast<const uint4 *>(rec + 24);  // attributes 1..4
    const uint32_t c = rec[28];                                  // attribute 5
    uint32_t f[mesh_reloc::FIELDS] = {a.x, a.w, b.x, b.y, b.z, b.w, c};
    const uint32_t changed = mesh_reloc::patch_fields(table, n, f);
    if (changed & 1u) rec[20] = f[0];
    if (changed & 2u) rec[23] = f[1];
    if (changed & 4u) rec[24] = f[2];
    if (changed & 8u) rec[25] = f[3];
    if (changed & 16u) rec[26] = f[4];
    if (changed & 32u) rec[27] = f[5];
    if (changed & 64u) rec[28] = f[6];
}

__global__ __launch_bounds__(256) void k_relocate_objects(uint32_t *__restrict__ objects, uint32_t capacity, const Entry *__restrict__ table,
                                                          uint32_t n) {
    __shared__ Entry s_table[mesh_reloc::LDS_TABLE_ENTRIES];
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const bool in_lds = n <= mesh_reloc::LDS_TABLE_ENTRIES;  // (uniform over the grid)
    if (in_lds) {
        if (threadIdx.x < n) s_table[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    if (slot >= capacity) return;
    uint32_t *rec = objects + (size_t)slot * mesh_reloc::RECORD_WORDS;
    if (in_lds) relocate_record(static_cast<const Entry *>(s_table), n, rec);
    else relocate_record(table, n, rec);
}

}  // namespace

// every record of objects[0, capacity) through the table (n entries, sorted by source, on the device)
extern "C" int r3n_internal_relocate_objects(uint32_t *objects, uint32_t capacity, const void *table, uint32_t n, hipStream_t stream) {
    if (!capacity || !n) return (int)hipSuccess;
    static_assert(mesh_reloc::LDS_TABLE_ENTRIES <= 256u, "one entry per thread of the workgroup");
    hipLaunchKernelGGL(k_relocate_objects, dim3((capacity + 255u) / 256u), dim3(256), 0, stream, objects, capacity,
                       static_cast<const Entry *>(table), n);
    return (int)hipGetLastError();
}
