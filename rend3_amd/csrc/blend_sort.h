// blend_sort.h -- the back-to-front order of the transparent pass, sorted on the device (blend_sort.hip): argument block, scratch
// size and launcher behind r3n_blend_sort (r3n.hip).
//
// The BLEND SET (r3n_blend_objects_write) is the blend-key objects' slots, strictly ascending, and their sorting locations; it
// changes when the world is edited.  The sort key depends on the camera location and changes every frame:
//     d = camera - location;  dist = (d.x * d.x + d.y * d.y) + d.z * d.z  (f32, one rounding per operation);  key = -dist
// ascending, ties by ascending slot (rend3-routine/src/culling/batching.rs:146-176 with Sorting::BLENDING; the tie rule is
// host.blend_draw_order's, the reference's unstable sort leaves ties open).  The result is a pure function of (key, slot).
// +inf distances are legal and tie with each other.  NaN locations (or a NaN camera) are outside the contract: such an object
// lands at some place in the order, nothing is read or written out of bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// n <= R3N_BLEND_SORT_SMALL: ONE launch of one workgroup (keys, bitonic sort of (key << 32 | index) and rank scan in LDS).
// Above: a stable LSD radix sort, 8 bits per pass over tiles of R3N_BLEND_SORT_TILE keys, and a tiled scan.
#define R3N_BLEND_SORT_SMALL 4096u
#define R3N_BLEND_SORT_TILE 4096u

struct BlendSortArgs {
    const uint32_t *slots;      // n, strictly ascending
    const float *locations;     // 3 n
    uint32_t n;
    float camera[3];
    const uint32_t *obj_meta;   // per object slot: triangle count of the object record (0 when disabled) in the low 30 bits
                                // (kernels_cull.h ObjSoA::meta)
    uint32_t *order;            // out, n: object slots back to front
    uint32_t *rank_base;        // out, n + 1: exclusive scan of the triangle counts in that order
    uint32_t *scratch;          // r3n_internal_blend_sort_scratch_words(n) words
};

// u32 words of scratch the sort of n objects needs (0 on the one-workgroup path): depends on n alone, so the buffer is sized when
// the set is uploaded
extern "C" size_t r3n_internal_blend_sort_scratch_words(uint32_t n);
// enqueues the sort on `stream`; every grid is a function of n alone.  Returns the hipError_t of the launches.
extern "C" int r3n_internal_blend_sort(const BlendSortArgs *a, hipStream_t stream);
