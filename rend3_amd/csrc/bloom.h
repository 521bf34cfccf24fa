// bloom.h -- plan and launchers of the bloom kernels (bloom.hip).  The rule is bloom_rule.h; the wiring (what runs when, on which
// stream, the pyramid's allocation) is r3n.hip; the composite is a flag of k_tonemap_op (exposure.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/r3n.h"
#include "bloom_rule.h"

static_assert(sizeof(r3n_bloom_opts) == 32, "include/r3n.h layouts");

#define R3N_BLOOM_TILE_X 32u           // destination texels of one workgroup of the tiled down kernel
#define R3N_BLOOM_TILE_Y 16u
#define R3N_BLOOM_TAIL_LDS 163840u     // the tail kernel's workgroup may hold this much (the whole LDS of a CU)
#define R3N_BLOOM_TAIL_TEXELS (R3N_BLOOM_TAIL_LDS / 8u)
#define R3N_BLOOM_TAIL_DEFAULT 4096u   // ctx.tune.bloom_tail (profiles/bloom.md)

// One pyramid: the levels one behind the other, a texel three halves and a pad (8 B), every level starting at an even texel.
//   tail: the first level the tail kernel takes (it takes all levels from there on); == lv.n: every level has launches of its own
struct BloomPlan {
    bloom_rule::Levels lv;
    uint32_t off[R3N_BLOOM_MAX_LEVELS];
    uint32_t total, tail;
};

// the plan for a W x H target: `tail_texels` is ctx.tune.bloom_tail (0: no tail kernel).  The tail starts at the first level that
// holds at most that many texels and whose levels from there on fit the tail kernel's LDS together.
inline BloomPlan bloom_plan(uint32_t W, uint32_t H, uint32_t max_levels, uint32_t tail_texels) {
    BloomPlan p{};
    p.lv = bloom_rule::levels(W, H, max_levels);
    uint32_t at = 0;
    for (uint32_t k = 0; k < p.lv.n; ++k) {
        p.off[k] = at;
        at += (p.lv.w[k] * p.lv.h[k] + 1u) & ~1u;
    }
    p.total = at;
    p.tail = p.lv.n;
    uint64_t behind = 0;
    for (uint32_t k = p.lv.n; k-- > 0u;) {
        const uint64_t n = (uint64_t)p.lv.w[k] * p.lv.h[k];
        behind += n;
        if (tail_texels == 0u || n > tail_texels || behind > R3N_BLOOM_TAIL_TEXELS) break;
        p.tail = k;
    }
    return p;
}

// Each returns the hipError_t of the launch as an int; they only enqueue.  d: the pyramid of the down chain, a: the pyramid of
// the up chain (the same block unless ctx.tune.bloom_keep_down).  scale_ptr != NULL: the exposure scale is loaded from there.
extern "C" {
// d_k from d_{k-1}, or (k == 0) from the bright pass of the HDR target
int r3n_internal_bloom_down(const ushort4 *hdr, uint32_t W, uint32_t H, ushort4 *d, const BloomPlan *plan, uint32_t k, const bloom_rule::Params *p,
                            const float *scale_ptr, float scale, hipStream_t stream);
// a_k = half(d_k + scatter * up(a_{k+1}))
int r3n_internal_bloom_up(const ushort4 *d, ushort4 *a, const BloomPlan *plan, uint32_t k, const bloom_rule::Params *p, hipStream_t stream);
// every level from plan->tail on, down and back up, in one workgroup: writes a_k (and d_k where d != a) of those levels
int r3n_internal_bloom_tail(const ushort4 *hdr, uint32_t W, uint32_t H, ushort4 *d, ushort4 *a, const BloomPlan *plan, const bloom_rule::Params *p,
                            const float *scale_ptr, float scale, hipStream_t stream);
}
