// exposure.h -- device block and launchers of the auto-exposure / tonemapping-operator kernels (exposure.hip).  The rule itself is
// exposure_rule.h; the wiring (what runs when, the commit at r3n_frame_end) is r3n.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/r3n.h"
#include "exposure_rule.h"

// One device block per context, allocated zeroed by the first metered r3n_tonemap.
//   counters : this frame's histogram + excluded count; k_exposure_update leaves them zero
//   state[2] : the state the previous frame committed and the one this frame produces (which is which: r3n_ctx::exp_committed)
//   lq, e    : the two host tables
struct ExposureBlock {
    uint32_t counters[R3N_EXP_BINS + 1];  // [256]: excluded
    uint32_t _pad[3];
    r3n_exposure_state state[2];
    int32_t lq[R3N_EXP_BINS];
    float e[R3N_EXP_E_ENTRIES];
    uint32_t _pad2[3];
};
static_assert(sizeof(r3n_exposure_state) == 1056 && sizeof(r3n_tonemap_opts) == 48, "include/r3n.h layouts");
static_assert(sizeof(ExposureBlock) % 16 == 0, "state[] stays 16-byte aligned");

#define R3N_EXP_HIST_GRID 1024u  // workgroups of k_luminance_histogram at most: four per CU, the rest of the target by grid stride

// what the operator kernel composites (r3n_bloom_set): level 0 of the up chain's pyramid (bw x bh texels of three halves and a
// pad) over a target `width` pixels wide
struct R3nBloomComposite {
    const ushort4 *a0;
    uint32_t bw, bh, width;
    float intensity;
};

// Each returns the hipError_t of the launch as an int; they only enqueue.
extern "C" {
// counters[bin] += pixels of [first_pixel, first_pixel + n_pixels) in that bin
int r3n_internal_luminance_histogram(const ushort4 *hdr, size_t first_pixel, size_t n_pixels, uint32_t *counters, hipStream_t stream);
// prev -> cur through exposure_rule::step; snapshots the histogram into cur and zeroes the counters.  prev_invalid: ignore prev.valid
int r3n_internal_exposure_update(ExposureBlock *block, int prev, int cur, const exposure_rule::Params *p, int prev_invalid, hipStream_t stream);
// k_tonemap with exposure and operator in front of the transfer; scale_ptr != NULL: the scale is loaded from there (AUTO);
// bloom != NULL: the bloom pyramid is composited in front of the operator (pixel indices must fit 32 bits then)
int r3n_internal_tonemap_op(const ushort4 *hdr, uchar4 *out, float4 *out_f32, size_t first_pixel, size_t n_pixels, const unsigned char *srgb_lut,
                            uint32_t output_format, uint32_t op, const float *scale_ptr, float scale, float white_sq, const R3nBloomComposite *bloom,
                            hipStream_t stream);
}
