// envlight.h -- argument block and launcher of the passes that read lights out of a cube level (envlight.hip,
// r3n_environment_lights).  The rule: envlight_rule.h.  Plain C++17 besides the stream type.
//
// The call's scratch block (grow-only, owned by the context):
//     [0, ENVLIGHT_STATE_BYTES)   envlight_rule::State, zeroed in front of the first pass
//     then, under plan 1 only     the plane: 6 n n uint4 (q_r, q_g, q_b: the low 32 bits of each; their bits 32 .. 39 as the three low
//                                 bytes of .w), then 6 n n f32 luminances -- 20 bytes per texel, written once by the quantise pass
// Launches of one call: 1 (e_max) + 1 (quantise, totals, the first seed) + 3 per light asked for (gather (b) twice; gather (c) fused with
// the seed search of the next light).  A launch whose light cannot exist any more (an earlier light was not emitted, or nothing
// is left to seed from) reads the state and returns: there is no host wait between the lights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "envlight_rule.h"

#define R3N_ENVLIGHT_PLANE_DEFAULT 0u    // R3N_TUNE envlight_plane (profiles/envlight.md: the passes are bound by their arithmetic, the plane buys nothing)
#define R3N_ENVLIGHT_BLOCKS_DEFAULT 0u   // R3N_TUNE envlight_blocks: 0 = one block per 1024 texels, at most R3N_ENVLIGHT_BLOCKS_AUTO
#define R3N_ENVLIGHT_BLOCKS_AUTO 2048u
#define R3N_ENVLIGHT_BLOCKS_MAX 4096u
#define R3N_ENVLIGHT_STATE_BYTES 4096u
static_assert(sizeof(envlight_rule::State) <= R3N_ENVLIGHT_STATE_BYTES, "the state has its 4 KiB in front of the plane");

struct EnvlightArgs {
    const uint32_t *level;        // the level's six bordered faces (cube_faces.h)
    const float *decode;          // 256 entries: the decode table of the cube's class (RGBA8 classes only)
    uint32_t n;                   // the level's extent, <= envlight_rule::MAX_EXTENT
    uint32_t f32_class;           // the texels are four f32 words
    envlight_rule::State *state;
    uint4 *plane_q;               // plan 1: the plane; plan 0: null
    float *plane_lum;
    envlight_rule::Params rule;
    uint32_t blocks;              // grid of every pass, 1 .. R3N_ENVLIGHT_BLOCKS_MAX
};
inline size_t envlight_scratch_bytes(uint32_t n, bool plane) { return R3N_ENVLIGHT_STATE_BYTES + (plane ? (size_t)6u * n * n * 20u : 0u); }
inline uint32_t envlight_grid(uint32_t n, uint32_t tuned) {
    const uint32_t texels = 6u * n * n, whole = (texels + 255u) / 256u;
    uint32_t blocks = tuned ? tuned : (texels + 1023u) / 1024u;
    if (!tuned && blocks > R3N_ENVLIGHT_BLOCKS_AUTO) blocks = R3N_ENVLIGHT_BLOCKS_AUTO;
    if (blocks > whole) blocks = whole;  // no block without a texel
    return blocks ? blocks : 1u;
}

// Enqueues the clear of the state and every pass.  taps (may be null): four events recorded in front of the e_max pass, behind it,
// behind the quantise pass and behind the last light pass.  Returns the hipError_t of the first failure; *launches counts kernels.
extern "C" int r3n_internal_envlight(const EnvlightArgs *a, hipEvent_t *taps, hipStream_t stream, uint64_t *launches);
