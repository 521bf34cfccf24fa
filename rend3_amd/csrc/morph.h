// morph.h -- glTF morph targets blended on the device (morph.hip): device record, argument block and launcher behind r3n_morph
// (r3n.hip).
//
// Contract (include/r3n.h): for every f32 word k of a morphed attribute run
//     acc = base[k];  for the instance's NON-ZERO weights in ascending target order: acc = fl(acc + fl(w * delta[target][k]));  out[k] = acc
// one rounding per operation (the unit is built with -ffp-contract=off).  A weight that compares equal to 0.0f is not a term
// (+0 and -0; NaN is one): r3n_morph compacts the (target, weight) pairs that are terms on the host, so all-zero weights copy the
// base run bit for bit and a skipped target costs no bytes.  There is no per-vertex structure: a run is 3 * vertex_count words.
#pragma once
#include "../../include/r3n.h"
#include "vertex_gather.h"

#define R3N_MORPH_WAVE_WORDS 256u  // words of every morphed run one wave covers: 64 lanes x 4 words (one dwordx4 each)

// One instance as the kernel reads it: 16 words = one s_load_dwordx16.
struct r3n_morph_rec64 {
    r3n_morph_input48 in;
    uint32_t pair_first;  // first entry of the instance's terms in `pairs`
    uint32_t n_active;    // how many (0: the runs are copies of the base)
    uint32_t _pad[2];
};
static_assert(sizeof(r3n_morph_rec64) == 64, "morph record is 16 dwords");

struct r3n_morph_pair {
    uint32_t target;
    float weight;
};

struct MorphArgs : vertex_gather::Args<r3n_morph_rec64> {
    const r3n_morph_pair *pairs;
};

// enqueues the ONE launch on `stream`; returns the hipError_t of the launch
extern "C" int r3n_internal_morph(const MorphArgs *a, hipStream_t stream);
