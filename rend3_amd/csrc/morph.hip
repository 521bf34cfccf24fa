// morph.hip -- glTF morph targets: out = base + sum of weight * delta over the instance's non-zero weights, for the private
// POSITION / NORMAL / TANGENT runs of every instance of one r3n_morph call, in ONE launch.  Contract and terms: morph.h.
//
// The operation is element-wise per f32 word, so a run is a flat array of 3 * vertex_count words.  A wave slot (wave map:
// vertex_gather.h) covers 256 words of each of its instance's morphed runs: lane l holds words 4 l .. 4 l + 3.  The 64-byte record
// and the (target, weight) terms are wave-uniform and come through scalar registers; the loop over the terms has the same trip
// count in every lane.
//
// Access width: a lane's four words are moved as one dwordx4 where the run's byte offset is a multiple of 16 (the delta and output
// runs the renderer allocates; a target's run inside the delta block only when 12 * vertex_count is one too), as four dword
// accesses otherwise (a base run add_mesh packed behind an odd-sized one).  The choice is per (run, target), wave-uniform, and moves
// the same words either way.  The last, partial quad of a run goes word by word: nothing is read or written past a run's end.
//
// HBM-bound stream: 12 * A * (2 + T_active) bytes per vertex for A morphed attributes, two flops per delta word.  No LDS, no
// atomics, no scratch.  -Rpass-analysis=kernel-resource-usage (gfx950): 27 VGPRs, 0 AGPRs, 47 SGPRs, 0 B scratch, 0 B LDS,
// occupancy 8 waves per SIMD.
#include <hip/hip_runtime.h>

#include "morph.h"

namespace {

#define MORPH_DEV __device__ __forceinline__

typedef float quad __attribute__((ext_vector_type(4)));  // a lane's four words; as a memory operand it is 16-byte aligned: one dwordx4

MORPH_DEV quad load_quad(const uint32_t *p, bool wide) {
    if (wide) return *reinterpret_cast<const quad *>(p);
    return quad{__uint_as_float(p[0]), __uint_as_float(p[1]), __uint_as_float(p[2]), __uint_as_float(p[3])};
}

MORPH_DEV void store_quad(uint32_t *p, const quad &v, bool wide) {
    if (wide) { *reinterpret_cast<quad *>(p) = v; return; }
    p[0] = __float_as_uint(v.x); p[1] = __float_as_uint(v.y); p[2] = __float_as_uint(v.z); p[3] = __float_as_uint(v.w);
}

MORPH_DEV void add_term(quad &acc, float w, const quad &d) {
    acc = acc + w * d;  // (-ffp-contract=off: every product and every sum rounds on its own)
}

MORPH_DEV r3n_morph_pair term(const r3n_morph_pair *__restrict__ pairs, uint32_t k) {
    r3n_morph_pair p;
    p.target = __builtin_amdgcn_readfirstlane(pairs[k].target);
    p.weight = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pairs[k].weight)));
    return p;
}

// one run of one instance: words [i, i + 4) of it, clipped to n_words.  Every argument but `i` is wave-uniform.
MORPH_DEV void blend_run(uint32_t *__restrict__ mesh, uint32_t base_off, uint32_t delta_off, uint32_t out_off, uint32_t n_words,
                         uint32_t i, const r3n_morph_pair *__restrict__ pairs, uint32_t n_active) {
    const uint32_t *base = mesh + base_off / 4u;
    const uint32_t *delta = mesh + delta_off / 4u;
    uint32_t *out = mesh + out_off / 4u;
    const uint32_t target_bytes = n_words * 4u;
    if (i + 4u <= n_words) {
        quad acc = load_quad(base + i, (base_off & 15u) == 0u);
        uint32_t k = 0;
        for (; k + 4u <= n_active; k += 4u) {  // four delta loads in flight, applied in target order
            r3n_morph_pair p[4];
            quad d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = term(pairs, k + u);
                d[u] = load_quad(delta + (size_t)p[u].target * n_words + i, ((delta_off + p[u].target * target_bytes) & 15u) == 0u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) add_term(acc, p[u].weight, d[u]);
        }
        for (; k < n_active; ++k) {
            const r3n_morph_pair p = term(pairs, k);
            add_term(acc, p.weight, load_quad(delta + (size_t)p.target * n_words + i, ((delta_off + p.target * target_bytes) & 15u) == 0u));
        }
        store_quad(out + i, acc, (out_off & 15u) == 0u);
    } else {
        for (uint32_t j = i; j < n_words; ++j) {  // the run's last one to three words
            float acc = __uint_as_float(base[j]);
            for (uint32_t k = 0; k < n_active; ++k) {
                const r3n_morph_pair p = term(pairs, k);
                acc = acc + p.weight * __uint_as_float(delta[(size_t)p.target * n_words + j]);
            }
            out[j] = __float_as_uint(acc);
        }
    }
}

__global__ __launch_bounds__(256) void k_morph(uint32_t *__restrict__ mesh, const r3n_morph_rec64 *__restrict__ recs,
                                               const r3n_morph_pair *__restrict__ pairs, const uint32_t *__restrict__ wave_instance,
                                               const uint32_t *__restrict__ wave_first, uint32_t total_waves) {
    const uint32_t w = vertex_gather::wave_index();
    if (w >= total_waves) return;
    uint32_t i;
    const r3n_morph_rec64 rec = vertex_gather::wave_record(w, recs, wave_instance, wave_first, R3N_MORPH_WAVE_WORDS, i);
    const uint32_t n_words = rec.in.vertex_count * 3u;
    if (i >= n_words) return;
    const r3n_morph_pair *terms = pairs + rec.pair_first;
    if (rec.in.delta_position_offset != 0xFFFFFFFFu)
        blend_run(mesh, rec.in.base_position_offset, rec.in.delta_position_offset, rec.in.updated_position_offset, n_words, i, terms, rec.n_active);
    if (rec.in.delta_normal_offset != 0xFFFFFFFFu)
        blend_run(mesh, rec.in.base_normal_offset, rec.in.delta_normal_offset, rec.in.updated_normal_offset, n_words, i, terms, rec.n_active);
    if (rec.in.delta_tangent_offset != 0xFFFFFFFFu)
        blend_run(mesh, rec.in.base_tangent_offset, rec.in.delta_tangent_offset, rec.in.updated_tangent_offset, n_words, i, terms, rec.n_active);
}

}  // namespace

extern "C" int r3n_internal_morph(const MorphArgs *a, hipStream_t stream) {
    if (a->total_waves == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_morph, dim3((a->total_waves + 3u) / 4u), dim3(256), 0, stream, a->mesh, a->recs, a->pairs, a->wave_instance,
                       a->wave_first, a->total_waves);
    return (int)hipGetLastError();
}
