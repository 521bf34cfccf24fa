// Device side of r3n_sample_probe (include/r3n.h): the instantiations of texture.h's sampler that the frame's kernels launch, run on
// a list of queries -- one thread per query, 64 consecutive queries one wavefront -- so that tests can reach every path of the
// sampler with chosen coordinates and gradients instead of through whole frames.  The kernel is handed the TextureArgs the resolve
// gets (r3n.hip texture_args); which queries a form may see is checked on the host (r3n_sample_probe): the short-path-only and
// batched forms read outside the pool when their preconditions do not hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_math.h"
#include "texture.h"

static_assert(sizeof(r3n_sample_query40) == 40 && sizeof(r3n_sample_result52) == 52, "ABI layout");

namespace {

template <uint32_t FORM>
__global__ __launch_bounds__(64) void k_sample_probe(TextureArgs t, const r3n_sample_query40 *__restrict__ queries, uint32_t n,
                                                    r3n_sample_result52 *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;  // (a last partial wave: the batched form's wave-wide votes count active lanes only)
    const r3n_sample_query40 q = queries[i];
    const bool nearest = q.nearest != 0u;
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k][0] = o[k][1] = o[k][2] = o[k][3] = 0.0f;
    uint32_t flags = 0u;
    if (FORM == R3N_PROBE_GRAD) {
        tex_sample_grad<MathExact, true>(t, q.id[0], nearest, q.u, q.v, q.ddx, q.ddy, o[0]);
    } else if (FORM == R3N_PROBE_GRAD_RGB) {
        tex_sample_grad<MathExact, false>(t, q.id[0], nearest, q.u, q.v, q.ddx, q.ddy, o[0]);
    } else if (FORM == R3N_PROBE_SHORT) {
        tex_sample_grad<MathExact, true, true>(t, q.id[0], false, q.u, q.v, q.ddx, q.ddy, o[0]);
    } else if (FORM == R3N_PROBE_SHORT_RGB) {
        tex_sample_grad<MathExact, false, true>(t, q.id[0], false, q.u, q.v, q.ddx, q.ddy, o[0]);
    } else if (FORM == R3N_PROBE_SHARE) {
        TexShare share;  // empty, as fragment_stage starts it
        share.width = 0u; share.height = 0u; share.mips = 0u; share.level = 0u; share.frac = 0.0f;
        tex_sample_grad<MathExact, true, true, true>(t, q.id[0], false, q.u, q.v, q.ddx, q.ddy, o[0], &share);
        tex_sample_grad<MathExact, true, true, true>(t, q.id[1], false, q.u, q.v, q.ddx, q.ddy, o[1], &share);
        tex_sample_grad<MathExact, false, true, true>(t, q.id[2], false, q.u, q.v, q.ddx, q.ddy, o[2], &share);
    } else if (FORM == R3N_PROBE_ALPHA || FORM == R3N_PROBE_ALPHA_SHORT) {
        // d = descs[id - 1] as the rasterisers fetch it once per triangle; an id the sampler answers with 0 needs no descriptor
        r3n_texture_desc32 d = {};
        if (q.id[0] != 0u && q.id[0] <= t.count) d = t.descs[q.id[0] - 1u];
        o[0][3] = tex_sample_alpha<MathExact, FORM == R3N_PROBE_ALPHA_SHORT>(t, q.id[0], d, FORM == R3N_PROBE_ALPHA && nearest, q.u, q.v, q.ddx, q.ddy);
    } else {
        flags = tex_sample3_batched<MathExact>(t, q.id, q.u, q.v, q.ddx, q.ddy, o) ? 1u : 0u;
        if (!flags) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k][0] = o[k][1] = o[k][2] = o[k][3] = 0.0f;
        }
    }
    r3n_sample_result52 r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.rgba[k][0] = o[k][0]; r.rgba[k][1] = o[k][1]; r.rgba[k][2] = o[k][2]; r.rgba[k][3] = o[k][3];
    }
    r.flags = flags;
    out[i] = r;
}

}  // namespace

extern "C" int r3n_internal_sample_probe(const TextureArgs *t, uint32_t form, const r3n_sample_query40 *queries, uint32_t n,
                                         r3n_sample_result52 *out, hipStream_t stream) {
    const dim3 grid((n + 63u) / 64u), block(64);
#define R3N_PROBE_CASE(F) case F: hipLaunchKernelGGL((k_sample_probe<F>), grid, block, 0, stream, *t, queries, n, out); break
    switch (form) {
        R3N_PROBE_CASE(R3N_PROBE_GRAD);
        R3N_PROBE_CASE(R3N_PROBE_GRAD_RGB);
        R3N_PROBE_CASE(R3N_PROBE_SHORT);
        R3N_PROBE_CASE(R3N_PROBE_SHORT_RGB);
        R3N_PROBE_CASE(R3N_PROBE_SHARE);
        R3N_PROBE_CASE(R3N_PROBE_ALPHA);
        R3N_PROBE_CASE(R3N_PROBE_ALPHA_SHORT);
        R3N_PROBE_CASE(R3N_PROBE_BATCHED);
        default: return (int)hipErrorInvalidValue;
    }
#undef R3N_PROBE_CASE
    return (int)hipGetLastError();
}
