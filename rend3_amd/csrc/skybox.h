// skybox.h -- the skybox node (rend3-routine/src/skybox.rs + skybox.wgsl): argument block and launcher of k_skybox (skybox.hip),
// and the layout of the cube-texture pool the three upload entries build (r3n_texture_cubes_write, _encoded, _sources; cube_plan.h).
//
// Cube pool: every cube is six faces in layer order +X, -X, +Y, -Y, +Z, -Z, each stored WITH A ONE-TEXEL BORDER: (N + 2) x (N + 2)
// texels, row-major, interior texel (i, j) at (i + 1, j + 1).  The border of an edge holds the adjacent face's texels across
// that edge (filled by k_cube_assemble for every entry, from the edge table of cube_faces.h), so the seamless footprint of
// DESIGN section 2 is a plain fetch; the four corner texels of a face are never read -- the kernel forms a corner from the three
// texels that exist.
//
// A texel is one RGBA8 word (classes 0 / 1: Rgba8Unorm / Rgba8UnormSrgb words) or four f32 words (class 2, the formats
// texture_jobs::is_float names).  A cube with `mips` levels holds level 0's six bordered faces, then level 1's (extent
// n_1 = max(1, N >> 1)), and so on; every level and every cube starts on a 4-word boundary, so an
// f32 texel is one aligned 16-byte access.  cube_faces.h has the arithmetic (level_start, face_words) and the edge table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/r3n.h"

struct SkyboxArgs {
    const unsigned long long *vis;     // visibility keys, `samples` per pixel
    const r3n_frame_uniforms496 *fu;   // inv_origin_view_proj
    const uint32_t *texels;            // the bound cube: level 0's six bordered faces, then the further levels
    const float *decode;               // 512 entries: [0, 256) c / 255, [256, 512) sRGB8 -> linear (texture.h TextureArgs::decode)
    uint32_t n;                        // face extent in texels
    uint32_t srgb;                     // 1: sRGB-encoded RGBA8 words
    uint32_t width, height, row_begin, row_end;
    ushort4 *hdr_out;                  // Rgba16Float
    uchar4 *ldr_out;                   // the fused tonemap blit, as the resolve writes it
    const unsigned char *srgb_lut;
    uint32_t out_bgr;
    // four samples: where the resolve left the per-sample colours.
    //   R3N_SKY_SAMPLES_ALL    every sample of every pixel is in `samples` (a transparent pass follows, or the unsplit resolve);
    //                          the sky's samples are written there too
    //   R3N_SKY_SAMPLES_EDGES  split resolve: `samples` holds the pixels whose four ids differ; a pixel whose ids are all equal
    //                          has four equal samples whose value IS hdr_out (the box average of four equal halves is exact)
    ushort4 *samples;
    uint32_t samples_form;
    uint32_t mips;                     // levels of the bound cube (read by the instantiations with level selection only)
    // r3n_skybox_set_level: fixed != 0 draws a cube with levels at fixed_level (<= mips - 1) mixed with the next by fixed_frac (0 on
    // the last level) instead of selecting the level per pixel; read by the FIXED instantiations only
    uint32_t fixed, fixed_level;
    float fixed_frac;
};
#define R3N_SKY_SAMPLES_ALL 0u
#define R3N_SKY_SAMPLES_EDGES 1u

// enqueues k_skybox over rows [row_begin, row_end); samples 1 | 4; f32_class: the cube's texels are four f32 words.  A cube with
// one level of RGBA8 words runs the instantiation without level selection.  Returns the hipError_t of the launch.
extern "C" int r3n_internal_skybox(const SkyboxArgs *a, uint32_t samples, uint32_t f32_class, hipStream_t stream);
