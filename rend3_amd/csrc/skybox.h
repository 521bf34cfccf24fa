// skybox.h -- the skybox node (rend3-routine/src/skybox.rs + skybox.wgsl): argument block and launcher of k_skybox (skybox.hip),
// and the layout of the cube-texture pool r3n_texture_cubes_write builds (r3n.hip).
//
// Cube pool: every cube is six faces in layer order +X, -X, +Y, -Y, +Z, -Z, each stored WITH A ONE-TEXEL BORDER: (N + 2) x (N + 2)
// RGBA8 words, row-major, interior texel (i, j) at (i + 1, j + 1).  The border of an edge holds the adjacent face's texels across
// that edge (filled on the host at upload), so the seamless footprint of DESIGN section 2 is a plain fetch; the four corner words
// of a face are never read -- the kernel forms a corner from the three texels that exist.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/r3n.h"

struct SkyboxArgs {
    const unsigned long long *vis;     // visibility keys, `samples` per pixel
    const r3n_frame_uniforms496 *fu;   // inv_origin_view_proj
    const uint32_t *texels;            // the bound cube's six bordered faces
    const float *decode;               // 512 entries: [0, 256) c / 255, [256, 512) sRGB8 -> linear (texture.h TextureArgs::decode)
    uint32_t n;                        // face extent in texels
    uint32_t srgb;                     // 1: R3N_TEXTURE_RGBA8_UNORM_SRGB
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
};
#define R3N_SKY_SAMPLES_ALL 0u
#define R3N_SKY_SAMPLES_EDGES 1u

// enqueues k_skybox over rows [row_begin, row_end); samples 1 | 4.  Returns the hipError_t of the launch.
extern "C" int r3n_internal_skybox(const SkyboxArgs *a, uint32_t samples, hipStream_t stream);
