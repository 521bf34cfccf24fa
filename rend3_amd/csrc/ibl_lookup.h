// ibl_lookup.h -- the two lookups of a prefiltered environment (r3n_environment_prefilter, ibl_rule.h): the specular chain by
// direction and roughness, and the ambient radiance of the nine SH coefficients by normal.  Device functions for a later resolve;
// today r3n_environment_probe (ibl.hip) is their only caller, and tests/ibl_reference.py restates them in numpy.
#pragma once
#include "cube_sample.h"
#include "ibl_rule.h"

struct IblCube {
    const uint32_t *texels;  // the cube's first pool word: level 0's six bordered faces, then the further levels
    const float *tab;        // the decode table of its class (RGBA8 classes only)
    uint32_t n0, mips;
};
struct IblSh {
    float sh[9][4];
};

// lod = roughness (mips - 1), clamped to [0, mips - 1] (a NaN roughness gives 0); level = floor(lod), fraction = lod - level; then
// cube_sample_level.  Level k of a chain of L levels was filtered for the roughness k / (L - 1).
template <bool F32>
R3N_DEV void ibl_specular(const IblCube &c, const float dir[3], float roughness, float out[3], uint32_t &level, float &frac) {
    const float top = (float)(c.mips - 1u);
    float lod = roughness * top;
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > top) lod = top;
    level = (uint32_t)lod;
    frac = lod - (float)level;
    cube_sample_level<F32>(c.texels, c.tab, c.n0, c.mips, dir, level, frac, out);
}
// E(n) / pi
R3N_DEV void ibl_irradiance(const IblSh &s, const float n[3], float out[3]) { ibl_rule::irradiance(s.sh, envlight_rule::vec3{n[0], n[1], n[2]}, out); }
