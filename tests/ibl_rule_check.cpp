// ibl_rule_check.cpp -- rend3_amd/csrc/ibl_rule.h compiled alone (no HIP, no context) into a stand-alone program that
// tests/test_ibl.py builds under the address and undefined-behaviour sanitizers and runs as a child process.  It reads a case from
// the file it is given and prints the header's words; the test compares them with tests/ibl_reference.py.
//     prefilter FILE    "S L", then for k = 0 .. L - 1 the 6 n_k n_k lines "r g b" (f32 bits, linear-index order) of source level k
//                       -> "refused" when the rule takes no such (S, L); else per result level its texels "r g b a" (f32 bits),
//                          then the SH source level, then 27 lines: sh[m][ch] (f32 bits)
//     irradiance FILE   27 words sh[m][ch], a count, then count lines "x y z" (f32 bits) -> per line "r g b" (f32 bits)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rend3_amd/csrc/ibl_rule.h"

namespace R = ibl_rule;

static float f32_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) { return envlight_rule::f32_bits(f); }
static bool word(FILE *in, float &v) {
    unsigned w;
    if (fscanf(in, "%u", &w) != 1) return false;
    v = f32_of(w);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[2], "r");
    if (!in) return 2;
    int status = 0;
    if (!strcmp(argv[1], "prefilter")) {
        unsigned S, L;
        if (fscanf(in, "%u %u", &S, &L) != 2 || S == 0 || S > R::MAX_EXTENT) return 3;
        if (L < 2u || L > R::max_levels(S, R::MAX_LEVELS)) {
            printf("refused\n");
            fclose(in);
            return 0;
        }
        std::vector<std::vector<float>> src(L), dst(L);
        std::vector<const float *> src_p(L);
        std::vector<float *> dst_p(L);
        for (uint32_t k = 0; k < L && !status; ++k) {
            const uint32_t n = R::level_extent(S, k);
            src[k].resize((size_t)18u * n * n);
            dst[k].resize((size_t)24u * n * n);
            for (float &v : src[k])
                if (!word(in, v)) status = 3;
            src_p[k] = src[k].data();
            dst_p[k] = dst[k].data();
        }
        if (!status) {
            R::prefilter(src_p.data(), S, L, dst_p.data());
            for (uint32_t k = 0; k < L; ++k)
                for (size_t t = 0; t < dst[k].size(); t += 4u) printf("%u %u %u %u\n", bits_of(dst[k][t]), bits_of(dst[k][t + 1u]), bits_of(dst[k][t + 2u]), bits_of(dst[k][t + 3u]));
            const uint32_t sk = R::sh_level(S, L);
            float sh[9][4];
            R::sh9(src[sk].data(), R::level_extent(S, sk), sh);
            printf("%u\n", sk);
            for (int m = 0; m < 9; ++m)
                for (int ch = 0; ch < 3; ++ch) printf("%u\n", bits_of(sh[m][ch]));
        }
    } else if (!strcmp(argv[1], "irradiance")) {
        float sh[9][4];
        for (int m = 0; m < 9 && !status; ++m) {
            sh[m][3] = 0.0f;
            for (int ch = 0; ch < 3; ++ch)
                if (!word(in, sh[m][ch])) status = 3;
        }
        unsigned count = 0;
        if (!status && fscanf(in, "%u", &count) != 1) status = 3;
        for (unsigned i = 0; i < count && !status; ++i) {
            envlight_rule::vec3 n;
            if (!word(in, n.x) || !word(in, n.y) || !word(in, n.z)) {
                status = 3;
                break;
            }
            float e[3];
            R::irradiance(sh, n, e);
            printf("%u %u %u\n", bits_of(e[0]), bits_of(e[1]), bits_of(e[2]));
        }
    } else {
        status = 2;
    }
    fclose(in);
    return status;
}
