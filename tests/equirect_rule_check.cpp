// equirect_rule_check.cpp -- rend3_amd/csrc/equirect_rule.h compiled alone (no HIP, no context) into a stand-alone program that
// tests/test_equirect.py builds under the address and undefined-behaviour sanitizers and runs as a child process.  It reads cases
// from stdin and prints the header's words; the test compares them with tests/equirect_reference.py.
//     rgbe      lines "r g b e"                      -> four f32 words per line
//     atan2     lines "ybits xbits"                  -> one f32 word per line
//     taps      lines "f n W H"                      -> per line n * n lines "c0 c1 r0 r1 fxbits fybits", row-major
//     faces     "n W H", then W * H lines of 4 words -> 6 * n * n lines of 4 words
//     chain     "s", then s * s lines of 4 words     -> d * d lines of 4 words
//     plan      lines "T count N0 m0 N1 m1 ..."      -> "faces levels tail launches tail_from0 tail_from1 ..."
//     sweep     (no input)                           -> "E_bits max_poly_error max_atan2_error" (errors in turns, as doubles)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rend3_amd/csrc/equirect_rule.h"

namespace R = equirect_rule;

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static void print4(const R::vec4 &v) { printf("%u %u %u %u\n", bits(v.x), bits(v.y), bits(v.z), bits(v.w)); }
static bool read4(R::vec4 &v) {
    unsigned a, b, c, d;
    if (scanf("%u %u %u %u", &a, &b, &c, &d) != 4) return false;
    v = R::vec4{R::bits_to_f32(a), R::bits_to_f32(b), R::bits_to_f32(c), R::bits_to_f32(d)};
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const char *cmd = argv[1];
    if (!strcmp(cmd, "rgbe")) {
        unsigned r, g, b, e;
        while (scanf("%u %u %u %u", &r, &g, &b, &e) == 4) print4(R::rgbe_decode(r | g << 8 | b << 16 | e << 24));
    } else if (!strcmp(cmd, "atan2")) {
        unsigned y, x;
        while (scanf("%u %u", &y, &x) == 2) printf("%u\n", bits(R::atan2_turns(R::bits_to_f32(y), R::bits_to_f32(x))));
    } else if (!strcmp(cmd, "taps")) {
        unsigned f, n, W, H;
        while (scanf("%u %u %u %u", &f, &n, &W, &H) == 4)
            for (unsigned j = 0; j < n; ++j)
                for (unsigned i = 0; i < n; ++i) {
                    const R::Taps t = R::face_taps(f, i, j, n, W, H);
                    printf("%u %u %u %u %u %u\n", t.c0, t.c1, t.r0, t.r1, bits(t.fx), bits(t.fy));
                }
    } else if (!strcmp(cmd, "faces")) {
        unsigned n, W, H;
        if (scanf("%u %u %u", &n, &W, &H) != 3) return 3;
        std::vector<R::vec4> src((size_t)W * H);
        for (auto &v : src)
            if (!read4(v)) return 3;
        for (unsigned f = 0; f < 6; ++f)
            for (unsigned j = 0; j < n; ++j)
                for (unsigned i = 0; i < n; ++i) {
                    const R::Taps t = R::face_taps(f, i, j, n, W, H);
                    print4(R::bilinear(src[(size_t)t.r0 * W + t.c0], src[(size_t)t.r0 * W + t.c1], src[(size_t)t.r1 * W + t.c0],
                                       src[(size_t)t.r1 * W + t.c1], t.fx, t.fy));
                }
    } else if (!strcmp(cmd, "chain")) {
        unsigned s;
        if (scanf("%u", &s) != 1) return 3;
        std::vector<R::vec4> src((size_t)s * s);
        for (auto &v : src)
            if (!read4(v)) return 3;
        const uint32_t d = R::half_extent(s);
        for (uint32_t y = 0; y < d; ++y)
            for (uint32_t x = 0; x < d; ++x) print4(R::chain_texel([&](uint32_t k) { return src.at(k); }, x, y, s, d));
    } else if (!strcmp(cmd, "plan")) {
        unsigned T, count;
        while (scanf("%u %u", &T, &count) == 2) {
            std::vector<uint32_t> n(count), m(count);
            for (unsigned i = 0; i < count; ++i)
                if (scanf("%u %u", &n[i], &m[i]) != 2) return 3;
            const R::Plan p = R::plan(n.data(), m.data(), count, T);
            printf("%u %u %u %u", p.faces, p.levels, p.tail, R::plan_launches(p));
            for (unsigned i = 0; i < count; ++i) printf(" %u", R::tail_from(n[i], m[i], T));
            printf("\n");
        }
    } else if (!strcmp(cmd, "sweep")) {
        const double two_pi = 6.283185307179586476925286766559;
        double worst_poly = 0.0, worst_atan2 = 0.0;
        for (uint32_t k = 0; k <= (1u << 22); ++k) {
            const float c = (float)k / 4194304.0f;
            const float ts[3] = {c, std::nextafterf(c, 0.0f), std::nextafterf(c, 1.0f)};
            for (float t : ts) {
                const double e = std::fabs((double)R::atan_turns_poly(t) - std::atan((double)t) / two_pi);
                if (e > worst_poly) worst_poly = e;
            }
        }
        for (uint32_t k = 0; k < (1u << 20); ++k) {  // the whole circle, at three radii
            const double a = two_pi * ((double)k + 0.37) / 1048576.0;
            for (double r : {1.0, 3.7e-3, 911.0}) {
                const float y = (float)(r * std::sin(a)), x = (float)(r * std::cos(a));
                double e = std::fabs((double)R::atan2_turns(y, x) - std::atan2((double)y, (double)x) / two_pi);
                if (e > 0.5) e = 1.0 - e;  // (-0.5 and 0.5 are one angle)
                if (e > worst_atan2) worst_atan2 = e;
            }
        }
        printf("%u %.9g %.9g\n", bits(R::ATAN2_TURNS_E), worst_poly, worst_atan2);
    } else {
        return 2;
    }
    return 0;
}
