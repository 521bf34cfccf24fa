// envlight_rule_check.cpp -- rend3_amd/csrc/envlight_rule.h compiled alone (no HIP, no context) into a stand-alone program that
// tests/test_envlight.py builds under the address and undefined-behaviour sanitizers and runs as a child process.  It reads cases
// from stdin and prints the header's words; the test compares them with tests/envlight_reference.py.
//     geometry  lines "n"                                          -> per line 6 n n lines "ux uy uz w dqx dqy dqz qw" (f32 bits; integers)
//     extract   "n max_lights cone_cos_bits min_share_bits", then
//               6 n n lines "r g b" (f32 bits, linear-index order) -> the state and the outputs, one integer per line, in the order
//                                                                     of tests/envlight_reference.py flat()
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rend3_amd/csrc/envlight_rule.h"

namespace R = envlight_rule;

static float f32_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static void put(uint64_t v) { printf("%" PRIu64 "\n", v); }
static void put_signed(int64_t v) { printf("%" PRId64 "\n", v); }
static void put(const R::Sums &s) {
    for (int c = 0; c < 3; ++c) put(s.q[c]);
    put(s.qy);
    put(s.qw);
    put(s.texels);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const char *cmd = argv[1];
    if (!strcmp(cmd, "geometry")) {
        unsigned n;
        while (scanf("%u", &n) == 1)
            for (uint32_t t = 0; t < 6u * n * n; ++t) {
                const R::Geometry g = R::geometry_at(t, n);
                printf("%u %u %u %u %d %d %d %" PRIu64 "\n", R::f32_bits(g.u.x), R::f32_bits(g.u.y), R::f32_bits(g.u.z), R::f32_bits(g.w), R::dir_q(g.u.x),
                       R::dir_q(g.u.y), R::dir_q(g.u.z), R::quantise_w(g.w));
            }
    } else if (!strcmp(cmd, "extract")) {
        unsigned n, max_lights, cone_bits, share_bits;
        if (scanf("%u %u %u %u", &n, &max_lights, &cone_bits, &share_bits) != 4 || n == 0 || n > R::MAX_EXTENT || max_lights > R::MAX_LIGHTS) return 3;
        std::vector<float> rgb((size_t)18u * n * n);
        for (auto &v : rgb) {
            unsigned w;
            if (scanf("%u", &w) != 1) return 3;
            v = f32_of(w);
        }
        const R::Params p{n, max_lights, f32_of(cone_bits), R::share_floor(f32_of(share_bits))};
        R::State s;
        R::extract(rgb.data(), p, s);
        const R::Outputs o = R::outputs(s, p);
        put(s.emax_bits);
        put(s.total);
        for (uint32_t k = 0; k <= R::MAX_LIGHTS; ++k) put(s.seed[k]);
        for (uint32_t k = 0; k < R::MAX_LIGHTS; ++k) {
            for (uint32_t step = 0; step < R::SHIFT_STEPS; ++step)
                for (int a = 0; a < 6; ++a) put_signed(s.shift[k][step][a]);
            put(s.light[k]);
        }
        put(o.n_lights);
        put(o.ran);
        put_signed(o.scale_exp);
        for (int c = 0; c < 4; ++c) put(R::f32_bits(o.ambient[c]));
        put(o.remainder);
        for (uint32_t k = 0; k < R::MAX_LIGHTS; ++k) {
            const R::LightOut &l = o.lights[k];
            put(R::f32_bits(l.direction.x));
            put(R::f32_bits(l.direction.y));
            put(R::f32_bits(l.direction.z));
            put(R::f32_bits(l.solid_angle));
            for (int c = 0; c < 3; ++c) put(R::f32_bits(l.irradiance[c]));
            put(l.texels);
        }
    } else {
        return 2;
    }
    return 0;
}
