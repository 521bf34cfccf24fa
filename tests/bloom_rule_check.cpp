// bloom_rule_check.cpp -- the host side of rend3_amd/csrc/bloom_rule.h as a stand-alone program (tests/test_bloom.py builds it
// with the address and undefined-behaviour sanitizers and compares what it prints with tests/bloom_reference.py).  Every number
// is read and printed as an unsigned integer: f32 and half bit patterns.
//   levels    < "W H max_levels" lines                  : "n w0 h0 w1 h1 ..." per line
//   bright    < params, then "r g b" half-bit lines     : the three half words of the bright pass per line
//     first line: scale intensity threshold knee scatter (f32 bits) max_levels
//   down      < "sw sh", then sw * sh "r g b" lines     : the (sw + 1) / 2 x (sh + 1) / 2 texels of one down step, three words each
//   up        < "cw ch w h scatter", cw * ch coarse texels, w * h texels of d : a = half(d + scatter * up(coarse)), three words each
//   composite < "v b intensity" lines (f32 bits)        : the bits of min(v + intensity * b, 65504)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rend3_amd/csrc/bloom_rule.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Image {
    int w = 0, h = 0;
    std::vector<uint16_t> t;  // three halves per texel
    bool read(int width, int height) {
        w = width; h = height;
        t.resize((size_t)w * (size_t)h * 3u);
        for (auto &v : t) {
            uint32_t u;
            if (scanf("%" SCNu32, &u) != 1 || u > 0xFFFFu) return false;
            v = (uint16_t)u;
        }
        return true;
    }
    float at(int x, int y, int c) const { return bloom_rule::half_to_f32(t[((size_t)y * (size_t)w + (size_t)x) * 3u + (size_t)c]); }
    void rgb(int x, int y, float out[3]) const {
        for (int c = 0; c < 3; ++c) out[c] = at(x, y, c);
    }
};

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "levels") {
        uint32_t W, H, m;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &W, &H, &m) == 3) {
            const bloom_rule::Levels l = bloom_rule::levels(W, H, m);
            printf("%u", l.n);
            for (uint32_t k = 0; k < l.n; ++k) printf(" %u %u", l.w[k], l.h[k]);
            printf("\n");
        }
        return 0;
    }
    if (cmd == "bright") {
        uint32_t w[5], max_levels;
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &w[0], &w[1], &w[2], &w[3], &w[4], &max_levels) != 6) return 2;
        const float scale = from_bits(w[0]);
        const bloom_rule::Params p = bloom_rule::make_params(from_bits(w[1]), from_bits(w[2]), from_bits(w[3]), from_bits(w[4]), max_levels);
        uint32_t c[3];
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &c[0], &c[1], &c[2]) == 3) {
            const uint16_t in[3] = {(uint16_t)c[0], (uint16_t)c[1], (uint16_t)c[2]};
            uint16_t out[3];
            bloom_rule::bright(in, scale, p, out);
            printf("%u %u %u\n", out[0], out[1], out[2]);
        }
        return 0;
    }
    if (cmd == "down") {
        int sw, sh;
        Image src;
        if (scanf("%d %d", &sw, &sh) != 2 || sw < 1 || sh < 1 || sw > 4096 || sh > 4096 || !src.read(sw, sh)) return 2;
        const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x) {
                uint16_t o[3];
                bloom_rule::down_at([&](int sx, int sy, float rgb[3]) { src.rgb(sx, sy, rgb); }, sw, sh, x, y, o);
                printf("%u %u %u\n", o[0], o[1], o[2]);
            }
        return 0;
    }
    if (cmd == "up") {
        int cw, ch, w, h;
        uint32_t sc;
        Image coarse, d;
        if (scanf("%d %d %d %d %" SCNu32, &cw, &ch, &w, &h, &sc) != 5 || cw < 1 || ch < 1 || w < 1 || h < 1 || cw > 4096 || ch > 4096 ||
            cw != (w + 1) / 2 || ch != (h + 1) / 2 || !coarse.read(cw, ch) || !d.read(w, h))
            return 2;
        const float scatter = from_bits(sc);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                float u[3];
                bloom_rule::up_at([&](int sx, int sy, float rgb[3]) { coarse.rgb(sx, sy, rgb); }, cw, ch, x, y, u);
                printf("%u %u %u\n", bloom_rule::up_store(d.at(x, y, 0), u[0], scatter), bloom_rule::up_store(d.at(x, y, 1), u[1], scatter),
                       bloom_rule::up_store(d.at(x, y, 2), u[2], scatter));
            }
        return 0;
    }
    if (cmd == "composite") {
        uint32_t v, b, i;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &v, &b, &i) == 3)
            printf("%u\n", exposure_rule::f32_bits(bloom_rule::composite(from_bits(v), from_bits(b), from_bits(i))));
        return 0;
    }
    fprintf(stderr, "usage: bloom_rule_check levels | bright | down | up | composite\n");
    return 2;
}
