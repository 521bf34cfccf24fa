// exposure_rule_check.cpp -- the host side of rend3_amd/csrc/exposure_rule.h as a stand-alone program (tests/test_tonemap_ops.py
// builds it with the address and undefined-behaviour sanitizers and compares what it prints with tests/tonemap_reference.py).
//   tables                      : Lq[0..255], then the bits of E[0..256]
//   bins   < f32 bit patterns   : the bin of each (-1: excluded)
//   exp2   < f32 bit patterns   : the bits of exp2_lin of each
//   steps  < params, histograms : a sequence of frames from an invalid state; per frame S, N and the five state words
//     first line: exposure_ev white_sq key_log2 min_ev max_ev adapt (f32 bit patterns) low_permille high_permille
//     then one line of 256 counts per frame
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rend3_amd/csrc/exposure_rule.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    static int32_t lq[R3N_EXP_BINS];
    static float e[R3N_EXP_E_ENTRIES];
    exposure_rule::build_tables(lq, e);
    if (cmd == "tables") {
        for (int j = 0; j < R3N_EXP_BINS; ++j) printf("%d\n", lq[j]);
        for (int k = 0; k < R3N_EXP_E_ENTRIES; ++k) printf("%u\n", exposure_rule::f32_bits(e[k]));
        return 0;
    }
    if (cmd == "bins" || cmd == "exp2") {
        uint32_t u;
        while (scanf("%" SCNu32, &u) == 1) {
            if (cmd == "bins") printf("%d\n", exposure_rule::bin_of(from_bits(u)));
            else printf("%u\n", exposure_rule::f32_bits(exposure_rule::exp2_lin(from_bits(u), e)));
        }
        return 0;
    }
    if (cmd == "steps") {
        exposure_rule::Params p{};
        uint32_t w[6];
        if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5],
                  &p.low_permille, &p.high_permille) != 8)
            return 2;
        p.exposure_mode = 1u;
        p.exposure_ev = from_bits(w[0]); p.white_sq = from_bits(w[1]); p.key_log2 = from_bits(w[2]);
        p.min_ev = from_bits(w[3]); p.max_ev = from_bits(w[4]); p.adapt = from_bits(w[5]);
        exposure_rule::Step st{};
        std::vector<uint32_t> hist(R3N_EXP_BINS);
        for (;;) {
            int got = 0;
            for (; got < R3N_EXP_BINS; ++got)
                if (scanf("%" SCNu32, &hist[(size_t)got]) != 1) break;
            if (got == 0) break;
            if (got != R3N_EXP_BINS) return 2;
            int64_t S;
            uint64_t N;
            exposure_rule::meter_serial(hist.data(), lq, p, S, N);
            st = exposure_rule::step(st, S, N, p, e);
            printf("%" PRId64 " %" PRIu64 " %u %u %u %u %u\n", S, N, st.valid, exposure_rule::f32_bits(st.mean_log2), exposure_rule::f32_bits(st.target_ev),
                   exposure_rule::f32_bits(st.current_ev), exposure_rule::f32_bits(st.scale));
        }
        return 0;
    }
    fprintf(stderr, "usage: exposure_rule_check tables | bins | exp2 | steps\n");
    return 2;
}
