// Stand-alone check of rend3_amd/csrc/texel_alloc.h (where r3n_textures_update places a texture) and texture_jobs.h (the job
// tables of the batched decode), built with the address and undefined-behaviour sanitizers and run as a child process by
// tests/test_texture_stream.py.  The allocator cases are checked here (a failed case prints FAIL and the exit status is 1); what
// the Python side restates -- the append offsets, the job tables -- is printed, one "name values" line each.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

#include "../rend3_amd/csrc/texel_alloc.h"
#include "../rend3_amd/csrc/texture_jobs.h"

using texel_alloc::align4;
using texel_alloc::NONE;
using texel_alloc::Pool;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL line_%d %s\n", __LINE__, #cond);             \
            ++failures;                                               \
        }                                                             \
    } while (0)

// xorshift: the same sequence everywhere
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void appends() {
    // sizes the Python side knows: i-th size = 1 + (i * 2654435761 mod 2^32 mod 997), every seventh one word
    Pool p;
    printf("appends");
    for (uint32_t i = 0; i < 300; ++i) {
        const uint64_t words = i % 7u == 0u ? 1u : 1u + ((uint32_t)(i * 2654435761u) % 997u);
        printf(" %llu", (unsigned long long)p.alloc(words));
    }
    printf(" %llu\n", (unsigned long long)p.end());
    // behind a whole-array write of 10 words: the next texture starts at 12
    Pool q;
    q.reset(10);
    CHECK(q.alloc(5) == 12 && q.end() == 17);
}

static void first_fit_and_coalescing() {
    Pool p;
    const uint64_t a = p.alloc(16), b = p.alloc(16), c = p.alloc(16), d = p.alloc(16), e = p.alloc(64), f = p.alloc(8);
    CHECK(a == 0 && b == 16 && c == 32 && d == 48 && e == 64 && f == 128);
    p.free(e, 64, false);
    p.free(b, 16, false);
    CHECK(p.holes().size() == 2);
    CHECK(p.alloc(8) == 16);  // both holes take it: the lowest address wins
    CHECK(p.alloc(8) == 24);
    p.free(16, 8, false);
    p.free(24, 8, false);
    CHECK(p.holes().size() == 2 && p.holes()[0].start == 16 && p.holes()[0].end == 32);
    // neighbours on both sides
    p.free(a, 16, false);
    CHECK(p.holes().size() == 2 && p.holes()[0].start == 0 && p.holes()[0].end == 32);
    p.free(d, 16, false);
    CHECK(p.holes().size() == 2 && p.holes()[1].start == 48 && p.holes()[1].end == 128);
    p.free(c, 16, false);
    CHECK(p.holes().size() == 1 && p.holes()[0].start == 0 && p.holes()[0].end == 128 && p.end() == 136);
    // free a, c, then b: one range
    Pool q;
    const uint64_t qa = q.alloc(10), qb = q.alloc(10), qc = q.alloc(10), qd = q.alloc(10);
    CHECK(qa == 0 && qb == 12 && qc == 24 && qd == 36);
    q.free(qa, 10, false);
    q.free(qc, 10, false);
    CHECK(q.holes().size() == 2);
    q.free(qb, 10, false);
    CHECK(q.holes().size() == 1 && q.holes()[0].start == 0 && q.holes()[0].end == 36);
    // exact fit (the padded hole takes up to 36 words) and one word too small
    CHECK(q.alloc(37) == 48);  // too small by one: appended behind d (46 -> 48)
    CHECK(q.alloc(36) == 0 && q.holes().empty());
    CHECK(q.end() == 85);
}

static void tail() {
    Pool p;
    const uint64_t a = p.alloc(10), b = p.alloc(7);
    CHECK(a == 0 && b == 12 && p.end() == 19);
    p.free(b, 7, false);  // a freed tail brings the mark down ...
    CHECK(p.end() == 12 && p.holes().empty());
    CHECK(p.alloc(3) == 12 && p.end() == 15);  // ... and is reused
    p.free(12, 3, false);
    p.free(a, 10, false);
    CHECK(p.end() == 0 && p.holes().empty());
    // a hole in front of a freed tail goes with it
    Pool q;
    q.alloc(4); q.alloc(4); q.alloc(4);
    q.free(4, 4, false);
    q.free(8, 4, false);
    CHECK(q.end() == 4 && q.holes().empty());
}

static void quarantine() {
    Pool p;
    p.alloc(16); p.alloc(16); p.alloc(16);
    p.free(0, 16, false);
    p.free(32, 16, true);  // the tail, parked: the mark stays, words behind it are fresh
    CHECK(p.end() == 48 && p.free_ranges() == 2);
    bool merged = true;
    CHECK(p.alloc(8, &merged) == 0 && !merged);  // a clean hole is preferred
    CHECK(p.alloc(8, &merged) == 8 && !merged);
    CHECK(p.alloc(8, &merged) == 32 && merged);  // none left: the parked tail is taken, the caller waits
    CHECK(p.end() == 40 && p.parked().empty());
    p.free(16, 16, true);
    CHECK(p.alloc(32, &merged) == 40 && !merged);  // the parked hole is too small: fresh words, no wait
    p.release();
    CHECK(p.holes().size() == 1 && p.holes()[0].start == 16);
}

static void limit() {
    Pool p;
    p.reset(0xFFFFFFF0ull);
    const Pool before = p;
    CHECK(p.alloc(16) == NONE);  // would end at 2^32
    CHECK(p.alloc(0x100000000ull) == NONE);
    CHECK(p.alloc(0) == NONE);
    CHECK(p.end() == before.end() && p.holes().empty() && p.parked().empty());
    CHECK(p.alloc(15) == 0xFFFFFFF0ull && p.end() == 0xFFFFFFFFull);
    CHECK(p.alloc(1) == NONE);
}

// 10^4 operations against a brute-force interval model
static void random_sequence() {
    Pool p;
    std::map<uint64_t, uint64_t> live;  // start -> words
    uint64_t allocs = 0, frees = 0;
    for (int op = 0; op < 10000; ++op) {
        const bool do_free = !live.empty() && (rnd() % 100u < 45u || live.size() > 200);
        if (do_free) {
            auto it = live.begin();
            std::advance(it, (long)(rnd() % live.size()));
            p.free(it->first, it->second, rnd() % 4u == 0u);
            live.erase(it);
            ++frees;
            if (rnd() % 16u == 0u) p.release();
            continue;
        }
        const uint64_t words = rnd() % 8u == 0u ? 1u + rnd() % 4u : 1u + rnd() % 300u;
        const uint64_t at = p.alloc(words);
        CHECK(at != NONE && (at & 3u) == 0u);
        // no overlap with any live range (padded)
        auto next = live.lower_bound(at);
        if (next != live.end()) CHECK(at + words <= next->first);
        if (next != live.begin()) {
            auto prev = std::prev(next);
            CHECK(prev->first + prev->second <= at);
        }
        CHECK(at + words <= p.end());
        live[at] = words;
        ++allocs;
        // holes and parked ranges are sorted, coalesced, 4-aligned, below the mark and disjoint from every live range
        for (const auto *list : {&p.holes(), &p.parked()}) {
            uint64_t last_end = 0;
            bool first = true;
            for (const texel_alloc::Range &r : *list) {
                CHECK((r.start & 3u) == 0u && (r.end & 3u) == 0u && r.start < r.end);
                CHECK(first || r.start > last_end);
                CHECK(r.start < p.end());
                auto nx = live.lower_bound(r.start);
                if (nx != live.end()) CHECK(r.end <= nx->first);
                if (nx != live.begin()) {
                    auto pv = std::prev(nx);
                    CHECK(pv->first + pv->second <= r.start);
                }
                last_end = r.end;
                first = false;
            }
        }
    }
    // with everything released, the first fit is the brute-force lowest gap
    p.release();
    for (int k = 0; k < 200; ++k) {
        const uint64_t words = 1u + rnd() % 64u, padded = align4(words);
        uint64_t want = NONE, cur = 0;
        for (const auto &kv : live) {
            if (kv.first >= cur + padded) { want = cur; break; }
            cur = align4(kv.first + kv.second);
        }
        if (want == NONE) want = live.empty() ? 0 : align4(live.rbegin()->first + live.rbegin()->second);
        const uint64_t at = p.alloc(words);
        CHECK(at == want);
        live[at] = words;
    }
    printf("random %llu %llu %zu\n", (unsigned long long)allocs, (unsigned long long)frees, live.size());
}

// the job tables of a mixed batch: every family's block, as words
static void jobs() {
    struct L { uint32_t format, w, h; };
    const L levels[] = {{R3N_TEXTURE_BC1_RGBA_UNORM, 8, 8}, {R3N_TEXTURE_BC1_RGBA_UNORM, 4, 4}, {R3N_TEXTURE_BC1_RGBA_UNORM, 2, 2},
                        {R3N_TEXTURE_BC1_RGBA_UNORM, 1, 1}, {R3N_TEXTURE_BC7_RGBA_UNORM, 64, 36}, {R3N_TEXTURE_R8_UNORM, 7, 5},
                        {R3N_TEXTURE_RGBA8_UNORM, 16, 16}, {R3N_TEXTURE_RG8_UNORM, 3, 3}, {R3N_TEXTURE_BC3_RGBA_UNORM, 5, 3},
                        {R3N_TEXTURE_BC6H_RGB_UFLOAT, 8, 8}, {R3N_TEXTURE_BC5_RG_SNORM, 33, 65}, {R3N_TEXTURE_RGBA16_FLOAT, 8, 4},
                        {R3N_TEXTURE_R32_FLOAT, 13, 11}, {R3N_TEXTURE_RGBA8_UNORM, 1, 1}, {R3N_TEXTURE_RGBA8_UNORM, 65, 1}};
    texture_jobs::Table t[texture_jobs::FAMILIES];
    uint64_t src = 0, dst = 0;
    for (const L &l : levels) {
        texture_jobs::add_level(t, l.format, l.w, l.h, src, (uint32_t)dst);
        src += 0x100000004ull;  // (a payload past 4 GiB: the offset takes both words)
        dst += (uint64_t)l.w * l.h * (texture_jobs::is_float(l.format) ? 4u : 1u);
    }
    CHECK(texture_jobs::finish(t));
    for (int f = 0; f < texture_jobs::FAMILIES; ++f) {
        printf("jobs_%d %zu %zu %zu %llu :", f, t[f].jobs.size(), t[f].layout.o_first, t[f].layout.o_inst, (unsigned long long)t[f].total_waves);
        for (uint32_t w : t[f].block) printf(" %u", w);
        printf("\n");
    }
    texture_jobs::Table none[texture_jobs::FAMILIES];
    CHECK(texture_jobs::finish(none) && none[0].block.empty() && none[3].total_waves == 0);
}

static bool refuses(const char *fault, const char *want) { return fault && std::string(fault) == want; }

// the chain walk against a chain written out by hand: 37 x 21, six levels; four pool words per texel for the words
static void chain_walk() {
    const uint32_t want[6][2] = {{37, 21}, {18, 10}, {9, 5}, {4, 2}, {2, 1}, {1, 1}};
    uint64_t texels = 0;
    for (uint32_t k = 0; k < 6; ++k) {
        const texture_jobs::Level l = texture_jobs::level_of(37, 21, k, 4);
        CHECK(l.w == want[k][0] && l.h == want[k][1] && l.words == 4ull * want[k][0] * want[k][1]);
        texels += (uint64_t)want[k][0] * want[k][1];
    }
    CHECK(texels == 777 + 180 + 45 + 8 + 2 + 1);
    CHECK(texture_jobs::chain_words(37, 21, 6, 1) == texels && texture_jobs::chain_words(37, 21, 6, 4) == 4 * texels);
    CHECK(texture_jobs::chain_words(37, 21, 1, 1) == 777 && texture_jobs::chain_words(37, 21, 0, 1) == 0);
    CHECK(texture_jobs::level_of(65535, 1, 15, 1).w == 1 && texture_jobs::level_of(65535, 1, 15, 1).h == 1);
    CHECK(texture_jobs::chain_words(65535, 65535, 1, 4) == 4ull * 65535 * 65535);  // past 2^32: counted in 64 bits
    // the shape check: 37 has six bits, so six levels and no more
    CHECK(texture_jobs::chain_fault(37, 21, 6) == nullptr && texture_jobs::chain_fault(1, 1, 1) == nullptr);
    CHECK(texture_jobs::chain_fault(65535, 65535, 16) == nullptr);
    CHECK(refuses(texture_jobs::chain_fault(37, 21, 7), "more mips than the extent has"));
    CHECK(refuses(texture_jobs::chain_fault(21, 37, 7), "more mips than the extent has"));
    CHECK(refuses(texture_jobs::chain_fault(1, 1, 2), "more mips than the extent has"));
    const uint32_t bad[5][3] = {{0, 4, 1}, {4, 0, 1}, {4, 4, 0}, {65536, 4, 1}, {4, 65536, 1}};
    for (const auto &b : bad) CHECK(refuses(texture_jobs::chain_fault(b[0], b[1], b[2]), "bad extent"));
}

int main() {
    chain_walk();
    appends();
    first_fit_and_coalescing();
    tail();
    quarantine();
    limit();
    random_sequence();
    jobs();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
