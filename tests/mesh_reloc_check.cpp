// Stand-alone check of rend3_amd/csrc/mesh_reloc.h (which address of an object record goes where after r3n_mesh_compact) together
// with the planner and the allocator it rides on (texel_compact.h, texel_alloc.h), built with the address and undefined-behaviour
// sanitizers and run as a child process by tests/test_mesh_stream.py.  A failed case prints FAIL and the exit status is 1.
//
//   mesh_reloc_check                 every section below; one "name values" line each
//   mesh_reloc_check pool OP...      drives a Pool the way the library does and prints what it hands out, one line per op:
//                                    A<words> add a block ("A offset merged"), R<k> remove the k-th added block (parked),
//                                    S a full wait (parked ranges become holes), C<max_words>:<stage_words> a compaction
//                                    ("C moves passes launches end" and one "M old new padded" line per move, in WORDS).
//                                    tests/test_mesh_stream_gpu.py compares the device with it.
//
// Sections of the plain run:
//   random      layouts of blocks and holes: the plan executed on a host word array, a host array of records patched through
//               mesh_reloc.h -- every live block's words arrive intact, every field that named word k of a live block names word
//               k of it afterwards, every other field is unchanged
//   case_*      the edge list of the lookup, printed as "T <entries: src end shift> F <7 fields> O <7 fields after>" so that the
//               numpy restatement (tests/mesh_reloc_reference.py) is held against the same cases
//   budget      a budget that stops in front of a block
//   pool_*      alloc / remove / alloc through Pool at mesh sizes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../rend3_amd/csrc/mesh_reloc.h"
#include "../rend3_amd/csrc/texel_compact.h"

using texel_alloc::align4;
using texel_alloc::Pool;
using namespace texel_compact;
using mesh_reloc::Entry;
using mesh_reloc::INVALID;

static int failures = 0;
static const char *context = "";
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            if (failures < 20) printf("FAIL line_%d %s [%s]\n", __LINE__, #cond, context);      \
            ++failures;                                                                         \
        }                                                                                       \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

struct Item {
    bool hole;
    uint64_t words;
};
static std::vector<Live> live_of(const std::vector<Item> &items) {
    std::vector<Live> live;
    uint64_t cur = 0;
    for (const Item &it : items) {
        const uint64_t at = align4(cur);
        if (!it.hole) live.push_back(Live{at, it.words, (uint32_t)live.size()});
        cur = at + it.words;
    }
    return live;
}

// the plan's launches, each as the device runs it: no launch reads a word it writes, so segment by segment in order is one of the
// valid executions (texel_compact_check.cpp holds the planner to every order)
static void execute(const Plan &p, std::vector<uint32_t> &pool) {
    std::vector<uint32_t> scratch((size_t)p.scratch_words + 4u, 0xDEADBEEFu);
    for (const Launch &l : p.launches) {
        std::vector<uint32_t> &from = l.kind == SCATTER ? scratch : pool, &to = l.kind == GATHER ? scratch : pool;
        for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s) {
            const Segment &g = p.segments[s];
            CHECK(g.src + g.words <= from.size() && g.dst + g.words <= to.size());
            if (g.src + g.words > from.size() || g.dst + g.words > to.size()) continue;
            for (uint64_t k = 0; k < g.words; ++k) to[g.dst + k] = from[g.src + k];
        }
    }
}

static std::vector<Entry> table_of(const Plan &p) {
    std::vector<mesh_reloc::Move> moves;
    for (size_t i = p.moves.size(); i-- > 0;) moves.push_back(mesh_reloc::Move{p.moves[i].src, p.moves[i].dst, p.moves[i].words});  // (any order in)
    std::vector<Entry> table;
    CHECK(mesh_reloc::build_table(moves, table));
    for (size_t i = 1; i < table.size(); ++i) CHECK(table[i - 1].end <= table[i].src);
    return table;
}

struct Stats {
    uint64_t cases = 0, moved_blocks = 0, fields_in_blocks = 0, fields_elsewhere = 0, budgeted = 0, staged = 0, records = 0, hint_hits = 0;
};

// one layout: plan, execute, patch, compare
static void check_layout(const std::vector<Live> &live, uint64_t max_words, uint64_t stage_words, Stats &st) {
    const Plan p = plan(live, max_words, stage_words);
    uint64_t reach = 0;
    for (const Live &t : live) reach = std::max(reach, align4(t.start + t.words));
    std::vector<uint32_t> pool((size_t)reach + 8u);
    for (uint32_t &w : pool) w = (uint32_t)rnd();
    const std::vector<uint32_t> before = pool;
    // ---- records: every field names word k of a live block (padding included), a hole word, the word past the end, or INVALID
    struct Named {
        int block;  // index into `live`, -1: none
        uint64_t k;
        uint32_t low;
    };
    const size_t n_rec = 8 + rnd() % 40;
    std::vector<uint32_t> recs(n_rec * 32u);
    std::vector<Named> named(n_rec * 7u);
    std::vector<uint8_t> is_live((size_t)reach + 8u, 0);
    for (const Live &t : live)
        for (uint64_t w = t.start; w < align4(t.start + t.words); ++w) is_live[w] = 1;
    for (size_t r = 0; r < n_rec; ++r) {
        for (uint32_t w = 0; w < 32u; ++w) recs[r * 32u + w] = (uint32_t)rnd();
        for (uint32_t f = 0; f < 7u; ++f) {
            Named nm{-1, 0, f ? (uint32_t)(rnd() % 4u) : 0u};
            uint32_t word;
            const uint64_t pick = rnd() % 10u;
            if (pick == 0 || live.empty()) word = INVALID;
            else if (pick == 1) {
                word = (uint32_t)(rnd() % (reach + 8u));
                if (is_live[word]) {  // (named below by the block that holds it)
                    for (size_t b = 0; b < live.size(); ++b)
                        if (word >= live[b].start && word < align4(live[b].start + live[b].words)) nm = Named{(int)b, word - live[b].start, nm.low};
                }
            } else {
                // a plain object names ONE block with every field; a skinned or morphed one two or three
                const size_t b = (pick < 7 && f) ? (size_t)named[r * 7u + f - 1u].block : rnd() % live.size();
                const size_t bb = b < live.size() ? b : rnd() % live.size();
                const uint64_t padded = align4(live[bb].words);
                const uint64_t k = rnd() % 4u == 0 ? (rnd() % 2u ? 0 : padded - 1u) : rnd() % padded;
                nm = Named{(int)bb, k, nm.low};
                word = (uint32_t)(live[bb].start + k);
            }
            named[r * 7u + f] = nm;
            uint32_t value = word;
            if (f && word != INVALID) value = (word << 2) | nm.low;
            if (f && word == INVALID) value = INVALID;
            recs[r * 32u + (f ? 22u + f : 20u)] = value;
        }
    }
    const std::vector<uint32_t> recs_before = recs;
    // ---- the device's part, on the host
    execute(p, pool);
    const std::vector<Entry> table = table_of(p);
    for (size_t r = 0; r < n_rec; ++r) mesh_reloc::patch_record(table.data(), (uint32_t)table.size(), recs.data() + r * 32u);
    // ---- every live block's words arrive intact (its padding is moved with it, but holds nothing)
    std::vector<uint64_t> new_start(live.size());
    CHECK(p.live.size() == live.size());
    for (const Live &t : p.live) new_start[t.slot] = t.start;
    for (size_t b = 0; b < live.size(); ++b) {
        const Live &t = live[b];
        CHECK(t.slot == b && new_start[b] <= t.start && new_start[b] % 4u == 0);
        for (uint64_t k = 0; k < t.words; ++k) CHECK(pool[new_start[b] + k] == before[t.start + k]);
        st.moved_blocks += new_start[b] != t.start;
    }
    // ---- the fields
    for (size_t r = 0; r < n_rec; ++r) {
        for (uint32_t w = 0; w < 32u; ++w)
            if (w != 20u && (w < 23u || w > 28u)) CHECK(recs[r * 32u + w] == recs_before[r * 32u + w]);
        for (uint32_t f = 0; f < 7u; ++f) {
            const Named &nm = named[r * 7u + f];
            const uint32_t got = recs[r * 32u + (f ? 22u + f : 20u)], was = recs_before[r * 32u + (f ? 22u + f : 20u)];
            if (nm.block < 0) {
                CHECK(got == was);
                ++st.fields_elsewhere;
            } else {
                const uint32_t word = (uint32_t)(new_start[nm.block] + nm.k);
                CHECK(got == (f ? (word << 2) | nm.low : word));
                ++st.fields_in_blocks;
            }
        }
    }
    ++st.cases;
    st.records += n_rec;
    st.budgeted += max_words != 0;
    for (const Pass &pass : p.passes) st.staged += pass.staged;
}

static void random_section() {
    Stats st;
    for (int c = 0; c < 3000; ++c) {
        std::vector<Item> items;
        const size_t n = 1 + rnd() % 24;
        for (size_t i = 0; i < n; ++i) {
            if (rnd() % 3u == 0) items.push_back(Item{true, 4u * (1 + rnd() % (rnd() % 4u ? 8u : 600u))});
            const uint64_t sizes[] = {1, 3, 4, 5, 8, 1020, 1024, 1028};
            items.push_back(Item{false, rnd() % 3u ? sizes[rnd() % 8u] : 1 + rnd() % 1500u});
        }
        const uint64_t stages[] = {256, 260, 4096};
        check_layout(live_of(items), rnd() % 3u == 0 ? 4u * (rnd() % 800u + 1) : 0, stages[rnd() % 3u], st);
    }
    context = "hand-made";
    const std::vector<std::vector<Item>> hand = {
        {},
        {{false, 16}},
        {{true, 4}, {false, 1000}},                                  // a 4-word hole in front of a long block: staged
        {{true, 1000}, {false, 1000}},                               // shift == length: one direct launch
        {{false, 16}, {true, 8}, {false, 100}, {false, 40}, {true, 12}, {false, 64}},
        {{false, 1}, {true, 4}, {false, 3}, {true, 4}, {false, 5}, {true, 4}, {false, 1028}},
    };
    for (const auto &items : hand)
        for (uint64_t stage : {256u, 4096u}) check_layout(live_of(items), 0, stage, st);
    context = "";
    printf("random %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)st.cases, (unsigned long long)st.moved_blocks,
           (unsigned long long)st.fields_in_blocks, (unsigned long long)st.fields_elsewhere, (unsigned long long)st.budgeted,
           (unsigned long long)st.staged, (unsigned long long)st.records);
}

// prints a case for the numpy restatement and checks it against `want`
static void print_case(const char *name, const std::vector<Entry> &table, const uint32_t in[7], const uint32_t want[7]) {
    context = name;
    uint32_t rec[32];
    for (uint32_t w = 0; w < 32u; ++w) rec[w] = 0xA5A50000u + w;
    rec[20] = in[0];
    for (uint32_t a = 0; a < 6u; ++a) rec[23 + a] = in[1 + a];
    const uint32_t changed = mesh_reloc::patch_record(table.data(), (uint32_t)table.size(), rec);
    printf("case_%s T", name);
    if (table.size() <= 4)
        for (const Entry &e : table) printf(" %u %u %u", e.src, e.end, e.shift);
    else printf(" ramp %zu", table.size());  // entry i: src = 8 + 16 i, end = src + 8, shift = 8 + 4 i
    printf(" F");
    for (uint32_t f = 0; f < 7u; ++f) printf(" %u", in[f]);
    printf(" O %u", rec[20]);
    for (uint32_t a = 0; a < 6u; ++a) printf(" %u", rec[23 + a]);
    printf("\n");
    CHECK(rec[20] == want[0]);
    for (uint32_t a = 0; a < 6u; ++a) CHECK(rec[23 + a] == want[1 + a]);
    for (uint32_t f = 0; f < 7u; ++f) CHECK(((changed >> f) & 1u) == (in[f] != want[f]));
    for (uint32_t w = 0; w < 32u; ++w)
        if (w != 20u && (w < 23u || w > 28u)) CHECK(rec[w] == 0xA5A50000u + w);
    context = "";
}

static std::vector<Entry> ramp(size_t n) {
    std::vector<Entry> t;
    for (size_t i = 0; i < n; ++i) t.push_back(Entry{(uint32_t)(8 + 16 * i), (uint32_t)(16 + 16 * i), (uint32_t)(8 + 4 * i), 0u});
    return t;
}

static void edge_section() {
    const uint32_t I = INVALID;
    // B0 [0, 16) stays; B1 [32, 44) (10 words, padded 12) -> 16; B2 [64, 72) -> 28; B3 [100, 104) -> 36
    const std::vector<Entry> t3 = {{32, 44, 16, 0}, {64, 72, 36, 0}, {100, 104, 64, 0}};
    {   // a plan gives exactly this table
        const Plan p = plan({Live{0, 16, 0}, Live{32, 10, 1}, Live{64, 8, 2}, Live{100, 4, 3}}, 0, 256);
        const std::vector<Entry> t = table_of(p);
        CHECK(t.size() == 3);
        for (size_t i = 0; i < t.size() && i < 3; ++i) CHECK(t[i].src == t3[i].src && t[i].end == t3[i].end && t[i].shift == t3[i].shift);
    }
    // first word, last word, last padding word, one past the padding, one before the start (first_index in words; the rest in bytes)
    { const uint32_t in[7] = {32, 32 * 4, 41 * 4, 43 * 4, 44 * 4, 31 * 4, I}, want[7] = {16, 16 * 4, 25 * 4, 27 * 4, 44 * 4, 31 * 4, I};
      print_case("block_edges", t3, in, want); }
    { const uint32_t in[7] = {41, 43 * 4 + 3, 44 * 4 + 1, 31 * 4 + 3, 32 * 4 + 2, I, I}, want[7] = {25, 27 * 4 + 3, 44 * 4 + 1, 31 * 4 + 3, 16 * 4 + 2, I, I};
      print_case("low_bits", t3, in, want); }
    { const uint32_t in[7] = {I, I, I, I, I, I, I}; print_case("invalid", t3, in, in); }
    { const uint32_t in[7] = {5, 0, 15 * 4, 16 * 4, 8 * 4, I, I}; print_case("below_first_move", t3, in, in); }  // B0, and the hole behind it
    { const uint32_t in[7] = {50, 50 * 4, 72 * 4, 99 * 4, 104 * 4, 2000 * 4, I}; print_case("holes", t3, in, in); }
    { const uint32_t in[7] = {33, 64 * 4, 100 * 4, 71 * 4, 103 * 4, 34 * 4, 65 * 4}, want[7] = {17, 28 * 4, 36 * 4, 35 * 4, 39 * 4, 18 * 4, 29 * 4};
      print_case("three_moves", t3, in, want); }
    {   // INVALID stays INVALID whatever the table says: a table that covers the top of the address space
        const std::vector<Entry> top = {{0xFFFFFFF0u, 0xFFFFFFFFu, 16, 0}};
        const uint32_t in[7] = {I, I, 0xFFFFFFF0u, I, I, I, I}, want[7] = {I, I, 0xFFFFFFF0u, I, I, I, I};
        print_case("invalid_under_a_table", top, in, want);
        const uint32_t in2[7] = {0xFFFFFFF0u, 0, 0, 0, 0, 0, 0}, want2[7] = {0xFFFFFFE0u, 0, 0, 0, 0, 0, 0};
        print_case("top_words", top, in2, want2);
    }
    { const uint32_t in[7] = {32, 32 * 4, 64 * 4, 100 * 4, 0, I, 7}; print_case("table_0", {}, in, in); }
    { const uint32_t in[7] = {32, 43 * 4, 64 * 4, 31 * 4, 44 * 4, I, 7}, want[7] = {16, 27 * 4, 64 * 4, 31 * 4, 44 * 4, I, 7};
      print_case("table_1", {t3[0]}, in, want); }
    { const uint32_t in[7] = {71, 43 * 4, 64 * 4, 100 * 4, 72 * 4, I, 63 * 4}, want[7] = {35, 27 * 4, 28 * 4, 100 * 4, 72 * 4, I, 63 * 4};
      print_case("table_2", {t3[0], t3[1]}, in, want); }
    // at and either side of the constant where the kernel's lookup changes form: first, last and middle entries, and their gaps
    for (size_t n : {(size_t)mesh_reloc::LDS_TABLE_ENTRIES - 1u, (size_t)mesh_reloc::LDS_TABLE_ENTRIES, (size_t)mesh_reloc::LDS_TABLE_ENTRIES + 1u}) {
        const std::vector<Entry> t = ramp(n);
        const uint32_t last = (uint32_t)n - 1u, mid = (uint32_t)n / 2u;
        const uint32_t in[7] = {8, (8 + 16 * last) * 4, (15 + 16 * last) * 4 + 1, (16 + 16 * last) * 4, 7 * 4, (8 + 16 * mid + 3) * 4 + 2, (16 * mid + 7) * 4};
        const uint32_t want[7] = {0, (8 + 16 * last - (8 + 4 * last)) * 4, (15 + 16 * last - (8 + 4 * last)) * 4 + 1, (16 + 16 * last) * 4, 7 * 4,
                                  (8 + 16 * mid + 3 - (8 + 4 * mid)) * 4 + 2, (16 * mid + 7) * 4};
        const std::string name = "table_" + std::to_string(n);
        print_case(name.c_str(), t, in, want);
    }
    printf("lds_table_entries %u\n", mesh_reloc::LDS_TABLE_ENTRIES);
}

static void budget_section() {
    context = "budget";
    // H8 T16 T16 H20 T16 with 32 words of budget: the first two move, the plan stops in front of the third
    const std::vector<Live> live = live_of({{true, 8}, {false, 16}, {false, 16}, {true, 20}, {false, 16}});
    const Plan p = plan(live, 32, 256);
    CHECK(p.moves.size() == 2 && p.words_moved == 32 && p.live.size() == 3 && p.live[2].start == live[2].start && p.end == live[2].start + 16);
    const std::vector<Entry> t = table_of(p);
    uint32_t rec[32] = {};
    rec[20] = (uint32_t)live[2].start + 3;                                 // the block behind the budget: unchanged
    rec[23] = (uint32_t)live[0].start * 4; rec[24] = (uint32_t)live[1].start * 4 + 60;  // the two that moved
    rec[25] = (uint32_t)(live[1].start + 16) * 4;                           // the hole in front of the third block
    rec[26] = rec[27] = rec[28] = INVALID;
    mesh_reloc::patch_record(t.data(), (uint32_t)t.size(), rec);
    CHECK(rec[20] == live[2].start + 3 && rec[23] == 0 && rec[24] == 16 * 4 + 60 && rec[25] == (live[1].start + 16) * 4 && rec[26] == INVALID);
    Pool pool;
    pool.reset(live[2].start + 16);
    rebuild(pool, p);
    CHECK(pool.holes().size() == 1 && pool.holes()[0].start == 32 && pool.holes()[0].end == live[2].start);
    const Plan one_short = plan(live, 31, 256);  // 31 < 32: only the first block fits
    CHECK(one_short.moves.size() == 1 && one_short.live[1].start == live[1].start);
    printf("budget %zu %llu %llu %zu\n", p.moves.size(), (unsigned long long)p.words_moved, (unsigned long long)p.end, one_short.moves.size());
    context = "";
}

static void pool_section() {
    context = "pool";
    Pool pool;
    // ascending appends: what the append cursor gave
    const uint64_t sizes[] = {4, 8, 1020, 1024, 1028, 1, 3, 5};
    uint64_t at[8], cur = 0;
    for (int i = 0; i < 8; ++i) {
        at[i] = pool.alloc(sizes[i]);
        CHECK(at[i] == align4(cur));
        cur = at[i] + sizes[i];
    }
    printf("pool_appends");
    for (int i = 0; i < 8; ++i) printf(" %llu", (unsigned long long)at[i]);
    printf("\n");
    // remove the 4-word and the 1024-word block while frames are in flight: parked.  What no parked range takes goes behind the
    // mark without a merge (fresh words, no wait)
    pool.free(at[0], 4, true);
    pool.free(at[3], 1024, true);
    bool merged = true;
    const uint64_t fresh = pool.alloc(2000, &merged);
    CHECK(fresh == align4(cur) && !merged && pool.parked().size() == 2);
    cur = fresh + 2000;
    // what a parked range takes is placed there, and says so: the caller waits once, and every parked range is a hole afterwards
    const uint64_t a4 = pool.alloc(3, &merged);       // 3 words pad to 4: the 4-word range
    CHECK(a4 == at[0] && merged && pool.parked().empty() && pool.holes().size() == 1);
    const uint64_t a1028 = pool.alloc(1028, &merged); // does not fit the 1024-word hole: appended
    CHECK(a1028 == align4(cur) && !merged);
    cur = a1028 + 1028;
    const uint64_t a1020 = pool.alloc(1020, &merged); // fits it, leaves 4 words
    CHECK(a1020 == at[3] && !merged);
    const uint64_t rest = pool.alloc(4, &merged);
    CHECK(rest == at[3] + 1020 && !merged && pool.holes().empty());
    // a parked hole is taken only when nothing else fits, and says so
    pool.free(at[2], 1020, true);
    pool.free(a1028, 1028, true);  // the tail: the mark stays until the merge
    CHECK(pool.end() == cur);
    const uint64_t again = pool.alloc(1024, &merged);  // the parked 1020-word range cannot take it; the parked tail can, after a merge
    CHECK(again == a1028 && merged && pool.parked().empty());
    const uint64_t late = pool.alloc(1020, &merged);   // the merge made the 1020-word range a clean hole
    CHECK(late == at[2] && !merged);
    printf("pool_reuse %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)fresh, (unsigned long long)a4, (unsigned long long)a1028,
           (unsigned long long)a1020, (unsigned long long)rest, (unsigned long long)again, (unsigned long long)late);
    // 1024 +- 4 around a 1024-word hole
    for (uint64_t want : {1020u, 1024u, 1028u}) {
        Pool q;
        const uint64_t x = q.alloc(8), h = q.alloc(1024), y = q.alloc(8);
        (void)x; (void)y;
        q.free(h, 1024, false);
        const uint64_t got = q.alloc(want);
        CHECK(want <= 1024 ? got == h : got == align4(y + 8));
        CHECK(q.free_ranges() == (want == 1020 ? 1u : want == 1024 ? 0u : 1u));
        printf("pool_hole_1024_takes_%llu %llu %zu\n", (unsigned long long)want, (unsigned long long)got, q.free_ranges());
    }
    context = "";
}

static int pool_mode(int argc, char **argv) {
    Pool pool;
    std::vector<std::pair<uint64_t, uint64_t>> added;  // (start, words) per A, start == NONE once removed
    std::vector<bool> live;
    for (int i = 2; i < argc; ++i) {
        const char op = argv[i][0];
        if (op == 'A') {
            const uint64_t words = strtoull(argv[i] + 1, nullptr, 10);
            bool merged = false;
            const uint64_t at = pool.alloc(words, &merged);
            if (merged) pool.release();  // (the library waits for every frame then)
            added.push_back({at, words});
            live.push_back(true);
            printf("A %llu %d\n", (unsigned long long)at, merged ? 1 : 0);
        } else if (op == 'R') {
            const size_t k = strtoull(argv[i] + 1, nullptr, 10);
            if (k >= added.size() || !live[k]) return 2;
            pool.free(added[k].first, added[k].second, true);
            live[k] = false;
            printf("R %llu\n", (unsigned long long)added[k].first);
        } else if (op == 'S') {
            pool.release();
            printf("S %llu\n", (unsigned long long)pool.end());
        } else if (op == 'C') {
            char *rest = nullptr;
            const uint64_t max_words = strtoull(argv[i] + 1, &rest, 10);
            const uint64_t stage = rest && *rest == ':' ? strtoull(rest + 1, nullptr, 10) : 0;
            std::vector<Live> lv;
            for (size_t k = 0; k < added.size(); ++k)
                if (live[k]) lv.push_back(Live{added[k].first, added[k].second, (uint32_t)k});
            const Plan p = plan(lv, max_words, stage ? stage : DEFAULT_STAGE_WORDS);
            if (!p.moves.empty()) {  // (nothing to move: no wait, parked ranges stay parked)
                rebuild(pool, p);
                for (const Live &t : p.live) added[t.slot].first = t.start;
            }
            printf("C %zu %zu %zu %llu\n", p.moves.size(), p.passes.size(), p.launches.size(), (unsigned long long)pool.end());
            for (const Move &m : p.moves) printf("M %llu %llu %llu\n", (unsigned long long)m.src, (unsigned long long)m.dst, (unsigned long long)m.words);
        } else {
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "pool")) return pool_mode(argc, argv);
    random_section();
    edge_section();
    budget_section();
    pool_section();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
