// Stand-alone check of rend3_amd/csrc/texel_compact.h (what r3n_textures_compact moves, in which launches) and of Pool::rebuild
// (texel_alloc.h), built with the address and undefined-behaviour sanitizers and run as a child process by
// tests/test_texture_compact.py.  Every plan is EXECUTED over a host array that models the pool -- each launch word by word in
// forward, reverse and a shuffled order, which must agree: a launch that wrote a word it reads elsewhere would differ -- and compared
// with the obvious reference, one memmove per texture in ascending order.  A failed case prints FAIL and the exit status is 1.
//
//   texel_compact_check                          the fixed edge list and the random cases; one "name values" line each
//   texel_compact_check plan STAGE MAX ITEM...   one layout (ITEM = T<words> a texture, H<words> a hole, in address order, each on
//                                                the 4-word boundary behind the one before): "passes launches words_moved
//                                                textures_moved end" -- tests/test_texture_compact_gpu.py compares the device with it
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../rend3_amd/csrc/texel_compact.h"

using texel_alloc::align4;
using texel_alloc::Pool;
using texel_alloc::Range;
using namespace texel_compact;

static int failures = 0;
static const char *context = "";
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) printf("FAIL line_%d %s [%s]\n", __LINE__, #cond, context); \
            ++failures;                                                    \
        }                                                                  \
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
// the live set of a layout: every item on the 4-word boundary behind the one before, as ascending appends place them
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

// one launch, word by word, in the given order (0 forward, 1 reverse, 2 shuffled) through the kernel's own table: wave slot -> segment
// -> units, so the table is checked with the plan
static void run_launch(const Plan &p, const Launch &l, const std::vector<uint32_t> &block, const vertex_block::layout &lo, std::vector<uint32_t> &pool,
                       std::vector<uint32_t> &scratch, int order) {
    struct Word {
        uint64_t src, dst;
    };
    std::vector<Word> words;
    const uint32_t *wave_first = block.data() + lo.o_first, *wave_segment = block.data() + lo.o_inst;
    for (uint64_t w = l.first_wave; w < l.first_wave + l.waves; ++w) {
        const uint32_t seg = wave_segment[w];
        CHECK(seg >= l.first_segment && seg < l.first_segment + l.segments);
        const uint32_t *r = block.data() + (size_t)seg * REC_WORDS;
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t k = 0; k < LOADS_PER_LANE; ++k) {
                const uint64_t u = (uint64_t)(w - wave_first[seg]) * UNITS_PER_WAVE + lane + 64u * k;
                if (u >= r[2]) continue;
                for (uint32_t c = 0; c < 4; ++c) words.push_back(Word{(uint64_t)r[0] + 4u * u + c, (uint64_t)r[1] + 4u * u + c});
            }
    }
    uint64_t want = 0;
    for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s) want += p.segments[s].words;
    CHECK(words.size() == want);  // (with the write-once check below: every word of every segment exactly once)
    if (order == 1) std::reverse(words.begin(), words.end());
    if (order == 2)
        for (size_t i = words.size(); i > 1; --i) std::swap(words[i - 1], words[rnd() % i]);
    std::vector<uint32_t> &from = l.kind == SCATTER ? scratch : pool, &to = l.kind == GATHER ? scratch : pool;
    for (const Word &w : words) {
        CHECK(w.src < from.size() && w.dst < to.size());
        if (w.src < from.size() && w.dst < to.size()) to[w.dst] = from[w.src];
    }
}

struct Outcome {
    uint64_t passes, launches, staged;
};
static Outcome check_layout(const std::vector<Live> &live, uint64_t max_words, uint64_t stage_words) {
    const Plan p = plan(live, max_words, stage_words);
    Outcome out{p.passes.size(), p.launches.size(), 0};
    uint64_t old_end = 0, old_reach = 0;
    for (const Live &t : live) {
        old_end = std::max(old_end, t.start + t.words);
        old_reach = std::max(old_reach, align4(t.start + t.words));
    }
    // ---- moves: multiples of 4, dst < src, ascending, the destinations one contiguous interval, the budget kept
    uint64_t moved = 0;
    for (size_t i = 0; i < p.moves.size(); ++i) {
        const Move &m = p.moves[i];
        CHECK(m.src % 4 == 0 && m.dst % 4 == 0 && m.words % 4 == 0 && m.words && m.dst < m.src);
        if (i) CHECK(m.dst == p.moves[i - 1].dst + p.moves[i - 1].words && m.src >= p.moves[i - 1].src + p.moves[i - 1].words);
        if (i) CHECK(m.src - m.dst >= p.moves[i - 1].src - p.moves[i - 1].dst);  // the shift only grows
        moved += m.words;
    }
    CHECK(moved == p.words_moved && (!max_words || moved <= max_words));
    CHECK(p.live.size() == live.size());
    if (!max_words && p.live.size() == live.size()) {  // the textures in place are a prefix: behind the first mover every texture moves
        std::vector<Live> sorted = live;
        std::sort(sorted.begin(), sorted.end(), [](const Live &a, const Live &b) { return a.start < b.start; });
        const size_t in_place = live.size() - p.moves.size();
        for (size_t i = 0; i < live.size(); ++i) CHECK(i < in_place ? p.live[i].start == sorted[i].start : p.live[i].start < sorted[i].start);
    }
    // ---- passes: they tile the stream, each at least min(stage_words, remaining) long; the launch bound
    uint64_t at = 0;
    for (const Pass &pass : p.passes) {
        CHECK(pass.position == at && pass.words % 4 == 0 && pass.words >= std::min(stage_words, p.words_moved - at));
        CHECK(!pass.staged || pass.words <= stage_words);
        const Launch &first = p.launches[pass.first_launch];
        CHECK(pass.staged ? first.kind == GATHER && p.launches[pass.first_launch + 1].kind == SCATTER : first.kind == DIRECT);
        out.staged += pass.staged;
        at += pass.words;
    }
    CHECK(at == p.words_moved);
    CHECK(p.launches.size() == p.passes.size() + out.staged);
    CHECK(p.launches.size() <= 2 * ((p.words_moved + stage_words - 1) / stage_words + 1));
    CHECK(p.scratch_words <= stage_words);
    for (const Segment &s : p.segments) CHECK(s.src % 4 == 0 && s.dst % 4 == 0 && s.words % 4 == 0 && s.words);
    // ---- within a launch no destination word is a source word of the same launch, and none is written twice
    std::vector<uint8_t> written(old_reach + 4, 0);
    for (const Launch &l : p.launches) {
        if (l.kind == GATHER) {  // reads the pool, writes scratch: [0, pass words) once
            uint64_t next = 0;
            for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s) {
                CHECK(p.segments[s].dst == next && p.segments[s].src + p.segments[s].words <= old_reach);
                next += p.segments[s].words;
            }
            CHECK(next <= p.scratch_words);
            continue;
        }
        for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s)
            for (uint64_t w = 0; w < p.segments[s].words; ++w) {
                CHECK(p.segments[s].dst + w < old_reach && !written[p.segments[s].dst + w]);
                written[p.segments[s].dst + w] = 1;
            }
        if (l.kind == DIRECT)
            for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s)
                for (uint64_t w = 0; w < p.segments[s].words; ++w) {
                    CHECK(p.segments[s].src + w < old_reach);
                    CHECK(!written[p.segments[s].src + w]);
                }
        else
            CHECK(l.segments == 1 && p.segments[l.first_segment].src == 0 && p.segments[l.first_segment].words <= p.scratch_words);
        for (size_t s = l.first_segment; s < l.first_segment + l.segments; ++s)
            for (uint64_t w = 0; w < p.segments[s].words; ++w) written[p.segments[s].dst + w] = 0;
    }
    // ---- execution against one memmove per texture
    {
        std::vector<uint32_t> block;
        vertex_block::layout lo{};
        CHECK(lay_out(p, block, lo));
        std::vector<uint32_t> start(old_reach + 4);
        for (size_t i = 0; i < start.size(); ++i) start[i] = 0xA0000000u + (uint32_t)i;  // every word its own value, padding included
        std::vector<uint32_t> want = start;
        for (size_t i = 0; i < p.live.size(); ++i) {  // p.live is ascending, and so are their sources
            const Live *from = nullptr;
            for (const Live &t : live)
                if (t.slot == p.live[i].slot) from = &t;
            CHECK(from && from->words == p.live[i].words && p.live[i].start <= from->start);
            if (from) memmove(want.data() + p.live[i].start, want.data() + from->start, from->words * 4u);
        }
        std::vector<uint32_t> got[3];
        for (int order = 0; order < 3; ++order) {
            got[order] = start;
            std::vector<uint32_t> scratch(p.scratch_words, 0xDEADBEEFu);
            for (const Launch &l : p.launches) run_launch(p, l, block, lo, got[order], scratch, order);
        }
        CHECK(got[0] == got[1] && got[0] == got[2]);
        for (const Live &t : p.live)
            CHECK(std::equal(want.begin() + t.start, want.begin() + t.start + t.words, got[0].begin() + t.start));
    }
    // ---- the allocator afterwards: holes = the complement of the padded live set below the mark
    Pool pool;
    rebuild(pool, p);
    std::vector<uint8_t> used(align4(p.end) + 4, 0);
    uint64_t new_end = 0;
    for (const Live &t : p.live) {
        for (uint64_t w = t.start; w < align4(t.start + t.words); ++w) {
            CHECK(!used[w]);
            used[w] = 1;
        }
        new_end = std::max(new_end, t.start + t.words);
    }
    CHECK(pool.end() == new_end && p.end == new_end && pool.parked().empty());
    std::vector<Range> holes;
    for (uint64_t w = 0; w < align4(new_end); ++w)
        if (!used[w]) {
            if (!holes.empty() && holes.back().end == w) ++holes.back().end;
            else holes.push_back(Range{w, w + 1});
        }
    CHECK(holes.size() == pool.holes().size());
    for (size_t i = 0; i < holes.size() && i < pool.holes().size(); ++i)
        CHECK(holes[i].start == pool.holes()[i].start && holes[i].end == pool.holes()[i].end);
    if (!max_words) {  // a full compaction: no holes, and the freed words are taken at the new mark
        CHECK(pool.holes().empty());
        for (size_t i = 0; i < p.live.size(); ++i) CHECK(p.live[i].start == (i ? align4(p.live[i - 1].start + p.live[i - 1].words) : 0));
        if (old_end > new_end) CHECK(pool.alloc(old_end - new_end) == align4(new_end));
    } else if (p.moves.size() && p.live.size() > 0) {
        // a budgeted one: the packed prefix, then at most one new hole in front of the first texture that stayed
        size_t stayed = 0;
        while (stayed < p.live.size() && (stayed == 0 ? p.live[0].start == 0 : p.live[stayed].start == align4(p.live[stayed - 1].start + p.live[stayed - 1].words))) ++stayed;
        for (size_t i = stayed; i < p.live.size(); ++i) {
            const Live *from = nullptr;
            for (const Live &t : live)
                if (t.slot == p.live[i].slot) from = &t;
            CHECK(from && from->start == p.live[i].start);  // untouched
        }
    }
    return out;
}

static void edges() {
    struct Edge {
        const char *name;
        std::vector<Item> items;
        uint64_t max_words;
    };
    const Item H4{true, 4}, T1000{false, 1000};
    const std::vector<Edge> list = {
        {"self_overlap", {H4, T1000}, 0},                                                 // must be staged
        {"shift_equals_length", {{true, 1000}, T1000}, 0},                                // dst_end == src: one direct launch
        {"shift_4_short", {{true, 996}, T1000}, 0},
        {"cut_by_pass", {{true, 256}, T1000, {false, 300}}, 0},                           // passes end inside both textures
        {"segment_lengths", {{true, 8}, {false, 3}, {false, 250}, {false, 256}, {false, 257}}, 0},  // padded 4, 252, 256, 260
        // "A texture already in place between two that move" cannot occur under this packing rule: the shift only grows, so behind the
        // first texture that moves every texture moves (check_layout asserts it for every plan).  What stands in for it: a texture in
        // place in FRONT of the movers, and one that sits flush behind a mover -- no hole of its own -- between two that have one.
        {"adjacent_between_movers", {{false, 16}, {true, 8}, {false, 100}, {false, 40}, {true, 12}, {false, 64}}, 0},
        {"last_moves", {{false, 16}, {true, 64}, {false, 30}}, 0},                        // the mark drops
        {"budget_at_end", {{true, 8}, {false, 16}, {false, 16}, {true, 20}, {false, 16}}, 32},
        {"budget_one_short", {{true, 8}, {false, 16}, {false, 16}, {true, 20}, {false, 16}}, 31},
        {"empty", {}, 0},
        {"no_holes", {{false, 16}, {false, 7}, {false, 64}}, 0},
    };
    for (const Edge &e : list) {
        context = e.name;
        const std::vector<Live> live = live_of(e.items);
        printf("edge_%s", e.name);
        for (uint64_t stage : {(uint64_t)256, (uint64_t)260, (uint64_t)4096, DEFAULT_STAGE_WORDS}) {
            const Outcome o = check_layout(live, e.max_words, stage);
            printf(" %llu %llu %llu", (unsigned long long)o.passes, (unsigned long long)o.launches, (unsigned long long)o.staged);
        }
        printf("\n");
    }
    context = "edges";
    // what the list is there to show, stated once more on the plans themselves
    {
        const Plan p = plan(live_of({H4, T1000}), 0, DEFAULT_STAGE_WORDS);
        CHECK(p.passes.size() == 1 && p.passes[0].staged && p.launches.size() == 2 && p.words_moved == 1000);
        const Plan q = plan(live_of({{true, 1000}, T1000}), 0, DEFAULT_STAGE_WORDS);
        CHECK(q.passes.size() == 1 && !q.passes[0].staged && q.moves[0].dst + q.moves[0].words == q.moves[0].src);
        const Plan r = plan(live_of({{true, 996}, T1000}), 0, 256);  // 996 words, then the last 4: both below their sources
        CHECK(r.passes.size() == 2 && !r.passes[0].staged && r.passes[0].words == 996 && !r.passes[1].staged && r.passes[1].words == 4);
        const Plan s = plan(live_of({{true, 256}, T1000, {false, 300}}), 0, 256);
        bool inside = false;
        for (const Pass &pass : s.passes) inside = inside || (pass.position + pass.words > 0 && pass.position + pass.words < 1000);
        CHECK(inside && s.passes.size() >= 5);
        const Plan t = plan(live_of({{true, 8}, {false, 3}, {false, 250}, {false, 256}, {false, 257}}), 0, 4096);
        CHECK(t.moves.size() == 4 && t.moves[0].words == 4 && t.moves[1].words == 252 && t.moves[2].words == 256 && t.moves[3].words == 260);
        const Plan u = plan(live_of({{false, 16}, {true, 8}, {false, 100}, {false, 40}, {true, 12}, {false, 64}}), 0, 4096);
        CHECK(u.moves.size() == 3 && u.live[0].start == 0);  // the first stays; behind a mover everything moves, adjacent or not
        const Plan v = plan(live_of({{false, 16}, {true, 64}, {false, 30}}), 0, 4096);
        CHECK(v.end == 46 && v.moves.size() == 1);
        const std::vector<Item> budget = {{true, 8}, {false, 16}, {false, 16}, {true, 20}, {false, 16}};
        const Plan b32 = plan(live_of(budget), 32, 4096), b31 = plan(live_of(budget), 31, 4096), b15 = plan(live_of(budget), 15, 4096);
        CHECK(b32.moves.size() == 2 && b32.words_moved == 32 && b31.moves.size() == 1 && b31.words_moved == 16 && b15.moves.empty());
        Pool pool;
        rebuild(pool, b32);
        CHECK(pool.holes().size() == 1 && pool.holes()[0].start == 32 && pool.holes()[0].end == 60 && pool.end() == 76);
        CHECK(plan({}, 0, 256).moves.empty() && plan({}, 0, 256).end == 0);
        CHECK(plan(live_of({{false, 16}, {false, 7}, {false, 64}}), 0, 256).moves.empty());
    }
}

static uint64_t size_between(uint64_t lo, uint64_t hi) {  // skewed small, the tail up to `hi`
    const uint64_t pick = rnd() % 100;
    const uint64_t top = std::min<uint64_t>(pick < 60 ? 64 : pick < 92 ? 600 : hi, hi);
    return lo + rnd() % (top - lo + 1);
}

static void random_cases() {
    context = "random";
    uint64_t cases = 0, staged = 0, direct = 0, budgeted = 0, words = 0, biggest = 0, widest_hole = 0;
    const uint64_t stages[3] = {256, 260, 4096};
    for (int n = 0; n < 10000; ++n) {
        std::vector<Item> items;
        const uint32_t textures = 1 + (uint32_t)(rnd() % 6);
        for (uint32_t i = 0; i < textures; ++i) {
            if (rnd() % 3 != 0) {
                items.push_back(Item{true, size_between(4, 5000)});
                widest_hole = std::max(widest_hole, items.back().words);
            }
            items.push_back(Item{false, size_between(1, 5000)});
            biggest = std::max(biggest, items.back().words);
        }
        const std::vector<Live> live = live_of(items);
        uint64_t total = 0;
        for (const Live &t : live) total += align4(t.words);
        const uint64_t max_words = rnd() % 3 == 0 ? 1 + rnd() % (total + 8) : 0;
        const Outcome o = check_layout(live, max_words, stages[n % 3]);
        ++cases;
        staged += o.staged;
        direct += o.passes - o.staged;
        budgeted += max_words != 0;
        words += total;
    }
    printf("random %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)staged, (unsigned long long)direct,
           (unsigned long long)budgeted, (unsigned long long)words, (unsigned long long)biggest, (unsigned long long)widest_hole);
    // one pool near the 2^32-word limit, planned only: the arithmetic stays in 64 bits and the table in 32
    context = "large";
    const Plan big = plan({{4, 0x7FFFFFF0ull, 0}, {0x80000000ull, 0x7FFFFFF1ull, 1}}, 0, DEFAULT_STAGE_WORDS);
    uint64_t at = 0;
    for (const Pass &pass : big.passes) {
        CHECK(pass.position == at && pass.words >= std::min(DEFAULT_STAGE_WORDS, big.words_moved - at));
        at += pass.words;
    }
    CHECK(at == big.words_moved && big.words_moved == 0x7FFFFFF0ull + 0x7FFFFFF4ull && big.end == 0x7FFFFFF0ull + 0x7FFFFFF1ull);
    CHECK(big.launches.size() <= 2 * ((big.words_moved + DEFAULT_STAGE_WORDS - 1) / DEFAULT_STAGE_WORDS + 1));
    CHECK(big.total_waves <= vertex_block::MAX_WAVES);
    for (const Segment &s : big.segments) CHECK(s.src + s.words <= 0x100000000ull && s.dst + s.words <= 0x100000000ull && s.words / 4u <= 0xFFFFFFFFull);
    printf("large %llu %llu\n", (unsigned long long)big.passes.size(), (unsigned long long)big.launches.size());
}

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "plan")) {
        const uint64_t stage = strtoull(argv[2], nullptr, 10), max_words = strtoull(argv[3], nullptr, 10);
        std::vector<Item> items;
        for (int i = 4; i < argc; ++i) items.push_back(Item{argv[i][0] == 'H', strtoull(argv[i] + 1, nullptr, 10)});
        const Plan p = plan(live_of(items), max_words, stage ? stage : DEFAULT_STAGE_WORDS);
        printf("%llu %llu %llu %llu %llu\n", (unsigned long long)p.passes.size(), (unsigned long long)p.launches.size(),
               (unsigned long long)p.words_moved, (unsigned long long)p.moves.size(), (unsigned long long)p.end);
        return 0;
    }
    edges();
    random_cases();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
