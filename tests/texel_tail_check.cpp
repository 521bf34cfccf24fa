// Stand-alone check of rend3_amd/csrc/texel_tail.h (what r3n_textures_from_texture derives, refuses and copies), built with the
// address and undefined-behaviour sanitizers and run as a child process by tests/test_texture_tail.py.  Every table is EXECUTED over
// a host array that models the pool block the way the kernel addresses it -- wave slot -> segment -> four units of four words per
// lane, unit indices clamped to the segment's last unit, a read allowed only below block end = high-water mark + 4 words, a store
// only for a unit of the segment -- in forward, reverse and a shuffled order, which must agree on every tail word, and compared with
// the obvious reference, one word-by-word copy per item.  A failed case prints FAIL and the exit status is 1.
//
//   texel_tail_check                                        every case below; one "name values" line each
//   texel_tail_check plan W H MIPS PER_TEXEL START COUNT    one tail: "width height mips src_word words units waves", or "refused"
//                                                           -- tests/test_texture_tail_gpu.py compares the device with it
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../rend3_amd/csrc/texel_tail.h"

using texel_alloc::align4;
using texel_alloc::Pool;
using texel_alloc::Range;
using namespace texel_tail;

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

// ---- the chain walk, restated: level k of (w, h) by halving k times
static uint64_t level_words(uint32_t w, uint32_t h, uint32_t k, uint32_t per) {
    for (uint32_t i = 0; i < k; ++i) {
        w = w > 1 ? w / 2 : 1;
        h = h > 1 ? h / 2 : 1;
    }
    return (uint64_t)w * h * per;
}
static uint32_t full_chain(uint32_t w, uint32_t h) {
    uint32_t n = 0;
    for (uint32_t m = w > h ? w : h; m; m /= 2) ++n;
    return n;
}

// every (start_mip, mip_count) of one chain, the two refusals at its edges included; returns the tails derived
static uint64_t check_chain(uint32_t w, uint32_t h, uint32_t per) {
    const Chain src{w, h, full_chain(w, h), per};
    uint64_t derived = 0;
    for (uint32_t start = 0; start <= src.mips + 1; ++start)
        for (uint32_t count = 0; count <= src.mips + 1; ++count) {
            const bool bad = start >= src.mips || count > src.mips - start;
            CHECK((fault(src, start, count) != nullptr) == bad);
            if (bad) continue;
            const Tail t = derive(src, start, count);
            const uint32_t levels = count ? count : src.mips - start;
            uint32_t lw = w, lh = h;
            uint64_t before = 0, words = 0;
            for (uint32_t k = 0; k < start; ++k) {
                before += (uint64_t)lw * lh * per;
                lw = lw > 1 ? lw / 2 : 1;
                lh = lh > 1 ? lh / 2 : 1;
            }
            for (uint32_t k = 0; k < levels; ++k) words += level_words(w, h, start + k, per);
            CHECK(t.chain.width == lw && t.chain.height == lh && t.chain.mips == levels && t.chain.per_texel == per);
            CHECK(t.src_word == before && t.words == words);
            // the tail is a valid chain by itself: its own walk gives the same levels
            uint64_t own = 0;
            for (uint32_t k = 0; k < levels; ++k) {
                CHECK(level_words(lw, lh, k, per) == level_words(w, h, start + k, per));
                own += level_words(lw, lh, k, per);
            }
            CHECK(own == words && texture_jobs::chain_fault(lw, lh, levels) == nullptr);
            ++derived;
        }
    return derived;
}

// ---- the kernel over a host block
struct UnitOp {
    uint64_t src, dst;  // first word read, first word stored
    bool store;
};
// `block` = the pool block (high-water mark + 4 words of slack).  order: 0 forward, 1 reverse, 2 shuffled.
static void run_table(const std::vector<uint32_t> &table, const vertex_block::layout &lo, uint64_t waves, uint32_t n, std::vector<uint32_t> &block, int order) {
    const uint32_t *wave_first = table.data() + lo.o_first, *wave_segment = table.data() + lo.o_inst;
    std::vector<UnitOp> ops;
    for (uint64_t w = 0; w < waves; ++w) {
        const uint32_t seg = wave_segment[w];
        CHECK(seg < n);
        if (seg >= n) return;
        const uint32_t *r = table.data() + (size_t)seg * REC_WORDS;
        const uint32_t units = r[2];
        CHECK(units >= 1 && w >= wave_first[seg]);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t first = (w - wave_first[seg]) * UNITS_PER_WAVE + lane;
            if (first >= units) continue;  // the lane leaves
            const uint64_t last = units - 1u;
            for (uint32_t k = 0; k < LOADS_PER_LANE; ++k) {
                const uint64_t u = first + 64u * k, read = u < last ? u : last;  // the loads are unconditional, clamped
                ops.push_back(UnitOp{(uint64_t)r[0] + 4u * read, (uint64_t)r[1] + 4u * u, u <= last});
            }
        }
    }
    if (order == 1) std::reverse(ops.begin(), ops.end());
    if (order == 2)
        for (size_t i = ops.size(); i > 1; --i) std::swap(ops[i - 1], ops[rnd() % i]);
    for (const UnitOp &op : ops) {
        CHECK(op.src + 4u <= block.size());  // a read below block end
        if (op.src + 4u > block.size()) continue;
        uint32_t v[4];
        memcpy(v, block.data() + op.src, 16);
        if (!op.store) continue;
        CHECK((op.dst & 3u) == 0u && op.dst + 4u <= block.size());
        if (op.dst + 4u <= block.size()) memcpy(block.data() + op.dst, v, 16);
    }
}

struct CopyStats {
    uint64_t items, words, waves;
};
// Lays the items out, executes them in the three orders over `block` (mark = its high-water mark) and checks: every destination's
// words equal the source tail's, no word outside the destinations' padded ranges changes, the orders agree on every tail word.
static CopyStats check_copy(const std::vector<Item> &items, const std::vector<uint32_t> &block, uint64_t mark) {
    CopyStats st{items.size(), 0, total_waves(items)};
    CHECK(block.size() == mark + 4u);
    CHECK(disjoint(items));
    std::vector<uint32_t> table;
    vertex_block::layout lo{};
    const bool laid = lay_out(items, table, lo);
    CHECK(laid);
    if (!laid) return st;
    CHECK(table.size() == items.size() * (REC_WORDS + 1u) + st.waves);
    uint64_t w = 0;
    for (size_t i = 0; i < items.size(); ++i) {  // the wave map: item i owns slots [w, w + waves_of(i))
        CHECK(table[lo.o_first + i] == w);
        CHECK(waves_of(items[i]) == (items[i].words + 1023u) / 1024u);  // 256 units of 4 words per wave slot
        for (uint64_t k = 0; k < waves_of(items[i]); ++k) CHECK(table[lo.o_inst + w + k] == i);
        w += waves_of(items[i]);
    }
    std::vector<uint32_t> want = block;
    std::vector<uint8_t> padded(block.size(), 0), tail(block.size(), 0);
    for (const Item &it : items) {
        CHECK((it.dst & 3u) == 0u && it.dst + align4(it.words) <= block.size() && it.src + it.words <= mark);
        for (uint64_t k = 0; k < it.words; ++k) {
            want[it.dst + k] = block[it.src + k];
            tail[it.dst + k] = 1;
        }
        for (uint64_t k = 0; k < align4(it.words); ++k) padded[it.dst + k] = 1;
        st.words += it.words;
    }
    for (int order = 0; order < 3; ++order) {
        std::vector<uint32_t> got = block;
        run_table(table, lo, st.waves, (uint32_t)items.size(), got, order);
        uint64_t bad_tail = 0, bad_outside = 0;
        for (size_t k = 0; k < got.size(); ++k) {
            if (tail[k] && got[k] != want[k]) ++bad_tail;
            if (!padded[k] && got[k] != block[k]) ++bad_outside;
        }
        CHECK(bad_tail == 0);
        CHECK(bad_outside == 0);
    }
    return st;
}

static std::vector<uint32_t> random_block(uint64_t mark) {
    std::vector<uint32_t> b(mark + 4u);
    for (uint32_t &v : b) v = (uint32_t)rnd();
    return b;
}

// source alignment 0 .. 3 x the lengths around a unit and a wave slot, every pair in ONE table, behind them two items that share a
// source; destinations from the allocator, behind the sources
static CopyStats check_alignments() {
    context = "alignments";
    static const uint64_t lengths[] = {1, 3, 4, 5, 1023, 1024, 1025};
    Pool pool;
    std::vector<Item> items;
    for (uint64_t len : lengths)
        for (uint64_t a = 0; a < 4; ++a) {
            const uint64_t at = pool.alloc(a + len);  // a texture whose tail starts `a` words in
            items.push_back(Item{at + a, 0, len});
        }
    items.push_back(Item{items[22].src, 0, items[22].words});      // the 1024-word source at alignment 2 again, whole
    items.push_back(Item{items[22].src + 5u, 0, 700});             // and a shorter tail of it
    for (Item &it : items) it.dst = pool.alloc(it.words);
    // the last destination ends at the mark: its padding lies in the slack
    CHECK(items.back().dst + items.back().words == pool.end());
    return check_copy(items, random_block(pool.end()), pool.end());
}

// The chains of the list as textures of a table; every (start, count) of each as one item of one call, through resolve(): slots,
// sources and the copy.  The LAST source's tails end at the mark before the destinations are placed, so with destinations in the
// holes in front of it the reads past a tail's end reach the block's slack.
static CopyStats check_table() {
    context = "table";
    struct Spec {
        uint32_t w, h, per;
    };
    static const Spec specs[] = {{1, 1, 1}, {7, 1, 1}, {16, 16, 1}, {64, 2, 1}, {8, 4, 4}, {5, 3, 1}};  // (5 x 3 last: its tails end off a unit)
    Pool pool;
    std::vector<Slot> table;
    const uint64_t hole = pool.alloc(20000);  // removed before the call: the destinations' words
    for (const Spec &s : specs) {
        const Chain c{s.w, s.h, full_chain(s.w, s.h), s.per};
        const uint64_t words = texture_jobs::chain_words(c.width, c.height, c.mips, c.per_texel);
        table.push_back(Slot{true, words, pool.alloc(words), c});
    }
    table.push_back(Slot{false, 0, 0, Chain{0, 0, 1, 1}});  // a removed slot
    pool.free(hole, 20000, false);
    const uint32_t n_table = (uint32_t)table.size();
    std::vector<r3n_texture_tail16> req;
    uint32_t next = n_table;
    for (uint32_t s = 0; s + 1 < n_table; ++s)
        for (uint32_t start = 0; start < table[s].chain.mips; ++start)
            for (uint32_t count = 0; count <= table[s].chain.mips - start; ++count)
                req.push_back(r3n_texture_tail16{req.empty() ? n_table - 1u : next++, s, start, count});  // the first into the removed slot
    std::vector<Resolved> got;
    const char *refused = resolve(n_table, [&](uint32_t s) { return table[s]; }, req.data(), (uint32_t)req.size(), got);
    CHECK(refused == nullptr);
    if (refused) return CopyStats{};
    const uint64_t mark = pool.end();
    std::vector<Item> items;
    bool all_in_holes = true;
    for (size_t i = 0; i < req.size(); ++i) {
        const Tail want = derive(table[req[i].src_slot].chain, req[i].start_mip, req[i].mip_count);
        CHECK(got[i].dst_slot == req[i].dst_slot && got[i].src == table[req[i].src_slot].offset + want.src_word && got[i].tail.words == want.words);
        const uint64_t at = pool.alloc(got[i].tail.words);
        all_in_holes = all_in_holes && at < hole + 20000;
        items.push_back(Item{got[i].src, at, got[i].tail.words});
    }
    CHECK(all_in_holes && pool.end() == mark);  // nothing appended: the last source's tails end at the mark
    uint32_t seen = 0;
    for (const Item &it : items) seen |= 1u << (it.src & 3u);
    CHECK(seen == 15u);  // the chains give every source alignment (5 x 3: levels at 0, 15, 17; 7 x 1: 0, 7, 10)
    return check_copy(items, random_block(mark), mark);
}

// 10^3 random calls: textures of random size with holes between them, tails at random words, destinations first fit
static CopyStats check_random() {
    context = "random";
    CopyStats total{0, 0, 0};
    for (int round = 0; round < 1000; ++round) {
        Pool pool;
        std::vector<Range> sources, holes;  // [start, end), unpadded
        const uint32_t n_src = 1u + (uint32_t)(rnd() % 6);
        for (uint32_t i = 0; i < n_src; ++i) {
            if (rnd() % 2) {
                const uint64_t words = 1u + rnd() % 3000, at = pool.alloc(words);
                holes.push_back(Range{at, at + words});
            }
            const uint64_t words = 1u + rnd() % (rnd() % 4 ? 40 : 3000);
            const uint64_t at = pool.alloc(words);
            sources.push_back(Range{at, at + words});
        }
        for (const Range &h : holes) pool.free(h.start, h.end - h.start, false);  // first fit finds them in front of the sources
        std::vector<Item> items;
        const uint32_t n = 1u + (uint32_t)(rnd() % 8);
        for (uint32_t i = 0; i < n; ++i) {
            const Range &s = sources[rnd() % sources.size()];
            const uint64_t len = s.end - s.start, skip = rnd() % len;
            items.push_back(Item{s.start + skip, 0, len - skip - (rnd() % 3 ? 0 : rnd() % (len - skip))});
        }
        for (Item &it : items) it.dst = pool.alloc(it.words);
        const CopyStats st = check_copy(items, random_block(pool.end()), pool.end());
        total.items += st.items;
        total.words += st.words;
        total.waves += st.waves;
    }
    return total;
}

static void check_refusals() {
    context = "refusals";
    const Chain c{16, 16, 5, 1};
    std::vector<Slot> table = {Slot{true, 341, 0, c}, Slot{false, 0, 0, Chain{0, 0, 1, 1}}, Slot{true, 0, 344, c}, Slot{true, 341, 688, c}};
    auto at = [&](uint32_t s) { return table[s]; };
    auto refused = [&](std::vector<r3n_texture_tail16> req) {
        std::vector<Resolved> out;
        return resolve((uint32_t)table.size(), at, req.data(), (uint32_t)req.size(), out) != nullptr;
    };
    CHECK(!refused({{4, 0, 1, 0}}));           // the lowest free index behind the table
    CHECK(!refused({{1, 0, 4, 1}}));           // a removed slot; the last level
    CHECK(!refused({{4, 0, 0, 5}, {5, 0, 2, 2}, {1, 3, 0, 0}}));  // one source twice; table + n - 1
    CHECK(refused({{4, 1, 0, 0}}));            // a removed source
    CHECK(refused({{5, 4, 0, 0}, {4, 0, 0, 0}}));  // a source that is a destination of the same call: never written before it
    CHECK(refused({{4, 7, 0, 0}}));            // a source past the table
    CHECK(refused({{4, 2, 0, 0}}));            // a source that owns no words
    CHECK(refused({{3, 0, 0, 0}}));            // a live destination
    CHECK(refused({{0, 0, 0, 0}}));            // its own source
    CHECK(refused({{5, 0, 0, 0}}));            // table + n
    CHECK(refused({{4, 0, 0, 0}, {6, 0, 0, 0}}));  // table + n among good ones
    CHECK(refused({{4, 0, 0, 0}, {4, 3, 1, 0}}));  // one destination twice
    CHECK(refused({{4, 0, 5, 0}}));            // start_mip == mips
    CHECK(refused({{4, 0, 5, 1}}));
    CHECK(refused({{4, 0, 2, 4}}));            // start_mip + mip_count > mips
    CHECK(refused({{4, 0, 0, 6}}));
    CHECK(refused({{4, 0, 0xFFFFFFFFu, 2}}));  // (no wrap of start_mip + mip_count)
    CHECK(refused({{4, 0, 2, 0xFFFFFFFFu}}));
    // overlap: a destination on a tail's words, two destinations on one range; the words read past a tail's end may be written
    CHECK(disjoint({Item{0, 8, 5}, Item{0, 16, 8}}));
    CHECK(disjoint({Item{3, 8, 5}}));  // reads [3, 11) as a unit, its tail is [3, 8)
    CHECK(!disjoint({Item{3, 4, 5}}));
    CHECK(!disjoint({Item{100, 96, 5}}));
    CHECK(!disjoint({Item{0, 8, 5}, Item{20, 8, 2}}));
    CHECK(!disjoint({Item{0, 8, 5}, Item{9, 40, 4}}));  // reads what the first one writes
    CHECK(!disjoint({Item{0, 8, 1}, Item{20, 8, 1}}));  // padded ranges collide
    // 2^31 wave slots, by arithmetic: an item of 2^32 - 1 words takes 2^22 wave slots, 512 of them 2^31 -- one more than the kernel
    // counts.  lay_out refuses before it sizes anything.
    const Item big{0, 0, 0xFFFFFFFFull};
    CHECK(waves_of(big) == (1ull << 22));
    std::vector<Item> many(512, big);
    CHECK(total_waves(many) == (1ull << 31) && total_waves(many) == vertex_block::MAX_WAVES + 1u);
    std::vector<uint32_t> table_words;
    vertex_block::layout lo{};
    CHECK(!lay_out(many, table_words, lo) && table_words.empty());
    many.pop_back();
    CHECK(total_waves(many) <= vertex_block::MAX_WAVES);  // (accepted: not laid out here, the table would take 8 GiB)
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        if (argc != 8) return 2;
        uint32_t v[6];
        for (int i = 0; i < 6; ++i) v[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
        const Chain src{v[0], v[1], v[2], v[3]};
        if (texture_jobs::chain_fault(src.width, src.height, src.mips) || (src.per_texel != 1 && src.per_texel != 4)) return 2;
        if (fault(src, v[4], v[5])) {
            printf("refused\n");
            return 0;
        }
        const Tail t = derive(src, v[4], v[5]);
        const Item it{t.src_word, 0, t.words};
        printf("%u %u %u %llu %llu %llu %llu\n", t.chain.width, t.chain.height, t.chain.mips, (unsigned long long)t.src_word, (unsigned long long)t.words,
               (unsigned long long)units_of(it), (unsigned long long)waves_of(it));
        return 0;
    }
    context = "chains";
    uint64_t derived = 0;
    derived += check_chain(1, 1, 1);
    derived += check_chain(5, 3, 1);
    derived += check_chain(7, 1, 1);
    derived += check_chain(16, 16, 1);
    derived += check_chain(64, 2, 1);
    derived += check_chain(8, 4, 4);
    printf("chains %llu\n", (unsigned long long)derived);
    CopyStats st = check_alignments();
    printf("alignments %llu %llu %llu\n", (unsigned long long)st.items, (unsigned long long)st.words, (unsigned long long)st.waves);
    st = check_table();
    printf("table %llu %llu %llu\n", (unsigned long long)st.items, (unsigned long long)st.words, (unsigned long long)st.waves);
    st = check_random();
    printf("random %llu %llu %llu\n", (unsigned long long)st.items, (unsigned long long)st.words, (unsigned long long)st.waves);
    check_refusals();
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
