// vertex_block_check.cpp -- TEST INFRASTRUCTURE: prints what rend3_amd/csrc/vertex_block.h computes at its edges.
// tests/test_vertex_block.py builds it with the address and undefined-behaviour sanitizers, runs it and compares every word.
#include <cstdio>

#include "../rend3_amd/csrc/vertex_block.h"

using namespace vertex_block;

// "<name> o_first o_inst o_tail size : words".  Records and tail are filled with 0xAAAAAAAA / 0xBBBBBBBB behind lay_out, so the
// output also shows that the two maps sit exactly between them.
static void print_layout(const char *name, const std::vector<uint32_t> &counts, size_t rec_words, size_t tail_words) {
    uint64_t total = 0;
    for (uint32_t c : counts) total += c;
    std::vector<uint32_t> block;
    const layout l = lay_out(block, (uint32_t)counts.size(), rec_words, total, [&](uint32_t i) { return counts[i]; }, tail_words);
    std::fill(block.begin(), block.begin() + l.o_first, 0xAAAAAAAAu);
    std::fill(block.begin() + l.o_tail, block.end(), 0xBBBBBBBBu);
    std::printf("%s %zu %zu %zu %zu :", name, l.o_first, l.o_inst, l.o_tail, block.size());
    for (uint32_t w : block) std::printf(" %u", w);
    std::printf("\n");
}

int main() {
    print_layout("layout_one", {1}, 8, NO_TAIL);
    print_layout("layout_tail", {0, 1, 5}, 16, 4);  // o_inst + total_waves = 57 is odd: the tail starts at 58
    print_layout("layout_no_tail", {0, 1, 5}, 16, NO_TAIL);
    print_layout("layout_empty_tail", {2}, 16, 0);  // a tail of no words still pads: 19 -> 20

    std::printf("aligned4");
    for (uint32_t o : {0u, 1u, 2u, 3u, 4u, 0xFFFFFFFCu, 0xFFFFFFFFu}) std::printf(" %d", (int)aligned4(o));
    std::printf("\n");

    // exactly at mesh_words and one past, from the buffer's start and from a byte offset
    std::printf("inside %d %d %d %d %d\n", (int)inside(words_at(0, 100), 100), (int)inside(words_at(0, 101), 100), (int)inside(words_at(16, 96), 100),
                (int)inside(words_at(16, 97), 100), (int)inside(words_at(400, 0), 100));
    // the last aligned byte offset and runs longer than 2^32 words: sums that would wrap in 32 bits
    const range far = words_at(0xFFFFFFFCu, 0xFFFFFFFFull * 3u);
    std::printf("far %llu %llu\n", (unsigned long long)far.first, (unsigned long long)far.words);
    const uint64_t far_end = far.first + far.words;
    std::printf("inside_far %d %d %d %d\n", (int)inside(far, far_end), (int)inside(far, far_end - 1u), (int)inside(far, 1ull << 32),
                (int)inside(words_at(0xFFFFFFFCu, (1ull << 32) + 1u), 1ull << 32));

    const range a = words_at(0, 4), touching = words_at(16, 4), lapping = words_at(12, 4), nested = words_at(4, 2), empty = words_at(8, 0);
    std::printf("overlaps %d %d %d %d %d %d %d %d %d\n", (int)overlaps(a, touching), (int)overlaps(touching, a), (int)overlaps(a, lapping),
                (int)overlaps(lapping, a), (int)overlaps(a, nested), (int)overlaps(nested, a), (int)overlaps(a, empty), (int)overlaps(empty, a),
                (int)overlaps(a, a));
    std::printf("overlaps_far %d %d\n", (int)overlaps(far, words_at(0, 0x40000000ull)), (int)overlaps(far, words_at(0, 0x3FFFFFFFull)));

    std::printf("waves");
    for (uint64_t n : {0ull, 1ull, 64ull, 65ull, 0xFFFFFFFFull}) std::printf(" %llu", (unsigned long long)waves(n, 64));
    std::printf(" %llu %llu %llu\n", (unsigned long long)waves(768, 256), (unsigned long long)waves(769, 256),
                (unsigned long long)waves(0xFFFFFFFFull * 3u, 256));
    return 0;
}
