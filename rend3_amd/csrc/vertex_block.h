// vertex_block.h -- host side of the vertex stages that rewrite runs of the mesh buffer in front of skinning (r3n_morph,
// r3n_vertex_normals, r3n_vertex_tangents; r3n_skinning for the range tests): mesh-buffer range arithmetic and the layout of the
// ONE host block a stage uploads per call.  Plain C++17, no HIP, no context: tests/vertex_block_check.cpp compiles it alone.
// Device side: vertex_gather.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace vertex_block {

// words [first, first + words) of the mesh buffer.  64-bit: a byte offset near 2^32 plus a long run does not wrap.
struct range {
    uint64_t first, words;
};
inline range words_at(uint32_t byte_offset, uint64_t words) { return {byte_offset / 4u, words}; }
inline bool aligned4(uint32_t byte_offset) { return (byte_offset & 3u) == 0u; }
inline bool inside(const range &r, uint64_t mesh_words) { return r.first + r.words <= mesh_words; }
// an empty range overlaps nothing
inline bool overlaps(const range &a, const range &b) {
    return a.words && b.words && a.first < b.first + b.words && b.first < a.first + a.words;
}

// wave slots that `count` elements take at `per_wave` elements each
inline uint64_t waves(uint64_t count, uint32_t per_wave) { return (count + per_wave - 1u) / per_wave; }
constexpr uint64_t MAX_WAVES = 0x7FFFFFFFull;  // of one call: the kernels count wave slots in 32 bits

// The block, in words: records (n * rec_words) | wave_first (n: every instance's first wave slot) | wave_instance (total_waves: the
// instance of every wave slot) [| tail, at the next even word: 8-byte entries].  Without a tail the block ends behind wave_instance.
struct layout {
    size_t o_first, o_inst, o_tail;
};
constexpr size_t NO_TAIL = ~(size_t)0;

// sizes `block` and fills the two maps; `waves_of(i)` is instance i's wave count, `total_waves` their sum.  Records and tail are the
// caller's to write.
template <class WavesOf>
layout lay_out(std::vector<uint32_t> &block, uint32_t n, size_t rec_words, uint64_t total_waves, WavesOf waves_of, size_t tail_words = NO_TAIL) {
    layout l;
    l.o_first = (size_t)n * rec_words;
    l.o_inst = l.o_first + n;
    l.o_tail = tail_words == NO_TAIL ? l.o_inst + (size_t)total_waves : (l.o_inst + (size_t)total_waves + 1u) & ~(size_t)1u;
    block.assign(l.o_tail + (tail_words == NO_TAIL ? 0u : tail_words), 0u);
    uint32_t w = 0;
    for (uint32_t i = 0; i < n; ++i) {
        block[l.o_first + i] = w;
        const uint32_t nw = (uint32_t)waves_of(i);
        std::fill(block.begin() + l.o_inst + w, block.begin() + l.o_inst + w + nw, i);
        w += nw;
    }
    return l;
}

}  // namespace vertex_block
