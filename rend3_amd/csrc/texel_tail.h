// texel_tail.h -- host side of r3n_textures_from_texture (texture_tail.hip): a new texture made of the levels [start_mip,
// start_mip + mip_count) of one the pool already holds -- Renderer::add_texture_2d_from_texture, TextureManager::fill_from_texture
// (rend3/src/managers/texture.rs:198-242), whose per-level copy_texture_to_texture is here ONE copy of pool words.  Plain C++17, no
// HIP, no context: tests/texel_tail_check.cpp compiles it alone.
//
// A texture is one contiguous run of decoded words, its levels back to back (texel_alloc.h, texture_jobs.h), so the tail is the
// contiguous word range behind the `start_mip` levels in front of it.  Level k of the tail has the extents of level start_mip + k of
// the source -- max(1, (w >> s) >> k) == max(1, w >> (s + k)) -- so the tail is a valid chain of a texture of level start_mip's
// size, and the derived descriptor is (those extents, the count, the source's pool class).
//
// The copy: the destination comes from the allocator and starts on a 4-word boundary; the source starts on ANY word boundary.  The
// kernel writes whole 16-byte units, ceil(words / 4) of them -- the up to 3 words of padding lie inside the destination's own padded
// range -- and reads unit u of a segment as the four words src + 4u .. src + 4u + 3: up to 3 words past the tail's end, inside the
// pool block because the block has 16 bytes of slack behind the high-water mark.  A wave slot takes UNITS_PER_WAVE destination units
// of ONE segment; records | wave_first | wave_instance as vertex_block.h lays them out.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "texel_alloc.h"
#include "texture_jobs.h"
#include "vertex_block.h"

namespace texel_tail {

using texel_alloc::align4;

// a texture as the device descriptor holds it: extents, levels, pool words per texel (1, or 4 for the float class)
struct Chain {
    uint32_t width, height, mips, per_texel;
};
struct Tail {
    Chain chain;        // the derived texture
    uint64_t src_word;  // first word of level start_mip, relative to the source's first word
    uint64_t words;     // of the tail (unpadded)
};
// nullptr, or what is refused about (start_mip, mip_count) for this source; mip_count 0 = all that remain
inline const char *fault(const Chain &src, uint32_t start_mip, uint32_t mip_count) {
    if (start_mip >= src.mips) return "start_mip is not a level of the source";
    if (mip_count > src.mips - start_mip) return "start_mip + mip_count exceeds the source's levels";
    return nullptr;
}
// (fault() == nullptr)
inline Tail derive(const Chain &src, uint32_t start_mip, uint32_t mip_count) {
    const texture_jobs::Level first = texture_jobs::level_of(src.width, src.height, start_mip, src.per_texel);
    Tail t;
    t.chain = Chain{first.w, first.h, mip_count ? mip_count : src.mips - start_mip, src.per_texel};
    t.src_word = texture_jobs::chain_words(src.width, src.height, start_mip, src.per_texel);
    t.words = texture_jobs::chain_words(t.chain.width, t.chain.height, t.chain.mips, t.chain.per_texel);
    return t;
}

// ---- a call's items against the table as it is before the call
struct Slot {
    bool live;       // holds a texture
    uint64_t words;  // pool words its range owns (0: none)
    uint64_t offset; // its first pool word
    Chain chain;
};
struct Resolved {
    uint32_t dst_slot;
    Tail tail;
    uint64_t src;  // first pool word of the tail
};
// nullptr and out[i] for every item, or what is refused (nothing in `out` is then meaningful).  slot_at(s) gives slot s < table.
// Sources must hold a live texture that owns its words; destinations must hold none -- removed, never written, or past the table,
// below table + n -- and may not be named twice; the levels must be the source's.
template <class SlotAt>
const char *resolve(uint32_t table, SlotAt slot_at, const r3n_texture_tail16 *items, uint32_t n, std::vector<Resolved> &out) {
    out.assign(n, Resolved{});
    std::vector<uint32_t> dsts(n);
    for (uint32_t i = 0; i < n; ++i) {
        const r3n_texture_tail16 &it = items[i];
        if (it.src_slot >= table) return "the source slot holds no texture (removed or never written)";
        const Slot src = slot_at(it.src_slot);
        if (!src.live) return "the source slot holds no texture (removed or never written)";
        if (!src.words) return "the source slot owns no words (a raw r3n_textures_write whose ranges are not ascending, disjoint and 4-word aligned)";
        if ((uint64_t)it.dst_slot >= (uint64_t)table + n) return "destination slot past table length + n (the lowest free index never is)";
        if (it.dst_slot < table && slot_at(it.dst_slot).live) return "the destination slot holds a texture (a live slot is not replaced)";
        if (const char *f = fault(src.chain, it.start_mip, it.mip_count)) return f;
        out[i].dst_slot = dsts[i] = it.dst_slot;
        out[i].tail = derive(src.chain, it.start_mip, it.mip_count);
        out[i].src = src.offset + out[i].tail.src_word;
    }
    std::sort(dsts.begin(), dsts.end());
    if (std::adjacent_find(dsts.begin(), dsts.end()) != dsts.end()) return "one destination slot named twice";
    return nullptr;
}

// ---- the kernel's table: one 4-word record per placed item
struct Item {
    uint64_t src, dst, words;  // pool words; dst a multiple of 4, words >= 1 (unpadded)
};
struct Record {
    uint32_t src, dst, units, pad;  // src / dst in words, units = ceil(words / 4)
};
static_assert(sizeof(Record) == 16, "a segment record is 4 words");
constexpr uint32_t REC_WORDS = sizeof(Record) / 4u, LOADS_PER_LANE = 4u, UNITS_PER_WAVE = 64u * LOADS_PER_LANE;

inline uint64_t units_of(const Item &it) { return (it.words + 3u) / 4u; }
inline uint64_t waves_of(const Item &it) { return vertex_block::waves(units_of(it), UNITS_PER_WAVE); }
inline uint64_t total_waves(const std::vector<Item> &items) {
    uint64_t waves = 0;
    for (const Item &it : items) waves += waves_of(it);
    return waves;
}
// words the kernel touches for an item: it reads [src, src + 4 * units), writes [dst, dst + 4 * units)
inline uint64_t reach(const Item &it) { return 4u * units_of(it); }
// No word written by the call is a tail word the call reads, and none is written twice (sources may be shared): the destinations
// come from free words, so this never fails -- the kernel has no ordering between threads and relies on it.  (The up to 3 words read
// past a tail's end may be words another item writes: they only ever reach the reader's own padding.)  One sweep in address order.
inline bool disjoint(const std::vector<Item> &items) {
    struct Span {
        uint64_t start, end;
        bool write;
    };
    std::vector<Span> spans;
    spans.reserve(2 * items.size());
    for (const Item &it : items) {
        spans.push_back(Span{it.src, it.src + it.words, false});
        spans.push_back(Span{it.dst, it.dst + reach(it), true});
    }
    std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.start < b.start; });
    uint64_t read_end = 0, write_end = 0;  // of the spans in front
    for (const Span &s : spans) {
        if (s.start < write_end || (s.write && s.start < read_end)) return false;
        (s.write ? write_end : read_end) = std::max(s.write ? write_end : read_end, s.end);
    }
    return true;
}

// false: more wave slots than the kernel counts (vertex_block::MAX_WAVES), decided before anything is allocated
inline bool lay_out(const std::vector<Item> &items, std::vector<uint32_t> &block, vertex_block::layout &layout) {
    const uint64_t waves = total_waves(items);
    if (waves > vertex_block::MAX_WAVES || items.size() > 0xFFFFFFFFull) return false;
    const uint32_t n = (uint32_t)items.size();
    layout = vertex_block::lay_out(block, n, REC_WORDS, waves, [&](uint32_t i) { return waves_of(items[i]); });
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t *r = block.data() + (size_t)i * REC_WORDS;
        r[0] = (uint32_t)items[i].src; r[1] = (uint32_t)items[i].dst; r[2] = (uint32_t)units_of(items[i]); r[3] = 0u;
    }
    return true;
}

}  // namespace texel_tail
