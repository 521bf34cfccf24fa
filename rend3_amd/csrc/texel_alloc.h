// texel_alloc.h -- host side of the streamed texture path (r3n_textures_update / r3n_textures_remove): where a texture's words go
// in the texel pool.  The reference keeps one wgpu texture per handle (rend3/src/managers/texture.rs: add / remove); here every
// texture is ONE contiguous range of pool words that starts on a 4-word boundary (the block decoder stores whole 16-byte rows),
// its levels back to back.  Plain C++17, no HIP, no context: tests/texel_alloc_check.cpp compiles it alone.
//
// First fit at the lowest address over a sorted, coalesced free list; what no hole takes is appended behind the high-water mark,
// which gives ascending appends the offsets of a whole-array write: cur = (cur + 3) & ~3, offset = cur, cur += words.  Holes are
// kept in padded form -- [start, (start + words + 3) & ~3) -- so that every hole starts and ends on a 4-word boundary.
//
// Quarantine: a range freed while frames are in flight may still be read by them.  free(.., true) parks it in a second list;
// alloc() takes a clean hole if one fits, and only otherwise merges the parked ranges in (telling the caller, who then waits for
// the frames once) -- a freed tail lowers the high-water mark only at that merge, so words behind the mark are always fresh.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace texel_alloc {

constexpr uint64_t LIMIT = 0xFFFFFFFFull;  // a texture ends at or below this pool word (offsets are 32-bit)
constexpr uint64_t NONE = ~0ull;

inline uint64_t align4(uint64_t v) { return (v + 3u) & ~3ull; }

struct Range {
    uint64_t start, end;  // [start, end), both multiples of 4
};

class Pool {
public:
    // one live prefix [0, words): the state a whole-array write leaves
    void reset(uint64_t words) {
        free_.clear();
        parked_.clear();
        end_ = words;
    }
    uint64_t end() const { return end_; }  // high-water mark: nothing lives at or behind this word
    const std::vector<Range> &holes() const { return free_; }
    const std::vector<Range> &parked() const { return parked_; }
    size_t free_ranges() const { return free_.size() + parked_.size(); }

    // `words` >= 1 words at the lowest address that takes them; NONE (and no change) when the texture would end past LIMIT.
    // *merged (may be null) is set when parked ranges had to be merged in: the caller must have waited for every reader.
    uint64_t alloc(uint64_t words, bool *merged = nullptr) {
        if (merged) *merged = false;
        if (words == 0 || words > LIMIT) return NONE;
        const uint64_t padded = align4(words);
        uint64_t at = take(free_, padded);
        if (at != NONE) return at;
        if (!parked_.empty()) {
            // would the parked ranges -- together with the clean holes and the tail they may free -- take it?
            Pool merged_pool = *this;
            merged_pool.release();
            at = take(merged_pool.free_, padded);
            if (at == NONE && merged_pool.end_ < end_ && align4(merged_pool.end_) + words <= LIMIT) at = merged_pool.append(words);
            if (at != NONE) {
                *this = merged_pool;
                if (merged) *merged = true;
                return at;
            }
        }
        if (align4(end_) + words > LIMIT) return NONE;
        return append(words);
    }

    // gives [start, start + words) back; `park` = frames in flight may still read it
    void free(uint64_t start, uint64_t words, bool park) {
        if (words == 0) return;
        insert(park ? parked_ : free_, Range{start, align4(start + words)});
        if (!park) trim();
    }

    // every reader has been waited for: parked ranges become clean holes
    void release() {
        for (const Range &r : parked_) insert(free_, r);
        parked_.clear();
        trim();
    }

    // The state a compaction leaves (texel_compact.h): `live` = the textures' words [start, end), ascending and disjoint in padded
    // form, start a multiple of 4 (end need not be).  Holes are the complement below the last texture's end, nothing is parked --
    // the caller has waited for every reader.
    void rebuild(const std::vector<Range> &live) {
        free_.clear();
        parked_.clear();
        uint64_t cur = 0;
        for (const Range &r : live) {
            if (r.start > cur) free_.push_back(Range{cur, r.start});
            cur = align4(r.end);
        }
        end_ = live.empty() ? 0 : live.back().end;
    }

private:
    std::vector<Range> free_, parked_;  // each sorted by start, coalesced; disjoint from each other
    uint64_t end_ = 0;

    uint64_t append(uint64_t words) {
        const uint64_t at = align4(end_);
        end_ = at + words;
        return at;
    }
    static uint64_t take(std::vector<Range> &list, uint64_t padded) {
        for (size_t i = 0; i < list.size(); ++i) {
            if (list[i].end - list[i].start < padded) continue;
            const uint64_t at = list[i].start;
            list[i].start += padded;
            if (list[i].start == list[i].end) list.erase(list.begin() + (ptrdiff_t)i);
            return at;
        }
        return NONE;
    }
    static void insert(std::vector<Range> &list, Range r) {
        auto it = std::lower_bound(list.begin(), list.end(), r, [](const Range &a, const Range &b) { return a.start < b.start; });
        if (it != list.end() && it->start <= r.end) {  // touches the hole behind
            r.end = std::max(r.end, it->end);
            it = list.erase(it);
        }
        if (it != list.begin() && (it - 1)->end >= r.start) {  // touches the hole in front
            (it - 1)->end = std::max((it - 1)->end, r.end);
            return;
        }
        list.insert(it, r);
    }
    // a clean hole that reaches the high-water mark is no hole: the mark comes down to its start.  (A parked range at the tail
    // keeps the mark where it is -- those words are not fresh yet -- and with it every hole in front of it.)
    void trim() {
        while (!free_.empty() && free_.back().end >= end_) {
            end_ = std::min(end_, free_.back().start);
            free_.pop_back();
        }
    }
};

}  // namespace texel_alloc
