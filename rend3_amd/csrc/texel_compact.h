// texel_compact.h -- host side of r3n_textures_compact (texture_compact.hip): which words of the texel pool move where, and in
// how many launches.  The streamed path's allocator (texel_alloc.h) never moves a live texture; this plans the slide of every live
// texture towards pool word 0 that closes the holes below the high-water mark.  Plain C++17, no HIP, no context:
// tests/texel_compact_check.cpp compiles it alone.
//
// Order and destinations: textures go in ascending address order, each to dst = align4(end of the one before); none is reordered.
// A texture already there makes no move -- and since the shift src - dst only grows along the pool, every texture behind the first
// one that moves moves too.  All lengths are the padded ones, align4(words): every src, dst and length is a multiple of 4 words (the
// kernel moves 16 bytes per access), the destinations of the moves are ONE contiguous interval, and dst < src for every move.  A
// budget (max_words != 0) stops the plan in front of the first texture whose padded words would exceed it.
//
// Passes: the moves, back to back, are a stream of words; at stream position p the shift is g(p) = src(p) - dst(p).  A thread of
// one launch cannot be ordered against a thread of another workgroup, so a launch never writes a word that the same launch reads
// elsewhere.  DIRECT pass: the next min(remaining, g) words -- their destinations end at or below the first of their sources (g
// only grows), one launch copies them pool -> pool.  STAGED pass, taken when the direct pass would be shorter than
// min(remaining, stage_words): that many words are gathered into a scratch block (one launch) and written from there to their
// destinations (a second launch; stream order is the barrier).  Every pass therefore moves at least min(stage_words, remaining)
// words: launches <= 2 * (ceil(total / stage_words) + 1).  A pass may end inside a texture, at any multiple of 4 words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "texel_alloc.h"
#include "vertex_block.h"

namespace texel_compact {

using texel_alloc::align4;

constexpr uint64_t MIN_STAGE_WORDS = 256;           // a staged pass is at least one wave-instruction pair per lane wide
constexpr uint64_t DEFAULT_STAGE_WORDS = 16u << 20; // 64 MiB of scratch (see r3n.h, r3n_textures_compact)

struct Live {
    uint64_t start, words;  // [start, start + words), start a multiple of 4, words >= 1 (unpadded)
    uint32_t slot;
};
struct Move {  // one texture
    uint32_t slot;
    uint64_t src, dst, words;  // words = the padded length
};
// words [src, src + words) -> [dst, dst + words); in a GATHER segment dst, in a SCATTER segment src counts scratch words
struct Segment {
    uint64_t src, dst, words;
};
enum Kind { DIRECT = 0, GATHER = 1, SCATTER = 2 };
struct Launch {
    Kind kind;
    size_t first_segment, segments;
    uint64_t first_wave, waves;  // its wave slots in the plan's table (lay_out below)
};
struct Pass {
    bool staged;
    uint64_t position, words;  // of the stream
    size_t first_launch;       // one launch (direct) or two (gather, scatter)
};
struct Plan {
    std::vector<Live> live;  // the live set afterwards, ascending
    std::vector<Move> moves;
    std::vector<Segment> segments;
    std::vector<Launch> launches;
    std::vector<Pass> passes;
    uint64_t words_moved = 0;    // the stream's length
    uint64_t scratch_words = 0;  // the longest staged pass
    uint64_t end = 0;            // the high-water mark afterwards
    uint64_t total_waves = 0;
};

// ---- the kernel's table (the wave map of texture_jobs.h / vertex_block.h): one 4-word record per segment, a wave slot takes
// UNITS_PER_WAVE consecutive 16-byte units of ONE segment
struct Record {
    uint32_t src, dst, units, pad;  // src / dst in words, units = words / 4
};
static_assert(sizeof(Record) == 16, "a segment record is 4 words");
constexpr uint32_t REC_WORDS = sizeof(Record) / 4u, LOADS_PER_LANE = 4u, UNITS_PER_WAVE = 64u * LOADS_PER_LANE;
constexpr uint64_t WORDS_PER_WAVE = 4ull * UNITS_PER_WAVE;

inline uint64_t waves_of(const Segment &s) { return vertex_block::waves(s.words / 4u, UNITS_PER_WAVE); }

// `live` in any order; ranges disjoint in padded form.  stage_words: a multiple of 4, >= MIN_STAGE_WORDS.
inline Plan plan(std::vector<Live> live, uint64_t max_words, uint64_t stage_words) {
    Plan p;
    std::sort(live.begin(), live.end(), [](const Live &a, const Live &b) { return a.start < b.start; });
    // ---- destinations
    uint64_t cur = 0;  // end of the one before
    size_t i = 0;
    for (; i < live.size(); ++i) {
        const Live &t = live[i];
        const uint64_t dst = align4(cur), padded = align4(t.words);
        if (dst != t.start) {
            if (max_words && p.words_moved + padded > max_words) break;
            p.moves.push_back(Move{t.slot, t.start, dst, padded});
            p.words_moved += padded;
        }
        p.live.push_back(Live{dst, t.words, t.slot});
        cur = dst + t.words;
    }
    for (; i < live.size(); ++i) p.live.push_back(live[i]);  // behind the budget: untouched
    p.end = p.live.empty() ? 0 : p.live.back().start + p.live.back().words;
    if (p.moves.empty()) return p;

    // ---- passes over the stream
    const uint64_t total = p.words_moved, dst0 = p.moves[0].dst;
    size_t m = 0;          // the move that holds stream position `at`
    uint64_t m_first = 0;  // its first stream position
    // appends the segments of stream words [at, at + n) to the current launch; advances (m, m_first) to the move holding at + n
    auto cut = [&](uint64_t at, uint64_t n, Kind kind) {
        Launch l{kind, p.segments.size(), 0, p.total_waves, 0};
        if (kind == SCATTER) {  // scratch and the destinations are both contiguous: one segment
            p.segments.push_back(Segment{0, dst0 + at, n});
        } else {
            size_t k = m;
            uint64_t k_first = m_first;
            for (uint64_t done = 0; done < n;) {
                const Move &mv = p.moves[k];
                const uint64_t inside = at + done - k_first, take = std::min(n - done, mv.words - inside);
                p.segments.push_back(Segment{mv.src + inside, kind == GATHER ? done : mv.dst + inside, take});
                done += take;
                if (inside + take == mv.words) {
                    k_first += mv.words;
                    ++k;
                }
            }
            if (kind == DIRECT || kind == GATHER) { m = k; m_first = k_first; }
        }
        l.segments = p.segments.size() - l.first_segment;
        for (size_t s = l.first_segment; s < p.segments.size(); ++s) l.waves += waves_of(p.segments[s]);
        p.total_waves += l.waves;
        p.launches.push_back(l);
    };
    for (uint64_t at = 0; at < total;) {
        const uint64_t remaining = total - at, g = p.moves[m].src - p.moves[m].dst;
        const uint64_t direct = std::min(remaining, g), staged = std::min(remaining, stage_words);
        Pass pass{direct < staged, at, direct < staged ? staged : direct, p.launches.size()};
        if (pass.staged) {
            cut(at, pass.words, GATHER);
            cut(at, pass.words, SCATTER);
            p.scratch_words = std::max(p.scratch_words, pass.words);
        } else {
            cut(at, pass.words, DIRECT);
        }
        p.passes.push_back(pass);
        at += pass.words;
    }
    return p;
}

// The plan's table, every launch's segments in launch order: records | wave_first | wave_instance (vertex_block.h).  A launch
// covers wave slots [first_wave, first_wave + waves).  false: more wave slots than the kernel counts.
inline bool lay_out(const Plan &p, std::vector<uint32_t> &block, vertex_block::layout &layout) {
    if (p.total_waves > vertex_block::MAX_WAVES || p.segments.size() > 0xFFFFFFFFull) return false;
    const uint32_t n = (uint32_t)p.segments.size();
    layout = vertex_block::lay_out(block, n, REC_WORDS, p.total_waves, [&](uint32_t i) { return waves_of(p.segments[i]); });
    for (uint32_t i = 0; i < n; ++i) {
        const Segment &s = p.segments[i];
        uint32_t *r = block.data() + (size_t)i * REC_WORDS;
        r[0] = (uint32_t)s.src; r[1] = (uint32_t)s.dst; r[2] = (uint32_t)(s.words / 4u); r[3] = 0u;
    }
    return true;
}

// the allocator after the plan: holes = the complement of the live set below the new mark, in padded form; nothing parked
inline void rebuild(texel_alloc::Pool &pool, const Plan &p) {
    std::vector<texel_alloc::Range> ranges;
    ranges.reserve(p.live.size());
    for (const Live &t : p.live) ranges.push_back(texel_alloc::Range{t.start, t.start + t.words});
    pool.rebuild(ranges);
}

}  // namespace texel_compact
