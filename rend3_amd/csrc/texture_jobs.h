// texture_jobs.h -- host side of the batched texture decode (texture_decode.hip, r3n_internal_decode_jobs): the walk over a
// texture's levels, and the job table that lets ONE launch per kernel family decode every stored level of every texture of a call
// (r3n_textures_write_encoded, r3n_textures_update).  Plain C++17, no HIP, no context: tests/texel_alloc_check.cpp compiles it alone.
//
// A job is one stored level.  Its work units are its 4x4 blocks (block formats: one lane decodes one block) or its texels
// (uncompressed formats: one lane expands one texel); a wave slot takes 64 consecutive units of ONE job, so the job record is
// wave-uniform and a job's last wave slot is partly idle.  The map from wave slot to job is the wave map of the vertex stages
// (vertex_block.h lays the block out, vertex_gather.h reads it): records | wave_first | wave_instance.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/r3n.h"
#include "vertex_block.h"

namespace texture_jobs {

// ---- the chain walk.  A texture is (width, height, mips, pool words per texel: 1 for RGBA8, 4 for f32 texels); its levels lie back
// to back in the pool, level 0 first.  Level k halves each side k times, rounded down, and never goes below 1.
struct Level {
    uint32_t w, h;
    uint64_t words;  // pool words of the level
};
inline Level level_of(uint32_t width, uint32_t height, uint32_t k, uint32_t per_texel) {
    const uint32_t w = std::max(1u, width >> k), h = std::max(1u, height >> k);
    return Level{w, h, (uint64_t)w * h * per_texel};
}
inline uint64_t chain_words(uint32_t width, uint32_t height, uint32_t mips, uint32_t per_texel) {
    uint64_t words = 0;
    for (uint32_t k = 0; k < mips; ++k) words += level_of(width, height, k, per_texel).words;
    return words;
}
// what a texture array refuses about a chain's shape, nullptr when nothing: sides 1 .. 65535, 1 .. floor(log2(longer side)) + 1 levels
inline const char *chain_fault(uint32_t width, uint32_t height, uint32_t mips) {
    if (!width || !height || !mips || width > 65535u || height > 65535u) return "bad extent";
    uint32_t max_mips = 0;
    for (uint32_t m = std::max(width, height); m; m >>= 1) ++max_mips;
    return mips > max_mips ? "more mips than the extent has" : nullptr;
}

enum Family { RGBA8_BLOCK = 0, RGBA8_EXPAND = 1, F32_BLOCK = 2, F32_EXPAND = 3, FAMILIES = 4 };

// one stored level; 8 words, so that a wave reads it as one scalar load
struct Job {
    uint32_t format, w, h;    // R3N_TEXTURE_* of the source, the level's extent
    uint32_t units;           // blocks or texels of the level
    uint32_t src_lo, src_hi;  // byte offset of the level in the staged payload
    uint32_t dst;             // first pool word of the level
    uint32_t pad;             // (the record is a power-of-two count of words; the work-unit prefix is the wave map's wave_first)
};
static_assert(sizeof(Job) == 32, "a job record is 8 words");
constexpr uint32_t REC_WORDS = sizeof(Job) / 4u, UNITS_PER_WAVE = 64u;

inline bool is_float(uint32_t format) { return format >= R3N_TEXTURE_R8_SNORM && format < R3N_TEXTURE_FORMAT_COUNT; }
inline bool is_block(uint32_t format) {
    return is_float(format) ? format >= R3N_TEXTURE_BC4_R_SNORM : format >= R3N_TEXTURE_BC1_RGBA_UNORM;
}
// the RGBA8-decoded formats whose pool words are sRGB-encoded
inline bool is_srgb(uint32_t format) {
    return format == R3N_TEXTURE_RGBA8_UNORM_SRGB || format == R3N_TEXTURE_BGRA8_UNORM_SRGB || format == R3N_TEXTURE_BC1_RGBA_UNORM_SRGB ||
           format == R3N_TEXTURE_BC2_RGBA_UNORM_SRGB || format == R3N_TEXTURE_BC3_RGBA_UNORM_SRGB || format == R3N_TEXTURE_BC7_RGBA_UNORM_SRGB;
}
// bytes of one w x h level in `format`; 0 for an unknown format
inline uint64_t level_bytes(uint32_t format, uint32_t w, uint32_t h) {
    switch (format) {
    case R3N_TEXTURE_RGBA8_UNORM: case R3N_TEXTURE_RGBA8_UNORM_SRGB: case R3N_TEXTURE_BGRA8_UNORM: case R3N_TEXTURE_BGRA8_UNORM_SRGB:
        return (uint64_t)w * h * 4u;
    case R3N_TEXTURE_R8_UNORM: return (uint64_t)w * h;
    case R3N_TEXTURE_RG8_UNORM: return (uint64_t)w * h * 2u;
    case R3N_TEXTURE_BC1_RGBA_UNORM: case R3N_TEXTURE_BC1_RGBA_UNORM_SRGB: case R3N_TEXTURE_BC4_R_UNORM:
        return (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) * 8u;
    case R3N_TEXTURE_BC2_RGBA_UNORM: case R3N_TEXTURE_BC2_RGBA_UNORM_SRGB: case R3N_TEXTURE_BC3_RGBA_UNORM:
    case R3N_TEXTURE_BC3_RGBA_UNORM_SRGB: case R3N_TEXTURE_BC5_RG_UNORM: case R3N_TEXTURE_BC7_RGBA_UNORM:
    case R3N_TEXTURE_BC7_RGBA_UNORM_SRGB: case R3N_TEXTURE_BC5_RG_SNORM: case R3N_TEXTURE_BC6H_RGB_UFLOAT: case R3N_TEXTURE_BC6H_RGB_FLOAT:
        return (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) * 16u;
    case R3N_TEXTURE_BC4_R_SNORM: return (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) * 8u;
    case R3N_TEXTURE_R8_SNORM: return (uint64_t)w * h;
    case R3N_TEXTURE_RG8_SNORM: case R3N_TEXTURE_R16_FLOAT: return (uint64_t)w * h * 2u;
    case R3N_TEXTURE_RGBA8_SNORM: case R3N_TEXTURE_RG16_FLOAT: case R3N_TEXTURE_R32_FLOAT: case R3N_TEXTURE_RGB10A2_UNORM:
    case R3N_TEXTURE_RG11B10_FLOAT: case R3N_TEXTURE_RGB9E5_UFLOAT:
        return (uint64_t)w * h * 4u;
    case R3N_TEXTURE_RGBA16_FLOAT: case R3N_TEXTURE_RG32_FLOAT: case R3N_TEXTURE_RGBA16_UNORM: case R3N_TEXTURE_RGBA16_SNORM:
        return (uint64_t)w * h * 8u;
    case R3N_TEXTURE_RGBA32_FLOAT: return (uint64_t)w * h * 16u;
    default: return 0;
    }
}
inline Family family_of(uint32_t format) {
    return is_float(format) ? (is_block(format) ? F32_BLOCK : F32_EXPAND) : (is_block(format) ? RGBA8_BLOCK : RGBA8_EXPAND);
}
inline uint64_t units_of(uint32_t format, uint32_t w, uint32_t h) {
    return is_block(format) ? (uint64_t)((w + 3u) / 4u) * ((h + 3u) / 4u) : (uint64_t)w * h;
}

// one family's upload: the block (vertex_block layout over `jobs`) and its totals
struct Table {
    std::vector<Job> jobs;
    std::vector<uint32_t> block;
    vertex_block::layout layout{};
    uint64_t total_waves = 0, total_units = 0;
};

// appends one stored level to its family's table
inline void add_level(Table tables[FAMILIES], uint32_t format, uint32_t w, uint32_t h, uint64_t src, uint32_t dst) {
    Table &t = tables[family_of(format)];
    const uint64_t units = units_of(format, w, h);  // < 2^32: extents are at most 65535
    t.jobs.push_back(Job{format, w, h, (uint32_t)units, (uint32_t)src, (uint32_t)(src >> 32), dst, 0u});
    t.total_units += units;
    t.total_waves += vertex_block::waves(units, UNITS_PER_WAVE);
}

// lays every family's block out; false: a family has more wave slots or units than its kernel counts in 32 bits
inline bool finish(Table tables[FAMILIES]) {
    for (int f = 0; f < FAMILIES; ++f) {
        Table &t = tables[f];
        if (t.total_waves > vertex_block::MAX_WAVES || t.total_units > 0xFFFFFFFFull) return false;
        const uint32_t n = (uint32_t)t.jobs.size();
        t.layout = vertex_block::lay_out(t.block, n, REC_WORDS, t.total_waves,
                                         [&](uint32_t i) { return vertex_block::waves(t.jobs[i].units, UNITS_PER_WAVE); });
        if (n) std::memcpy(t.block.data(), t.jobs.data(), (size_t)n * sizeof(Job));
    }
    return true;
}

// a call's four tables and the ONE block it uploads: every table on an 8-word boundary, table f at job_at[f]
struct Work {
    Table tables[FAMILIES];
    size_t job_at[FAMILIES];
    std::vector<uint32_t> job_block;
};
// lays the filled tables out as the ONE block: false when a family has more wave slots than its kernel counts
inline bool finish_work(Work &work) {
    if (!finish(work.tables)) return false;
    size_t words = 0;
    for (int f = 0; f < FAMILIES; ++f) {
        work.job_at[f] = words;
        words += (work.tables[f].block.size() + 7u) & ~(size_t)7u;
    }
    work.job_block.assign(std::max<size_t>(words, 1), 0u);
    for (int f = 0; f < FAMILIES; ++f) std::copy(work.tables[f].block.begin(), work.tables[f].block.end(), work.job_block.begin() + work.job_at[f]);
    return true;
}

}  // namespace texture_jobs
