// cube_plan.h -- host side of the cube-texture uploads (r3n_texture_cubes_write, r3n_texture_cubes_write_encoded,
// r3n_texture_cubes_write_sources): everything the three entries decide before the first HIP call.  What a source is refused for,
// where every cube, level and face lies in the pool (cube_faces.h) and in the call's scratch block, the decode jobs of the stored
// levels (texture_jobs.h), the records that resample panoramas and build their chains (equirect.h, equirect_rule.h), the records
// of the launch that borders every face of the call (k_cube_assemble), and the byte offsets of the scratch block's parts.  Plain
// C++17, no HIP, no context: tests/cube_plan_check.cpp compiles it alone.
//
// The scratch block of one call, every part on a 256-byte boundary:
//     payload | job tables | assemble table | equirect tables | dense
// "dense", in 32-bit words: a panorama that is not RGBE8 decoded to one level, and the six dense (borderless) faces of every level
// of every cube, a level's faces back to back, each on a 4-word boundary.  Stored levels are decoded into them, a panorama's level 0
// is resampled into them and its chain built face by face; the assemble launch reads them all and writes the pool.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/r3n.h"
#include "cube_faces.h"
#include "equirect.h"
#include "texture_jobs.h"
#include "vertex_block.h"

namespace cube_plan {

// a cube as the context holds it: first pool word, extent, whether its words are sRGB-encoded, levels, pool class (0: RGBA8 words,
// 1: sRGB RGBA8 words, 2: four f32 per texel)
struct Cube { size_t first_word; uint32_t n, srgb, mips = 1, cls = 0; };

// One cube of a call.  from_desc: made of an r3n_texture_desc32 (stored faces; face_extent = width) -- the checks, their order and
// their words are then those of r3n_texture_cubes_write_encoded, which alone looks at stored_mips; otherwise those of
// r3n_texture_cubes_write_sources.  `offset` in bytes of the payload: 64 bits, the plain entry's texel offsets times four.
struct Source {
    uint32_t kind, format, width, height, face_extent, mips, stored_mips;
    uint64_t offset;
    bool from_desc;
};
inline Source from_source(const r3n_cube_source &s) { return Source{s.kind, s.format, s.width, s.height, s.face_extent, s.mips, 0u, s.offset, false}; }
inline Source from_desc(const r3n_texture_desc32 &d) {
    return Source{R3N_CUBE_SOURCE_CUBE, d.format, d.width, d.height, d.width, d.mips, d.stored_mips, d.offset, true};
}

// R3N_OK, or an R3N_ERR_* code and the tail of the message behind the entry's name
struct Refusal { int code = R3N_OK; const char *why = nullptr; };

// bytes of the chain of ONE stored face: its levels lie back to back (LayerMajor)
inline uint64_t face_chain_bytes(uint32_t format, uint32_t n0, uint32_t mips) {
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < mips; ++k) bytes += texture_jobs::level_bytes(format, cube_faces::level_extent(n0, k), cube_faces::level_extent(n0, k));
    return bytes;
}

// what one source is refused for by itself and against the payload
inline Refusal fault(const Source &s, uint64_t payload_bytes) {
    const bool equi = !s.from_desc && s.kind == R3N_CUBE_SOURCE_EQUIRECT, rgbe = equi && s.format == R3N_CUBE_ENCODING_RGBE8;
    if (s.from_desc) {
        if (s.format >= R3N_TEXTURE_FORMAT_COUNT) return {R3N_ERR_INVALID_ARG, "unknown format id"};
        if (s.width != s.height) return {R3N_ERR_INVALID_ARG, "a cube's faces are square"};
        if (!s.width || s.width > equirect_rule::MAX_FACE_EXTENT) return {R3N_ERR_INVALID_ARG, "bad extent"};
        if (const char *chain = texture_jobs::chain_fault(s.width, s.height, s.mips)) return {R3N_ERR_INVALID_ARG, chain};
        if (s.stored_mips && s.stored_mips != s.mips)
            return {R3N_ERR_UNSUPPORTED, "a cube carries all its levels (no MipmapSource::Generated for cubes, rend3/src/managers/texture.rs:147)"};
        if ((s.offset & 3u) != 0u) return {R3N_ERR_INVALID_ARG, "face +X level 0 must start on a 4-byte boundary"};
    } else {
        if (s.kind != R3N_CUBE_SOURCE_CUBE && s.kind != R3N_CUBE_SOURCE_EQUIRECT) return {R3N_ERR_INVALID_ARG, "unknown source kind"};
        if (!rgbe && s.format >= R3N_TEXTURE_FORMAT_COUNT) return {R3N_ERR_INVALID_ARG, "unknown format id"};
        if (!s.width || !s.height || !s.face_extent) return {R3N_ERR_INVALID_ARG, "zero extent"};
        if (s.width > equirect_rule::MAX_SOURCE_EXTENT || s.height > equirect_rule::MAX_SOURCE_EXTENT) return {R3N_ERR_INVALID_ARG, "a source extent above 65535"};
        if (s.face_extent > equirect_rule::MAX_FACE_EXTENT) return {R3N_ERR_INVALID_ARG, "a face extent above 16384"};
        if (!equi && (s.width != s.height || s.width != s.face_extent)) return {R3N_ERR_INVALID_ARG, "a cube's faces are square, of the face extent"};
        if (!s.mips || s.mips > equirect_rule::max_mips(s.face_extent)) return {R3N_ERR_INVALID_ARG, "more mips than the extent has"};
        if ((s.offset & 3u) != 0u) return {R3N_ERR_INVALID_ARG, "a source must start on a 4-byte boundary"};
    }
    const uint64_t bytes = !equi ? 6u * face_chain_bytes(s.format, s.face_extent, s.mips)
                                 : (rgbe ? (uint64_t)s.width * s.height * 4u : texture_jobs::level_bytes(s.format, s.width, s.height));
    if (s.offset > payload_bytes || bytes > payload_bytes - s.offset) return {R3N_ERR_INVALID_ARG, s.from_desc ? "faces outside the payload" : "data outside the payload"};
    return {};
}

// ---- a wave-mapped table: records | wave_first | wave_instance (vertex_block.h), a wave slot taking `per_wave` units of ONE record
struct WaveTable {
    std::vector<uint32_t> block;
    vertex_block::layout layout{};
    uint64_t waves = 0;
};
// lays the table out over `recs` (a record type of whole words with a `units` member); false: more wave slots than a kernel counts
template <class Rec>
bool lay_table(WaveTable &t, const std::vector<Rec> &recs, uint32_t per_wave) {
    static_assert(sizeof(Rec) % 4u == 0u, "a record is whole words");
    t.waves = 0;
    for (const Rec &r : recs) t.waves += vertex_block::waves(r.units, per_wave);
    if (t.waves > vertex_block::MAX_WAVES || recs.size() > 0xFFFFFFFFull) return false;
    t.layout = vertex_block::lay_out(t.block, (uint32_t)recs.size(), sizeof(Rec) / 4u, t.waves, [&](uint32_t i) { return vertex_block::waves(recs[i].units, per_wave); });
    if (!recs.empty()) std::memcpy(t.block.data(), recs.data(), recs.size() * sizeof(Rec));
    return true;
}

// ---- the six assemble records of ONE level of one cube: the only statement of where a level's dense faces lie in a dense block
// (six faces `dense_face_words` apart from `dense_at`) and where its bordered faces lie in the pool (from `level_at`).  Returns the
// words from one dense face to the next.
inline uint64_t add_level_records(std::vector<cube_faces::Record> &recs, uint32_t nk, uint32_t per_texel, uint64_t dense_at, uint64_t level_at) {
    const uint64_t stride = cube_faces::dense_face_words(nk, per_texel), units = (uint64_t)(nk + 2u) * (nk + 2u);
    for (uint32_t f = 0; f < 6u; ++f)
        recs.push_back(cube_faces::Record{nk, f, per_texel, (uint32_t)units, (uint32_t)dense_at, (uint32_t)stride,
                                          (uint32_t)(level_at + f * cube_faces::face_words(nk, per_texel)), 0u});
    return stride;
}

// ---- the plan of one call
struct Launch { size_t at; vertex_block::layout layout; uint64_t waves; };  // one wave-mapped table inside eq_block, from word `at`
struct Plan {
    std::vector<Cube> cubes;
    uint64_t pool_words = 0, dense_words = 0;
    texture_jobs::Work jobs;  // the stored levels (and the panoramas that are not RGBE8), decoded into `dense`
    WaveTable assemble;       // cube_faces::Record per (cube, level, face)
    // the equirect tables as ONE block: faces | level 1 | level 2 | ... | tail records, each on a 16-word boundary
    std::vector<uint32_t> eq_block;
    std::vector<Launch> eq_launches;  // [0]: k_equirect_faces, then the level launches
    size_t tail_at = 0;               // first word of the tail records in eq_block
    uint32_t tail_recs = 0;
    // byte offsets of the parts of the scratch block, and its size
    uint64_t jobs_at = 0, asm_at = 0, eq_at = 0, dense_at = 0, scratch_bytes = 0;
};

inline uint64_t align256(uint64_t bytes) { return (bytes + 255u) & ~255ull; }

// R3N_OK and `out`, or the refusal of the first source in array order that has one (nothing in `out` is then meaningful).
// equirect_tail: a panorama's face of at most this extent builds the rest of its chain in one launch (equirect_rule::tail_from).
inline Refusal plan(const Source *sources, uint32_t n, uint64_t payload_bytes, uint32_t equirect_tail, Plan &out) {
    out = Plan{};
    out.cubes.resize(n);
    std::vector<cube_faces::Record> recs;
    std::vector<equirect::FaceRec> face_recs;
    std::vector<std::vector<equirect::ChainRec>> level_recs;  // [k - 1]: level launch k
    std::vector<equirect::ChainRec> tail_recs;
    uint64_t pool_words = 0, dense_words = 0;
    for (uint32_t ci = 0; ci < n; ++ci) {
        const Source &s = sources[ci];
        const Refusal refused = fault(s, payload_bytes);
        if (refused.code != R3N_OK) return refused;
        const bool equi = s.kind == R3N_CUBE_SOURCE_EQUIRECT, rgbe = equi && s.format == R3N_CUBE_ENCODING_RGBE8;
        const uint32_t N = s.face_extent, per_texel = equi || texture_jobs::is_float(s.format) ? 4u : 1u;
        const uint64_t words = cube_faces::cube_words(N, s.mips, per_texel);
        if (pool_words + words > 0xFFFFFFFFull) return {R3N_ERR_CAPACITY, "the cube pool exceeds 2^32 words"};
        const bool srgb = !equi && texture_jobs::is_srgb(s.format);
        out.cubes[ci] = {(size_t)pool_words, N, srgb ? 1u : 0u, s.mips, per_texel == 4u ? 2u : (srgb ? 1u : 0u)};
        // an equirect source that is not RGBE is decoded by the 2D job tables into the scratch block, in front of the cube's faces
        uint64_t decoded_at = 0;
        uint32_t mode = equirect::SOURCE_RGBE8;
        if (equi && !rgbe) {
            const bool f32 = texture_jobs::is_float(s.format);
            mode = f32 ? equirect::SOURCE_F32 : (texture_jobs::is_srgb(s.format) ? equirect::SOURCE_RGBA8_SRGB : equirect::SOURCE_RGBA8);
            decoded_at = dense_words;
            dense_words += ((uint64_t)s.width * s.height * (f32 ? 4u : 1u) + 3u) & ~3ull;
            if (dense_words > 0xFFFFFFFFull) return {R3N_ERR_CAPACITY, "the scratch block exceeds 2^32 words"};
            texture_jobs::add_level(out.jobs.tables, s.format, s.width, s.height, s.offset, (uint32_t)decoded_at);
        }
        const uint32_t from = equi ? equirect_rule::tail_from(N, s.mips, equirect_tail) : 0u;
        const uint64_t face_bytes = equi ? 0u : face_chain_bytes(s.format, N, s.mips);
        uint64_t level_at = pool_words, above_at = 0, level_byte = 0;  // level_byte: of level k inside a stored face's chain
        for (uint32_t k = 0; k < s.mips; ++k) {
            const uint32_t nk = cube_faces::level_extent(N, k);
            const uint64_t stride = cube_faces::dense_face_words(nk, per_texel);
            if (dense_words + 6u * stride > 0xFFFFFFFFull) return {R3N_ERR_CAPACITY, "the scratch block exceeds 2^32 words"};
            add_level_records(recs, nk, per_texel, dense_words, level_at);
            for (uint32_t f = 0; f < 6u; ++f) {
                const uint32_t dense_face = (uint32_t)(dense_words + f * stride);
                if (!equi) {
                    // LayerMajor: face f's levels lie back to back
                    texture_jobs::add_level(out.jobs.tables, s.format, nk, nk, s.offset + f * face_bytes + level_byte, dense_face);
                } else if (k == 0u) {
                    equirect::FaceRec r{};
                    r.n = N; r.face = f; r.mode = mode; r.W = s.width; r.H = s.height;
                    r.src_lo = rgbe ? (uint32_t)s.offset : (uint32_t)decoded_at;
                    r.src_hi = rgbe ? (uint32_t)(s.offset >> 32) : 0u;
                    r.dst = dense_face;
                    r.units = N * N;
                    face_recs.push_back(r);
                } else if (k <= from) {
                    const uint32_t sk = cube_faces::level_extent(N, k - 1u);
                    if (level_recs.size() < k) level_recs.resize(k);
                    level_recs[k - 1u].push_back(equirect::ChainRec{sk, nk, (uint32_t)(above_at + f * cube_faces::dense_face_words(sk, 4u)), dense_face, nk * nk, f, 1u, 0u});
                } else if (k == from + 1u) {
                    tail_recs.push_back(equirect::ChainRec{cube_faces::level_extent(N, from), nk, (uint32_t)above_at, (uint32_t)dense_words, 0u, f, s.mips - 1u - from, 0u});
                }
            }
            above_at = dense_words;
            dense_words += 6u * stride;
            level_at += cube_faces::level_words(nk, per_texel);
            if (!equi) level_byte += texture_jobs::level_bytes(s.format, nk, nk);
        }
        pool_words += words;
    }
    out.pool_words = pool_words;
    out.dense_words = dense_words;
    if (!texture_jobs::finish_work(out.jobs) || !lay_table(out.assemble, recs, cube_faces::UNITS_PER_WAVE))
        return {R3N_ERR_CAPACITY, "more than 2^31 wave slots of decode or assemble work in one call"};
    auto add_table = [&](const auto &table_recs) {
        WaveTable t;
        if (!lay_table(t, table_recs, equirect::UNITS_PER_WAVE)) return false;
        out.eq_launches.push_back(Launch{out.eq_block.size(), t.layout, t.waves});
        out.eq_block.insert(out.eq_block.end(), t.block.begin(), t.block.end());
        out.eq_block.resize((out.eq_block.size() + 15u) & ~(size_t)15u, 0u);
        return true;
    };
    bool fits = true;
    if (!face_recs.empty()) {
        fits = add_table(face_recs);
        for (size_t k = 0; k < level_recs.size() && fits; ++k) fits = add_table(level_recs[k]);
    }
    if (!fits) return {R3N_ERR_CAPACITY, "more than 2^31 wave slots of resampling work in one call"};
    out.tail_at = out.eq_block.size();
    out.tail_recs = (uint32_t)tail_recs.size();
    out.eq_block.resize(out.tail_at + tail_recs.size() * equirect::CHAIN_REC_WORDS, 0u);
    if (!tail_recs.empty()) std::memcpy(out.eq_block.data() + out.tail_at, tail_recs.data(), tail_recs.size() * sizeof(equirect::ChainRec));
    out.jobs_at = align256(std::max<uint64_t>(payload_bytes, 4));
    out.asm_at = align256(out.jobs_at + out.jobs.job_block.size() * 4u);
    out.eq_at = align256(out.asm_at + out.assemble.block.size() * 4u);
    out.dense_at = align256(out.eq_at + out.eq_block.size() * 4u);
    out.scratch_bytes = out.dense_at + std::max<uint64_t>(dense_words, 4) * 4u;
    return {};
}

// ---- one more cube of the f32 class behind the array's last (r3n_environment_prefilter): where it lies in the pool, the first word
// of every level's six dense faces in a dense block of the call's own (the same dense layout as above: a level's faces back to
// back), and the assemble table of its faces.  The existing cubes keep their words.
struct Append {
    Cube cube;
    uint64_t pool_words = 0, dense_words = 0;  // the pool with the new cube; the dense block
    std::vector<uint32_t> level_dense;         // [k]: first dense word of level k
    WaveTable assemble;
};
inline uint64_t pool_end(const std::vector<Cube> &cubes) {
    if (cubes.empty()) return 0u;
    const Cube &last = cubes.back();
    return last.first_word + cube_faces::cube_words(last.n, last.mips, last.cls == 2u ? 4u : 1u);
}
inline Refusal plan_append(const std::vector<Cube> &cubes, uint32_t N, uint32_t mips, Append &out) {
    out = Append{};
    constexpr uint32_t per_texel = 4u;
    const uint64_t first = pool_end(cubes), words = cube_faces::cube_words(N, mips, per_texel);
    if (first + words > 0xFFFFFFFFull) return {R3N_ERR_CAPACITY, "the cube pool exceeds 2^32 words"};
    out.cube = Cube{(size_t)first, N, 0u, mips, 2u};
    std::vector<cube_faces::Record> recs;
    uint64_t level_at = first, dense_words = 0;
    for (uint32_t k = 0; k < mips; ++k) {
        const uint32_t nk = cube_faces::level_extent(N, k);
        if (dense_words + 6u * cube_faces::dense_face_words(nk, per_texel) > 0xFFFFFFFFull) return {R3N_ERR_CAPACITY, "the scratch block exceeds 2^32 words"};
        out.level_dense.push_back((uint32_t)dense_words);
        dense_words += 6u * add_level_records(recs, nk, per_texel, dense_words, level_at);
        level_at += cube_faces::level_words(nk, per_texel);
    }
    out.pool_words = first + words;
    out.dense_words = dense_words;
    if (!lay_table(out.assemble, recs, cube_faces::UNITS_PER_WAVE)) return {R3N_ERR_CAPACITY, "more than 2^31 wave slots of assemble work in one call"};
    return {};
}

}  // namespace cube_plan
