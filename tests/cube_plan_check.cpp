// Stand-alone check of rend3_amd/csrc/cube_plan.h (what the three cube-upload entries refuse, lay out and tabulate before their
// first HIP call), built plain and with the address and undefined-behaviour sanitizers and run as a child process by
// tests/test_cube_plan.py.  Every plan is walked the way the launches read it -- decode jobs, k_equirect_faces, the level launches,
// the tail launch, k_cube_assemble -- over sets of word ranges instead of memory.  A failed case prints FAIL and the exit status is 1.
//
//   cube_plan_check                                         every array below; one "name values" line each
//   cube_plan_check refuse ENTRY PAYLOAD_BYTES TAIL N (KIND FORMAT WIDTH HEIGHT EXTENT MIPS OFFSET STORED) x N
//                                                           ENTRY = encoded | sources: "code message" of the planner for that array,
//                                                           "0 accepted" when it plans
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../rend3_amd/csrc/cube_plan.h"

using namespace cube_plan;

static int failures = 0;
static const char *context = "";
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) printf("FAIL line_%d %s [%s]\n", __LINE__, #cond, context); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// ---- the formats of the arrays, restated: bytes of a level, pool words per texel
static const uint32_t RGBA8 = R3N_TEXTURE_RGBA8_UNORM, RGBA8_SRGB = R3N_TEXTURE_RGBA8_UNORM_SRGB, BC6H = R3N_TEXTURE_BC6H_RGB_UFLOAT,
                      RGBE8 = R3N_CUBE_ENCODING_RGBE8;
static uint64_t bytes_of(uint32_t format, uint32_t w, uint32_t h) {
    if (format == BC6H) return (uint64_t)((w + 3) / 4) * ((h + 3) / 4) * 16;
    return (uint64_t)w * h * 4;  // RGBA8, RGBA8_SRGB, RGBE8
}
static uint32_t halved(uint32_t n, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i) n = n > 1 ? n / 2 : 1;
    return n;
}
static uint32_t full_chain(uint32_t n) {
    uint32_t m = 0;
    for (; n; n /= 2) ++m;
    return m;
}

// an array under construction: every source appended at a 4-byte boundary of the payload
struct Array {
    std::vector<r3n_cube_source> sources;
    uint64_t payload_bytes = 0;
    void stored(uint32_t format, uint32_t n, uint32_t mips) {
        payload_bytes = (payload_bytes + 3u) & ~3ull;
        sources.push_back(r3n_cube_source{R3N_CUBE_SOURCE_CUBE, format, n, n, n, mips, payload_bytes});
        for (uint32_t k = 0; k < mips; ++k) payload_bytes += 6u * bytes_of(format, halved(n, k), halved(n, k));
    }
    void panorama(uint32_t format, uint32_t w, uint32_t h, uint32_t n, uint32_t mips) {
        payload_bytes = (payload_bytes + 3u) & ~3ull;
        sources.push_back(r3n_cube_source{R3N_CUBE_SOURCE_EQUIRECT, format, w, h, n, mips, payload_bytes});
        payload_bytes += bytes_of(format, w, h);
    }
    void append(const Array &other) {
        for (const r3n_cube_source &s : other.sources) {
            if (s.kind == R3N_CUBE_SOURCE_CUBE) stored(s.format, s.face_extent, s.mips);
            else panorama(s.format, s.width, s.height, s.face_extent, s.mips);
        }
    }
};

static Refusal plan_sources(const Array &a, uint32_t tail, Plan &out) {
    std::vector<Source> sources;
    for (const r3n_cube_source &s : a.sources) sources.push_back(from_source(s));
    return plan(sources.data(), (uint32_t)sources.size(), a.payload_bytes, tail, out);
}

static bool same_table(const texture_jobs::Table &a, const texture_jobs::Table &b) {
    return a.block == b.block && a.layout.o_first == b.layout.o_first && a.layout.o_inst == b.layout.o_inst && a.total_waves == b.total_waves &&
           a.total_units == b.total_units;
}
static bool same_plan(const Plan &a, const Plan &b) {
    bool same = a.cubes.size() == b.cubes.size() && a.pool_words == b.pool_words && a.dense_words == b.dense_words;
    for (size_t i = 0; same && i < a.cubes.size(); ++i)
        same = a.cubes[i].first_word == b.cubes[i].first_word && a.cubes[i].n == b.cubes[i].n && a.cubes[i].srgb == b.cubes[i].srgb &&
               a.cubes[i].mips == b.cubes[i].mips && a.cubes[i].cls == b.cubes[i].cls;
    for (int f = 0; same && f < texture_jobs::FAMILIES; ++f) same = same_table(a.jobs.tables[f], b.jobs.tables[f]) && a.jobs.job_at[f] == b.jobs.job_at[f];
    return same && a.jobs.job_block == b.jobs.job_block && a.assemble.block == b.assemble.block && a.assemble.waves == b.assemble.waves &&
           a.assemble.layout.o_first == b.assemble.layout.o_first && a.assemble.layout.o_inst == b.assemble.layout.o_inst && a.eq_block == b.eq_block &&
           a.eq_launches.size() == b.eq_launches.size() && a.tail_at == b.tail_at && a.tail_recs == b.tail_recs && a.jobs_at == b.jobs_at &&
           a.asm_at == b.asm_at && a.eq_at == b.eq_at && a.dense_at == b.dense_at && a.scratch_bytes == b.scratch_bytes;
}

// records | wave_first | wave_instance: the maps give every record's wave count back, and the counts add up to the launch's total
static void check_wave_map(const uint32_t *block, size_t block_words, const vertex_block::layout &l, uint32_t n, size_t rec_words, size_t units_word,
                           uint32_t per_wave, uint64_t total) {
    CHECK(l.o_first == (size_t)n * rec_words && l.o_inst == l.o_first + n && l.o_inst + total <= block_words);
    if (l.o_inst + total > block_words) return;
    uint64_t slot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t waves = ((uint64_t)block[i * rec_words + units_word] + per_wave - 1u) / per_wave;
        CHECK(block[l.o_first + i] == slot);
        for (uint64_t w = 0; w < waves && slot + w < total; ++w) CHECK(block[l.o_inst + slot + w] == i);
        slot += waves;
    }
    CHECK(slot == total);
}

static uint64_t arrays = 0, records = 0, jobs = 0, resampled = 0;

struct Face {  // a dense face of the scratch block: whose it is, and whether a launch in front of the assemble has written it
    uint32_t cube, level, face, n, per_texel;
    bool written;
};

static void check_plan(const Array &a, uint32_t tail, const Plan &p) {
    ++arrays;
    const uint32_t n = (uint32_t)a.sources.size();
    CHECK(p.cubes.size() == n);
    if (p.cubes.size() != n) return;
    // ---- the scratch block: payload | job tables | assemble table | equirect tables | dense
    CHECK(p.jobs_at >= a.payload_bytes && p.asm_at >= p.jobs_at + p.jobs.job_block.size() * 4u && p.eq_at >= p.asm_at + p.assemble.block.size() * 4u &&
          p.dense_at >= p.eq_at + p.eq_block.size() * 4u && p.scratch_bytes >= p.dense_at + p.dense_words * 4u);
    CHECK(p.jobs_at % 256u == 0u && p.asm_at % 256u == 0u && p.eq_at % 256u == 0u && p.dense_at % 256u == 0u);
    CHECK(p.dense_words <= 0xFFFFFFFFull && p.pool_words <= 0xFFFFFFFFull);

    // ---- the assemble records: 6 per level, in cube, level, face order; bordered faces inside their cube, levels on 4 words
    uint32_t total_recs = 0;
    for (const r3n_cube_source &s : a.sources) total_recs += 6u * s.mips;
    CHECK(p.assemble.block.size() >= (size_t)total_recs * cube_faces::REC_WORDS);
    if (p.assemble.block.size() < (size_t)total_recs * cube_faces::REC_WORDS) return;
    const cube_faces::Record *recs = reinterpret_cast<const cube_faces::Record *>(p.assemble.block.data());
    check_wave_map(p.assemble.block.data(), p.assemble.block.size(), p.assemble.layout, total_recs, cube_faces::REC_WORDS, 3, cube_faces::UNITS_PER_WAVE, p.assemble.waves);
    std::map<uint64_t, Face> dense;            // by first word
    std::map<uint64_t, uint64_t> pool_ranges;  // first word -> end, of every bordered face
    uint32_t ri = 0;
    uint64_t cube_end = 0;
    for (uint32_t ci = 0; ci < n; ++ci) {
        const r3n_cube_source &s = a.sources[ci];
        const Cube &cube = p.cubes[ci];
        const bool equi = s.kind == R3N_CUBE_SOURCE_EQUIRECT;
        const uint32_t per = equi || s.format == BC6H ? 4u : 1u;
        CHECK(cube.n == s.face_extent && cube.mips == s.mips && cube.cls == (per == 4u ? 2u : (s.format == RGBA8_SRGB ? 1u : 0u)) &&
              cube.srgb == (!equi && s.format == RGBA8_SRGB ? 1u : 0u));
        CHECK(cube.first_word % 4u == 0u && cube.first_word >= cube_end);
        // the cube's words, restated: per level 6 (n + 2)^2 per_texel, padded to 4
        uint64_t words = 0;
        for (uint32_t k = 0; k < s.mips; ++k) {
            const uint64_t nk = halved(s.face_extent, k), level_start = cube.first_word + words;
            CHECK(level_start % 4u == 0u);
            for (uint32_t f = 0; f < 6u; ++f, ++ri) {
                const cube_faces::Record &r = recs[ri];
                CHECK(r.n == nk && r.face == f && r.per_texel == per && r.units == (nk + 2u) * (nk + 2u));
                CHECK(r.dst == level_start + f * (nk + 2u) * (nk + 2u) * per);
                CHECK(pool_ranges.emplace(r.dst, r.dst + (uint64_t)r.units * per).second);
                CHECK(r.src % 4u == 0u && r.src_stride % 4u == 0u && r.src_stride >= nk * nk * per);
                const uint64_t at = r.src + (uint64_t)f * r.src_stride;
                CHECK(at + nk * nk * per <= p.dense_words);
                CHECK(dense.emplace(at, Face{ci, k, f, (uint32_t)nk, per, false}).second);
            }
            words += (6u * (nk + 2u) * (nk + 2u) * per + 3u) & ~3ull;
        }
        cube_end = cube.first_word + words;
        for (auto it = pool_ranges.lower_bound(cube.first_word); it != pool_ranges.end(); ++it) CHECK(it->second <= cube_end);
    }
    CHECK(cube_end == p.pool_words || (n == 0 && p.pool_words == 0));
    records += total_recs;
    uint64_t prev_end = 0;
    for (const auto &range : pool_ranges) {  // no two bordered faces overlap
        CHECK(range.first >= prev_end);
        prev_end = range.second;
    }
    prev_end = 0;
    for (const auto &face : dense) {  // nor two dense faces
        CHECK(face.first >= prev_end);
        prev_end = face.first + (uint64_t)face.second.n * face.second.n * face.second.per_texel;
    }

    // ---- the decode jobs: sources inside the payload, destinations inside `dense`; a stored level is its cube's dense face
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> decoded;  // a panorama decoded to one level: first word -> (w, h)
    size_t block_at = 0;
    for (int f = 0; f < texture_jobs::FAMILIES; ++f) {
        const texture_jobs::Table &t = p.jobs.tables[f];
        CHECK(p.jobs.job_at[f] == block_at && block_at % 8u == 0u && block_at + t.block.size() <= p.jobs.job_block.size());
        CHECK(t.block.empty() || memcmp(p.jobs.job_block.data() + block_at, t.block.data(), t.block.size() * 4u) == 0);
        block_at += (t.block.size() + 7u) & ~(size_t)7u;
        check_wave_map(t.block.data(), t.block.size(), t.layout, (uint32_t)t.jobs.size(), texture_jobs::REC_WORDS, 3, texture_jobs::UNITS_PER_WAVE, t.total_waves);
        for (const texture_jobs::Job &j : t.jobs) {
            ++jobs;
            const uint64_t src = j.src_lo | (uint64_t)j.src_hi << 32, per = j.format == BC6H ? 4u : 1u;
            CHECK(src % 4u == 0u && src + bytes_of(j.format, j.w, j.h) <= a.payload_bytes);
            CHECK(j.dst % 4u == 0u && j.dst + (uint64_t)j.w * j.h * per <= p.dense_words);
            auto face = dense.find(j.dst);
            if (face != dense.end() && a.sources[face->second.cube].kind == R3N_CUBE_SOURCE_CUBE) {
                CHECK(!face->second.written && j.w == face->second.n && j.h == face->second.n && per == face->second.per_texel);
                face->second.written = true;
                // LayerMajor: face f's levels back to back from the source's offset
                const r3n_cube_source &s = a.sources[face->second.cube];
                uint64_t chain = 0, above = 0;
                for (uint32_t k = 0; k < s.mips; ++k) {
                    if (k < face->second.level) above += bytes_of(s.format, halved(s.face_extent, k), halved(s.face_extent, k));
                    chain += bytes_of(s.format, halved(s.face_extent, k), halved(s.face_extent, k));
                }
                CHECK(src == s.offset + face->second.face * chain + above && j.format == s.format);
            } else {
                CHECK(face == dense.end());  // a panorama's level: in front of its cube's faces, no dense face
                CHECK(decoded.emplace(j.dst, std::make_pair(j.w, j.h)).second);
            }
        }
    }

    // ---- the equirect launches in order: faces, level 1, level 2, ..., tail
    std::vector<uint32_t> eq_extents, eq_mips;
    for (const r3n_cube_source &s : a.sources)
        if (s.kind == R3N_CUBE_SOURCE_EQUIRECT) {
            eq_extents.push_back(s.face_extent);
            eq_mips.push_back(s.mips);
        }
    const equirect_rule::Plan want = equirect_rule::plan(eq_extents.data(), eq_mips.data(), (uint32_t)eq_extents.size(), tail);
    CHECK(p.eq_launches.size() == want.faces + want.levels && (p.tail_recs != 0u) == (want.tail != 0u));
    CHECK(p.tail_at + (size_t)p.tail_recs * equirect::CHAIN_REC_WORDS == p.eq_block.size() && p.tail_at % 16u == 0u);
    for (size_t li = 0; li < p.eq_launches.size(); ++li) {
        const Launch &l = p.eq_launches[li];
        const size_t rec_words = li == 0 ? equirect::FACE_REC_WORDS : equirect::CHAIN_REC_WORDS;
        CHECK(l.at % 16u == 0u && l.layout.o_inst + l.waves <= p.eq_block.size() - l.at);
        if (l.layout.o_inst + l.waves > p.eq_block.size() - l.at) return;
        const size_t end = li + 1 < p.eq_launches.size() ? p.eq_launches[li + 1].at : p.tail_at;
        CHECK(l.at + l.layout.o_inst + l.waves <= end);
        const uint32_t count = (uint32_t)(l.layout.o_first / rec_words);
        const uint32_t *block = p.eq_block.data() + l.at;
        check_wave_map(block, end - l.at, l.layout, count, rec_words, li == 0 ? 8 : 4, equirect::UNITS_PER_WAVE, l.waves);
        for (uint32_t i = 0; i < count; ++i) {
            ++resampled;
            if (li == 0) {
                equirect::FaceRec r;
                memcpy(&r, block + (size_t)i * rec_words, sizeof r);
                auto face = dense.find(r.dst);
                CHECK(face != dense.end());
                if (face == dense.end()) continue;
                const r3n_cube_source &s = a.sources[face->second.cube];
                CHECK(s.kind == R3N_CUBE_SOURCE_EQUIRECT && face->second.level == 0u && face->second.face == r.face && !face->second.written);
                CHECK(r.n == s.face_extent && r.units == r.n * r.n && r.W == s.width && r.H == s.height);
                if (s.format == RGBE8) {
                    CHECK(r.mode == equirect::SOURCE_RGBE8 && (r.src_lo | (uint64_t)r.src_hi << 32) == s.offset);
                } else {
                    auto src = decoded.find(r.src_lo);
                    CHECK(r.src_hi == 0u && src != decoded.end() && src->second == std::make_pair(s.width, s.height));
                    CHECK(r.mode == (s.format == BC6H ? equirect::SOURCE_F32 : s.format == RGBA8_SRGB ? equirect::SOURCE_RGBA8_SRGB : equirect::SOURCE_RGBA8));
                }
                face->second.written = true;
            } else {
                equirect::ChainRec r;
                memcpy(&r, block + (size_t)i * rec_words, sizeof r);
                auto dst = dense.find(r.dst), src = dense.find(r.src);
                CHECK(dst != dense.end() && src != dense.end());
                if (dst == dense.end() || src == dense.end()) continue;
                // a chain record's source is the level above of the same face of the same cube, written by the launch in front
                CHECK(dst->second.level == li && src->second.level == li - 1 && src->second.cube == dst->second.cube && src->second.face == dst->second.face);
                CHECK(src->second.written && !dst->second.written && r.face == dst->second.face && r.levels == 1u);
                CHECK(r.s == src->second.n && r.d == dst->second.n && r.units == r.d * r.d);
                dst->second.written = true;
            }
        }
    }
    for (uint32_t i = 0; i < p.tail_recs; ++i) {  // workgroup i: face `face`, `levels` levels behind the level at `src`
        ++resampled;
        equirect::ChainRec r;
        memcpy(&r, p.eq_block.data() + p.tail_at + (size_t)i * equirect::CHAIN_REC_WORDS, sizeof r);
        auto src = dense.find(r.src + (uint64_t)r.face * r.s * r.s * 4u);
        CHECK(src != dense.end() && r.s <= equirect_rule::TAIL_CAP && r.levels >= 1u);
        if (src == dense.end()) continue;
        const r3n_cube_source &s = a.sources[src->second.cube];
        CHECK(src->second.written && src->second.face == r.face && src->second.n == r.s && src->second.level + r.levels == s.mips - 1u);
        CHECK(src->second.level == equirect_rule::tail_from(s.face_extent, s.mips, tail));
        uint64_t level_at = r.src;  // the six faces of a level, then the next level's
        uint32_t nk = r.s;
        for (uint32_t k = 1; k <= r.levels; ++k) {
            level_at += 6u * (((uint64_t)nk * nk * 4u + 3u) & ~3ull);
            nk = nk > 1 ? nk / 2 : 1;
            if (k == 1u) CHECK(level_at == r.dst && nk == r.d);
            auto dst = dense.find(level_at + (uint64_t)r.face * (((uint64_t)nk * nk * 4u + 3u) & ~3ull));
            CHECK(dst != dense.end() && !dst->second.written && dst->second.cube == src->second.cube && dst->second.level == src->second.level + k &&
                  dst->second.face == r.face && dst->second.n == nk);
            if (dst != dense.end()) dst->second.written = true;
        }
    }
    // ---- every dense face the assemble reads has been written
    for (const auto &face : dense) CHECK(face.second.written);
}

static void accepted(const char *name, const Array &a, uint32_t tail = R3N_EQUIRECT_TAIL_DEFAULT) {
    context = name;
    Plan p;
    const Refusal refused = plan_sources(a, tail, p);
    CHECK(refused.code == R3N_OK && refused.why == nullptr);
    if (refused.code != R3N_OK) return;
    check_plan(a, tail, p);
    // stored faces alone: the descs the encoded adapter builds give the same plan, and so do the plain entry's for one-level RGBA8
    bool all_stored = true, all_plain = true;
    for (const r3n_cube_source &s : a.sources) {
        all_stored = all_stored && s.kind == R3N_CUBE_SOURCE_CUBE && s.offset <= 0xFFFFFFFFull;
        all_plain = all_plain && s.kind == R3N_CUBE_SOURCE_CUBE && s.mips == 1u && (s.format == RGBA8 || s.format == RGBA8_SRGB);
    }
    if (all_stored) {
        std::vector<Source> encoded, plain;
        for (const r3n_cube_source &s : a.sources) {
            r3n_texture_desc32 d{};
            d.offset = (uint32_t)s.offset; d.width = d.height = s.face_extent; d.mips = s.mips; d.format = s.format;
            encoded.push_back(from_desc(d));
            d.offset = (uint32_t)(s.offset / 4u);  // in texels
            Source t = from_desc(d);
            t.offset = 4ull * d.offset;
            plain.push_back(t);
        }
        Plan q;
        CHECK(plan(encoded.data(), (uint32_t)encoded.size(), a.payload_bytes, tail, q).code == R3N_OK && same_plan(p, q));
        for (Source &s : encoded) s.stored_mips = s.mips;  // (stored_mips == mips is the same as 0)
        CHECK(plan(encoded.data(), (uint32_t)encoded.size(), a.payload_bytes, tail, q).code == R3N_OK && same_plan(p, q));
        if (all_plain) CHECK(plan(plain.data(), (uint32_t)plain.size(), 4u * ((a.payload_bytes + 3u) / 4u), tail, q).code == R3N_OK && same_plan(p, q));
    }
}

static int refuse(int argc, char **argv) {
    if (argc < 6) return 2;
    const bool encoded = strcmp(argv[2], "encoded") == 0;
    const uint64_t payload_bytes = strtoull(argv[3], nullptr, 0);
    const uint32_t tail = (uint32_t)strtoul(argv[4], nullptr, 0), n = (uint32_t)strtoul(argv[5], nullptr, 0);
    if (argc != 6 + 8 * (int)n) return 2;
    std::vector<Source> sources;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t v[8];
        for (int k = 0; k < 8; ++k) v[k] = strtoull(argv[6 + 8 * i + k], nullptr, 0);
        if (encoded) {
            r3n_texture_desc32 d{};
            d.format = (uint32_t)v[1]; d.width = (uint32_t)v[2]; d.height = (uint32_t)v[3]; d.mips = (uint32_t)v[5]; d.offset = (uint32_t)v[6]; d.stored_mips = (uint32_t)v[7];
            sources.push_back(from_desc(d));
        } else {
            sources.push_back(from_source(r3n_cube_source{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]}));
        }
    }
    Plan p;
    const Refusal refused = plan(sources.data(), n, payload_bytes, tail, p);
    printf("%d %s\n", refused.code, refused.code == R3N_OK ? "accepted" : refused.why);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "refuse") == 0) return refuse(argc, argv);
    Array mixed;
    for (uint32_t n : {1u, 2u, 3u, 5u}) {
        Array a;
        a.stored(n == 2u ? RGBA8_SRGB : RGBA8, n, full_chain(n));
        accepted("a stored RGBA8 cube, full chain", a);
        Array one;
        one.stored(n == 2u ? RGBA8_SRGB : RGBA8, n, 1u);
        accepted("a stored RGBA8 cube, one level", one);
        mixed.append(a);
    }
    Array plain;  // what the plain entry is sent: one-level RGBA8 cubes, odd extents in front of others
    for (uint32_t n : {1u, 3u, 4u, 5u}) plain.stored(n == 3u ? RGBA8_SRGB : RGBA8, n, 1u);
    accepted("one-level RGBA8 cubes", plain);
    Array bc6h;
    bc6h.stored(BC6H, 8, 4);
    accepted("a BC6H cube", bc6h);
    Array rgbe;
    rgbe.panorama(RGBE8, 7, 5, 5, full_chain(5));
    accepted("an RGBE panorama", rgbe);
    Array bc6h_pano;
    bc6h_pano.panorama(BC6H, 9, 5, 4, full_chain(4));
    accepted("a BC6H panorama", bc6h_pano);
    Array wide;
    wide.panorama(RGBE8, 130, 65, 65, 3);
    accepted("a 130 x 65 panorama, tail 0", wide, 0u);
    accepted("a 130 x 65 panorama, tail 64", wide, 64u);
    for (const Array *a : {&bc6h, &rgbe, &bc6h_pano, &wide}) mixed.append(*a);
    Array srgb_pano;  // (the fourth source mode)
    srgb_pano.panorama(RGBA8_SRGB, 6, 3, 2, 2);
    mixed.append(srgb_pano);
    for (uint32_t tail : {0u, 1u, 4u, 64u}) accepted("the mixed array", mixed, tail);
    accepted("the empty array", Array{});
    printf("arrays %llu\nrecords %llu\njobs %llu\nresampled %llu\nfailures %d\n", (unsigned long long)arrays, (unsigned long long)records,
           (unsigned long long)jobs, (unsigned long long)resampled, failures);
    return failures ? 1 : 0;
}
