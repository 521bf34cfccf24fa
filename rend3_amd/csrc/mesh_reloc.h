// mesh_reloc.h -- relocation of mesh-buffer addresses after r3n_mesh_compact (mesh_reloc.hip; the reference never moves a mesh:
// MeshManager frees and reuses ranges, rend3/src/managers/mesh.rs:123-211, and grows its buffer when no hole fits, :232-308).  A
// compaction slides whole blocks of mesh words towards word 0 (texel_compact.h plans the moves); every 128-byte object record names
// mesh words by ADDRESS -- first_index in words, six vertex_attribute_start_offsets in bytes (r3n.h, r3n_object128) -- so the
// records follow on the device.  This header holds the table, the lookup and the patch of one record, defined ONCE: the kernel
// (mesh_reloc.hip), the library's host code (r3n.hip) and tests/mesh_reloc_check.cpp all compile it.  Plain C++17, no HIP types.
//
// The table: the moves sorted by source, one 16-byte entry each: words [src, end) become word - shift (end = src + padded words).
// The rule: a word address w inside [src, end) of an entry becomes w - shift; every other address is unchanged -- an address in a
// block that did not move, in a hole, one past a block's padding -- and 0xFFFFFFFF (INVALID) is never changed, whatever the table
// says.  A byte offset b is relocated as word b >> 2 and keeps its low two bits.  Each of a record's seven fields is looked up on
// its own (an object bound to a skeleton or a morph instance names two or three blocks); the entry that served the previous field
// is tried before the search (`hint`).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MESH_RELOC_HD __host__ __device__ inline
#else
#define MESH_RELOC_HD inline
#endif

namespace mesh_reloc {

constexpr uint32_t INVALID = 0xFFFFFFFFu;
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;

struct Entry {
    uint32_t src, end, shift, pad;  // words; src < end, shift = src - dst > 0
};
static_assert(sizeof(Entry) == 16, "a table entry is one 16-byte load");

// The one place where the lookup changes form: the kernel keeps a table of up to this many entries in LDS (every thread of a
// 256-thread workgroup fetches one entry, 4 KiB per workgroup); a longer table stays in global memory, where the binary search's
// upper levels hit in L2.  The rule is the same on both sides.
constexpr uint32_t LDS_TABLE_ENTRIES = 256u;

// the object record's fields that hold addresses (r3n_object128): word 20 = first_index (a WORD address), words 23..28 =
// vertex_attribute_start_offsets (BYTE offsets).  The kernel loads words 20..28 (bytes 80..115) and writes nothing else.
constexpr uint32_t RECORD_WORDS = 32u, FIRST_INDEX_WORD = 20u, ATTRIBUTE_WORD = 23u, ATTRIBUTES = 6u, FIELDS = 1u + ATTRIBUTES;
constexpr uint32_t LOAD_FIRST_WORD = 20u, LOAD_WORDS = 9u;

// the entry that holds word w, or NO_ENTRY.  Table: any random-access range of Entry (global pointer, LDS array, host vector data)
template <class Table>
MESH_RELOC_HD uint32_t find(Table table, uint32_t n, uint32_t w, uint32_t hint) {
    if (hint < n) {
        const Entry h = table[hint];
        if (w >= h.src && w < h.end) return hint;
    }
    uint32_t lo = 0u, hi = n;  // the first entry with src > w
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (table[mid].src <= w) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == 0u) return NO_ENTRY;
    return w < table[lo - 1u].end ? lo - 1u : NO_ENTRY;
}

// a word address; *hint: in, the entry to try first; out, the entry that held w (unchanged when none did)
template <class Table>
MESH_RELOC_HD uint32_t relocate_word(Table table, uint32_t n, uint32_t w, uint32_t *hint) {
    if (w == INVALID || n == 0u) return w;
    const uint32_t e = find(table, n, w, *hint);
    if (e == NO_ENTRY) return w;
    *hint = e;
    return w - table[e].shift;
}

// a byte offset: word b >> 2, the low two bits kept
template <class Table>
MESH_RELOC_HD uint32_t relocate_bytes(Table table, uint32_t n, uint32_t b, uint32_t *hint) {
    if (b == INVALID) return b;
    return (relocate_word(table, n, b >> 2, hint) << 2) | (b & 3u);
}

// One record.  f[0] = first_index, f[1..6] = the attribute offsets, rewritten in place; returns bit k set where f[k] changed.
template <class Table>
MESH_RELOC_HD uint32_t patch_fields(Table table, uint32_t n, uint32_t f[FIELDS]) {
    uint32_t hint = NO_ENTRY, changed = 0u;
    const uint32_t fi = relocate_word(table, n, f[0], &hint);
    if (fi != f[0]) changed |= 1u;
    f[0] = fi;
    for (uint32_t a = 0u; a < ATTRIBUTES; ++a) {
        const uint32_t v = relocate_bytes(table, n, f[1u + a], &hint);
        if (v != f[1u + a]) changed |= 2u << a;
        f[1u + a] = v;
    }
    return changed;
}

// a whole 32-word record, as the host holds it
template <class Table>
MESH_RELOC_HD uint32_t patch_record(Table table, uint32_t n, uint32_t *rec) {
    uint32_t f[FIELDS];
    f[0] = rec[FIRST_INDEX_WORD];
    for (uint32_t a = 0u; a < ATTRIBUTES; ++a) f[1u + a] = rec[ATTRIBUTE_WORD + a];
    const uint32_t changed = patch_fields(table, n, f);
    if (changed & 1u) rec[FIRST_INDEX_WORD] = f[0];
    for (uint32_t a = 0u; a < ATTRIBUTES; ++a)
        if (changed & (2u << a)) rec[ATTRIBUTE_WORD + a] = f[1u + a];
    return changed;
}

}  // namespace mesh_reloc

// ---- host side: the table of a plan
#include <algorithm>
#include <vector>

namespace mesh_reloc {

struct Move {
    uint64_t src, dst, words;  // words = the padded length; all three multiples of 4, dst < src
};

// the moves in any order -> the table, sorted by source.  false: an address does not fit 32 bits, or a move that moves nothing
inline bool build_table(const std::vector<Move> &moves, std::vector<Entry> &table) {
    table.clear();
    table.reserve(moves.size());
    for (const Move &m : moves) {
        if (m.src + m.words > 0xFFFFFFFFull || m.dst >= m.src || m.words == 0u) return false;
        table.push_back(Entry{(uint32_t)m.src, (uint32_t)(m.src + m.words), (uint32_t)(m.src - m.dst), 0u});
    }
    std::sort(table.begin(), table.end(), [](const Entry &a, const Entry &b) { return a.src < b.src; });
    return true;
}

}  // namespace mesh_reloc
