"""The relocation rule of rend3_amd/csrc/mesh_reloc.h restated in numpy, for the tests: by brute force over the table, with no
search and no hint, so that it shares nothing with the code it is held against (the header's binary search, the kernel's two table
forms, Renderer's relocate_offsets).

A table is an integer array of rows (src, end, shift) in WORDS: words [src, end) become word - shift.  A word address inside a row's
range follows it; every other address is unchanged; 0xFFFFFFFF is never changed.  A byte offset is relocated as word b >> 2 and
keeps its low two bits.  Of a 32-word object record, word 20 (first_index) is a word address, words 23..28
(vertex_attribute_start_offsets) are byte offsets, and nothing else is written."""
import numpy as np

INVALID = 0xFFFFFFFF
FIRST_INDEX_WORD, ATTRIBUTE_WORDS = 20, slice(23, 29)


def table_from_moves(moves):
    """rows (old byte offset, new byte offset, padded words) -> rows (src, end, shift) in words, sorted by src"""
    m = np.asarray(moves, dtype=np.int64).reshape(-1, 3)
    t = np.stack([m[:, 0] // 4, m[:, 0] // 4 + m[:, 2], (m[:, 0] - m[:, 1]) // 4], axis=1)
    return t[np.argsort(t[:, 0])]


def ramp(n):
    """The long tables of tests/mesh_reloc_check.cpp and the GPU test: entry i moves words [8 + 16 i, 16 + 16 i) down by 8 + 4 i."""
    i = np.arange(n, dtype=np.int64)
    return np.stack([8 + 16 * i, 16 + 16 * i, 8 + 4 * i], axis=1)


def relocate_words(words, table):
    w = np.asarray(words, dtype=np.int64)
    out = w.copy()
    for src, end, shift in np.asarray(table, dtype=np.int64).reshape(-1, 3):
        inside = (w >= src) & (w < end) & (w != INVALID)
        out[inside] = w[inside] - shift
    return out


def relocate_bytes(offsets, table):
    b = np.asarray(offsets, dtype=np.int64)
    moved = (relocate_words(b >> 2, table) << 2) | (b & 3)
    return np.where(b == INVALID, b, moved)


def relocate_records(records, table):
    """uint32[n, 32] -> the records after the relocation"""
    out = np.array(records, dtype=np.uint32).reshape(-1, 32).copy()
    out[:, FIRST_INDEX_WORD] = relocate_words(out[:, FIRST_INDEX_WORD], table).astype(np.uint32)
    out[:, ATTRIBUTE_WORDS] = relocate_bytes(out[:, ATTRIBUTE_WORDS], table).astype(np.uint32)
    return out
