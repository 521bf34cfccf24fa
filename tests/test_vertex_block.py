"""rend3_amd/csrc/vertex_block.h on the CPU: the mesh-buffer range arithmetic and the wave-block layout behind r3n_morph,
r3n_vertex_normals and r3n_vertex_tangents, at the edges no GPU test reaches (nobody allocates a 16 GB mesh buffer in a test).
tests/vertex_block_check.cpp is built as a stand-alone program with the address and undefined-behaviour sanitizers, run as a child
process, and every word it prints is compared with the layout restated here."""
import os
import subprocess

import numpy as np
import pytest

import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vertex_block_check.cpp")
HEADER = os.path.join(HERE, "..", "rend3_amd", "csrc", "vertex_block.h")


@pytest.fixture(scope="module")
def printed():
    exe = host_check.program(SRC, [HEADER])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == ""  # a sanitizer report goes there
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in lines
        lines[name] = rest
    return lines


def layout(counts, rec_words, tail_words=None):
    """The block as r3n.hip has always laid it out: records | wave_first | wave_instance [| tail at the next even word]."""
    n, total = len(counts), sum(counts)
    o_first = n * rec_words
    o_inst = o_first + n
    o_tail = o_inst + total if tail_words is None else (o_inst + total + 1) & ~1
    block = np.zeros(o_tail + (tail_words or 0), np.uint32)
    block[:o_first] = 0xAAAAAAAA
    block[o_first:o_inst] = np.cumsum([0] + counts[:-1])
    block[o_inst:o_inst + total] = np.repeat(np.arange(n), counts)
    block[o_tail:] = 0xBBBBBBBB
    return f"{o_first} {o_inst} {o_tail} {block.size} : " + " ".join(str(w) for w in block)


@pytest.mark.parametrize("name,counts,rec_words,tail_words", [
    ("layout_one", [1], 8, None),
    ("layout_tail", [0, 1, 5], 16, 4),
    ("layout_no_tail", [0, 1, 5], 16, None),
    ("layout_empty_tail", [2], 16, 0),
])
def test_layout(printed, name, counts, rec_words, tail_words):
    assert printed[name] == layout(counts, rec_words, tail_words)


def test_layout_pads_the_tail_to_an_even_word(printed):
    o_first, o_inst, o_tail, size = (int(x) for x in printed["layout_tail"].split(" :")[0].split())
    assert (o_first, o_inst, o_tail, size) == (48, 51, 58, 62)  # 51 + 6 = 57 is odd
    assert printed["layout_no_tail"].split(" :")[0] == "48 51 57 57"


def test_ranges(printed):
    assert printed["aligned4"] == "1 0 0 0 1 1 0"
    assert printed["inside"] == "1 0 1 0 1"
    first, words = 0xFFFFFFFC // 4, 0xFFFFFFFF * 3
    assert printed["far"] == f"{first} {words}"
    assert (first + words) % 2**32 < 2**32 < first + words  # the case is one that wraps in 32 bits
    assert printed["inside_far"] == "1 0 0 0"
    assert printed["overlaps"] == "0 0 1 1 1 1 0 0 1"  # touching, lapping, nested, empty (each both ways), itself
    assert printed["overlaps_far"] == "1 0"


def test_waves(printed):
    want = [-(-n // 64) for n in (0, 1, 64, 65, 0xFFFFFFFF)] + [3, 4, -(-(0xFFFFFFFF * 3) // 256)]
    assert want[4] == 2**26 and want[7] == 50331648  # both sums wrap in 32-bit arithmetic
    assert printed["waves"] == " ".join(str(w) for w in want)
