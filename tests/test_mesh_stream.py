"""Pooled mesh blocks and their compaction (r3n_mesh_blocks_add / _remove / r3n_mesh_compact) on the CPU: the relocation rule of
rend3_amd/csrc/mesh_reloc.h, the planner and the allocator at mesh sizes through tests/mesh_reloc_check.cpp -- a stand-alone
program built with the address and undefined-behaviour sanitizers and run as a child process -- the numpy restatement
tests/mesh_reloc_reference.py against the program's printed cases, and the declarations of the new entries in the header, the
ctypes table, the Python renderer and the viewer.  The GPU side is tests/test_mesh_stream_gpu.py, which asks the same program
what the allocator hands out."""
import os
import re
import subprocess

import numpy as np
import pytest

import host_check
import mesh_reloc_reference as MR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "mesh_reloc_check.cpp")
HEADERS = [os.path.join(ROOT, "rend3_amd", "csrc", h) for h in ("mesh_reloc.h", "texel_compact.h", "texel_alloc.h", "vertex_block.h")]
INVALID = 0xFFFFFFFF


def program(sanitize=True):
    """Path of the built check program (built once, when its sources are newer).  sanitize=True: with the address and
    undefined-behaviour sanitizers, for the CPU tests of this file; sanitize=False: a plain build under a name of its own, which is
    what tests/test_mesh_stream_gpu.py asks for the allocator's answers -- no sanitizer runs beside the GPU."""
    return host_check.program(SRC, HEADERS, sanitize=sanitize)


def pool_ops(ops, sanitize=True):
    """The program's pool mode: a list of result rows, one per op -- ("A", offset, merged), ("R", offset), ("S", mark),
    ("C", moves, passes, launches, mark) followed by one ("M", old, new, padded) per move, all in words."""
    res = subprocess.run([program(sanitize), "pool"] + list(ops), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stdout + res.stderr
    return [(line.split()[0],) + tuple(int(x) for x in line.split()[1:]) for line in res.stdout.splitlines()]


@pytest.fixture(scope="module")
def printed():
    res = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # a sanitizer report goes there
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in lines and name != "FAIL", line
        lines[name] = rest
    return lines


def test_plans_and_relocation_over_random_layouts_under_the_sanitizers(printed):
    """Inside the program, over 3 000 random layouts (blocks of 1, 3, 4, 5, 8, 1 020, 1 024, 1 028 and random sizes up to 1 500 words,
    holes of 4 to 2 400 words, stage_words 256 / 260 / 4 096, a budget in a third) and the hand-made ones: the plan executed on a
    host word array, 8 to 47 records per layout patched through mesh_reloc.h.  Every live block's words arrive intact, every field
    that named word k of a live block (padding included) names word k of it afterwards, every other field and every other word of
    a record is unchanged."""
    assert printed["failures"] == "0"
    cases, moved, in_blocks, elsewhere, budgeted, staged, records = (int(x) for x in printed["random"].split())
    assert cases == 3012 and moved > 10000 and in_blocks > 300000 and elsewhere > 30000 and 800 < budgeted < 1200 and staged > 1000
    assert records * 7 == in_blocks + elsewhere


def _case(text):
    t, rest = text[1:].split(" F ")  # "T <table> F <fields> O <fields>"; the table may be empty
    f, o = rest.split(" O ")
    t = t.strip()
    if t.startswith("ramp"):
        table = MR.ramp(int(t.split()[1]))
    else:
        table = np.array([int(x) for x in t.split()], dtype=np.int64).reshape(-1, 3)
    return table, [int(x) for x in f.split()], [int(x) for x in o.split()]


CASES = ("block_edges", "low_bits", "invalid", "below_first_move", "holes", "three_moves", "invalid_under_a_table", "top_words",
         "table_0", "table_1", "table_2")


def test_edge_list_against_the_numpy_restatement(printed):
    """The program prints every edge case as table, fields in, fields out; the numpy restatement gives the same fields out.  The
    list: the first word of a block, the last word, the last padding word, one past the padding, one before the start, INVALID
    (also under a table that covers the top of the address space), a field in a block below the first move, fields in holes, a
    record whose fields fall in three different moves, tables of 0, 1 and 2 entries, and tables at and either side of the
    constant where the kernel's lookup changes form."""
    lds = int(printed["lds_table_entries"])
    names = list(CASES) + [f"table_{n}" for n in (lds - 1, lds, lds + 1)]
    assert sorted(k for k in printed if k.startswith("case_")) == sorted("case_" + n for n in names)
    for name in names:
        table, fields, out = _case(printed["case_" + name])
        rec = np.arange(32, dtype=np.uint32) + 7
        rec[20], rec[23:29] = fields[0], fields[1:]
        want = MR.relocate_records(rec, table)[0]
        assert [int(want[20])] + [int(x) for x in want[23:29]] == out, name
        other = np.ones(32, dtype=bool)
        other[20], other[23:29] = False, False
        assert np.array_equal(want[other], rec[other]), name
    # a few of them by hand: B1 [32, 44) -> 16 is 10 words padded to 12
    _, fields, out = _case(printed["case_block_edges"])
    assert fields == [32, 128, 164, 172, 176, 124, INVALID] and out == [16, 64, 100, 108, 176, 124, INVALID]
    assert _case(printed["case_three_moves"])[2] == [17, 112, 144, 140, 156, 72, 116]
    assert _case(printed["case_invalid"])[2] == [INVALID] * 7
    for name in ("below_first_move", "holes", "table_0"):
        _, fields, out = _case(printed["case_" + name])
        assert fields == out, name


def test_renderer_restates_the_rule():
    """Renderer's relocate_offsets (what fixes the host mirrors after a compaction) against the brute-force restatement, over the
    edge table and random addresses, bytes and words."""
    from rend3_amd.renderer import relocate_offsets
    moves = np.array([(32 * 4, 16 * 4, 12), (64 * 4, 28 * 4, 8), (100 * 4, 36 * 4, 4)], dtype=np.uint64)
    table = MR.table_from_moves(moves)
    assert table.tolist() == [[32, 44, 16], [64, 72, 36], [100, 104, 64]]
    rng = np.random.default_rng(0x3E5)
    words = np.concatenate([rng.integers(0, 120, 500), [INVALID, 0, 31, 32, 43, 44, 63, 64, 71, 72, 99, 100, 103, 104]]).astype(np.uint32)
    assert np.array_equal(relocate_offsets(words, moves, words=True), MR.relocate_words(words, table).astype(np.uint32))
    offs = np.concatenate([rng.integers(0, 480, 500), [INVALID, 127, 128, 175, 176]]).astype(np.uint32)
    assert np.array_equal(relocate_offsets(offs, moves), MR.relocate_bytes(offs, table).astype(np.uint32))
    assert np.array_equal(relocate_offsets(offs.reshape(-1, 5), moves[::-1]), MR.relocate_bytes(offs, table).astype(np.uint32).reshape(-1, 5))
    assert np.array_equal(relocate_offsets(offs, np.zeros((0, 3))), offs)


def test_budget_stops_in_front_of_a_block(printed):
    assert printed["budget"] == "2 32 76 1"  # two blocks move, 32 words, the mark stays at the third block's end; one word less: one block


def test_pool_at_mesh_sizes(printed):
    """Ascending appends land where the append cursor put them; a parked range is taken (and reported) when it fits, what no parked
    range takes goes behind the mark; after the wait first fit at the lowest address; 1 020 / 1 024 / 1 028 words at a 1 024-word
    hole."""
    assert printed["pool_appends"] == "0 4 12 1032 2056 3084 3088 3092"
    assert printed["pool_reuse"] == "3100 0 5100 1032 2052 5100 12"
    assert printed["pool_hole_1024_takes_1020"] == "8 1" and printed["pool_hole_1024_takes_1024"] == "8 0"
    assert printed["pool_hole_1024_takes_1028"] == "1040 1"
    rows = pool_ops(["A16", "A10", "A8", "R1", "A4", "S", "A4", "C0:256"])
    assert rows == [("A", 0, 0), ("A", 16, 0), ("A", 28, 0), ("R", 16), ("A", 16, 1), ("S", 36), ("A", 20, 0), ("C", 1, 1, 2, 32), ("M", 28, 24, 8)]


def test_header_declares_the_calls():
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    for decl in ("int r3n_mesh_blocks_add(r3n_ctx *ctx, const r3n_mesh_block24 *blocks, uint32_t n, const void *payload, uint64_t payload_bytes,",
                 "int r3n_mesh_blocks_remove(r3n_ctx *ctx, const uint64_t *byte_offsets, uint32_t n);",
                 "int r3n_mesh_compact(r3n_ctx *ctx, const r3n_mesh_compact_opts *opts, r3n_mesh_compact_result *result, r3n_mesh_move24 *moves_out,",
                 "int r3n_mesh_stats(r3n_ctx *ctx, r3n_mesh_counters *out, int reset);",
                 "int r3n_readback_objects(r3n_ctx *ctx, uint32_t first_slot, r3n_object128 *records, uint32_t n);",
                 "#define R3N_MESH_BLOCK_ZERO 1u",
                 "uint64_t old_byte_offset, new_byte_offset, padded_words;"):
        assert decl in hdr, decl
    assert re.search(r"#define\s+R3N_STAGE_COUNT\s+25\b", hdr)  # no new stage
    contract = hdr[hdr.index("pooled mesh blocks"):hdr.index("int r3n_mesh_blocks_add")]
    for word in ("mesh.rs:123-184", "mesh.rs:197-211", "skeleton.rs:139-147", "R3N_ERR_STATE", "R3N_ERR_INVALID_ARG", "R3N_ERR_CAPACITY",
                 "without any wait"):
        assert word in contract, word
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    for name in ("r3n_mesh_blocks_add", "r3n_mesh_blocks_remove", "r3n_mesh_compact", "r3n_mesh_stats", "r3n_readback_objects", "r3n_mesh_move24"):
        assert name in rs, name
    reloc = open(os.path.join(ROOT, "rend3_amd", "csrc", "mesh_reloc.h")).read()
    assert "#include <hip" not in reloc and "hipStream" not in reloc and "LDS_TABLE_ENTRIES" in reloc  # plain C++; the named threshold


def test_ffi_signatures_and_structs():
    import ctypes

    from rend3_amd import _ffi
    vp, u32, u64, cint = _ffi.vp, _ffi.u32, _ffi.u64, _ffi.cint
    assert _ffi.SIGNATURES["r3n_mesh_blocks_add"] == (cint, [vp, vp, u32, vp, u64, vp])
    assert _ffi.SIGNATURES["r3n_mesh_blocks_remove"] == (cint, [vp, vp, u32])
    assert _ffi.SIGNATURES["r3n_mesh_compact"] == (cint, [vp, vp, vp, vp, u32])
    assert _ffi.SIGNATURES["r3n_mesh_stats"] == (cint, [vp, vp, cint])
    assert _ffi.SIGNATURES["r3n_readback_objects"] == (cint, [vp, u32, vp, u32])
    assert [n for n, _ in _ffi.MeshBlock24._fields_] == ["payload_offset", "words", "flags", "_pad"] and ctypes.sizeof(_ffi.MeshBlock24) == 24
    assert [n for n, _ in _ffi.MeshMove24._fields_] == ["old_byte_offset", "new_byte_offset", "padded_words"]
    assert [n for n, _ in _ffi.MeshCompactOpts._fields_] == ["max_words", "stage_words"]
    assert [n for n, _ in _ffi.MeshCompactResult._fields_] == ["blocks_moved", "words_moved", "passes", "kernel_launches", "full_syncs",
                                                              "pool_words_before", "pool_words_after", "free_ranges_after", "relocate_ns"]
    assert ctypes.sizeof(_ffi.MeshCompactResult) == 72
    assert [n for n, _ in _ffi.MeshCounters._fields_] == ["add_calls", "remove_calls", "compact_calls", "bytes_staged", "launches", "full_waits",
                                                         "growths", "blocks_live", "live_words", "pool_words", "free_ranges", "buffer_words"]
    assert _ffi.MESH_BLOCK_ZERO == 1 and len(_ffi.STAGE_TABLE) == 25
    lib = _ffi.lib()
    for name in ("r3n_mesh_blocks_add", "r3n_mesh_blocks_remove", "r3n_mesh_compact", "r3n_mesh_stats", "r3n_readback_objects"):
        assert hasattr(lib, name), name


def test_build_lists_the_translation_unit():
    from rend3_amd import build
    assert build.UNITS["mesh_reloc.hip"] == ["mesh_reloc.h"] and "mesh_reloc.h" in build.UNITS["r3n.hip"]


def test_renderer_and_viewer():
    import argparse
    import inspect

    from rend3_amd import scene_viewer as sv
    from rend3_amd.renderer import Renderer
    params = inspect.signature(Renderer.__init__).parameters
    assert params["mesh_upload"].default == "append" and params["mesh_compact"].default is None
    r = object.__new__(Renderer)  # (no device here: the mode checks come before any call into the library)
    r._mesh_upload = "append"
    for call in (lambda: r.remove_mesh(0), lambda: r.remove_skeleton(0), lambda: r.remove_morph_instance(0), r.compact_meshes):
        with pytest.raises(ValueError):
            call()
    for bad in (0.0, 1.5, -0.25):
        with pytest.raises(ValueError):
            r.mesh_compact = bad
    r.mesh_compact = 0.25
    assert r.mesh_compact == 0.25
    r.meshes, r.skeletons, r.morphs = [], [], []
    with pytest.raises(ValueError):
        r.mesh_upload = "pooled"
    r.mesh_upload = "stream"
    r.meshes = [None]
    with pytest.raises(ValueError):
        r.mesh_upload = "append"
    ap = sv.add_arguments(argparse.ArgumentParser())
    s = sv.settings_from(ap.parse_args([]))
    assert s["mesh_upload"] == "append" and s["mesh_compact"] is None
    s = sv.settings_from(ap.parse_args(["--mesh-upload", "stream", "--mesh-compact", "0.25"]))
    assert s["mesh_upload"] == "stream" and s["mesh_compact"] == 0.25
