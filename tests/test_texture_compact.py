"""Compaction of the streamed texel pool (r3n_textures_compact) on the CPU: the planner of rend3_amd/csrc/texel_compact.h and the
allocator's rebuild through tests/texel_compact_check.cpp -- a stand-alone program built with the address and undefined-behaviour
sanitizers and run as a child process -- and the declarations of the new entry point in the header, the ctypes table, the Python
renderer and the viewer.  The GPU side is tests/test_texture_compact_gpu.py, which asks the same program for the plan of a layout."""
import os
import re
import subprocess

import pytest

import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "texel_compact_check.cpp")
HEADERS = [os.path.join(ROOT, "rend3_amd", "csrc", h) for h in ("texel_compact.h", "texel_alloc.h", "vertex_block.h")]

# the edge list of texel_compact_check.cpp: (name, layout items in address order, budget)
EDGES = [
    ("self_overlap", ["H4", "T1000"], 0),
    ("shift_equals_length", ["H1000", "T1000"], 0),
    ("shift_4_short", ["H996", "T1000"], 0),
    ("cut_by_pass", ["H256", "T1000", "T300"], 0),
    ("segment_lengths", ["H8", "T3", "T250", "T256", "T257"], 0),
    ("adjacent_between_movers", ["T16", "H8", "T100", "T40", "H12", "T64"], 0),
    ("last_moves", ["T16", "H64", "T30"], 0),
    ("budget_at_end", ["H8", "T16", "T16", "H20", "T16"], 32),
    ("budget_one_short", ["H8", "T16", "T16", "H20", "T16"], 31),
    ("empty", [], 0),
    ("no_holes", ["T16", "T7", "T64"], 0),
]


def program(sanitize=True):
    """Path of the built check program (built once, when its sources are newer).  sanitize=True: with the address and
    undefined-behaviour sanitizers, for the CPU tests of this file; sanitize=False: a plain build under a name of its own, which is
    what tests/test_texture_compact_gpu.py asks for a layout's plan -- no sanitizer runs beside the GPU."""
    return host_check.program(SRC, HEADERS, sanitize=sanitize)


def planned(items, stage_words=0, max_words=0, sanitize=True):
    """What the planner makes of a layout: dict(passes, launches, words_moved, textures_moved, end)."""
    res = subprocess.run([program(sanitize), "plan", str(stage_words), str(max_words)] + list(items), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stdout + res.stderr
    return dict(zip(("passes", "launches", "words_moved", "textures_moved", "end"), (int(x) for x in res.stdout.split())))


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


def test_plans_execute_to_the_memmove_reference_under_the_sanitizers(printed):
    """Inside the program, for the edge list and 10^4 random live sets (sizes 1-5000, holes 4-5000, stage_words 256 / 260 / 4096,
    a budget in a third of them): every launch executed word by word through the kernel's table in forward, reverse and shuffled
    order with one result, equal to one memmove per texture; multiples of 4, dst < src, no destination word among a launch's
    sources, the launch bound, the rebuilt Pool against a brute-force complement, and the next alloc at the new mark."""
    assert printed["failures"] == "0"
    cases, staged, direct, budgeted, words, biggest, widest_hole = (int(x) for x in printed["random"].split())
    assert cases == 10000 and staged > 1000 and direct > 1000 and 2500 < budgeted < 4200
    assert biggest > 4500 and widest_hole > 4500 and words > 10 ** 6
    passes, launches = (int(x) for x in printed["large"].split())
    assert passes <= launches <= 2 * passes and launches <= 2 * (2 ** 32 // (16 << 20) + 1)


def test_edge_list(printed):
    """(passes, launches, staged passes) at stage_words 256, 260, 4096 and the default, per edge."""
    got = {name: [int(x) for x in printed["edge_" + name].split()] for name, _, _ in EDGES}
    assert len(printed) == len(EDGES) + 3
    # a 4-word shift under a 1000-word texture: all staged, ceil(1000 / stage) pieces of two launches
    assert got["self_overlap"] == [4, 8, 4, 4, 8, 4, 1, 2, 1, 1, 2, 1]
    # dst_end == src: one direct launch whatever the cap
    assert got["shift_equals_length"] == [1, 1, 0] * 4
    # 996 words below their sources, then the last 4 -- unless the cap takes all 1000 at once: 996 < 1000, so through scratch
    assert got["shift_4_short"] == [2, 2, 0, 2, 2, 0, 1, 2, 1, 1, 2, 1]
    # shift 256 under 1300 words: direct pieces of 256 where the cap is no longer; through scratch where it is
    assert got["cut_by_pass"][:3] == [6, 6, 0] and got["cut_by_pass"][6:] == [1, 2, 1, 1, 2, 1]
    assert got["empty"] == [0, 0, 0] * 4 and got["no_holes"] == [0, 0, 0] * 4
    assert got["budget_at_end"] == [1, 2, 1] * 4 and got["budget_one_short"] == [1, 2, 1] * 4  # shift 8 under 32 and 16 words: one staged pass
    for name, items, budget in EDGES:  # the one-layout mode the GPU test uses agrees with the list
        for k, stage in enumerate((256, 0)):
            p = planned(items, stage, budget)
            assert [p["passes"], p["launches"]] == got[name][9 * k: 9 * k + 2], (name, stage)
    assert planned(["T16", "H64", "T30"])["end"] == 46 and planned(["H8", "T3", "T250", "T256", "T257"])["words_moved"] == 4 + 252 + 256 + 260


def test_header_declares_the_call_and_keeps_the_counters():
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    for decl in ("int r3n_textures_compact(r3n_ctx *ctx, const r3n_texture_compact_opts *opts, r3n_texture_compact_result *out);",
                 "uint64_t max_words, stage_words;",
                 "uint64_t textures_moved, words_moved, passes, kernel_launches, full_syncs, pool_words_before, pool_words_after, free_ranges_after;",
                 # r3n_texture_counters has kept its eight fields
                 "uint64_t update_calls, kernel_launches, bytes_staged, full_syncs, pool_grows, pool_words, live_words, free_ranges;"):
        assert decl in hdr, decl
    assert re.search(r"#define\s+R3N_STAGE_COUNT\s+25\b", hdr)
    contract = hdr[hdr.index("int r3n_textures_remove"):hdr.index("int r3n_textures_compact")]
    for word in ("R3N_ERR_STATE", "R3N_ERR_INVALID_ARG", "64 MiB", "full_syncs == 0"):
        assert word in contract, word


def test_ffi_signature_and_structs():
    import ctypes

    from rend3_amd import _ffi
    assert _ffi.SIGNATURES["r3n_textures_compact"] == (_ffi.cint, [_ffi.vp, _ffi.vp, _ffi.vp])
    assert [n for n, _ in _ffi.TextureCompactOpts._fields_] == ["max_words", "stage_words"] and ctypes.sizeof(_ffi.TextureCompactOpts) == 16
    assert [n for n, _ in _ffi.TextureCompactResult._fields_] == ["textures_moved", "words_moved", "passes", "kernel_launches", "full_syncs",
                                                                 "pool_words_before", "pool_words_after", "free_ranges_after"]
    assert ctypes.sizeof(_ffi.TextureCompactResult) == 64
    assert [n for n, _ in _ffi.TextureCounters._fields_] == ["update_calls", "kernel_launches", "bytes_staged", "full_syncs", "pool_grows",
                                                            "pool_words", "live_words", "free_ranges"]
    assert len(_ffi.STAGE_TABLE) == 25
    assert hasattr(_ffi.lib(), "r3n_textures_compact")


def test_renderer_and_viewer():
    import argparse
    import inspect

    from rend3_amd import scene_viewer as sv
    from rend3_amd.renderer import Renderer
    assert inspect.signature(Renderer.__init__).parameters["texture_compact"].default is None
    r = object.__new__(Renderer)  # (no device here: the mode check comes before any call into the library)
    r._texture_upload = "whole"
    with pytest.raises(ValueError):
        r.compact_textures()
    for bad in (0.0, 1.5, -0.25):
        with pytest.raises(ValueError):
            r.texture_compact = bad
    r.texture_compact = 0.25
    assert r.texture_compact == 0.25
    ap = sv.add_arguments(argparse.ArgumentParser())
    assert sv.settings_from(ap.parse_args([]))["texture_compact"] is None
    assert sv.settings_from(ap.parse_args(["--texture-upload", "stream", "--texture-compact", "0.25"]))["texture_compact"] == 0.25
