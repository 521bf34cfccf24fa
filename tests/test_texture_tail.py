"""A texture made of another one's mip tail (r3n_textures_from_texture, Renderer::add_texture_2d_from_texture) on the CPU: the
derivation, the refusals and the copy table of rend3_amd/csrc/texel_tail.h through tests/texel_tail_check.cpp -- a stand-alone
program built with the address and undefined-behaviour sanitizers and run as a child process -- and the declarations of the new
entry point in the header, the ctypes table, the Python renderer, the loader, the viewer and the generated Rust bindings.  The GPU
side is tests/test_texture_tail_gpu.py, which asks the same program for the tail of a chain."""
import os
import subprocess
import sys

import numpy as np
import pytest

import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "texel_tail_check.cpp")
HEADERS = [os.path.join(ROOT, "rend3_amd", "csrc", h) for h in ("texel_tail.h", "texel_alloc.h", "texture_jobs.h", "vertex_block.h")]
HEADERS.append(os.path.join(ROOT, "include", "r3n.h"))

# the chains of texel_tail_check.cpp: (width, height, pool words per texel), each with its full chain
CHAINS = [(1, 1, 1), (5, 3, 1), (7, 1, 1), (16, 16, 1), (64, 2, 1), (8, 4, 4)]


def program(sanitize=True):
    """Path of the built check program (built once, when its sources are newer).  sanitize=True: with the address and
    undefined-behaviour sanitizers, for the CPU tests of this file; sanitize=False: a plain build under a name of its own, which is
    what tests/test_texture_tail_gpu.py asks for a chain's tail -- no sanitizer runs beside the GPU."""
    return host_check.program(SRC, HEADERS, sanitize=sanitize)


def full_chain(w, h):
    return int(max(w, h)).bit_length()


def planned(w, h, mips, per_texel, start_mip, mip_count, sanitize=True):
    """The tail of a chain as the header derives it: dict(width, height, mips, src_word, words, units, waves), or None when refused."""
    res = subprocess.run([program(sanitize), "plan"] + [str(int(v)) for v in (w, h, mips, per_texel, start_mip, mip_count)],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stdout + res.stderr
    if res.stdout.strip() == "refused":
        return None
    return dict(zip(("width", "height", "mips", "src_word", "words", "units", "waves"), (int(x) for x in res.stdout.split())))


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


def test_tables_execute_to_the_copy_reference_under_the_sanitizers(printed):
    """Inside the program: every (start_mip, mip_count) of the six chains derived against the halving walk, with the refusals at the
    edges; source alignments 0-3 x lengths 1, 3, 4, 5, 1023, 1024, 1025 and two items of one source in one table; every tail of the
    chains through resolve() into the holes of a pool whose last texture ends at the mark; 10^3 random calls -- each table executed
    unit by unit as the kernel addresses the block, in three orders, against one word-by-word copy per item; and the refusal list,
    the overlap check and the 2^31 wave-slot refusal by arithmetic."""
    assert set(printed) == {"chains", "alignments", "table", "random", "failures"}
    assert printed["failures"] == "0"
    tails = sum(sum(full_chain(w, h) - s + 1 for s in range(full_chain(w, h))) for w, h, _ in CHAINS)
    assert int(printed["chains"]) == tails == 89
    items, words, waves = (int(x) for x in printed["alignments"].split())
    lengths = (1, 3, 4, 5, 1023, 1024, 1025)
    assert items == 4 * len(lengths) + 2 and words == 4 * sum(lengths) + 1024 + 700
    assert waves == 4 * (6 * 1 + 2) + 1 + 1  # 1025 words are two wave slots, 1024 one
    items, words, waves = (int(x) for x in printed["table"].split())
    assert items == tails and waves == tails and words > 5000
    items, words, waves = (int(x) for x in printed["random"].split())
    assert items > 3000 and words > 5 * 10 ** 5 and waves > items


def test_one_tail_mode_agrees_with_the_walk():
    """The mode the GPU file uses, against the chain walk written out here."""
    for w, h, per in CHAINS:
        mips = full_chain(w, h)
        levels = [max(1, w >> k) * max(1, h >> k) * per for k in range(mips)]
        for start in range(mips + 1):
            for count in range(mips + 2):
                got = planned(w, h, mips, per, start, count)
                if start >= mips or start + count > mips:
                    assert got is None, (w, h, start, count)
                    continue
                n = count or mips - start
                words = sum(levels[start:start + n])
                assert got == dict(width=max(1, w >> start), height=max(1, h >> start), mips=n, src_word=sum(levels[:start]), words=words,
                                   units=-(-words // 4), waves=-(-words // 1024)), (w, h, start, count)
    assert planned(2049, 1, 12, 1, 1, 1) == dict(width=1024, height=1, mips=1, src_word=2049, words=1024, units=256, waves=1)
    assert planned(2050, 1, 12, 1, 1, 1)["waves"] == 2


def test_header_declares_the_call_and_keeps_the_counters():
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    for decl in ("int r3n_textures_from_texture(r3n_ctx *ctx, const r3n_texture_tail16 *items, uint32_t n, r3n_texture_tail_result *out);",
                 "uint32_t dst_slot, src_slot, start_mip, mip_count;",
                 "uint64_t textures, words_copied, kernel_launches, full_syncs, pool_words_after;",
                 # r3n_texture_counters has kept its eight fields
                 "uint64_t update_calls, kernel_launches, bytes_staged, full_syncs, pool_grows, pool_words, live_words, free_ranges;"):
        assert decl in hdr, decl
    contract = hdr[hdr.index("int r3n_textures_compact(r3n_ctx"):hdr.index("int r3n_textures_from_texture")]
    for word in ("texture.rs:198-242", "add_texture_2d_from_texture", "R3N_ERR_INVALID_ARG", "R3N_ERR_CAPACITY", "R3N_ERR_STATE", "R3N_ERR_HIP",
                 "n == 0", "bytes_staged"):
        assert word in contract, word


def test_ffi_signature_and_structs():
    import ctypes

    from rend3_amd import _ffi
    assert _ffi.SIGNATURES["r3n_textures_from_texture"] == (_ffi.cint, [_ffi.vp, _ffi.vp, _ffi.u32, _ffi.vp])
    assert [n for n, _ in _ffi.TextureTail16._fields_] == ["dst_slot", "src_slot", "start_mip", "mip_count"] and ctypes.sizeof(_ffi.TextureTail16) == 16
    assert [n for n, _ in _ffi.TextureTailResult._fields_] == ["textures", "words_copied", "kernel_launches", "full_syncs", "pool_words_after"]
    assert ctypes.sizeof(_ffi.TextureTailResult) == 40
    assert [n for n, _ in _ffi.TextureCounters._fields_] == ["update_calls", "kernel_launches", "bytes_staged", "full_syncs", "pool_grows",
                                                            "pool_words", "live_words", "free_ranges"]
    assert hasattr(_ffi.lib(), "r3n_textures_from_texture")


def test_renderer_loader_and_viewer():
    import argparse
    import inspect
    import types

    from rend3_amd import gltf
    from rend3_amd import scene_viewer as sv
    from rend3_amd.renderer import Renderer
    sig = inspect.signature(Renderer.add_texture_2d_from_texture)
    assert list(sig.parameters) == ["self", "src", "start_mip", "mip_count"] and sig.parameters["mip_count"].default is None
    r = object.__new__(Renderer)  # (no device here: the checks come before any call into the library)
    r._texture_upload = "whole"
    with pytest.raises(ValueError, match="texture_upload='stream'"):
        r.add_texture_2d_from_texture(0, 1)
    # "stream": the queue alone -- the lowest free slot, the order of a flush, the refusals the host can make
    r._texture_upload = "stream"
    r._tex_live, r._tex_mips, r._tex_queue, r._tex_removals, r._tex_tails = [], [], [], [], []
    a = r._append_texture(np.zeros(64 + 16 + 4, dtype=np.uint8), 4, 4, 3, 0)
    assert a == 0 and r.add_texture_2d_from_texture(a, 1) == 1 and r.add_texture_2d_from_texture(a, 0, 2) == 2
    assert r._tex_tails == [(1, 0, 1, 2), (2, 0, 0, 2)] and r._tex_mips == [3, 2, 2]
    for bad in ((a, 3), (a, 1, 3), (a, 0, 0), (a, -1), (7, 0)):
        with pytest.raises(ValueError):
            r.add_texture_2d_from_texture(*bad)
    assert len(r._tex_tails) == 2 and r._tex_live == [True] * 3
    flushed = []
    r._flush_textures = lambda before_frame=False: flushed.append(list(r._tex_tails)) or r._tex_tails.clear() or r._tex_queue.clear()
    assert r.add_texture_2d_from_texture(2, 1) == 3 and len(flushed) == 1  # a tail of a queued tail: what is queued goes first
    assert r._tex_tails == [(3, 2, 1, 1)]
    r.remove_texture(2)  # the source of a queued tail: sent before the removal is queued
    assert len(flushed) == 2 and r._tex_removals == [2] and r._tex_live == [True, True, False, True]
    assert inspect.signature(gltf.instance_scene).parameters["texture_skip_mips"].default == 0
    ap = sv.add_arguments(argparse.ArgumentParser())
    assert sv.settings_from(ap.parse_args([]))["texture_skip_mips"] == 0
    assert sv.settings_from(ap.parse_args(["--texture-upload", "stream", "--texture-skip-mips", "2"]))["texture_skip_mips"] == 2
    with pytest.raises(ValueError, match="--texture-upload stream"):  # (refused in front of everything that needs a renderer)
        sv.build(types.SimpleNamespace(handedness=sv.RIGHT, texture_upload="whole"), None, None, sv.default_settings(texture_skip_mips=1))


def test_generated_bindings_are_current():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_sys
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert gen_rust_sys.generate() == rs, "bindings/rend3-amd-sys/src/lib.rs is stale: run python tools/gen_rust_sys.py"
    for item in ("pub struct r3n_texture_tail16", "pub struct r3n_texture_tail_result",
                 "pub fn r3n_textures_from_texture(ctx: *mut r3n_ctx, items: *const r3n_texture_tail16, n: u32, out: *mut r3n_texture_tail_result) -> c_int;"):
        assert item in rs, item
    patch = open(os.path.join(ROOT, "bindings", "rend3-hooks.patch")).read()
    assert "fill_from_texture" not in patch  # (no hook there: INTEGRATION.md names the call the hook would make)
    assert "r3n_textures_from_texture" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
