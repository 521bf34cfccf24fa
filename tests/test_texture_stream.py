"""The streamed texture path (r3n_textures_update / r3n_textures_remove) on the CPU: the texel allocator and the job tables of the
batched decode through tests/texel_alloc_check.cpp -- a stand-alone program built with the address and undefined-behaviour
sanitizers and run as a child process -- and the declarations of the new entry points in the header, the ctypes table and the
Python renderer.  The GPU side is tests/test_texture_stream_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "texel_alloc_check.cpp")
HEADERS = [os.path.join(ROOT, "rend3_amd", "csrc", h) for h in ("texel_alloc.h", "texture_jobs.h", "vertex_block.h")]


@pytest.fixture(scope="module")
def printed():
    exe = host_check.program(SRC, HEADERS)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # a sanitizer report goes there
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in lines and name != "FAIL", line
        lines[name] = rest
    return lines


def test_allocator_cases_pass_under_the_sanitizers(printed):
    """First fit at the lowest address, coalescing, the freed tail, exact-fit and one-word-too-small holes, the 2^32 limit, the
    quarantine, and 10^4 random operations against a brute-force interval model: checked inside the program."""
    assert printed["failures"] == "0"
    allocs, frees, live = (int(x) for x in printed["random"].split())
    assert allocs + frees == 10000 and allocs > 3000 and frees > 3000 and live > 0


def test_ascending_appends_reproduce_the_whole_array_offsets(printed):
    """Renderer.readback_texels' formula: cur = (cur + 3) & ~3; offset = cur; cur += words."""
    got = [int(x) for x in printed["appends"].split()]
    sizes = [1 if i % 7 == 0 else 1 + (i * 2654435761 % 2**32) % 997 for i in range(300)]
    assert sizes.count(1) >= 43
    want, cur = [], 0
    for n in sizes:
        cur = (cur + 3) & ~3
        want.append(cur)
        cur += n
    assert got == want + [cur]


# the batch of texel_alloc_check.cpp jobs(): (format id, w, h)
BC1, BC3, BC7, R8, RG8, RGBA8, BC6H_U, BC5_S, RGBA16F, R32F = 6, 10, 14, 2, 3, 0, 32, 31, 21, 22
LEVELS = [(BC1, 8, 8), (BC1, 4, 4), (BC1, 2, 2), (BC1, 1, 1), (BC7, 64, 36), (R8, 7, 5), (RGBA8, 16, 16), (RG8, 3, 3), (BC3, 5, 3),
          (BC6H_U, 8, 8), (BC5_S, 33, 65), (RGBA16F, 8, 4), (R32F, 13, 11), (RGBA8, 1, 1), (RGBA8, 65, 1)]
FAMILY = {BC1: 0, BC3: 0, BC7: 0, R8: 1, RG8: 1, RGBA8: 1, BC6H_U: 2, BC5_S: 2, RGBA16F: 3, R32F: 3}


def test_job_tables_cover_every_unit_exactly_once(printed):
    """Per family: the records and the wave-slot -> job map of texture_jobs.h (wave_first = the work-unit prefix in wave slots).  Every 4x4 block (block
    formats) or texel (uncompressed formats) of every level is some lane's unit exactly once, and no lane has a unit outside."""
    want = {f: [] for f in range(4)}
    src = dst = 0
    for fmt, w, h in LEVELS:
        fam = FAMILY[fmt]
        units = -(-w // 4) * -(-h // 4) if fam in (0, 2) else w * h
        want[fam].append([fmt, w, h, units, src & 0xFFFFFFFF, src >> 32, dst, 0])
        src += 0x100000004
        dst += w * h * (4 if fam >= 2 else 1)
    seen_levels = 0
    for fam in range(4):
        head, _, words = printed[f"jobs_{fam}"].partition(" :")
        n, o_first, o_inst, total_waves = (int(x) for x in head.split())
        block = np.array([int(x) for x in words.split()], dtype=np.int64)
        jobs = block[:n * 8].reshape(n, 8)
        assert jobs.tolist() == want[fam]
        units = jobs[:, 3]
        waves = -(-units // 64)
        assert (o_first, o_inst, len(block), total_waves) == (n * 8, n * 8 + n, n * 9 + waves.sum(), waves.sum())
        wave_first, wave_job = block[o_first:o_inst], block[o_inst:]
        assert wave_first.tolist() == (np.cumsum(waves) - waves).tolist()
        # what the kernel's prologue does: lane l of wave slot w takes unit (w - wave_first[job]) * 64 + l of job wave_job[w]
        slot = np.repeat(np.arange(total_waves), 64)
        lane = np.tile(np.arange(64), total_waves)
        job = wave_job[slot]
        unit = (slot - wave_first[job]) * 64 + lane
        inside = unit < units[job]
        counts = np.zeros(units.sum(), dtype=np.int64)
        first_unit = np.cumsum(units) - units  # a global numbering of the family's units
        np.add.at(counts, first_unit[job[inside]] + unit[inside], 1)
        assert (counts == 1).all() and inside.sum() == units.sum()
        assert (unit >= 0).all() and (np.diff(wave_job) >= 0).all()
        assert any(u % 64 for u in units)  # jobs that end inside a wave slot
        seen_levels += n
    assert seen_levels == len(LEVELS)


def test_header_declares_the_entry_points_and_no_new_stage():
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    for decl in ("int r3n_textures_update(r3n_ctx *ctx, const uint32_t *slots, const r3n_texture_desc32 *descs, uint32_t n, const void *payload,",
                 "int r3n_textures_remove(r3n_ctx *ctx, const uint32_t *slots, uint32_t n);",
                 "int r3n_readback_texture_descs(r3n_ctx *ctx, r3n_texture_desc32 *descs, uint32_t capacity, uint32_t *n_slots);",
                 "int r3n_texture_stats(r3n_ctx *ctx, r3n_texture_counters *out, int reset);",
                 "uint64_t update_calls, kernel_launches, bytes_staged, full_syncs, pool_grows, pool_words, live_words, free_ranges;"):
        assert decl in hdr, decl
    assert re.search(r"#define\s+R3N_STAGE_COUNT\s+25\b", hdr)
    assert "texture.rs" in hdr[hdr.index("int r3n_textures_update") - 2500:hdr.index("int r3n_textures_update")]


def test_ffi_signatures():
    import ctypes

    from rend3_amd import _ffi
    vp, u32, u64, cint = _ffi.vp, _ffi.u32, _ffi.u64, _ffi.cint
    assert _ffi.SIGNATURES["r3n_textures_update"] == (cint, [vp, vp, vp, u32, vp, u64])
    assert _ffi.SIGNATURES["r3n_textures_remove"] == (cint, [vp, vp, u32])
    assert _ffi.SIGNATURES["r3n_readback_texture_descs"] == (cint, [vp, vp, u32, vp])
    assert _ffi.SIGNATURES["r3n_texture_stats"] == (cint, [vp, vp, cint])
    assert ctypes.sizeof(_ffi.TextureCounters) == 64 and len(_ffi.STAGE_TABLE) == 25
    lib = _ffi.lib()
    for name in ("r3n_textures_update", "r3n_textures_remove", "r3n_readback_texture_descs", "r3n_texture_stats"):
        assert hasattr(lib, name)


def test_renderer_modes():
    from rend3_amd.renderer import Renderer
    with pytest.raises(ValueError):
        Renderer(texture_upload="bogus")
    r = object.__new__(Renderer)  # (no device here: the mode checks come before any call into the library)
    r._texture_upload = "whole"
    with pytest.raises(ValueError):
        r.remove_texture(0)
    for name in ("remove_texture", "readback_texture_descs", "texture_stats"):
        assert callable(getattr(Renderer, name))


def test_scene_viewer_flag():
    import argparse

    from rend3_amd import scene_viewer as sv
    ap = sv.add_arguments(argparse.ArgumentParser())
    assert sv.settings_from(ap.parse_args([]))["texture_upload"] == "whole"
    assert sv.settings_from(ap.parse_args(["--texture-upload", "stream"]))["texture_upload"] == "stream"
    with pytest.raises(SystemExit):
        ap.parse_args(["--texture-upload", "sometimes"])
