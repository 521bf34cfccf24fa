"""The fragment stage's light loop (kernels_shade.h fragment_stage; its staging stage_lights / k_stage_view_lights / ViewLights;
its shadow lookup shadow_pcf5 / shadow_pcf5_general) at its limits and at the edge of every shortcut, on the GPU, against the
oracle, which evaluates every light in full.  The light sets are tests/light_worlds.py; tests/test_lights.py holds, on the oracle
alone, the conditions this file rests on (each set reaches the path it is named for).  Every comparison is
test_gpu_parity.compare_frames: the sets of every camera, the keys, the shadow atlas as u32 words, HDR f16 bit for bit.

What these tests notice (each change made to a scratch copy of kernels_shade.h, the file run against it):
  the directional loop stops at n_dir & ~1u   counts at the odd counts, zero_paths, frustum_edges (1 and 3 lights), in_flight
  the point loop stops at 255                 counts (15, 256) and (16, 256)
  the nl == 0 skip without its guard          counts, zero_paths, frustum_edges, in_flight (the roughness-0 sphere)
  skip_ok forced true                         the same, and zero_paths from_below at 1e6 (the mirror)
  skip_ok with roughness from 1e-9 and magnitudes up to 1e30 (as it was)   zero_paths from_below at 1e6 (the mirror)
  shadow_pcf5_general clamps, does not wrap   frustum_edges
  `||` of the bounds test becomes `&&`        counts, zero_paths, frustum_edges, in_flight
  the `sane` bound 1e6 becomes 1e7            nothing: inside skip_ok |(fd + fr) * colour| <= 6e37 at 1e6 by the proof beside skip_ok,
                                              and the factor of 5 left to the overflow is the worst case of D, V and f0 at once,
                                              ten orders above what a pixel of a stage reaches -- no input tells 1e7 from 1e6
"""
import ctypes
import functools

import numpy as np
import pytest

import light_worlds as lw
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


# every copy of the light loop: (samples, textured, blend, environment)
FORMS = {
    "scalar_lists": (1, False, False, {}),                             # record-based single-sample resolve: lights by scalar loads
    "class_kernels": (1, True, False, {}),                             # one kernel per material class
    "general_kernel": (1, True, False, {"R3N_RESOLVE_CLASSES": "0"}),  # the general kernel for every tile
    "split": (4, False, False, {}),                                    # the split four-sample resolve
    "split_overflow": (4, True, False, {"R3N_EDGE_CAPACITY": "8"}),    # overflowed pixels shade all their triangles in the first pass
    "unsplit_blend": (4, True, True, {}),                              # unsplit four-sample resolve + k_blend_apply<4>
    "blend_single": (1, False, True, {}),                              # k_blend_apply<1>
}


def light_set(key):
    """key -> (directional lights, point lights, stage options)"""
    if key[0] == "counts":
        return lw.counts(key[1], key[2]) + ({},)
    if key[0] == "zero":
        return lw.zero_paths(key[1], lw.ZERO_COLOURS[0]) + (lw.ZERO_STAGE,)
    if key[0] == "frustum":
        return lw.frustum_edges(key[1]) + ({},)
    if key[0] == "in_flight":
        return lw.in_flight_start() + ({},)
    raise KeyError(key)


def build(r, mk, key, textured, blend):
    dirs, points, options = light_set(key)
    lw.build_stage(r, oh, mk, textured=textured, blend=blend, cutout=textured, **options)
    lw.set_camera(r, oh)
    lw.apply_lights(r, dirs, points)


def step(r, key, frame):
    """the world edit in front of frame `frame` of the set's sequence"""
    if key[0] == "zero" and frame > 0:
        v = lw.ZERO_COLOURS[frame]
        r.update_directional_light(key[1], color=(v, v, v))
    if key[0] == "in_flight":
        lw.in_flight_step(r, frame)


def n_frames(key):
    return {"zero": len(lw.ZERO_COLOURS), "in_flight": lw.IN_FLIGHT_FRAMES}.get(key[0], 2)  # two: the second draws the predicted set


def render(r, samples, **kw):
    return r.render(lw.W, lw.H, samples=samples, ambient=lw.AMBIENT, clear_color=lw.CLEAR, **kw)


@functools.lru_cache(maxsize=None)
def oracle_frames(key, samples, textured, blend):
    """the oracle's frames of a set: one answer for every environment switch"""
    o = OracleRenderer(oh.LEFT, lw.aspect())
    build(o, omk, key, textured, blend)
    out = []
    for f in range(n_frames(key)):
        step(o, key, f)
        out.append(render(o, samples))
    return out


def product(r3, monkeypatch, key, form):
    samples, textured, blend, env = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = r3.Renderer(oh.LEFT, lw.aspect())
    build(p, r3.material_record, key, textured, blend)
    return p, oracle_frames(key, samples, textured, blend), samples


def run_and_compare(r3, monkeypatch, key, form, tags=None):
    p, want, samples = product(r3, monkeypatch, key, form)
    try:
        for f, fo in enumerate(want):
            step(p, key, f)
            fp = render(p, samples)
            compare_frames(fo, fp, f"{key} {form} frame {f}" + (f" ({tags[f]})" if tags else ""))
    finally:
        p.close()
    return want


# ------------------------------------------------------------------ 1. counts on every copy of the loop
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n_dir,n_point", lw.COUNT_PAIRS, ids=[f"{d}dir_{p}point" for d, p in lw.COUNT_PAIRS])
def test_counts_on_every_copy_of_the_loop(r3, monkeypatch, n_dir, n_point, form):
    """0 .. 16 directional and 0 .. 256 point lights (the limits; odd and even counts; 255 and 256: the last thread of the staging
    block) on every form of the resolve and on both of k_blend_apply; two frames, the second draws the predicted set."""
    want = run_and_compare(r3, monkeypatch, ("counts", n_dir, n_point), form)
    if FORMS[form][2]:
        assert len(want[-1]["blend_list"][0]) > 0


# ------------------------------------------------------------------ 2. zero_paths
@pytest.mark.parametrize("form", ["scalar_lists", "class_kernels", "split"])
@pytest.mark.parametrize("which", [lw.ZERO_BELOW, lw.ZERO_OCCLUDED], ids=["from_below", "occluded"])
def test_zero_paths_every_colour_value(r3, monkeypatch, which, form):
    """The light from below (nl == 0 on the floor) or the light above the slab (shadow == 0 under it) takes 3, 1e6, the next f32,
    +inf, -inf, NaN, -5 and 1e7 in turn, one frame per value: where the kernel skips a zero term the oracle's full expression
    must be +0 too, where the oracle's is inf * 0 = NaN (an infinite colour; roughness 0; the mirror's highlight from 1e6 on)
    the kernel must not skip."""
    run_and_compare(r3, monkeypatch, ("zero", which), form, tags=lw.ZERO_COLOUR_IDS)


# ------------------------------------------------------------------ 3. frustum_edges
@pytest.mark.parametrize("form", ["scalar_lists", "class_kernels", "unsplit_blend"])
@pytest.mark.parametrize("n_lights", [1, 2, 3])
def test_frustum_edges(r3, monkeypatch, n_lights, form):
    """shadow boxes that end inside the stage: lookups that leave the light's map through the `any` of the bounds test, into a
    neighbour's map or round the atlas (shadow_pcf5_general's Repeat addressing), depth outside [0, 1]"""
    run_and_compare(r3, monkeypatch, ("frustum", n_lights), form)


# ------------------------------------------------------------------ 4. in_flight
@pytest.mark.parametrize("frame_nodes", [False, True], ids=["one_call_frame", "per_node_frame"])
def test_lights_change_between_frames_in_flight(r3, monkeypatch, frame_nodes):
    """Six frames, a light edit in front of each (a point light added, a directional light turned and resized -- the atlas is laid
    out again --, a recolour, a third directional light, nothing, a point light moved): submitted back to back without a
    read-back the last frame equals the oracle's; then the same sequence with a read-back every frame, every frame compared."""
    if frame_nodes:
        monkeypatch.setenv("R3N_FRAME_NODES", "1")
    else:
        monkeypatch.delenv("R3N_FRAME_NODES", raising=False)
    key = ("in_flight",)
    p, want, samples = product(r3, monkeypatch, key, "scalar_lists")
    assert p.frame_nodes == frame_nodes
    try:
        for f in range(len(want)):
            step(p, key, f)
            fp = render(p, samples, readback=(f == len(want) - 1))
        compare_frames(want[-1], fp, "in flight, last frame")
    finally:
        p.close()
    run_and_compare(r3, monkeypatch, key, "scalar_lists")


# ------------------------------------------------------------------ 5. refusal
def direct_frame(p, ev):
    """one more frame of the last descriptor with directional_buffer NULL: "keep what the context has" (include/r3n.h) -- the
    lights the frame uses are the context's own, not the host mirror's"""
    d = p._fc["desc"]
    keep = d.directional_buffer
    d.directional_buffer = None
    try:
        p._check(p.lib.r3n_render_frame(p.ctx, ctypes.byref(d)), "r3n_render_frame")
    finally:
        d.directional_buffer = keep
    return p.readback_frame(ev, lw.W, lw.H, 1)


def same_frame(a, b):
    return (np.array_equal(a["hdr16"], b["hdr16"]) and np.array_equal(a["vis"], b["vis"])
            and np.array_equal(a["atlas"].view(np.uint32), b["atlas"].view(np.uint32)))


def test_light_lists_beyond_the_limits_are_refused_whole(r3, monkeypatch):
    """r3n_lights_write at the ABI: 17 directional or 257 point lights, or a count word beyond the buffer, are refused with a
    message that names the list, and a refused call changes NOTHING -- not the directional list either when it is the point list
    that is too long (the directional list goes up every frame: a half-taken call would light the next frame)."""
    from rend3_amd import _ffi
    monkeypatch.delenv("R3N_FRAME_NODES", raising=False)
    p = r3.Renderer(oh.LEFT, lw.aspect())
    key = ("counts", 2, 3)
    build(p, r3.material_record, key, False, False)
    lib, ctx = p.lib, p.ctx
    try:
        for f in range(3):  # the temporal sets have settled: a frame repeats
            ev = p.render_frame(lw.W, lw.H, 1, lw.AMBIENT, lw.CLEAR)
        fr = p._fc["frame"]
        dir_now = np.frombuffer(bytes(bytearray(fr.directional_buffer)[: fr.directional_bytes]), dtype=np.uint8).copy()
        point_now = np.ascontiguousarray(p._fc["point"]).copy()
        before = direct_frame(p, ev)
        assert same_frame(before, direct_frame(p, ev)), "a frame of unchanged inputs repeats"
        fo = oracle_frames(key, 1, False, False)[-1]
        assert np.array_equal(fo["hdr16"], before["hdr16"]) and np.array_equal(fo["vis"], before["vis"])

        problems = []  # every refusal is tried before the test fails: one run names all that is wrong

        def refused(what, code, dir_buf, point_buf, word):
            got = lib.r3n_lights_write(ctx, _ffi.ptr(dir_buf), dir_buf.nbytes, _ffi.ptr(point_buf), point_buf.nbytes)
            msg = lib.r3n_last_error(ctx)
            if got != code:
                problems.append(f"{what}: returned {got}, not {code}")
            if not (word in msg and b"light list" in msg):
                problems.append(f"{what}: the message does not name the {word.decode()} light list: {msg!r}")
            if not same_frame(before, direct_frame(p, ev)):
                problems.append(f"{what}: the next frame is not the frame rendered before the refused call")
                assert lib.r3n_lights_write(ctx, _ffi.ptr(dir_now), dir_now.nbytes, _ffi.ptr(point_now), point_now.nbytes) == 0
                assert same_frame(before, direct_frame(p, ev))

        def with_count(buf, n, stride):
            out = np.zeros(16 + stride * n, dtype=np.uint8)
            m = min(len(buf), len(out))
            out[:m] = buf[:m]
            out[:4] = np.array([n], dtype=np.uint32).view(np.uint8)
            return out

        # a valid NEW directional list: the same shadow views, other colours
        dir_new = dir_now.copy()
        for k in range(2):
            dir_new[16 + 128 * k + 64: 16 + 128 * k + 76] = np.array([0.1, 2.0, 0.1], dtype=f32).view(np.uint8)
        refused("17 directional lights", -5, with_count(dir_now, 17, 128), point_now, b"directional")
        refused("257 point lights", -5, dir_now, with_count(point_now, 257, 32), b"point")
        refused("a new directional list with 257 point lights", -5, dir_new, with_count(point_now, 257, 32), b"point")  # the half-taken call
        short = dir_now.copy()
        short[:4] = np.array([3], dtype=np.uint32).view(np.uint8)       # three lights in a buffer of two
        refused("a directional count beyond the buffer", -1, short, point_now, b"directional")
        short = point_now.copy()
        short[:4] = np.array([0xFFFFFFFF], dtype=np.uint32).view(np.uint8)
        refused("a point count beyond the buffer", -1, dir_new, short, b"point")
        assert not problems, "\n".join(problems)
        # the limits themselves are taken, and the new list, once accepted, does light the frame
        assert lib.r3n_lights_write(ctx, _ffi.ptr(with_count(dir_now, 16, 128)), 16 + 128 * 16, _ffi.ptr(with_count(point_now, 256, 32)), 16 + 32 * 256) == 0
        assert lib.r3n_lights_write(ctx, _ffi.ptr(dir_new), dir_new.nbytes, _ffi.ptr(point_now), point_now.nbytes) == 0
        after = direct_frame(p, ev)
        assert not np.array_equal(before["hdr16"], after["hdr16"]) and np.array_equal(before["vis"], after["vis"])
        assert lib.r3n_lights_write(ctx, _ffi.ptr(dir_now), dir_now.nbytes, _ffi.ptr(point_now), point_now.nbytes) == 0
        assert same_frame(before, direct_frame(p, ev))
    finally:
        p.close()


@pytest.mark.parametrize("frame_nodes", [False, True], ids=["one_call_frame", "per_node_frame"])
def test_a_seventeenth_shadow_casting_light_raises_from_render(r3, monkeypatch, frame_nodes):
    from rend3_amd import _ffi
    monkeypatch.setenv("R3N_FRAME_NODES", "1" if frame_nodes else "0")
    p = r3.Renderer(oh.LEFT, lw.aspect())
    key = ("counts", 16, 0)
    build(p, r3.material_record, key, False, False)
    try:
        assert p.frame_nodes == frame_nodes
        compare_frames(oracle_frames(key, 1, False, False)[0], render(p, 1), "sixteen lights")
        p.add_directional_light(color=(1, 1, 1), intensity=1.0, direction=(0.1, -1.0, 0.1), distance=60.0, resolution=32)
        with pytest.raises(_ffi.R3nError, match="light list"):
            render(p, 1)
    finally:
        p.close()
