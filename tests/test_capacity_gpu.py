"""GPU: the rasteriser's fixed-size buffers at and past capacity.

Every other parity test runs at the default capacities (2 Mi raster work items in 32 sub-queues, 32 Mi blend fragment nodes), where
no queue fills.  Here the test hooks of r3n_create (R3N_BIG_CAPACITY: entries per work sub-queue; R3N_FRAG_CAPACITY: fragment nodes)
and r3n_config.max_big_items shrink them, so that:
  * the opaque / cutout / shadow producers take their queue-full path (kernels_raster.h raster_small_body: the producer scans the
    region itself) -- the frames stay bit-identical to the oracle and nothing is reported;
  * the transparent pass drops exactly the work past capacity (k_blend_setup: the last work item; shade_pixel<BLEND>: one
    fragment) and r3n_frame_end / r3n_sync / a read-back report R3N_ERR_CAPACITY exactly ONCE, while the next frame renders
    bit-identically again (the per-frame resets of the node counter, the list heads and the queue counters);
  * k_blend_apply blends every layer of a list exactly as long as the node buffer.
Each test checks that it reached its path: the work items a call queued (r3n_readback_raster_stats, counted as requested, so a
call above 32 x capacity overflowed a sub-queue by pigeonhole), the exact number of reports, fragment counts known by construction.
"""
import math
import os
import sys

import numpy as np
import pytest

import scenes
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu
f32 = np.float32
BIGQ, TILE = 32, 32  # layouts.h R3N_BIGQ, kernels_raster.h R3N_TILE
ERR_CAPACITY = -6    # R3N_ERR_CAPACITY
AMBIENT, CLEAR = (0.1, 0.1, 0.1, 1.0), (0.02, 0.03, 0.05, 1.0)


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def hip(r3, monkeypatch, env, handedness, aspect, **kw):
    """A HIP renderer created under `env` (the hooks are read once, by r3n_create) that records capacity reports instead of raising."""
    for k in ("R3N_BIG_CAPACITY", "R3N_FRAG_CAPACITY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    p = r3.Renderer(handedness, aspect, **kw)
    p.capacity_reports = []
    return p


def codes(p):
    return [c for _, c in p.capacity_reports]


def peak_items(p):
    return int(p.raster_stats().max())


def images_from(dst, src, region=None):
    """`dst` with the tonemapper's inputs and outputs (HDR, 8-bit and float image) taken from `src`, in `region` (y, x slices) or
    everywhere: what compare_frames then checks on the rest -- sets, keys, atlas -- stays `dst`'s."""
    out = dict(dst)
    for k in ("hdr16", "rgba8", "rgba_f32"):
        a = np.array(dst[k], copy=True)
        if region is None:
            a[...] = src[k]
        else:
            a[region] = src[k][region]
        out[k] = a
    return out


def hdr_f32(frame):
    return frame["hdr16"].view(np.float16).astype(np.float32)


# ------------------------------------------------------------------ scenes
LAYER_TRI = [(-40.0, -40.0, 0.0), (0.0, 40.0, 0.0), (40.0, -40.0, 0.0)]  # one triangle far larger than the view of a camera 1..5 units away


def add_layers(r, mk, n, origin=(0.0, 0.0, 0.0), unlit=None):
    """`n` translucent screen-covering layers, one triangle each, 1 + 0.25 k units in front of a camera at `origin` looking down +z:
    every sample of the target is covered by every layer (n fragments per sample where nothing opaque is in front)."""
    m = r.add_mesh(LAYER_TRI, [0, 1, 2], normals=[(0.0, 0.0, -1.0)] * 3)
    hs = []
    for k in range(n):
        col = (0.15 + 0.8 * ((k * 7) % 11) / 10.0, 0.15 + 0.8 * ((k * 3 + 5) % 7) / 6.0, 0.15 + 0.8 * ((k * 5 + 2) % 13) / 12.0,
               0.3 + 0.2 * (k % 3))
        flat = (k % 2 == 0) if unlit is None else unlit
        mat = r.add_material(mk(albedo=col, albedo_mode="value", roughness=0.5, unlit=flat), scenes.BLEND)
        hs.append(r.add_object(m, mat, oh.translation((origin[0], origin[1], origin[2] + 1.0 + 0.25 * k))))
    return hs


def layer_camera(r, origin=(0.0, 0.0, 0.0)):
    r.set_camera_data(oh.look_at_lh(origin, (origin[0], origin[1], origin[2] + 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def layer_scene(r, mk, n, lights=True):
    hs = add_layers(r, mk, n)
    if lights:
        r.add_point_light((0.3, 0.4, 0.5), (1.0, 0.9, 0.8), 4.0, 6.0)
    layer_camera(r)
    return hs


# ------------------------------------------------------------------ a. the producers' queue-full path: bit-exact, never reported
_MSAA_FRAMES = {}


def _msaa_scene(r, mk, scene):
    if scene == "random_cutout":
        return scenes.build_random_scene(r, oh, mk, 200, 0xCA9A, lights=2, shadow_res=1024, with_cutout=True)
    return scenes.build_textured_scene(r, oh, mk, 120, 0xCA9B, lights=2, shadow_res=1024, encoded=True)


def _msaa_camera(r, f):
    r.set_camera_data(oh.look_at_lh((-12.0 + 3.0 * f, 3.0 + f, -12.0 + 2.0 * f), (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))


@pytest.mark.parametrize("scene", ["random_cutout", "textured_encoded"])
def test_queue_full_fallback_msaa(r3, monkeypatch, scene):
    """MSAA x4 with cutout (vertex alpha, textured alpha, the uniform-alpha shortcut) and with encoded textures: work sub-queues of
    1, 3 and 64 entries.  Every frame is bit-identical to the oracle, nothing is reported (not even after r3n_sync), and some call
    queued more than 32 x capacity items, so the producers' own scan of a region ran."""
    W, H, S = 320, 192, 4
    if scene not in _MSAA_FRAMES:
        o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
        _msaa_scene(o, omk, scene)
        frames = []
        for f in range(2):
            _msaa_camera(o, f)
            frames.append(o.render(W, H, samples=S, ambient=AMBIENT, clear_color=CLEAR))
        _MSAA_FRAMES[scene] = frames
    for cap in (1, 3, 64):
        p = hip(r3, monkeypatch, {"R3N_BIG_CAPACITY": cap}, oh.LEFT, f32(W) / f32(H))
        _msaa_scene(p, r3.material_record, scene)
        peak = 0
        for f, fo in enumerate(_MSAA_FRAMES[scene]):
            _msaa_camera(p, f)
            fp = p.render(W, H, samples=S, ambient=AMBIENT, clear_color=CLEAR)
            compare_frames(fo, fp, f"{scene} capacity {cap} frame {f}")
            peak = max(peak, peak_items(p))
        p.sync()
        assert codes(p) == [], f"{scene} capacity {cap}: the producers' fallback must not report ({p.capacity_reports})"
        assert peak > BIGQ * cap, f"{scene} capacity {cap}: no call queued more than {BIGQ * cap} items (peak {peak}): the fallback did not run"
        p.close()


class _Probe:
    """Stands in for the rend3_amd module inside tools/fuzz_parity.py: its Renderer records capacity reports and the work items of
    every frame."""

    def __init__(self, r3):
        probes = self.renderers = []

        class Renderer(r3.Renderer):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                self.capacity_reports, self.peak = [], 0
                probes.append(self)

            def render(self, *a, **kw):
                out = super().render(*a, **kw)
                self.peak = max(self.peak, peak_items(self))
                self.sync()
                return out

        self.Renderer, self.host, self.material_record = Renderer, r3.host, r3.material_record


@pytest.mark.parametrize("mutate,first,count", [(False, 1000, 60), (True, 5000, 30)])
def test_queue_full_fallback_campaign_slice(r3, monkeypatch, mutate, first, count):
    """Drawn cases of the randomised campaign (tools/fuzz_parity.py) with one entry per work sub-queue and no translucent objects
    (the transparent pass shares the queue and drops what does not fit; flips to the blend key are redrawn as opaque): every frame
    bit-identical to the oracle, no report, and the producers' fallback ran in most cases."""
    import fuzz_parity as F
    monkeypatch.setenv("R3N_BIG_CAPACITY", "1")
    probe = _Probe(r3)
    failed = []
    with F.oracle_threads(32):
        for seed in range(first, first + count):
            c = F.draw_case(seed)
            c["blend"], c["blend_flips"] = False, False
            try:
                (F.run_mutating_case if mutate else F.run_case)(probe, c)
            except AssertionError as e:
                failed.append((seed, str(e)[:300]))
    assert not failed, f"{len(failed)} of {count} cases differ from the oracle at R3N_BIG_CAPACITY=1: {failed[:5]}"
    assert len(probe.renderers) == count
    reported = [(p_i, p.capacity_reports) for p_i, p in enumerate(probe.renderers) if p.capacity_reports]
    assert not reported, f"the producers' fallback reported R3N_ERR_CAPACITY: {reported[:5]}"
    hit = sum(p.peak > BIGQ for p in probe.renderers)
    assert hit >= count // 2, f"the fallback ran in only {hit} of {count} cases"


def test_queue_full_fallback_at_the_abi_floor(r3):
    """r3n_config.max_big_items = 1 is raised to the floor of 1 024 entries per sub-queue.  A thread queues all the work items of its
    triangle into its wave's one sub-queue: at 1920x1080 a ground triangle whose box is the screen is 60 x 34 = 2 040 items, beyond
    the floor, so the producer scans the rest itself; the 2048^2 shadow view of the same ground is drawn at that capacity too."""
    W, H = 1920, 1080
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    p = r3.Renderer(oh.LEFT, f32(W) / f32(H), max_big_items=1)
    p.capacity_reports = []
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.add_directional_light(color=(1, 1, 1), intensity=1.0, direction=(-1.0, -1.0, 1.0), distance=5.0, resolution=2048)
        r.add_object(scenes.plane_mesh(r), scenes.lit(r, mk, (0.25, 0.5, 0.75, 1.0)), oh.mat4_mul(oh.rotation_x(-math.pi / 2), oh.scale((50.0, 50.0, 50.0))))
        r.add_object(scenes.cube_mesh(r), scenes.lit(r, mk, (0.75, 0.5, 0.25, 1.0)), oh.mat4_mul(oh.translation((0.25, 0.25, -0.25)), oh.scale((0.25, 0.25, 0.25))))
        r.set_camera_data(oh.look_at_lh((0.0, 1.0, -1.0), (0, 0, 0), (0, 1, 0)), ("orthographic", (2.5, 2.5 * H / W, 5.0)))
    fo = o.render(W, H, ambient=AMBIENT, clear_color=CLEAR)
    fp = p.render(W, H, ambient=AMBIENT, clear_color=CLEAR)
    compare_frames(fo, fp, "1080p ground at the floor capacity")
    stats = p.raster_stats()
    p.sync()
    assert codes(p) == []
    assert fo["shadows"] and fo["shadows"][0]["pass"].sum() > 0
    assert stats[:16].max() >= 2 * 60 * 34, f"work items per call {stats.tolist()}"  # (both ground triangles in one call)
    p.close()


# ------------------------------------------------------------------ b. the transparent pass's work queue, exact boundary
def _blend_queue_scene(r, mk, with_layer):
    scenes.build_random_scene(r, oh, mk, 60, 0xB0B, lights=1, with_cutout=True)
    eye = (0.0, 1.0, -12.0)
    if with_layer:
        add_layers(r, mk, 1, origin=eye, unlit=False)
    layer_camera(r, eye)


@pytest.mark.parametrize("samples", [1, 4])
def test_blend_work_queue_exact_boundary(r3, monkeypatch, samples):
    """One translucent triangle larger than the target: the box is clamped to the viewport (device_math.h tri_bounds), so its one
    thread of k_blend_setup queues exactly n = ceil(W/32) * ceil(H/32) items into one sub-queue.  Capacity n: bit-exact, no report.
    Capacity n - 1: the last item -- the bottom-right region -- is dropped and reported once; that region shows the frame without the
    triangle, the rest of the frame and every set, key and the atlas stay the oracle's."""
    W, H = 100, 70
    tx, ty = -(-W // TILE), -(-H // TILE)
    n = tx * ty
    region = (slice(TILE * (ty - 1), H), slice(TILE * (tx - 1), W))
    aspect = f32(W) / f32(H)
    o, o_bare = OracleRenderer(oh.LEFT, aspect), OracleRenderer(oh.LEFT, aspect)
    _blend_queue_scene(o, omk, True)
    _blend_queue_scene(o_bare, omk, False)
    kw = dict(samples=samples, ambient=AMBIENT, clear_color=CLEAR)
    fo, fo_bare = o.render(W, H, **kw), o_bare.render(W, H, **kw)
    assert len(fo["blend_list"][0]) == 1
    assert (fo["hdr16"][region] != fo_bare["hdr16"][region]).any(axis=-1).mean() > 0.5, "the triangle must show in the dropped region"
    for cap, expect in ((n, fo), (n - 1, images_from(fo, fo_bare, region))):
        p = hip(r3, monkeypatch, {"R3N_BIG_CAPACITY": cap}, oh.LEFT, aspect)
        _blend_queue_scene(p, r3.material_record, True)
        fp = p.render(W, H, **kw)
        stats = p.raster_stats()
        p.sync()
        assert (stats[:16] == n).any(), f"no viewport call queued exactly n = {n} items: {stats[:16].tolist()}"
        assert codes(p) == ([] if cap == n else [ERR_CAPACITY]), f"capacity {cap} of n = {n}: reports {p.capacity_reports}"
        compare_frames(expect, fp, f"blend queue capacity {cap} (n = {n}), {samples} samples")
        p.close()


# ------------------------------------------------------------------ c. the fragment node buffer, exact boundary and deep lists
@pytest.mark.parametrize("samples", [1, 4])
def test_fragment_buffer_exact_boundary(r3, monkeypatch, samples):
    """L screen-covering translucent layers over an empty background: every sample passes the depth test, so the pass makes exactly
    N = W * H * S * L fragments.  Capacity N: bit-exact, no report.  Capacity N - 1: one fragment is dropped and reported once: at most
    one pixel differs from the oracle, every value stays finite, sets / keys / atlas are the oracle's."""
    W, H, L = 45, 29, 3
    N = W * H * samples * L
    aspect = f32(W) / f32(H)
    o = OracleRenderer(oh.LEFT, aspect)
    layer_scene(o, omk, L)
    kw = dict(samples=samples, ambient=AMBIENT, clear_color=CLEAR)
    fo = o.render(W, H, **kw)
    assert len(fo["blend_list"][0]) == L
    for cap in (N, N - 1):
        p = hip(r3, monkeypatch, {"R3N_FRAG_CAPACITY": cap}, oh.LEFT, aspect)
        layer_scene(p, r3.material_record, L)
        fp = p.render(W, H, **kw)
        p.sync()
        tag = f"fragment capacity {cap} of N = {N}, {samples} samples"
        if cap == N:
            assert codes(p) == [], tag + f": reports {p.capacity_reports}"
            compare_frames(fo, fp, tag)
        else:
            assert codes(p) == [ERR_CAPACITY], tag + f": reports {p.capacity_reports}"
            assert np.isfinite(hdr_f32(fp)).all(), tag + ": non-finite HDR"
            differ = int((fo["hdr16"] != fp["hdr16"]).any(axis=2).sum())
            assert differ <= 1, tag + f": {differ} px differ"
            compare_frames(images_from(fo, fp), fp, tag)
        p.close()


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("size", [1, 2])
def test_fragment_lists_as_long_as_the_buffer(r3, monkeypatch, size, samples):
    """1x1 and 2x2 targets, 1, 2 and 17 layers, the node buffer exactly as large as the fragment count: on the single-sample 1x1
    target the one list holds `capacity` nodes, where both bounds of k_blend_apply's loops meet the list's length -- every layer
    must still be blended, bit-exact."""
    for L in (1, 2, 17):
        N = size * size * samples * L
        o = OracleRenderer(oh.LEFT, f32(1.0))
        layer_scene(o, omk, L)
        kw = dict(samples=samples, ambient=AMBIENT, clear_color=CLEAR)
        fo = o.render(size, size, **kw)
        p = hip(r3, monkeypatch, {"R3N_FRAG_CAPACITY": N}, oh.LEFT, f32(1.0))
        layer_scene(p, r3.material_record, L)
        fp = p.render(size, size, **kw)
        p.sync()
        assert codes(p) == [], f"{size}x{size}, {L} layers, capacity {N}: reports {p.capacity_reports}"
        compare_frames(fo, fp, f"{size}x{size}, {samples} samples, {L} layers, capacity {N}")
        p.close()


# ------------------------------------------------------------------ d. the report contract and the frame after an overflow
@pytest.mark.parametrize("env", [{}, {"R3N_PIPELINE": "0"}, {"R3N_FRAME_NODES": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "defaults")
@pytest.mark.parametrize("overflow", ["fragments", "work_queue"])
def test_capacity_report_once_and_the_next_frame_recovers(r3, monkeypatch, env, overflow):
    """Frame 1 overflows (two screen-covering layers where one fits: the node buffer, or the work queue of the transparent pass) and is
    submitted without a read-back; frames 0 and 2 show one layer, the other moved out of view.  From frame 1's render to the r3n_sync
    after frame 2 exactly one call reports R3N_ERR_CAPACITY, no frame is refused, and frames 0 and 2 are the oracle's, bit for bit --
    the node counter, the list heads and the queue counters are reset for every frame."""
    W, H, S = 96, 64, 4
    aspect = f32(W) / f32(H)
    if overflow == "fragments":
        hook = {"R3N_FRAG_CAPACITY": W * H * S}
    else:
        hook = {"R3N_BIG_CAPACITY": -(-W // TILE) * -(-H // TILE)}  # both layers' items land in the one sub-queue of the first wave
    o = OracleRenderer(oh.LEFT, aspect)
    p = hip(r3, monkeypatch, dict(env, **hook), oh.LEFT, aspect)
    assert p.frame_nodes == (env.get("R3N_FRAME_NODES") == "1")
    ho = layer_scene(o, omk, 2)
    hp = layer_scene(p, r3.material_record, 2)
    kw = dict(samples=S, ambient=AMBIENT, clear_color=CLEAR)
    for f in range(3):
        for r, hs in ((o, ho), (p, hp)):
            r.set_object_transform(hs[1], oh.translation((0.0, 0.0, 1.25)) if f == 1 else oh.translation((200.0, 0.0, 1.25)))
        fo = o.render(W, H, **kw)
        fp = p.render(W, H, readback=f != 1, **kw)
        if f == 0:
            p.sync()
            assert codes(p) == [], f"frame 0 fits: reports {p.capacity_reports}"
        if f == 1:
            assert len(fo["blend_list"][0]) == 2 and fp is None
        if f == 2:
            assert len(fo["blend_list"][0]) == 1
            compare_frames(fo, fp, f"{overflow} {env}: the frame after the overflow")
            assert np.isfinite(hdr_f32(fp)).all()
    p.sync()
    assert codes(p) == [ERR_CAPACITY], f"{overflow} {env}: the overflow of frame 1 must be reported exactly once: {p.capacity_reports}"
    p.close()


# ------------------------------------------------------------------ e. the default node buffer at a real shape
def test_default_fragment_capacity_at_4k_msaa(r3, monkeypatch):
    """No hooks: 3840x2160 at 4 samples, two screen-covering translucent layers are 66.4 M fragments against 32 Mi (33.6 M) nodes --
    reported once, every HDR value finite; the next frame with one layer (33.2 M fragments) fits: nothing reported, and every pixel
    is the oracle's one-layer colour."""
    W, H, S = 3840, 2160, 4
    assert W * H * S * 2 > 32 << 20 >= W * H * S
    aspect = f32(W) / f32(H)
    p = hip(r3, monkeypatch, {}, oh.LEFT, aspect)
    hp = layer_scene(p, r3.material_record, 2, lights=False)
    o = OracleRenderer(oh.LEFT, aspect)  # unlit layers: the one-layer colour is the same everywhere; a small target gives it
    ho = layer_scene(o, omk, 2, lights=False)
    o.set_object_transform(ho[1], oh.translation((200.0, 0.0, 1.25)))
    ref = o.render(64, 36, samples=S, ambient=AMBIENT, clear_color=CLEAR)["hdr16"]
    assert (ref == ref[0, 0]).all()
    hdr = np.zeros((H, W, 4), dtype=np.uint16)
    for f in range(2):
        if f == 1:
            p.set_object_transform(hp[1], oh.translation((200.0, 0.0, 1.25)))
        p.render(W, H, samples=S, ambient=AMBIENT, clear_color=CLEAR, readback=False)
        p._check(p.lib.r3n_readback_hdr(p.ctx, hdr.ctypes.data), "r3n_readback_hdr")
        p.sync()
        assert np.isfinite(hdr.view(np.float16)).all(), f"frame {f}: non-finite HDR"
        assert codes(p) == [ERR_CAPACITY], f"frame {f}: reports {p.capacity_reports}"
    assert (hdr == ref[0, 0]).all(), "the one-layer frame after the overflow differs from the oracle's colour"
    p.close()
