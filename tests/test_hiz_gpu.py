"""The Hi-Z pyramid builder (r3n_hi_z: k_hiz_head, k_hiz_downsample, k_hiz_tail) on every launch plan it can take, and the
triangle cull's reads of it (hiz_sample_min), on the GPU -- bit for bit against tests/hiz_reference.py and against the oracle.

Scenes only ever produce depth in about 0 .. 0.012 and pyramids whose windows hardly matter; here an ARBITRARY depth plane is given
to both sides instead: the product's at the "pass1" exchange site, where r3n_exchange_depth hands out the device address of mip 0
(between the pass-1 raster and Hi-Z, on the one-call frame and on the per-node frame), the oracle's at its "pass1_depth" hook.
Only the depth plane is ever written, never the key buffer (later stages take object and triangle numbers from the keys).
tests/test_hiz.py holds the conditions this file rests on: reference == oracle at every extent, the extents reach every plan."""
import ctypes
import functools

import numpy as np
import pytest

import hiz_reference as hz
import scenes
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


class Inject:
    """The `exchange` callable of Renderer.render: while `plane` is set, the pass-1 depth plane is overwritten with it -- a copy
    ordered on the context's stream (behind the pass-1 raster and k_hiz_mip0, in front of r3n_hi_z), as parallel.Exchange orders
    its collectives.  With `plane` None the site does nothing: Hi-Z then reads the keys."""

    def __init__(self, renderer):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", 0)
        self.stream = torch.cuda.ExternalStream(renderer.lib.r3n_stream(renderer.ctx), device=self.device)
        self.plane = None
        self.calls = 0

    def __call__(self, what, renderer, ev=None, samples=1):
        from rend3_amd import parallel
        if what != "pass1" or self.plane is None:
            return
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        renderer._check(renderer.lib.r3n_exchange_depth(renderer.ctx, ctypes.byref(p), ctypes.byref(n)), "r3n_exchange_depth")
        host = np.ascontiguousarray(self.plane, dtype=f32).reshape(-1)
        assert n.value == host.size, "the plane r3n_exchange_depth hands out is the target's"
        with self.torch.cuda.stream(self.stream):
            parallel.device_tensor(p.value, n.value, "<f4", self.device).copy_(self.torch.from_numpy(host))
        self.calls += 1


def oracle_hook(plane):
    def hook(what, buf, **_kw):
        if what == "pass1_depth" and plane is not None:
            buf[:] = plane.reshape(-1)
    return hook


def assert_pyramid(p, w, h, fo_hiz, plane, tag):
    """the product's pyramid == the oracle's == (for a known plane) the numpy reference's, as u32 words"""
    got = p.readback_hiz(w, h)
    if plane is not None:
        diff = hz.first_difference(hz.pyramid(plane), got, w, h)
        assert diff is None, f"{tag}: against the numpy reference: {diff}"
    diff = hz.first_difference(fo_hiz, got, w, h)
    assert diff is None, f"{tag}: against the oracle: {diff}"


def empty_pair(r3):
    o, p = OracleRenderer(oh.LEFT), r3.Renderer(oh.LEFT)
    for r in (o, p):
        r.set_camera_data(oh.identity(), ("raw", oh.identity()))
    return o, p


# ------------------------------------------------------------------ pyramid bits at the extent matrix, both frame paths
@pytest.mark.parametrize("frame_nodes", [False, True], ids=["one_call_frame", "per_node_frame"])
@pytest.mark.parametrize("group", sorted(hz.EXTENT_GROUPS))
def test_injected_plane_pyramid_at_every_launch_plan(r3, monkeypatch, group, frame_nodes):
    """One context, an empty world, every extent of the group x every recipe: head with 0 .. 4 levels (stopped by an odd side, by
    the cap, by the mip count), unit sides, tiles partly outside the target, the grid downsample, the 256- and the 1024-thread
    tail, tail levels in LDS array A, in B and in neither (hiz_reference.launch_plan; test_extents_reach_every_launch_plan)."""
    if frame_nodes:
        monkeypatch.setenv("R3N_FRAME_NODES", "1")
    o, p = empty_pair(r3)
    assert p.frame_nodes == frame_nodes
    inj = Inject(p)
    try:
        for w, h in hz.EXTENT_GROUPS[group]:
            for name in sorted(hz.RECIPES):
                plane = hz.RECIPES[name](w, h, seed=w * 131 + h)
                fo = o.render(w, h, exchange=oracle_hook(plane))
                inj.plane = plane
                calls = inj.calls
                p.render(w, h, readback=False, exchange=inj)
                assert inj.calls == calls + 1
                assert_pyramid(p, w, h, fo["hiz"], plane, f"{w}x{h} {name} {hz.launch_plan(w, h)}")
    finally:
        p.close()


def test_pyramid_follows_the_target_through_a_sequence_of_extents(r3):
    """One context, the extents change every frame and only every other frame injects: the pyramid is reallocated, its descriptor
    recomputed, and hiz_plane_ready must not outlive its frame -- a frame WITHOUT injection over an empty world builds its
    pyramid from the (cleared) keys, all zeros, whatever an earlier, larger frame left in the buffer."""
    o, p = empty_pair(r3)
    inj = Inject(p)
    try:
        frame = 0
        for phase in (0, 1):  # second time round the other half of the frames injects
            for w, h in ((256, 160), (37, 19), (801, 481), (202, 118)):
                plane = hz.planted(w, h, seed=frame) if frame % 2 == phase else None
                fo = o.render(w, h, exchange=oracle_hook(plane))
                inj.plane = plane
                p.render(w, h, readback=False, exchange=inj)
                assert_pyramid(p, w, h, fo["hiz"], plane, f"frame {frame} {w}x{h} injected={plane is not None}")
                if plane is None:
                    assert not p.readback_hiz(w, h).view(np.uint32).any(), f"frame {frame}: nothing drawn, nothing injected"
                frame += 1
    finally:
        p.close()


# ------------------------------------------------------------------ real scenes: the keys path and the multisample resolve
def scene_pair(r3, w, h):
    """scene and camera of test_gpu_parity.test_hiz_pyramid_matches_oracle"""
    o, p = OracleRenderer(oh.LEFT, f32(w) / f32(h)), r3.Renderer(oh.LEFT, f32(w) / f32(h))
    scenes.build_random_scene(o, oh, omk, 120, 7, lights=0)
    scenes.build_random_scene(p, oh, r3.material_record, 120, 7, lights=0)
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((0, 2, -8), (0, 0, 0), (0, 1, 0)), ("perspective", 70.0, 0.1))
    return o, p


@pytest.mark.parametrize("samples,w,h", [(1, 201, 121), (1, 202, 118), (1, 401, 241),
                                         (4, 211, 140), (4, 202, 118), (4, 64, 64), (4, 401, 241)])
def test_scene_pyramid_from_keys_and_from_the_multisample_resolve(r3, samples, w, h):
    """No injection: mip 0 from the visibility keys (samples == 1) or as resolve_depth_min over the four samples, at extents
    that take the grid downsample and both tail sizes.  Frame 0 draws everything in pass 2; frame 1's pass 1 draws the predicted
    triangles, so its pyramid is not trivial."""
    o, p = scene_pair(r3, w, h)
    try:
        o.render(w, h, samples=samples)
        p.render(w, h, samples=samples, readback=False)
        fo = o.render(w, h, samples=samples)
        p.render(w, h, samples=samples, readback=False)
        assert fo["hiz"].max() > 0
        # above its own level 0 (the keys' depth, or their resolve) the oracle's chain is the numpy reference's
        assert hz.first_difference(hz.pyramid(fo["depth_pass1"]), fo["hiz"], w, h) is None
        assert_pyramid(p, w, h, fo["hiz"], fo["depth_pass1"], f"{w}x{h} samples={samples} {hz.launch_plan(w, h, samples)}")
    finally:
        p.close()


# ------------------------------------------------------------------ the cull against injected pyramids
CULL_PLANES = {
    "blocks16": lambda w, h, seed: hz.blocks(w, h, seed, 16, 0.03),
    "blocks4": lambda w, h, seed: hz.blocks(w, h, seed, 4, 0.03),
    "planted": lambda w, h, seed: (hz.planted(w, h, seed) * f32(0.03)).astype(f32),
}


@functools.lru_cache(maxsize=None)
def passes_with_a_zero_plane(w, h):
    """how many triangles of the scene pass the cull when the pyramid occludes nothing (oracle only; frames 0 and 1)"""
    o = OracleRenderer(oh.LEFT, f32(w) / f32(h))
    scenes.build_random_scene(o, oh, omk, 120, 7, lights=0)
    o.set_camera_data(oh.look_at_lh((0, 2, -8), (0, 0, 0), (0, 1, 0)), ("perspective", 70.0, 0.1))
    zero = np.zeros((h, w), dtype=f32)
    return tuple(int(o.render(w, h, exchange=oracle_hook(zero))["pass"].sum()) for _ in range(2))


# (recipe, extent, the seed of frame 0's and of frame 1's plane).  The seeds are chosen on the oracle's result alone, so that the
# condition below holds.  `planted` has 20 % background texels: from level 2 up nearly every window holds a 0.0 and occludes
# nothing, only triangles about a texel long can be rejected -- at 37 x 19 that is 4 % .. 13 % of them by seed (2 % at 201 x 121),
# hence the small target and seeds 6 and 10 (12.6 % and 12.1 %).
CULL_CASES = [("blocks16", 201, 121, (1, 2)), ("blocks16", 202, 118, (1, 2)), ("blocks16", 37, 19, (1, 2)), ("blocks16", 256, 160, (1, 2)),
              ("blocks4", 201, 121, (1, 2)), ("planted", 37, 19, (6, 10))]


@pytest.mark.parametrize("recipe,w,h,seeds", CULL_CASES, ids=[f"{r}-{w}x{h}" for r, w, h, _s in CULL_CASES])
def test_cull_decisions_against_an_injected_pyramid(r3, recipe, w, h, seeds):
    """hiz_sample_min fed pyramids no scene produces: occluders of the scene's own depth range (0 .. 0.03) in blocks, so a
    triangle passes or not by WHICH texels of WHICH level it reads.  Both frames inject (a different plane each, so frame 1 has
    residual triangles); both frames are compared whole (sets, keys, image) and so are their pyramids.
    Condition, on the oracle alone: the injected pyramid rejects 10 % .. 90 % of the triangles that pass against an all-zero one."""
    o, p = scene_pair(r3, w, h)
    inj = Inject(p)
    free = passes_with_a_zero_plane(w, h)
    try:
        for f in range(2):
            plane = CULL_PLANES[recipe](w, h, seeds[f])
            fo = o.render(w, h, exchange=oracle_hook(plane))
            rejected = 1.0 - int(fo["pass"].sum()) / free[f]
            print(f"{recipe} {w}x{h} frame {f}: {int(fo['pass'].sum())} of {free[f]} pass, {100 * rejected:.1f} % rejected")
            assert 0.10 <= rejected <= 0.90, "the decisions must depend on the texels read"
            inj.plane = plane
            fp = p.render(w, h, exchange=inj)
            compare_frames(fo, fp, f"{recipe} {w}x{h} frame {f}")
            assert_pyramid(p, w, h, fo["hiz"], plane, f"{recipe} {w}x{h} frame {f}")
        assert fo["residual"].sum() > 0, "frame 1's plane uncovers triangles frame 0's hid"
    finally:
        p.close()
