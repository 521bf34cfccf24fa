"""The rasteriser (kernels_raster.h k_raster_small, k_raster_big, k_blend_setup; device_math.h setup_triangle, tri_bounds, the edge
and depth evaluation) on every scan path, sample for sample against tests/raster_reference.py -- an exact integer restatement of
the contract -- and, the worlds being small, against whole oracle frames as well.

The paths, and what reaches them here (tests/test_raster.py asserts from plan() that the worlds do):
  in-place scan            boxes up to 8 x 8 px, one thread (every world)
  work items, fine blocks  larger boxes split into 32 px tiles whose columns start on 16 px; 8 x 2 blocks, four per step.  One sample,
                           opaque: shade_pixel_cmpx (the 64-bit atomic on the key target, the 32-bit one in the shadow views);
                           four samples and the cutout key: the generic shade_pixel with its pre-read of the target
  coarse 8 x 8 blocks      ONLY k_blend_setup's items reach them: k_raster_big takes the fine mode when rx1 - (rx0 & ~15) < 32 and
                           ry1 - ry0 < 32, and an opaque producer's item starts at its column's aligned origin or -- first column --
                           at the box's own left edge less than 16 px after it, and ends at most 31 px after that origin; rows are
                           32 px.  k_blend_setup splits from the box's left edge, so an item whose left edge is x0 mod 16 = r is
                           coarse as soon as it is more than 32 - r px wide.  It runs with shade_pixel<BLEND>
                           (test_blend_coverage; test_raster.py::test_the_matrix_reaches_every_scan_path asserts both halves)
  queue full               R3N_BIG_CAPACITY=1: the producer scans its items itself
  shadow views             vp_x / vp_y non-zero and target_pitch != vp_w with two lights
  threshold packing        every work item: the top-left rule of fans and strips whose shared edges run through sample points
-0: a triangle at z = -0 is in the depth world, and the reference stores it as +0 -- but at w = 1 neither the oracle nor the kernels
ever FORM a depth of -0 in the viewport: z = (gx px + gy py) + c is -0 only when gx, gy and c all are, gx = gy = -0 makes
c = (zn0 - gx sx0) - gy sy0 = -0 only for sx0 < 0 and sy0 < 0, and a triangle of the viewport's winding with those gradient signs and
vertex 0 above and left of the target covers no pixel of it.  The sign-bit mask of shade_pixel_cmpx is therefore not reachable from
this file's worlds (it guards the plane of triangles with a vertex at w <= 0, which the oracle frames cover).
Which items a call queued is read from r3n_readback_raster_stats and compared with plan()'s count.  A failure names the first
differing sample, the triangles expected and found there, and the path, work item and block plan() assigns to it."""
import numpy as np
import pytest

import raster_reference as rr
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32, u32, u64 = np.float32, np.uint32, np.uint64
KINDS = ("edges", "boxes", "depth", "random")
FRAME_PATHS = pytest.mark.parametrize("frame_nodes", [False, True], ids=["one_call_frame", "per_node_frame"])
IDENT = oh.identity()


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def hip(r3, monkeypatch, frame_nodes, W, H, env=None):
    """A HIP renderer created under `env` (read once, by r3n_create) that records capacity reports instead of raising."""
    for k in ("R3N_BIG_CAPACITY", "R3N_FRAG_CAPACITY"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("R3N_FRAME_NODES", "1" if frame_nodes else "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    p = r3.Renderer(oh.LEFT, f32(W) / f32(H))
    p.capacity_reports = []
    assert p.frame_nodes == frame_nodes
    p.set_camera_data(IDENT, ("raw", IDENT))
    return p


def oracle(W, H, world, resolutions=(), **material):
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    rr.load(o, omk, world, IDENT, **material)
    for res in resolutions:
        o.add_directional_light(resolution=res, **rr.LIGHT)
    o.set_camera_data(IDENT, ("raw", IDENT))
    return o


def queued(stats):
    """the non-zero item counts of the viewport's forward calls in call order, of the shadow lanes' sorted"""
    return [int(v) for v in stats[:16] if v], sorted(int(v) for v in stats[16:] if v)


def check_viewport(world, view, ref, fp, tag, first_frame=True):
    msg = rr.describe_first_difference(world, view, ref, fp["vis"])
    assert msg is None, f"{tag}: {msg}"
    n = len(ref["pass"])
    if first_frame:
        assert np.array_equal(fp["pass"][:n], ref["pass"]), f"{tag}: pass set differs at {np.flatnonzero(fp['pass'][:n] != ref['pass'])[:8]}"
        assert np.array_equal(fp["residual"][:n], ref["pass"]), tag
    else:  # drawn through the predicted source: nothing is left for the second pass (the pyramid may cull what the first drew)
        assert not fp["residual"].any() and not (fp["pass"][:n] & ~ref["pass"]).any(), tag


def check_atlas(world, W, H, kind, fp, resolutions, tag, empty=False):
    aw, ah, rects = rr.atlas_layout(resolutions)
    assert tuple(fp["atlas_size"]) == (aw, ah), tag
    atlas = fp["atlas"].view(u32).copy()
    items = []
    for k, (x, y, size) in enumerate(rects):
        view, ref = rr.frame(kind, W, H, 1, size)
        if empty:
            assert not atlas[y:y + size, x:x + size].any(), f"{tag}: view {k} is not empty"
        else:
            msg = rr.describe_first_difference(world, view, ref, np.ascontiguousarray(atlas[y:y + size, x:x + size]))
            assert msg is None, f"{tag} view {k} at ({x}, {y}) of a {aw} x {ah} atlas: {msg}"
        assert np.array_equal(fp["shadows"][k]["pass"][: len(ref["pass"])], ref["pass"]), f"{tag}: view {k} pass set"
        atlas[y:y + size, x:x + size] = 0
        items.append(rr.item_count(view, ref["recs"]))
    assert not atlas.any(), f"{tag}: texels outside the views were written"
    return sorted(n for n in items if n)


# ------------------------------------------------------------------ forward: keys, pass sets, items, two frames
@FRAME_PATHS
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("W,H", rr.EXTENTS)
def test_forward_keys_pass_sets_and_items(r3, monkeypatch, W, H, samples, frame_nodes):
    """Every world of the extent, two frames of the unchanged world each: frame 0 draws the residual source, frame 1 the predicted
    one and leaves an empty residual set; both give the reference's keys as u64, the first its pass set, each call the item count
    plan() predicts; both are the oracle's whole frames."""
    for kind in KINDS:
        world = rr.worlds(W, H)[kind]
        view, ref = rr.frame(kind, W, H, samples)
        want = rr.item_count(view, ref["recs"])
        p, o = hip(r3, monkeypatch, frame_nodes, W, H), oracle(W, H, world)
        try:
            rr.load(p, r3.material_record, world, IDENT)
            for f in range(2):
                tag = f"{kind} {W}x{H}x{samples} frame {f}"
                fp = p.render(W, H, samples=samples)
                stats = queued(p.raster_stats())
                check_viewport(world, view, ref, fp, tag, first_frame=f == 0)
                assert stats == ([want] if want else [], []), f"{tag}: work items queued {stats}, plan() says {want}"
                compare_frames(o.render(W, H, samples=samples), fp, tag)
            p.sync()
            assert p.capacity_reports == [], kind
        finally:
            p.close()


# ------------------------------------------------------------------ shadow views
@FRAME_PATHS
@pytest.mark.parametrize("W,H", rr.EXTENTS)
def test_shadow_atlas_words(r3, monkeypatch, W, H, frame_nodes):
    """One light (a 64 px view at the atlas origin) and two (the 32 px view at x = 64 of a 128 x 64 atlas: vp_x != 0, pitch != width):
    the atlas as u32 words, the views' pass sets, the items their depth-only calls queued, zero outside the views."""
    for kind in KINDS:
        world = rr.worlds(W, H)[kind]
        vview, vref = rr.frame(kind, W, H, 1)
        for resolutions in ((64,), (64, 32)):
            tag = f"{kind} {W}x{H} lights {resolutions}"
            p, o = hip(r3, monkeypatch, frame_nodes, W, H), oracle(W, H, world, resolutions)
            try:
                rr.load(p, r3.material_record, world, IDENT)
                for res in resolutions:
                    p.add_directional_light(resolution=res, **rr.LIGHT)
                fp = p.render(W, H)
                stats = queued(p.raster_stats())
                want = check_atlas(world, W, H, kind, fp, resolutions, tag)
                check_viewport(world, vview, vref, fp, tag)
                assert stats[1] == want, f"{tag}: the depth-only calls queued {stats[1]} items, plan() says {want}"
                compare_frames(o.render(W, H), fp, tag)
            finally:
                p.close()


# ------------------------------------------------------------------ the cutout key: generic shade_pixel in work items
@FRAME_PATHS
@pytest.mark.parametrize("W,H", rr.EXTENTS)
def test_cutout_key_above_and_below_the_cutoff(r3, monkeypatch, W, H, frame_nodes):
    """The same worlds under an untextured cutout material (alpha-mode key 1).  Alpha 0.75 against a cutoff of 0.5: keys and atlas
    identical to the opaque run -- drawn by the generic shade_pixel with its read of the target in front of the alpha test, in place
    and in work items, at one and four samples and in the shadow view.  Alpha 0.25: nothing is drawn anywhere."""
    for kind in KINDS:
        world = rr.worlds(W, H)[kind]
        for alpha in (0.75, 0.25):
            material = dict(albedo=(0.5, 0.25, 0.75, alpha), cutout=0.5)
            for samples in (1, 4):
                tag = f"{kind} {W}x{H}x{samples} cutout alpha {alpha}"
                view, ref = rr.frame(kind, W, H, samples)
                p = hip(r3, monkeypatch, frame_nodes, W, H)
                try:
                    rr.load(p, r3.material_record, world, IDENT, key=rr.CUTOUT, **material)
                    p.add_directional_light(resolution=64, **rr.LIGHT)
                    fp = p.render(W, H, samples=samples)
                    stats = queued(p.raster_stats())
                    want = rr.item_count(view, ref["recs"])
                    assert stats[0] == ([want] if want else []), f"{tag}: {stats} items, plan() says {want}"
                    if alpha > 0.5:
                        check_viewport(world, view, ref, fp, tag)
                        check_atlas(world, W, H, kind, fp, (64,), tag)
                    else:
                        assert not fp["vis"].any(), f"{tag}: {int((fp['vis'] != 0).sum())} samples drawn below the cutoff"
                        check_atlas(world, W, H, kind, fp, (64,), tag, empty=True)
                        assert np.array_equal(fp["pass"][: len(ref["pass"])], ref["pass"]), tag
                    if samples == 1:
                        compare_frames(oracle(W, H, world, (64,), key=rr.CUTOUT, **material).render(W, H), fp, tag)
                finally:
                    p.close()


# ------------------------------------------------------------------ queue full: the producer scans its items itself
@FRAME_PATHS
@pytest.mark.parametrize("W,H", rr.EXTENTS)
def test_queue_full_scan_gives_the_same_samples(r3, monkeypatch, W, H, frame_nodes):
    """The boxes world with one entry per work sub-queue, one and four samples and the shadow view: keys and atlas unchanged, nothing
    reported, and in every call some triangle queued more items than its sub-queue holds."""
    world = rr.worlds(W, H)["boxes"]
    for samples in (1, 4):
        tag = f"boxes {W}x{H}x{samples} R3N_BIG_CAPACITY=1"
        view, ref = rr.frame("boxes", W, H, samples)
        p = hip(r3, monkeypatch, frame_nodes, W, H, {"R3N_BIG_CAPACITY": 1})
        try:
            rr.load(p, r3.material_record, world, IDENT)
            p.add_directional_light(resolution=64, **rr.LIGHT)
            fp = p.render(W, H, samples=samples)
            stats = queued(p.raster_stats())
            check_viewport(world, view, ref, fp, tag)
            want_shadow = check_atlas(world, W, H, "boxes", fp, (64,), tag)
            assert stats == ([rr.item_count(view, ref["recs"])], want_shadow), f"{tag}: {stats}"
            # a thread queues all the items of its triangle into ONE sub-queue: a triangle of two items overflows a queue of one entry
            for v, r in ((view, ref), rr.frame("boxes", W, H, 1, 64)):
                assert max(len(rr.plan(v, s)[1]) for s in r["recs"] if s["passes"]) >= 2, f"{tag}: no sub-queue overflows in {v.name}"
            p.sync()
            assert p.capacity_reports == [], f"{tag}: the producers' own scan must not report ({p.capacity_reports})"
        finally:
            p.close()


# ------------------------------------------------------------------ blend coverage: the coarse blocks
CLEAR = (0.02, 0.03, 0.05, 1.0)
FAR = oh.translation((100.0, 0.0, 0.0))
BLEND_ALBEDO = (0.9, 0.2, 0.1, 0.5)


@FRAME_PATHS
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("W,H", rr.EXTENTS)
def test_blend_coverage(r3, monkeypatch, W, H, samples, frame_nodes):
    """One unlit translucent triangle per case of the boxes world, alone in the frame over a clear colour it differs from, with an
    opaque layer at z = 9/128 over the lower left half of the target in front of the first cases: the pixels whose HDR value differs
    from the frame without the triangle are exactly those with a sample the reference covers at a depth not behind the opaque
    one.  k_blend_setup splits from the box's own left edge: some of these items are scanned in coarse 8 x 8 blocks."""
    view, opaque_world, opaque, depth_bits, cases = rr.blend_setup(W, H, samples)
    p = hip(r3, monkeypatch, frame_nodes, W, H)
    try:
        rr.load(p, r3.material_record, opaque_world, IDENT)
        handles = []
        for t, _s in cases:
            handles += rr.load(p, r3.material_record, rr.blend_object(t), FAR, key=rr.BLEND, albedo=BLEND_ALBEDO)
        bare = p.render(W, H, samples=samples, clear_color=CLEAR)["hdr16"]
        assert len(np.unique(bare.reshape(-1, 4), axis=0)) >= 2, "the clear colour and the opaque layer"
        occ_items = rr.item_count(view, opaque["recs"])
        coarse = hidden = partly = 0
        for n, ((t, s), h) in enumerate(zip(cases, handles)):
            tag = f"boxes {W}x{H}x{samples} case {n} (box {s['box']})"
            p.set_object_transform(h, IDENT)
            fp = p.render(W, H, samples=samples, clear_color=CLEAR)
            stats = queued(p.raster_stats())
            p.set_object_transform(h, FAR)
            want, dropped = rr.blend_expected(view, s, depth_bits)
            hidden += dropped
            partly += bool(dropped and want.any())
            got = (fp["hdr16"] != bare).any(axis=2)
            if not np.array_equal(got, want):
                d = np.argwhere(got != want)
                y, x = int(d[0][0]), int(d[0][1])
                raise AssertionError(f"{tag}: {len(d)} px differ, first ({x}, {y}): blended {bool(got[y, x])}, reference {bool(want[y, x])}; "
                                     f"{rr.locate(view, s, x, y, blend=True)}")
            items = len(rr.plan(view, s, blend=True)[1]) if s["passes"] else 0
            coarse += sum(not it["fine"] for it in rr.plan(view, s, blend=True)[1]) if want.any() else 0
            assert stats[0] in ([occ_items, items], [occ_items]) and (stats[0] == [occ_items, items] or not want.any()), f"{tag}: {stats} items, plan() says {items}"
            msg = rr.describe_first_difference(opaque_world, view, opaque, fp["vis"])
            assert msg is None, f"{tag}: the transparent pass writes no keys: {msg}"
        assert coarse >= (3 if W >= 64 else 1), "items scanned in coarse blocks"
        assert hidden > 0 and partly > 0, "cases behind the opaque layer, in part and wholly"
        p.sync()
        assert p.capacity_reports == []
    finally:
        p.close()
