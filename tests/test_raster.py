"""tests/raster_reference.py against the oracle, without a GPU, and the conditions tests/test_raster_gpu.py rests on: every world is
on the exact tier, the reference's keys, atlas texels and pass sets are the oracle's at every sample, the worlds reach every scan
path of kernels_raster.h, and the features planted in them are there.

Counts of the planted features, computed by the reference alone (samples; one sample per pixel / four; shadow view 64 / 32):
  edges   samples exactly on an edge, accepted / rejected: 64x64 189 / 235 and 250 / 294, 96x40 158 / 150 and 19 / 19,
          33x17 235 / 229 and 229 / 247; slivers removed by the rint rule that cover a pixel centre: 3 at every extent at one
          sample, none at four (the rule is off: the pass set grows by exactly those 3)
  depth   samples whose winning depth is held by two or more triangles (won by slot): 64x64 970 and 3 878, 96x40 906 and 3 636,
          33x17 138 and 534; samples removed by the z < 0 / z > 1 planes: 64x64 67 / 80 and 268 / 323 (sloped triangles, only
          where the doubled area is a power of two), shadow views 64: 80 / 29 (64x64 world) and 29 / 29, 32: 15 / 7 and 7 / 7
The floors asserted below are those figures rounded down."""
import numpy as np
import pytest

import raster_reference as rr
from oracle import host as oh
from oracle.world import OracleRenderer, material_record as omk

f32, u32 = np.float32, np.uint32
KINDS = ("edges", "boxes", "depth", "random")


def test_constants_are_the_kernels():
    for name, found in rr.kernel_defines().items():
        assert found == [rr.DEFINES[name]], (name, found)


def oracle_frame(kind, W, H, samples, resolutions=()):
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    rr.load(o, omk, rr.worlds(W, H)[kind], oh.identity())
    for res in resolutions:
        o.add_directional_light(resolution=res, **rr.LIGHT)
    o.set_camera_data(oh.identity(), ("raw", oh.identity()))
    return o.render(W, H, samples=samples)


@pytest.mark.parametrize("W,H", rr.EXTENTS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_world_is_on_the_exact_tier(kind, W, H):
    """render() runs with the guard on: every intermediate of every triangle, in the viewport at one and four samples and in both
    shadow views, is held by a f32 (rr.Inexact otherwise)"""
    for samples in (1, 4):
        rr.frame(kind, W, H, samples)
    for res in rr.SHADOW_RESOLUTIONS:
        rr.frame(kind, W, H, 1, res)
    world = rr.worlds(W, H)[kind]
    assert 3 <= len(world["objects"]) <= 6 and sum(len(ob["tris"]) for ob in world["objects"]) <= 400
    assert all(len(ob["tris"]) > 1 for ob in world["objects"][:-1]), "tri_base is not trivial"


def test_the_guard_refuses_what_a_f32_rounds():
    Fr = rr.Fr
    with pytest.raises(rr.Inexact):
        rr.f32(Fr(1, 3))
    with pytest.raises(rr.Inexact):
        rr.f32(Fr((1 << 24) + 1))
    rr.f32(Fr((1 << 24) + 2))
    with pytest.raises(rr.Inexact):
        rr.f32_all(np.array([3 << 10, ((1 << 24) + 1) << 5]))
    view = rr.View(96, 40)
    sloped = ((Fr(0), Fr(0), Fr(0)), (Fr(1, 2), Fr(0), Fr(1)), (Fr(0), Fr(-1, 2), Fr(1, 2)))  # 24 x 10 px legs: area 240, no power of two
    with pytest.raises(rr.Inexact):
        rr.setup(view, sloped)
    assert rr.setup(rr.View(64, 64), sloped)["z"] == (Fr(1, 16), Fr(1, 32), Fr(-3))
    assert rr.f32_bits(1, 0) == 0x3F800000 and rr.f32_bits(3, 2) == 0x3F400000 and rr.f32_bits(1, 21) == 0x35000000 and rr.f32_bits(0, 5) == 0


@pytest.mark.parametrize("W,H", rr.EXTENTS)
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_the_oracle_in_the_viewport(kind, samples, W, H):
    view, ref = rr.frame(kind, W, H, samples)
    fo = oracle_frame(kind, W, H, samples)
    assert fo["vis"].shape == ref["target"].shape
    msg = rr.describe_first_difference(rr.worlds(W, H)[kind], view, ref, fo["vis"])
    assert msg is None, msg
    assert np.array_equal(fo["pass"], ref["pass"]), np.flatnonzero(fo["pass"] != ref["pass"])
    assert np.array_equal(fo["residual"], ref["pass"]) and fo["visible"][: len(rr.worlds(W, H)[kind]["objects"])].all()


@pytest.mark.parametrize("W,H", rr.EXTENTS)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_equals_the_oracle_in_the_shadow_views(kind, W, H):
    """one light (64), then two (64 and 32): the second view sits at a non-zero atlas offset in an atlas wider than either view,
    and the texels outside both rectangles stay 0"""
    world = rr.worlds(W, H)[kind]
    for resolutions in ((64,), (64, 32)):
        fo = oracle_frame(kind, W, H, 1, resolutions)
        aw, ah, rects = rr.atlas_layout(resolutions)
        assert fo["atlas_size"] == (aw, ah)
        assert [(d["offset"][0], d["offset"][1], d["size"], d["handle"]) for d in fo["shadow_descs"]] == [r + (k,) for k, r in enumerate(rects)]
        atlas = fo["atlas"].view(u32).copy()
        for k, (x, y, size) in enumerate(rects):
            view, ref = rr.frame(kind, W, H, 1, size)
            msg = rr.describe_first_difference(world, view, ref, atlas[y:y + size, x:x + size])
            assert msg is None, msg
            assert np.array_equal(fo["shadows"][k]["pass"], ref["pass"])
            atlas[y:y + size, x:x + size] = 0
        assert not atlas.any()
        if len(rects) == 2:
            assert rects[1][0] != 0 and aw not in (rects[0][2], rects[1][2]) and aw * ah > sum(r[2] ** 2 for r in rects)


def drawn_plans(blend=False):
    for W, H in rr.EXTENTS:
        for kind in KINDS:
            views = [rr.frame(kind, W, H, 1)] + ([] if blend else [rr.frame(kind, W, H, 1, res) for res in rr.SHADOW_RESOLUTIONS])
            for view, ref in views:
                for s in ref["recs"]:
                    if s["passes"]:
                        yield view, s, rr.plan(view, s, blend)


def test_the_matrix_reaches_every_scan_path():
    paths = {"in_place": 0, "fine": 0, "coarse": 0, "columns": 0, "rows": 0, "left": 0, "right": 0, "top": 0, "bottom": 0, "empty_first_column": 0}
    for view, s, (path, items) in drawn_plans():
        if path == "in_place":
            paths["in_place"] += 1
            assert s["box"][2] - s["box"][0] < 8 and s["box"][3] - s["box"][1] < 8
            continue
        if path == "none":  # passes the cull and lies outside the target: no pixel to scan
            assert s["box"] is None
            continue
        assert path == "items" and items
        xs, ys = [a[0] for a in s["h"]], [a[1] for a in s["h"]]
        paths["left"] += min(xs) < 0
        paths["right"] += max(xs) > view.W
        paths["top"] += min(ys) < 0
        paths["bottom"] += max(ys) > view.H
        paths["columns"] += items[0]["tx"] > 1
        paths["rows"] += items[0]["ty"] > 1
        for it in items:
            # the opaque producers' items start on a multiple of R3N_ITEM_ALIGN or at the box's own left edge: always fine
            assert it["fine"], (view.name, s["box"], it)
            assert it["rect"][2] - it["gx0"] < 32 and it["rect"][0] >= s["box"][0] and it["rect"][2] <= s["box"][2]
            paths["fine"] += 1
            paths["empty_first_column"] += it["empty"]
    for view, s, (path, items) in drawn_plans(blend=True):
        if path == "none":
            continue
        assert path == "items"
        paths["coarse"] += sum(not it["fine"] for it in items)
        for it in items:
            assert it["fine"] == ((it["rect"][0] & 15) + it["rect"][2] - it["rect"][0] < 32 and it["rect"][3] - it["rect"][1] < 32)
    print(paths)
    assert paths["empty_first_column"] == 0
    for name in ("in_place", "fine", "coarse", "columns", "rows", "left", "right", "top", "bottom"):
        assert paths[name] >= 3, (name, paths)


def test_plan_by_hand():
    Fr = rr.Fr
    view = rr.View(64, 64)

    def tri(x0, y0, x1, y1):  # window-space right triangle with the visible winding
        cx, cy = (lambda X: Fr(X, 32) - 1), (lambda Y: 1 - Fr(Y, 32))
        return rr.setup(view, ((cx(x0), cy(y0), Fr(1, 2)), (cx(x1), cy(y0), Fr(1, 2)), (cx(x0), cy(y1), Fr(1, 2))))
    s = tri(17, 10, 23, 16)
    assert s["visible"] and s["box"] == (16, 9, 24, 17) and rr.plan(view, s)[0] == "items"  # 9 x 9 px: one work item
    assert [it["rect"] for it in rr.plan(view, s)[1]] == [(16, 9, 24, 17)]
    s = tri(17, 10, 22, 15)
    assert s["box"] == (16, 9, 23, 16) and rr.plan(view, s) == ("in_place", [])  # 8 x 8 px
    assert len(rr.plan(view, s, blend=True)[1]) == 1
    s = tri(Fr(63, 2), 2, 50, 40)  # x0 = 30: columns start at 16; 48, 0: the box reaches x = 51
    assert s["box"] == (30, 1, 51, 41)
    path, items = rr.plan(view, s)
    assert [it["rect"] for it in items] == [(30, 1, 47, 32), (48, 1, 51, 32), (30, 33, 47, 41), (48, 33, 51, 41)] and all(it["fine"] for it in items)
    path, items = rr.plan(view, s, blend=True)  # unaligned: 22 px from x = 30 reach past 16 + 32
    assert [it["rect"] for it in items] == [(30, 1, 51, 32), (30, 33, 51, 41)] and [it["fine"] for it in items] == [False, False]
    assert "coarse" in rr.locate(view, s, 40, 20, blend=True) and "work item 1 of 4" in rr.locate(view, s, 49, 2)


FLOORS = {  # (world, extent): {samples or "shadow <res>": {feature: floor}}
    ("edges", (64, 64)): {1: dict(edge_accepted=180, edge_rejected=230, rint_covering=3), 4: dict(edge_accepted=250, edge_rejected=290)},
    ("edges", (96, 40)): {1: dict(edge_accepted=150, edge_rejected=150, rint_covering=3), 4: dict(edge_accepted=19, edge_rejected=19)},
    ("edges", (33, 17)): {1: dict(edge_accepted=230, edge_rejected=220, rint_covering=3), 4: dict(edge_accepted=220, edge_rejected=240)},
    ("depth", (64, 64)): {1: dict(ties=900, below=60, above=80), 4: dict(ties=3800, below=260, above=320), "shadow 64": dict(ties=700, below=80, above=29),
                          "shadow 32": dict(ties=170, below=15, above=7)},
    ("depth", (96, 40)): {1: dict(ties=900), 4: dict(ties=3600), "shadow 64": dict(ties=700, below=29, above=29), "shadow 32": dict(ties=180, below=7, above=7)},
    ("depth", (33, 17)): {1: dict(ties=130), 4: dict(ties=530), "shadow 64": dict(ties=700, below=29, above=29), "shadow 32": dict(ties=180, below=7, above=7)},
}


@pytest.mark.parametrize("kind,extent", sorted(FLOORS))
def test_planted_features_are_there(kind, extent):
    W, H = extent
    for where, floors in FLOORS[(kind, extent)].items():
        _view, ref = rr.frame(kind, W, H, where) if isinstance(where, int) else rr.frame(kind, W, H, 1, int(where.split()[1]))
        print(kind, extent, where, ref["count"])
        for name, floor in floors.items():
            assert ref["count"][name] >= floor, (kind, extent, where, name, ref["count"])
    if kind == "edges":  # under multisampling the rint rule is off: exactly the slivers come back
        one, four = rr.frame(kind, W, H, 1)[1], rr.frame(kind, W, H, 4)[1]
        assert four["count"]["rint_covering"] == 0 and int(four["pass"].sum()) == int(one["pass"].sum()) + one["count"]["rint_covering"]
        assert sum(s["why"] == "rint" for s in one["recs"]) >= 3
    if kind == "depth":  # depth 0 drawn (a key with zero depth bits), -0 as +0, depth 1 drawn, the dyadics outside removed
        ref = rr.frame(kind, W, H, 1)[1]
        t = ref["target"]
        zero = (t != 0) & (t >> np.uint64(32) == 0)
        slots = set(((t[zero] & np.uint64(0xFFFFFFFF)) - np.uint64(1)).tolist())
        special = [s for s in ref["recs"] if s["object"] == 1 and s["passes"]]
        assert len(special) == 4 and {s["slot"] for s in special if s["z"][2] == 0} == slots and len(slots) == 2
        assert (t >> np.uint64(32) == 0x3F800000).any()
        assert sum(s["why"] == "hiz" for s in ref["recs"]) == 3, "the triangles behind z = 0 fall to the all-zero pyramid"
        sh = rr.frame(kind, W, H, 1, 64)[1]
        assert (sh["target"] == 0x3F800000).any() and sh["count"]["above"] > 0 and sh["count"]["below"] > 0


@pytest.mark.parametrize("W,H", rr.EXTENTS)
@pytest.mark.parametrize("samples", [1, 4])
def test_blend_coverage_expected_is_the_oracles(samples, W, H):
    """What test_raster_gpu.py::test_blend_coverage expects, on the oracle: one translucent triangle per case of the boxes world moved
    into the frame in turn; the pixels whose HDR value differs from the frame without it are the reference's mask -- covered samples
    not behind the opaque layer.  Some cases lie behind the layer in part, and k_blend_setup's split makes some items coarse."""
    clear, far = (0.02, 0.03, 0.05, 1.0), oh.translation((100.0, 0.0, 0.0))
    view, opaque_world, opaque, depth_bits, cases = rr.blend_setup(W, H, samples)
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    o.set_camera_data(oh.identity(), ("raw", oh.identity()))
    rr.load(o, omk, opaque_world, oh.identity())
    handles = [rr.load(o, omk, rr.blend_object(t), far, key=rr.BLEND, albedo=(0.9, 0.2, 0.1, 0.5))[0] for t, _s in cases]
    bare = o.render(W, H, samples=samples, clear_color=clear)["hdr16"]
    coarse = hidden = partly = 0
    for n, ((_t, s), h) in enumerate(zip(cases, handles)):
        o.set_object_transform(h, oh.identity())
        fo = o.render(W, H, samples=samples, clear_color=clear)
        o.set_object_transform(h, far)
        want, dropped = rr.blend_expected(view, s, depth_bits)
        got = (fo["hdr16"] != bare).any(axis=2)
        assert np.array_equal(got, want), (n, s["box"], np.argwhere(got != want)[:4])
        assert np.array_equal(fo["vis"], opaque["target"])
        hidden += dropped
        partly += bool(dropped and want.any())
        coarse += sum(not it["fine"] for it in rr.plan(view, s, blend=True)[1]) if want.any() else 0
    assert coarse >= (3 if W >= 64 else 1) and hidden > 0 and partly > 0, (coarse, hidden, partly)
