"""tests/object_pass_reference.py against the oracle, without a GPU, and the conditions tests/test_object_pass_gpu.py rests on:
the reference's constants are the kernels', the capacity lists reach every launch plan and parameter edge of the object pass,
the exact tier is exact, the random tier straddles the frustum, and the palette's triangles pass the triangle cull whatever is
drawn around them."""
import os
import re

import numpy as np
import pytest

import object_pass_reference as op
from oracle import host as oh
from oracle.world import OracleRenderer, material_record as omk

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "rend3_amd", "csrc", "kernels_cull.h")).read()
    for name, value in op.DEFINES.items():
        found = re.findall(r"^#define\s+" + name + r"\s+(\d+)u?\b", text, flags=re.M)
        assert found == [str(value)], (name, found)
    assert op.VIS_DRAWN == int(re.search(r"^#define R3N_VIS_DRAWN (\d+)u", text, flags=re.M).group(1))
    assert op.VIS_INSIDE == int(re.search(r"^#define R3N_VIS_INSIDE (\d+)u", text, flags=re.M).group(1))
    # the host logic launch_plan restates
    host = open(os.path.join(ROOT, "rend3_amd", "csrc", "r3n.hip")).read()
    assert "if (cap <= R3N_FUSED_OBJECT_PASS_MAX)" in host and "dim3(nblocks <= 64u ? 64 : 1024)" in host
    assert "chained_rounds(c) <= R3N_CHAINED_OBJECT_PASS_MAX_ROUNDS" in host


def test_launch_plans_by_hand():
    P = op.launch_plan
    assert P(1, False)["plan"] == "fused" and P(1024, False)["plan"] == "fused"
    assert P(1025, False) == dict(plan="three_launch", canonical="three_launch", scan_width=64, scan_iterations=1, rounds=None, grid=None, fits=None)
    assert (P(16_384, False)["scan_width"], P(16_385, False)["scan_width"]) == (64, 1024)
    assert (P(262_144, False)["scan_iterations"], P(262_145, False)["scan_iterations"]) == (1, 2)
    assert P(1, True)["plan"] == "chained" and (P(1, True)["rounds"], P(1, True)["grid"]) == (1, 1)
    assert (P(131_072, True)["rounds"], P(131_072, True)["grid"]) == (1, 512)
    assert (P(131_073, True)["rounds"], P(131_073, True)["grid"]) == (2, 257)
    assert (P(262_145, True)["rounds"], P(524_289, True)["rounds"], P(1_966_081, True)["rounds"]) == (3, 5, 16)
    assert (P(2_097_152, True)["rounds"], P(2_097_152, True)["grid"]) == (16, 512)
    assert P(2_097_153, True)["plan"] == "three_launch" and P(2_097_153, True)["fits"] is False and P(2_097_153, True)["scan_iterations"] == 9
    assert P(1024, True)["canonical"] == "fused" and P(1025, True)["canonical"] == "three_launch" and P(1025, True)["scan_width"] == 64


def test_capacity_lists_reach_every_plan_and_parameter_edge():
    node = [op.launch_plan(c, False) for c in op.NODE_CAPACITIES]
    one = [op.launch_plan(c, True) for c in op.ONE_CALL_CAPACITIES]
    assert {p["plan"] for p in node} == {"fused", "three_launch"}
    assert {p["plan"] for p in one} == {"chained", "three_launch"}
    assert {p["scan_width"] for p in node if p["plan"] == "three_launch"} == {64, 1024}
    assert {p["scan_iterations"] for p in node if p["plan"] == "three_launch"} == {1, 2}
    assert {p["rounds"] for p in one if p["plan"] == "chained"} == {1, 2, 3, 5, 16}
    assert sum(p["grid"] == op.CHAINED_OBJECT_PASS_MAX_BLOCKS for p in one if p["plan"] == "chained") >= 2  # rounds 1 and rounds 16
    assert any(p["fits"] is False for p in one), "the in-frame fallback above MAX_BLOCKS x MAX_ROUNDS x 256 slots"
    # both sides of every switch, and capacities that are no power of two, no multiple of a wave or of a block
    for lst in (op.NODE_CAPACITIES, op.ONE_CALL_CAPACITIES):
        assert {1024, 1025} <= set(lst) and any(c % 64 for c in lst) and any(c % 256 and c > 256 for c in lst)
    assert {16_384, 16_385, 262_144, 262_145} <= set(op.NODE_CAPACITIES)
    assert {131_072, 131_073, 2_097_152, 2_097_153} <= set(op.ONE_CALL_CAPACITIES)
    for c in op.BOUNDARY_CAPACITIES:  # each is the first capacity of another plan on one of the paths
        assert any(op.launch_plan(c, oc) != op.launch_plan(c - 1, oc) and
                   {k: v for k, v in op.launch_plan(c, oc).items() if k != "grid"} != {k: v for k, v in op.launch_plan(c - 1, oc).items() if k != "grid"}
                   for oc in (False, True)), c


# ------------------------------------------------------------------ the exact tier
def exact_world():
    w = op.build_world(2048, "exact", "tier")
    names = [n for n, _s in op.exact_specials()]
    free = np.arange(2048)
    at = free[(np.arange(len(names)) * 7 + 3) % len(free)]
    w["enabled"][at] = True
    w["ntri"][at] = 1
    return w, dict(zip(names, at))


@pytest.mark.parametrize("frame", [0, 1])
def test_flags_exact_equal_the_oracle_on_the_exact_tier(frame):
    """Every special row is kept: flags_exact and r3o_frustum_cull agree on NaN and on +-inf centres and radii."""
    w, at = exact_world()
    recs = op.records(w, op.NoMesh)
    view, proj = op.cameras("exact", oh)[frame]
    hdr = op.oracle_header(view, proj, len(recs))
    assert np.array_equal(hdr[36:56].view(np.uint32), op.EXACT_PLANES[frame].view(np.uint32)), "the planes are exactly representable"
    meta = op.meta_words(recs, op.MATERIAL_KEYS)
    got = op.flags_exact(hdr[36:56], recs.view(f32)[:, 16:20], meta, np.ones(len(recs), dtype=bool))
    want = op.oracle_inside(hdr, recs)
    assert np.array_equal((got & op.VIS_INSIDE) != 0, want), np.flatnonzero(((got & op.VIS_INSIDE) != 0) != want)
    assert np.array_equal((got & op.VIS_DRAWN) != 0, want)
    assert 0.2 < want.mean() < 0.8
    if frame == 0:
        inside = {n: bool(want[k]) for n, k in at.items()}
        for side in ("left", "right", "top", "bottom", "near"):
            assert inside[f"tie_{side}"] and not inside[f"ulp_outside_{side}"], side
        assert inside["radius0_inside"] and inside["radius0_on_plane"] and inside["radius0_corner"] and not inside["radius0_outside"]
        assert inside["huge_radius"] and inside["inf_radius"] and inside["inf_radius_far"] and inside["neg_zero"] and inside["no_far_plane"]
        for n in ("far_corner", "negative_radius", "nan_centre", "nan_radius", "inf_centre", "neg_inf_centre", "neg_inf_radius", "inf_both"):
            assert not inside[n], n


def test_exact_tier_arithmetic_is_exact_in_any_order():
    """centres on the 1/8 grid with |c| <= 1024, dyadic radii, plane normals of 0 and +-1, plane distances 1, 2, 4: every
    product is the operand or zero, every sum has at most 14 + 3 significant bits"""
    w, _at = exact_world()
    s = w["spheres"][np.isfinite(w["spheres"]).all(axis=1)].astype(np.float64)
    assert np.array_equal(s[:, :3] * 8, np.round(s[:, :3] * 8)) and np.abs(s[:, :3]).max() <= 1024
    m, _e = np.frexp(np.abs(s[:, 3]))
    assert np.isin(m, (0.0, 0.5)).all() or np.array_equal(s[:, 3], s[:, 3].astype(f32)), "dyadic, or one ulp below"
    for planes in op.EXACT_PLANES:
        p = planes.reshape(5, 4)
        assert np.isin(p[:, :3], (-1.0, 0.0, 1.0)).all() and np.isin(p[:, 3], (1.0, 2.0, 4.0)).all()
        d = s[:, :3] @ p[:, :3].T.astype(np.float64) + p[:, 3]
        assert np.array_equal(d.astype(f32).astype(np.float64), d)


def test_flags_follow_ownership_only_in_the_drawn_bit():
    w = op.build_world(1025, "exact", "tier", blend=True)
    recs = op.records(w, op.NoMesh, op.NoMesh)
    meta = op.meta_words(recs, op.MATERIAL_KEYS)
    owned = np.arange(1025) % 3 == 1
    all_, mine = (op.flags_exact(op.EXACT_PLANES[0], w["spheres"], meta, o) for o in (np.ones(1025, dtype=bool), owned))
    assert np.array_equal(all_ & op.VIS_INSIDE, mine & op.VIS_INSIDE)
    blend = (meta >> 30) == op.BLEND
    inside = (all_ & op.VIS_INSIDE) != 0
    assert np.array_equal((mine & op.VIS_DRAWN) != 0, inside & (owned | blend))
    assert (inside & blend & ~owned).any() and (inside & ~blend & ~owned).any()


# ------------------------------------------------------------------ the conditions of the two tiers
@pytest.mark.parametrize("tier", op.TIERS)
def test_palette_triangles_pass_whatever_else_is_drawn(tier):
    """>= 90 % of the palette's triangles pass in both frames (a missing list entry then shows as missing pass bits), and the
    verdict against the pyramid of the WHOLE palette equals the verdict against an all-zero pyramid (object_pass_reference.verdicts)."""
    full, zero = op.verdicts(tier), op.verdicts(tier, zero_plane=True)
    for f in range(3):  # cameras 0, 1, 0: the last two frames with history
        assert full[f].mean() >= 0.9, (tier, f, full[f].mean())
        assert np.array_equal(full[f], zero[f]), (tier, f)
    assert np.array_equal(full[0], full[2]), "a camera's verdict is the same with and without history"
    shadow = op.verdicts(tier, light=True)
    assert np.array_equal(shadow[0], shadow[2]) and (tier != "exact" or shadow[0].mean() >= 0.9)
    print(tier, "shadow view verdicts", [float(v.mean()) for v in shadow])


@pytest.mark.parametrize("capacity", [257, 1025, 16_385, 131_073])
def test_random_tier_draws_30_to_70_percent(capacity):
    w = op.build_world(capacity, "random", "tier", big_ntri_every=op.big_ntri_every(capacity))
    recs = op.records(w, op.NoMesh)
    for view, proj in op.cameras("random", oh):
        inside = op.oracle_inside(op.oracle_header(view, proj, capacity), recs)
        share = inside.sum() / w["enabled"].sum()
        assert 0.30 <= share <= 0.70, share
    a, b = (op.oracle_inside(op.oracle_header(v, p, capacity), recs) for v, p in op.cameras("random", oh))
    assert (a & ~b).any() and (b & ~a).any(), "frame 1's use_prev set differs from its own inside set"


@pytest.mark.parametrize("capacity", [1, 63, 257, 1025, 131_073])
def test_worlds_hold_what_the_patterns_promise(capacity):
    w = op.build_world(capacity, "exact", "mix", big_ntri_every=op.big_ntri_every(capacity))
    recs = op.records(w, op.NoMesh)
    meta = op.meta_words(recs, op.MATERIAL_KEYS)
    drawn = (op.flags_exact(op.EXACT_PLANES[0], w["spheres"], meta, np.ones(capacity, dtype=bool)) & op.VIS_DRAWN) != 0
    ntri = meta & op.META_NTRI_MASK
    assert drawn[0] and drawn[-1] and ntri[0] > 2048
    if capacity > 256:
        waves = drawn[: capacity // 64 * 64].reshape(-1, 64)
        assert waves.all(axis=1).any() and (~waves).all(axis=1).any()
        assert drawn[256:512].all() and ntri[-1] > 2048
        assert drawn[128:192].all() and (ntri[128:192] > 2048).sum() >= 3, "three wavefront-wide objects in one drawn wave"
    if capacity > 1024:
        assert not drawn[768:1024].any()
        assert set(op.NTRI_VALUES) <= set(ntri[drawn].tolist())
        assert {0, 1} <= set((meta[drawn] >> 30).tolist())
    for pattern, count in (("all", capacity), ("none", 0), ("first", 1), ("last", 1)):
        w = op.build_world(capacity, "random", pattern)
        recs = op.records(w, op.NoMesh)
        inside = op.oracle_inside(op.oracle_header(*op.cameras("random", oh)[0], capacity), recs)
        assert inside.sum() == count and (count != 1 or inside[0 if pattern == "first" else -1]), pattern


# ------------------------------------------------------------------ expected() against whole oracle frames
@pytest.mark.parametrize("pattern", ["tier", "mix"])
@pytest.mark.parametrize("tier", op.TIERS)
def test_expected_equals_an_oracle_frame(tier, pattern):
    """A 300-slot world (no power of two), two frames with history, opaque + cutout + blend: tri_base, pass set, residual set and
    the per-key call counts of expected() are the oracle's."""
    o = OracleRenderer(oh.LEFT, f32(1.0))
    meshes = op.setup_renderer(o, omk)
    w = op.build_world(300, tier, pattern, blend=True, big_ntri_every=8)
    recs = op.load_oracle(o, w, meshes)
    meta = op.meta_words(recs, op.MATERIAL_KEYS)
    prev = None
    for f, (view, proj) in enumerate(op.cameras(tier, oh)):
        o.set_camera_data(view, proj)
        fo = o.render(op.TARGET, op.TARGET)
        hdr = op.oracle_header(view, proj, 300)
        assert np.array_equal(hdr.view(np.uint32), fo["header"].view(np.uint32))
        if tier == "exact":
            flags = op.flags_exact(hdr[36:56], recs.view(f32)[:, 16:20], meta, np.ones(300, dtype=bool))
        else:
            flags = op.flags_from_inside(op.oracle_inside(hdr, recs), meta, np.ones(300, dtype=bool))
        e = op.expected(meta, flags, op.verdicts(tier)[f][w["pal"]], prev)
        assert np.array_equal((flags & op.VIS_DRAWN), fo["visible"])
        assert np.array_equal(e["tri_base"], fo["tri_base"]) and e["total"] == len(fo["pass"])
        assert np.array_equal(e["pass"], fo["pass"]), f"frame {f}"
        assert np.array_equal(e["residual"], fo["residual"]), f"frame {f}"
        tri_obj = np.searchsorted(fo["tri_base"], np.arange(e["total"]), side="right") - 1
        keys = fo["material_keys"][fo["objects"][tri_obj, 22]]
        for k in range(3):
            assert e["calls"][k] == 3 * int((fo["pass"].astype(bool) & (keys == k)).sum())
            assert e["calls"][3 + k] == 3 * int((fo["residual"].astype(bool) & (keys == k)).sum())
        assert e["calls"][:3].min() > 0
        assert fo["pass"].sum() > 0.3 * (flags & op.VIS_DRAWN != 0).sum()
        prev = e
    if pattern == "tier":  # (300 slots of "mix" are forced ones: the same set in both frames)
        assert 0 < e["residual"].sum() < e["pass"].sum(), "frame 1 has history: some passing triangles are not residual"
