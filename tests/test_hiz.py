"""The numpy reference of the Hi-Z pyramid (tests/hiz_reference.py) against the oracle, without a GPU, and the conditions the GPU
tests of tests/test_hiz_gpu.py rest on: the extents reach every launch plan r3n_hi_z can choose, and the `distinct` recipe keeps
the comparison from being about zeros.  Every comparison is on u32 words."""
import numpy as np
import pytest

import hiz_reference as hz
from oracle import host as oh
from oracle.lib import get as get_lib
from oracle.world import OracleRenderer

f32 = np.float32


def oracle_pyramid(o, w, h, plane):
    """The oracle's pyramid of an injected plane (None: of what it drew): `plane` replaces the pass-1 depth in place at the
    "pass1_depth" hook, in front of r3o_hiz_build."""
    def hook(what, buf, **_kw):
        if what == "pass1_depth" and plane is not None:
            buf[:] = plane.reshape(-1)
    return o.render(w, h, exchange=hook)["hiz"]


@pytest.fixture(scope="module")
def empty_world():
    o = OracleRenderer(oh.LEFT)
    o.set_camera_data(oh.identity(), ("raw", oh.identity()))
    return o


@pytest.mark.parametrize("recipe", sorted(hz.RECIPES))
@pytest.mark.parametrize("w,h", hz.EXTENTS)
def test_reference_pyramid_equals_the_oracle(empty_world, w, h, recipe):
    plane = hz.RECIPES[recipe](w, h, seed=w * 131 + h)
    assert plane.shape == (h, w) and plane.dtype == f32
    got = oracle_pyramid(empty_world, w, h, plane)
    assert hz.first_difference(hz.pyramid(plane), got, w, h) is None, hz.first_difference(hz.pyramid(plane), got, w, h)


def test_empty_world_without_injection_is_an_all_zero_pyramid(empty_world):
    got = oracle_pyramid(empty_world, 37, 19, None)
    assert got.size == hz.mip_offsets(37, 19)[1] and not got.view(np.uint32).any()
    assert not hz.pyramid(np.zeros((19, 37), dtype=f32)).view(np.uint32).any()


@pytest.mark.parametrize("samples", [1, 4])
def test_resolve_depth_min_equals_the_oracle(samples):
    lib = get_lib()
    rng = np.random.default_rng(samples)
    n = 1000
    depth = rng.uniform(2.0 ** -20, 1.0, size=n * samples).astype(f32)
    u = rng.random(n * samples)
    depth[u < 0.2] = f32(0.0)   # cleared samples
    depth[u >= 0.9] = f32(1.0)  # on the near plane
    keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=n * samples, dtype=np.uint64)
    got = np.full(n, -1.0, dtype=f32)
    lib.r3o_vis_to_depth(lib.ptr(keys), n, samples, lib.ptr(got))
    want = hz.resolve_depth_min(keys, samples)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    if samples == 4:  # the minimum is really over all four: each sample position decides somewhere
        d = depth.reshape(n, 4)
        assert set(np.argmin(d, axis=1).tolist()) == {0, 1, 2, 3}


def test_recipes_hold_only_values_min_is_defined_alike_on():
    tiny = np.finfo(f32).tiny
    for name, make in hz.RECIPES.items():
        for w, h in ((37, 19), (256, 2), (1, 7)):
            p = make(w, h, seed=5)
            assert np.isfinite(p).all() and not np.signbit(p).any(), name
            assert ((p == 0) | (p >= tiny)).all() and (p <= 1).all(), name
    d = hz.distinct(801, 481, seed=3)
    assert len(np.unique(d.view(np.uint32))) == d.size and d.min() > 0 and d.max() == 1
    p = hz.planted(200, 120, seed=3)
    assert 0.15 < (p == 0).mean() < 0.25 and 0.07 < (p == 1).mean() < 0.13
    b = hz.blocks(64, 48, 3, 16, 0.03)
    assert 0 < b.min() and b.max() < 0.03
    # one level per block: within a block the texels differ by the 0.9 .. 1.0 factor only
    assert (b[:16, :16].max() / b[:16, :16].min()) < 1.0 / 0.9 + 1e-3


def test_distinct_pyramids_hold_no_zero_where_the_window_stays_inside():
    """A level whose source has both sides >= 2 never loads past the source, so over a `distinct` plane (all values > 0) it
    holds no 0.0 -- and every one of its texels is a value of the plane, which names the source texel it came from."""
    for w, h in hz.EXTENTS:
        plane = hz.distinct(w, h, seed=w * 131 + h)
        lv = hz.levels(plane)
        values = set(plane.view(np.uint32).reshape(-1).tolist())
        for k in range(1, len(lv)):
            sh, sw = lv[k - 1].shape
            if sw >= 2 and sh >= 2:
                assert (lv[k] > 0).all(), (w, h, k)
                assert set(lv[k].view(np.uint32).reshape(-1).tolist()) <= values, (w, h, k)
            else:
                assert not lv[k].any(), (w, h, k, "a unit side: the three-wide window reads 0.0")


def test_extents_reach_every_launch_plan():
    plans = {e: hz.launch_plan(*e) for e in hz.EXTENTS}
    assert {p["head_levels"] for p in plans.values()} == {0, 1, 2, 3, 4}
    assert {p["head_stop"] for p in plans.values()} == {"cap", "mips", "odd"}
    assert {p["downsample"] for p in plans.values()} == {False, True}
    assert {p["tail_threads"] for p in plans.values()} == {None, 256, 1024}
    placements = {where for p in plans.values() for _k, where in p["tail"]}
    assert placements == {"A", "B", "miss_A", "miss_B"}
    assert any(a[1] == "A" and b[1] == "miss_B" for p in plans.values() for a, b in zip(p["tail"], p["tail"][1:])), \
        "a level kept in A whose successor is too large for B: the successor reads LDS and is written to memory only"
    assert any(a[1] == "miss_A" and b[1] == "miss_B" for p in plans.values() for a, b in zip(p["tail"], p["tail"][1:]))
    # the plan of every extent, derived by hand from r3n_hi_z
    assert plans[(1, 1)] == dict(head_levels=0, head_stop="mips", mip0="keys", downsample=False, tail_threads=None, tail=[])
    assert plans[(2, 2)]["head_stop"] == "mips" and plans[(2, 2)]["head_levels"] == 1 and plans[(2, 2)]["tail_threads"] is None
    assert plans[(16, 16)]["head_levels"] == 4 and plans[(16, 16)]["tail_threads"] is None
    for e in ((1, 7), (5, 1), (37, 19)):
        assert plans[e]["head_levels"] == 0 and plans[e]["head_stop"] == "odd" and plans[e]["tail_threads"] == 256
    assert plans[(256, 2)]["head_levels"] == 1
    assert [plans[e]["head_levels"] for e in ((202, 118), (204, 116), (200, 120))] == [1, 2, 3]
    for e in ((256, 160), (48, 32)):
        assert plans[e]["head_levels"] == 4 and plans[e]["head_stop"] == "cap" and plans[e]["tail_threads"] == 256
    assert plans[(201, 121)]["downsample"] and plans[(201, 121)]["tail_threads"] == 256 and plans[(201, 121)]["head_levels"] == 0
    assert plans[(401, 241)]["downsample"] and plans[(401, 241)]["tail_threads"] == 1024 and plans[(401, 241)]["tail"][0] == (2, "A")
    assert plans[(801, 481)]["tail"][:2] == [(2, "miss_A"), (3, "miss_B")]
    assert plans[(20001, 1)]["tail_threads"] == 1024 and plans[(20001, 1)]["tail"][:2] == [(2, "A"), (3, "miss_B")]
    assert hz.launch_plan(64, 64, 4)["mip0"] == "resolve"
