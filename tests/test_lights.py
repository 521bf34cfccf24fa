"""The conditions tests/test_lights_gpu.py rests on, on the oracle alone (no GPU): every light set of tests/light_worlds.py
really reaches the path it is named for.  A GPU pass over a set that never met the edge would be worthless, so each condition
is an assertion with a stated cap; the stage's geometry and the shadow distances were chosen until the oracle met them."""
import functools

import numpy as np
import pytest

import light_worlds as lw
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk

f32 = np.float32
HALF_INF = 0x7C00


def stage(dirs, points, **options):
    o = OracleRenderer(oh.LEFT, lw.aspect())
    handles = lw.build_stage(o, oh, omk, **options)
    lw.set_camera(o, oh)
    lw.apply_lights(o, dirs, points)
    return o, handles


def frame(o):
    return o.render(lw.W, lw.H, ambient=lw.AMBIENT, clear_color=lw.CLEAR)


def rendered(dirs, points, **options):
    o, handles = stage(dirs, points, **options)
    return frame(o), handles


def changed(fa, fb):
    """per pixel: the HDR of two frames differs (bits)"""
    return (fa["hdr16"] != fb["hdr16"]).any(axis=2)


def test_no_set_puts_a_nan_into_the_hdr_target():
    """f16 NaN payloads are no part of the contract: the final max(ambient * albedo, colour) drops NaN, infinities stay"""
    sets = [lw.zero_paths(w, v) for w in (lw.ZERO_BELOW, lw.ZERO_OCCLUDED) for v in lw.ZERO_COLOURS]
    for dirs, points in sets:
        fo, _ = rendered(dirs, points, **lw.ZERO_STAGE)
        h = fo["hdr16"].view(np.float16)
        assert not np.isnan(h).any()


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("n_dir,n_point", [p for p in lw.COUNT_PAIRS if p != (0, 0)])
def test_counts_the_last_light_of_each_list_matters(n_dir, n_point):
    """index n - 1 of either list is read and changes the frame"""
    dirs, points = lw.counts(n_dir, n_point)
    assert len({d["color"] for d in dirs}) == len(dirs) and len({(p["color"], p["position"]) for p in points}) == len(points)
    full, _ = rendered(dirs, points)
    geo = lw.geometry_mask(full)
    assert geo.mean() > 0.4
    if n_dir:
        less, _ = rendered(dirs[:-1], points)
        n = int((changed(full, less) & geo).sum())
        print(f"counts({n_dir}, {n_point}): without the last directional light {n} px change")
        assert n >= 0.05 * geo.sum()
        if n_dir >= 4:  # the quadtree: maps of more than one size, more than one root or level
            assert len({s["size"] for s in full["shadow_descs"]}) == 3
    if n_point:
        less, _ = rendered(dirs, points[:-1])
        n = int((changed(full, less) & geo).sum())
        print(f"counts({n_dir}, {n_point}): without the last point light {n} px change")
        assert n >= 20


# ------------------------------------------------------------------ zero_paths
@functools.lru_cache(maxsize=None)
def zero_frame(which, value_bits):
    dirs, points = lw.zero_paths(which, np.array([value_bits], dtype=np.uint32).view(f32)[0])
    return rendered(dirs, points, **lw.ZERO_STAGE)


def bits(v):
    return int(np.array([v], dtype=f32).view(np.uint32)[0])


@pytest.mark.parametrize("which", [lw.ZERO_BELOW, lw.ZERO_OCCLUDED], ids=["from_below", "occluded"])
def test_zero_paths_zero_term_and_live_term_both_occur(which):
    """colour 3.0 -> 6.0 on the one light: the HDR stays identical on >= 20 % of the geometry pixels (the light adds its zero
    term there) and changes on >= 20 % (it is live there)"""
    f3, _ = zero_frame(which, bits(3.0))
    f6, _ = zero_frame(which, bits(6.0))
    geo = lw.geometry_mask(f3)
    ch = changed(f3, f6) & geo
    share = ch.sum() / geo.sum()
    print(f"light {which}: {100 * share:.1f} % of {geo.sum()} geometry pixels change with the colour")
    assert 0.20 <= share <= 0.80


def test_zero_paths_roughness_zero_poisons_the_pixel_where_nl_is_zero():
    """D * V = 0 * inf on the roughness-0 sphere where a light has nl == 0: the colour is NaN, the final max() leaves
    ambient * albedo -- what the `roughness` guard of the kernel's nl == 0 shortcut exists for"""
    fo, handles = zero_frame(lw.ZERO_BELOW, bits(3.0))
    m = lw.object_mask(fo, handles["rough0"])
    assert m.sum() > 100
    want = (np.array(lw.AMBIENT[:3], dtype=f32) * np.array((0.4, 0.7, 0.9), dtype=f32)).astype(np.float16).view(np.uint16)
    hit = (fo["hdr16"][m][:, :3] == want).all(axis=1)
    print(f"roughness-0 sphere: {hit.sum()} of {m.sum()} px are f16(ambient * albedo)")
    assert hit.sum() >= 0.5 * m.sum()
    # ... and nowhere else is that the rule: the other spheres' pixels are lit
    other = lw.object_mask(fo, handles["rough05"])
    want = (np.array(lw.AMBIENT[:3], dtype=f32) * np.array((0.9, 0.5, 0.3), dtype=f32)).astype(np.float16).view(np.uint16)
    assert (fo["hdr16"][other][:, :3] == want).all(axis=1).mean() < 0.5


@pytest.mark.parametrize("which", [lw.ZERO_BELOW, lw.ZERO_OCCLUDED], ids=["from_below", "occluded"])
def test_zero_paths_infinite_colour_overflows_some_pixels_only(which):
    fo, handles = zero_frame(which, bits(np.inf))
    geo = lw.geometry_mask(fo) & ~lw.object_mask(fo, handles["huge"])
    rgb = fo["hdr16"][geo][:, :3]
    inf_px = (rgb == HALF_INF).any(axis=1)
    print(f"light {which} at +inf: {inf_px.sum()} of {geo.sum()} px hold 0x7C00")
    assert inf_px.sum() >= 50 and (~inf_px).sum() >= 50
    assert np.isfinite(rgb[~inf_px].view(np.float16)).all()


def test_zero_paths_every_colour_value_changes_the_frame():
    """the seven values give different frames on either light -- but 1e6 and its successor, one f32 rounding apart on the oracle
    and the same after the rounding to f16 (on the kernel they are the two sides of the `sane` bound), and -inf and NaN, which
    both poison what the light reaches"""
    for which in (lw.ZERO_BELOW, lw.ZERO_OCCLUDED):
        frames = [zero_frame(which, bits(v))[0] for v in lw.ZERO_COLOURS]
        for a in range(len(frames)):
            for b in range(a + 1, len(frames)):
                if {a, b} in ({1, 2}, {4, 5}):
                    continue
                assert changed(frames[a], frames[b]).any(), (which, lw.ZERO_COLOUR_IDS[a], lw.ZERO_COLOUR_IDS[b])


def test_zero_paths_the_huge_albedo_passes_the_magnitude_bound():
    """the kernel may skip a zero term only while the sum of the magnitudes of the pixel inputs is below 1e30"""
    fo, handles = zero_frame(lw.ZERO_OCCLUDED, bits(3.0))
    m = lw.object_mask(fo, handles["huge"])
    assert m.sum() > 50 and lw.HUGE_ALBEDO > 1e30
    assert (fo["hdr16"][m][:, :3] == HALF_INF).all()  # ambient * albedo alone overflows f16: +inf, not NaN


def _half(rgb):
    return np.array(rgb, dtype=f32).astype(np.float16).view(np.uint16)


def test_zero_paths_the_mirror_overflows_under_a_colour_the_kernel_calls_harmless():
    """On the mirror quad (ao = 0: every light term is x * 0; f0 = 3.1e29; roughness 0.1) the from-below light's (fd + fr) * colour
    overflows f32 in the highlight for a colour of 1e6 already -- the largest the kernel's bound on the light colour lets pass --
    and for none at 3.0.  The term is then inf * 0 = NaN: a kernel that skips zero terms must not skip this one, so the bound on
    the colour alone is not enough, f0 has to be bounded too.  A poisoned pixel shows ambient * albedo, a clean one the emission."""
    ambient = np.array(lw.AMBIENT[:3], dtype=f32) * np.array(lw.MIRROR_ALBEDO, dtype=f32)
    counts = {}
    for c in (3.0, 1e6, 1e7):
        fo, handles = zero_frame(lw.ZERO_BELOW, bits(c))
        m = lw.object_mask(fo, handles["mirror"])
        px = fo["hdr16"][m][:, :3]
        poisoned, clean = (px == _half(ambient)).all(axis=1), (px == _half((2.0, 1.5, 1.0))).all(axis=1)
        assert m.sum() >= 200 and (poisoned | clean).all()
        counts[c] = int(poisoned.sum())
    print(f"mirror: poisoned pixels by light colour {counts}")
    assert counts[3.0] == 0 and counts[1e6] >= 3 and counts[1e7] >= counts[1e6]


def test_zero_paths_the_ao_zero_sphere_tells_a_zero_term_from_a_poisoned_one():
    """ao = 0: a finite colour leaves the emission, an infinite one (inf * 0) ambient * albedo"""
    ambient = np.array(lw.AMBIENT[:3], dtype=f32) * np.array((0.5, 0.9, 0.5), dtype=f32)
    for which in (lw.ZERO_BELOW, lw.ZERO_OCCLUDED):
        fo, handles = zero_frame(which, bits(3.0))
        m = lw.object_mask(fo, handles["ao0"])
        assert m.sum() >= 80 and (fo["hdr16"][m][:, :3] == _half((0.3, 0.2, 0.1))).all()
        fo, _ = zero_frame(which, bits(np.inf))
        assert (fo["hdr16"][m][:, :3] == _half(ambient)).all()


def test_zero_paths_parallel_direction_gives_nan_shadow_matrices():
    fo, _ = zero_frame(lw.ZERO_BELOW, bits(3.0))
    k = [s["handle"] for s in fo["shadow_descs"]].index(3)
    assert np.isnan(fo["shadow_descs"][k]["camera"].view_proj).any()


# ------------------------------------------------------------------ frustum_edges
@pytest.mark.parametrize("n_lights", [1, 2, 3])
def test_frustum_edges_cut_the_visible_stage(n_lights):
    near, _ = rendered(*lw.frustum_edges(n_lights))
    far, _ = rendered(*lw.frustum_edges(n_lights, distance=60.0))
    geo = lw.geometry_mask(near)
    share = (changed(near, far) & geo).sum() / geo.sum()
    print(f"frustum_edges({n_lights}): {100 * share:.1f} % of the geometry pixels differ from distance = 60")
    assert share >= 0.10
    total = len(near["pass"])
    for k, sh in enumerate(near["shadows"]):
        n = int(sh["pass"].sum())
        print(f"  shadow view {k}: {n} of {total} triangles pass")
        assert 0 < n < total


def test_frustum_edges_lookups_leave_the_map_every_way():
    """the bounds test recomputed in float64 for every geometry pixel (light_worlds.shadow_lookup_census): lookups leave their
    light's map in x only, in y only and in both; some land in a neighbour's map, some leave the atlas (Repeat addressing: the
    general form of the PCF lookup); part of the stage is outside [0, 1] in depth"""
    o, _ = stage(*lw.frustum_edges(3))
    fo = frame(o)
    assert fo["atlas_size"] == (128, 64) and [s["size"] for s in fo["shadow_descs"]] == [64, 32, 32]
    census = lw.shadow_lookup_census(fo, o.camera)
    for k, c in enumerate(census):
        print(f"frustum_edges(3) light {k}: {c}")
    assert census[0]["out_y_only"] >= 100 and census[0]["wrapped"] >= 100
    assert census[1]["out_x_only"] >= 100 and census[1]["wrapped"] == 0   # at offset (64, 0): x beyond its map is a neighbour's map
    c = census[2]
    assert min(c["out_x_only"], c["out_y_only"], c["out_both"]) >= 50 and c["wrapped"] >= 100 and c["depth_out"] >= 100
    assert c["looked_up"] >= 1000
    # at distance 60 nothing of the kind happens: that is every other scene of the suite
    o, _ = stage(*lw.frustum_edges(3, distance=60.0))
    for c in lw.shadow_lookup_census(frame(o), o.camera):
        assert c["out_x_only"] == c["out_y_only"] == c["out_both"] == c["wrapped"] == c["depth_out"] == 0


# ------------------------------------------------------------------ in_flight
def test_in_flight_every_step_changes_the_frame_but_the_idle_one():
    o, _ = stage(*lw.in_flight_start())
    prev = frame(o)
    for f in range(lw.IN_FLIGHT_FRAMES):
        lw.in_flight_step(o, f)
        cur = frame(o)
        n = int(changed(prev, cur).sum())
        print(f"in_flight frame {f}: {n} px differ from the frame before")
        if f == 4:
            assert n == 0  # nothing changed: the lights are not uploaded again
        else:
            assert n >= 20
        prev = cur
    assert len(o.dir_lights) == 3 and len(o.point_lights) == 4


# ------------------------------------------------------------------ options
def test_stage_options_reach_their_paths():
    plain, _ = rendered(*lw.counts(2, 3))
    tex, _ = rendered(*lw.counts(2, 3), textured=True)
    assert changed(plain, tex).sum() > 500
    bl, handles = rendered(*lw.counts(2, 3), blend=True)
    assert len(bl["blend_list"][0]) == 4 and changed(plain, bl).sum() > 200
    cut, _ = rendered(*lw.counts(2, 3), cutout=True)
    assert int(cut["material_keys"][1]) == lw.CUTOUT
