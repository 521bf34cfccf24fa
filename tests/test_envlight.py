"""CPU-only: environment lights (DESIGN.md section 2 "Environment lights", include/r3n.h r3n_environment_lights).  The rule header
the kernels share with the host (rend3_amd/csrc/envlight_rule.h) is compiled into a stand-alone program under the address and
undefined-behaviour sanitizers, runs the whole extraction serially and must print the words of the numpy restatement
(tests/envlight_reference.py); the restatement is held to independent float64 evaluations and to the properties the rule is there
for; the ABI is present in every layer; the Python layer and the viewer refuse what they must.  The GPU side is
tests/test_envlight_gpu.py."""
import argparse
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import envlight_reference as E
import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "envlight_rule_check.cpp")
CSRC = os.path.join(ROOT, "rend3_amd", "csrc")
RULES = [os.path.join(CSRC, h) for h in ("envlight_rule.h", "equirect_rule.h", "exposure_rule.h")]
f32 = np.float32
CONE6 = f32(math.cos(math.radians(6.0)))


def program():
    return host_check.program(SRC, RULES, fp_contract_off=True)


def run(cmd, text=""):
    res = subprocess.run([program(), cmd], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]  # a sanitizer report goes to stderr
    return res.stdout.split("\n")[:-1]


def header_extract(rgb, max_lights, cone_cos, min_share):
    n = rgb.shape[1]
    body = "\n".join(" ".join(map(str, row)) for row in E.bits(rgb).reshape(-1, 3).tolist())
    return [int(v) for v in run("extract", f"{n} {max_lights} {E.word(cone_cos)} {E.word(min_share)}\n{body}\n")]


_SKIES = {}


def sky_case(n):
    """the issue's synthetic sky at extent n, extracted once: (rgb, state)"""
    if n not in _SKIES:
        rgb = E.sky(n)
        _SKIES[n] = (rgb, E.extract(rgb, 4, CONE6, 0.02))
    return _SKIES[n]


def nasty_world(n, seed, huge=True):
    """random radiance over 12 octaves with every kind of texel the rule must survive.  huge: one channel of 1e30, which puts every
    ordinary texel below the 2^-40 quantisation floor -- the search then ends behind the first light, with nothing left to take"""
    rng = np.random.default_rng(seed)
    rgb = (np.exp2(rng.uniform(-6, 6, (6, n, n, 1))) * rng.uniform(0.05, 1.0, (6, n, n, 3))).astype(f32)
    flat = rgb.reshape(-1, 3)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 1e-45, 1e-39, 1e30 if huge else 100.0, 0.0, -0.0)):
        flat[(k * 7 + 3) % len(flat), k % 3] = v
    return rgb


# ------------------------------------------------------------------ 1. the rule header against the restatement, word for word
def test_rule_header_geometry():
    extents = [1, 2, 3, 5, 33]
    got = run("geometry", "\n".join(map(str, extents)) + "\n")
    at = 0
    for n in extents:
        u, w = E.geometry(n)
        g = np.array([[int(v) for v in ln.split()] for ln in got[at:at + 6 * n * n]], dtype=np.int64)
        at += 6 * n * n
        assert np.array_equal(g[:, :3].astype(np.uint32), E.bits(u).reshape(-1, 3)), n
        assert np.array_equal(g[:, 3].astype(np.uint32), E.bits(w).reshape(-1)), n
        assert np.array_equal(g[:, 4:7], E.dir_q(u).reshape(-1, 3)), n
        assert np.array_equal(g[:, 7].astype(np.uint64), E.quantise_w(w).reshape(-1)), n
        assert np.abs(E.dir_q(u)).max() <= 32767
    assert at == len(got)
    # an odd extent has a texel exactly on each axis; the grid is exactly antisymmetric
    u, w = E.geometry(33)
    assert np.array_equal(u[0, 16, 16], [1, 0, 0]) and np.array_equal(u[3, 16, 16], [0, -1, 0]) and w[0, 16, 16] == f32(4) / f32(33 * 33)
    assert np.array_equal(u[4, :, ::-1, 0], -u[4, :, :, 0]) and np.array_equal(w[2], w[2][::-1, ::-1])


@pytest.mark.parametrize("n", [32, 64, 256])
def test_rule_header_extracts_the_synthetic_sky(n):
    rgb, st = sky_case(n)
    assert header_extract(rgb, 4, CONE6, 0.02) == E.flat(st)


@pytest.mark.parametrize("huge", [False, True])
@pytest.mark.parametrize("case", [(1, 16, 0.5, 0.0), (2, 16, 0.99, 0.0), (3, 16, 0.5, 0.0), (5, 16, 0.9, 0.0), (5, 0, 0.9, 0.0), (5, 1, 0.9, 0.5), (9, 16, 0.98, 0.0),
                                  (9, 16, 0.98, 0.05), (17, 16, 0.5, 0.0), (33, 7, 0.995, 0.001)])
def test_rule_header_extracts_worlds_with_corrupt_texels(case, huge):
    n, max_lights, cone_cos, min_share = case
    rgb = nasty_world(n, n * 100 + max_lights, huge)
    st = E.extract(rgb, max_lights, f32(cone_cos), f32(min_share))
    assert header_extract(rgb, max_lights, f32(cone_cos), f32(min_share)) == E.flat(st)
    assert st["n_lights"] <= max_lights and all(np.isfinite(st["ambient"]))
    for l in st["lights"]:
        assert np.all(np.isfinite(l["direction"])) and np.all(np.isfinite(l["irradiance"])) and math.isfinite(float(l["solid_angle"]))
    if huge and max_lights:
        assert st["n_lights"] == 1 and st["remainder"]["qy"] == 0, "nothing else reaches the quantisation floor"
    elif min_share == 0.0 and max_lights == 16 and n >= 9 and cone_cos > 0.9:
        assert st["n_lights"] == 16, "sixteen narrow cones do not exhaust this level"


def test_rule_header_black_and_corrupt_only_levels():
    for fill in (0.0, -3.0, np.nan, np.inf):
        rgb = np.full((6, 3, 3, 3), fill, dtype=f32)
        st = E.extract(rgb, 4, f32(0.9), f32(0.0))
        assert header_extract(rgb, 4, f32(0.9), f32(0.0)) == E.flat(st)
        assert st["n_lights"] == 0 and st["ran"] == 0 and st["scale_exp"] == 0 and [float(a) for a in st["ambient"]] == [0.0, 0.0, 0.0, 1.0]
    # the smallest energy there is: one subnormal channel
    rgb = np.zeros((6, 2, 2, 3), dtype=f32)
    rgb[3, 1, 0, 1] = 1e-44
    st = E.extract(rgb, 2, f32(0.9), f32(0.0))
    assert header_extract(rgb, 2, f32(0.9), f32(0.0)) == E.flat(st)
    assert st["emax_bits"] != 0 and st["n_lights"] == 1 and st["lights"][0]["seed"] == (3 * 2 + 1) * 2 + 0


# ------------------------------------------------------------------ 2. the pieces of the rule against exact arithmetic
def test_quantisation_is_the_floor_of_the_exact_product():
    rng = np.random.default_rng(11)
    e = np.concatenate([np.exp2(rng.uniform(-140, 60, 4000)).astype(f32), np.array([1e-45, 1.1754944e-38, 1.1754942e-38, 3.0, 0.0], dtype=f32)])
    for emax in (e.max(), f32(7.5), f32(1e-40)):
        sel = e[e <= emax]
        eb, mb = E.bits(sel), int(E.bits(emax).reshape(-1)[0])
        q = E.quantise(eb, mb)
        s = E.scale_exp_of(mb)
        for x, got in zip(sel.tolist()[::37], q.tolist()[::37]):
            assert got == math.floor(Fraction(x) * Fraction(2) ** s), (x, float(emax))
        assert int(q.max()) < 2 ** 40 and int(E.quantise(np.uint32(mb), mb)) >= (2 ** 39 if emax >= 1.1754944e-38 else 1)
    for n in (1, 2, 7, 1024):
        w = E.geometry(n)[1][0]
        qw = E.quantise_w(w)
        assert all(Fraction(int(a)) == Fraction(float(b)) * 2 ** 44 for a, b in zip(qw.reshape(-1)[::max(1, n * n // 50)], w.reshape(-1)[::max(1, n * n // 50)])), \
            "qw is exact for every n <= 1024"


def test_the_overflow_bounds_the_header_states():
    texels = 6 * 1024 * 1024
    qmax = 2 ** 40 - 1
    assert sum(E.WEIGHTS) == 65536 and sum(E.WEIGHTS) * qmax < 2 ** 64
    assert texels * qmax < 2 ** 63
    assert texels * (qmax >> 20) * 32767 < 2 ** 63 and texels * 0xFFFFF * 32767 < 2 ** 63
    assert E.isum(E.quantise_w(E.geometry(1024)[1])) < 2 ** 49 and E.isum(E.quantise_w(E.geometry(1)[1])) == 24 * 2 ** 44
    header = open(RULES[0]).read()
    for claim in ("OVERFLOW", "2^62.6", "2^57.6", "(u128)", "MAX_EXTENT = 1024u"):
        assert claim in header
    # the share test is exact: one unit of energy decides it
    share = E.share_floor(f32(0.25))
    assert share == 2 ** 30 and E.emits(25, 100, share) and not E.emits(24, 100, share) and not E.emits(0, 100, 0) and E.emits(1, 10 ** 18, 0)
    assert E.share_floor(np.nextafter(f32(1), f32(0))) == 2 ** 32 - 256


# ------------------------------------------------------------------ 3. float64 evaluations that do not use the rule's code
def exact_solid_angles(n):
    """the solid angle of every texel of a face from the corner formula A(x, y) = atan2(x y, sqrt(x^2 + y^2 + 1)), float64"""
    edges = (2.0 * np.arange(n + 1) - n) / n
    x, y = np.meshgrid(edges, edges)
    a = np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))
    return a[1:, 1:] - a[1:, :-1] - a[:-1, 1:] + a[:-1, :-1]


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 16, 33, 64, 256, 1024])
def test_solid_angles_sum_to_the_sphere(n):
    w = E.geometry(n)[1]
    ratio = float(np.sum(w.astype(np.float64))) / (4 * math.pi)
    assert abs(ratio - 1) <= 0.3 / n ** 2, (n, (ratio - 1) * n * n)
    assert abs(6 * exact_solid_angles(n).sum() / (4 * math.pi) - 1) < 1e-12
    quantised = E.isum(E.quantise_w(w)) / 2.0 ** 44
    assert abs(quantised / (4 * math.pi) - 1) <= 0.3 / n ** 2


def axis_of(k):
    a = np.asarray(E.SUNS[k][0], dtype=np.float64)
    return a / np.linalg.norm(a)


@pytest.mark.parametrize("n", [32, 64, 256])
def test_synthetic_sky_gives_its_two_suns(n):
    rgb, st = sky_case(n)
    assert st["n_lights"] == 2 and st["ran"] == 3, "exactly two lights; a third candidate ran and was refused by the share test"
    third = st["light"][2]["qy"]
    assert third > 0 and (third << 32) < E.share_floor(f32(0.02)) * st["total"]["qy"]
    first, second = st["lights"]
    assert first["irradiance"][0] > second["irradiance"][0], "the brighter first"
    w64, rgb64 = E.solid_angles64(n), rgb.astype(np.float64)
    for k, l in enumerate(st["lights"]):
        d = l["direction"].astype(np.float64)
        assert abs(np.linalg.norm(d) - 1) < 1e-6
        off = math.acos(min(1.0, float(d @ axis_of(k))))
        assert off <= 0.5 / n, (n, k, math.degrees(off))
        mask = st["masks"][k]
        for c in range(3):
            want = float(np.sum(rgb64[..., c][mask] * w64[mask]))
            assert abs(float(l["irradiance"][c]) - want) <= 1e-6 * want, (n, k, c)
        assert abs(float(l["solid_angle"]) - float(np.sum(w64[mask]))) <= 1e-6 * float(np.sum(w64[mask]))
        assert l["texels"] == int(mask.sum())
    assert not (st["masks"][0] & st["masks"][1]).any()
    # energy is conserved: the lights and the remainder are the level, integer for integer
    for c in range(3):
        assert st["remainder"]["q"][c] + sum(st["light"][k]["q"][c] for k in range(2)) == st["total"]["q"][c]
    rest = ~(st["masks"][0] | st["masks"][1])
    want = float(np.sum(rgb64[..., 0][rest] * w64[rest])) / (4 * math.pi)
    assert abs(float(st["ambient"][0]) - want) <= 1e-6 * want and float(st["ambient"][3]) == 1.0


def test_sky_without_suns_gives_no_light_and_the_mean():
    n = 16
    rgb = E.sky(n, suns=())
    st = E.extract(rgb, 4, CONE6, 0.02)
    assert st["n_lights"] == 0 and st["ran"] == 1
    exact = np.broadcast_to(exact_solid_angles(n), (6, n, n))
    mean = float(np.sum(rgb[..., 0].astype(np.float64) * exact)) / (4 * math.pi)
    assert abs(mean - 1.0) < 1e-3, "1 + 0.5 u.y averages to 1 over the sphere"
    for c in range(3):
        assert abs(float(st["ambient"][c]) - mean) <= 1e-3
    assert header_extract(rgb, 4, CONE6, 0.02) == E.flat(st)


def test_equal_peaks_break_to_the_lower_index_and_a_wide_cone_kills_its_texels():
    n = 9
    rgb = np.full((6, n, n, 3), 0.01, dtype=f32)
    rgb[4, 4, 4] = 50.0  # +Z centre, linear index (4 * 9 + 4) * 9 + 4
    rgb[1, 4, 4] = 50.0  # -X centre: the lower index
    st = E.extract(rgb, 16, f32(0.5), f32(0.0))
    assert [l["seed"] for l in st["lights"][:2]] == [(1 * 9 + 4) * 9 + 4, (4 * 9 + 4) * 9 + 4]
    assert np.array_equal(st["lights"][0]["direction"], [-1, 0, 0]), "a symmetric neighbourhood leaves the centre on the axis"
    second = st["lights"][1]["direction"]  # (its neighbourhood lost the texels the first cone took: it leans away from -X)
    assert second[2] > 0.999 and second[0] > 0 and second[1] == 0
    u, _ = E.geometry(n)
    in_first = E.dot3(u, st["lights"][0]["direction"]) >= f32(0.5)
    assert np.array_equal(in_first, st["masks"][0]) and st["lights"][0]["texels"] == int(in_first.sum()) > 6 * n * n // 8
    for k in range(1, st["n_lights"]):
        assert not (st["masks"][k] & in_first).any(), "later lights skip dead texels"
        assert not in_first.reshape(-1)[st["lights"][k]["seed"]]
    assert sum(l["texels"] for l in st["lights"]) + st["remainder"]["texels"] == 6 * n * n


# ------------------------------------------------------------------ 4. the ABI is declared everywhere
def test_abi_is_declared_in_every_layer():
    from rend3_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    assert re.search(r"int r3n_environment_lights\(r3n_ctx \*ctx, const r3n_env_lights_params \*params, r3n_env_lights_result \*out\);", hdr)
    assert "#define R3N_ENV_MAX_LIGHTS 16u" in hdr and "rend3-routine/src/skybox.rs only draws the cube" in hdr
    assert _ffi.SIGNATURES["r3n_environment_lights"] == (_ffi.cint, [_ffi.vp, _ffi.vp, _ffi.vp])
    assert [(n, getattr(_ffi.EnvLightsParams, n).offset) for n, _ in _ffi.EnvLightsParams._fields_] == \
        [("cube", 0), ("level", 4), ("max_lights", 8), ("cone_cos", 12), ("min_share", 16)]
    assert ctypes.sizeof(_ffi.EnvLightsParams) == 20 and ctypes.sizeof(_ffi.EnvSums) == 48 and ctypes.sizeof(_ffi.EnvLight) == 192
    assert ctypes.sizeof(_ffi.EnvLightsResult) == 3336 and _ffi.EnvLightsResult.lights.offset == 264 and _ffi.EnvLight.sums.offset == 144
    assert _ffi.ENV_MAX_LIGHTS == E.MAX_LIGHTS == 16
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert "pub fn r3n_environment_lights(ctx: *mut r3n_ctx, params: *const r3n_env_lights_params, out: *mut r3n_env_lights_result) -> c_int;" in rs
    assert "pub struct r3n_env_lights_result {" in rs and "pub lights: [r3n_env_light; 16]," in rs and "pub shift: [[i64; 6]; 2]," in rs
    assert "pub const R3N_ENV_MAX_LIGHTS: u32 = 16;" in rs
    assert set(build.UNITS["envlight.hip"]) >= {"envlight.h", "envlight_rule.h", "equirect_rule.h", "exposure_rule.h"}
    assert {"envlight.h", "envlight_rule.h"} <= set(build.UNITS["r3n.hip"])
    hip = open(os.path.join(CSRC, "r3n.hip")).read()
    assert '{"envlight_plane", &envlight_plane, 0, 1, 1}' in hip and '{"envlight_blocks", &envlight_blocks, 0, R3N_ENVLIGHT_BLOCKS_MAX, 1}' in hip
    rule = open(RULES[0]).read()
    assert f"SHIFT_STEPS = {E.SHIFT_STEPS}u" in rule and f"W_SCALE_EXP = {E.W_SCALE_EXP};" in rule
    assert all(f"WEIGHT_{c} = {w}u" in rule for c, w in zip("RGB", E.WEIGHTS)) and "FOUR_PI = 12.566370614359172;" in rule
    assert E.FOUR_PI == 4 * math.pi
    lib = _ffi.lib()
    assert hasattr(lib, "r3n_environment_lights")
    assert lib.r3n_environment_lights(None, None, None) == -1  # (no context: refused before anything is touched)


# ------------------------------------------------------------------ 5. the Python layer and the viewer
def test_python_layer_refusals_and_viewer_flags():
    from rend3_amd import renderer as R
    from rend3_amd import scene_viewer as V
    assert all(hasattr(R.Renderer, m) for m in ("environment_lights", "add_environment_lights", "environment_mean"))
    assert "environment_lights" in R.Renderer.environment_mean.__doc__

    class Stub:  # the checks in front of the library call need no context
        cubes = [(np.zeros((6, 4, 4, 4), dtype=np.uint8), True)]
        dir_lights = []
        _cube_extent_and_mips = R.Renderer._cube_extent_and_mips

        def _flush_cubes(self):
            pass

    for kw, match in ((dict(cube=1), "no such cube"), (dict(cube=-1), "no such cube"), (dict(cube=0, max_lights=17), "max_lights"),
                      (dict(cube=0, max_lights=-1), "max_lights"), (dict(cube=0, cone_degrees=0.0), "cone_degrees"),
                      (dict(cube=0, cone_degrees=61.0), "cone_degrees"), (dict(cube=0, cone_degrees=float("nan")), "cone_degrees"),
                      (dict(cube=0, min_share=1.0), "min_share"), (dict(cube=0, min_share=-0.1), "min_share"), (dict(cube=0, min_share=float("nan")), "min_share")):
        with pytest.raises(ValueError, match=match):
            R.Renderer.environment_lights(Stub(), **kw)

    class Big(Stub):
        cubes = [R._EquirectCube(0, 8, 4, b"", 4096, 2)]  # levels of extent 4096 and 2048

    with pytest.raises(ValueError, match="no level of extent <= 1024"):
        R.Renderer.environment_lights(Big(), 0)

    class Full(Stub):  # what add_environment_lights asks of a renderer
        dir_lights = [None] * 15

        def environment_lights(self, *a):
            return [dict(direction=np.array([0, 1, 0], dtype=f32), irradiance=np.array([1, 2, 3], dtype=f32))] * 2, np.array([0.5, 0.25, 1, 1], dtype=f32)

    with pytest.raises(ValueError, match="at most 16 directional lights"):
        R.Renderer.add_environment_lights(Full(), 0)

    class Room(Full):
        def __init__(self):
            self.dir_lights = []

        def add_directional_light(self, **kw):
            self.dir_lights.append(kw)
            return len(self.dir_lights) - 1

    r = Room()
    ids, ambient = R.Renderer.add_environment_lights(r, 0, scale=2.0, distance=50.0, resolution=512)
    assert ids == [0, 1] and ambient.tolist() == [1.0, 0.5, 2.0, 1.0]
    assert r.dir_lights[0] == dict(color=(1.0, 2.0, 3.0), intensity=2.0, direction=(-0.0, -1.0, -0.0), distance=50.0, resolution=512)

    flags = ["--skybox", "sky.hdr", "--lights-from-skybox", "3", "--skybox-light-cone", "4.5", "--skybox-light-share", "0.1", "--skybox-light-scale", "0.5"]
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(flags))
    assert (s["lights_from_skybox"], s["skybox_light_cone"], s["skybox_light_share"], s["skybox_light_scale"]) == (3, 4.5, 0.1, 0.5)
    assert s["ambient"] == 0.1 and s["ambient_given"] is False
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(["--ambient", "0.1"]))
    assert s["ambient"] == 0.1 and s["ambient_given"] is True
    d = V.default_settings()
    assert (d["lights_from_skybox"], d["skybox_light_cone"], d["skybox_light_share"], d["skybox_light_scale"], d["ambient_given"]) == (0, 6.0, 0.02, 1.0, False)

    class NoSky:
        handedness = V.RIGHT

    with pytest.raises(ValueError, match="--lights-from-skybox needs a skybox"):
        V.build(NoSky(), None, None, V.default_settings(lights_from_skybox=2))
    with pytest.raises(ValueError, match="1 .. 16"):
        V.build(NoSky(), None, None, V.default_settings(lights_from_skybox=17))
