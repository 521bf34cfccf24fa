"""CPU-only: the environment prefilter (DESIGN.md section 2 "Environment prefilter", include/r3n.h r3n_environment_prefilter).  The
rule header the kernels share with the host (rend3_amd/csrc/ibl_rule.h) is compiled into a stand-alone program under the address
and undefined-behaviour sanitizers, runs `prefilter` and `sh9` serially and must print the words of the numpy restatement
(tests/ibl_reference.py); the restatement is held to float64 evaluations of the same formulas from the same float32 inputs, within
the bound the header derives, and to the properties the rule is there for; the lookups are held to the skybox's bilinear; the ABI
is present in every layer.  The GPU side is tests/test_ibl_gpu.py."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import envlight_reference as E
import host_check
import ibl_reference as I
import skybox_lod_reference as lodref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "ibl_rule_check.cpp")
CSRC = os.path.join(ROOT, "rend3_amd", "csrc")
RULES = [os.path.join(CSRC, h) for h in ("ibl_rule.h", "envlight_rule.h", "equirect_rule.h", "exposure_rule.h")]
f32 = np.float32
EPS = 2.0 ** -24


def program():
    return host_check.program(SRC, RULES, fp_contract_off=True)


def run(cmd, text, tmp_path):
    case = tmp_path / f"{cmd}.txt"
    case.write_text(text)
    res = subprocess.run([program(), cmd, str(case)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]  # a sanitizer report goes to stderr
    return res.stdout.split("\n")[:-1]


def case_text(S, L, levels):
    rows = [f"{S} {L}"]
    for lv in levels:
        rows += [" ".join(map(str, r)) for r in E.bits(lv).reshape(-1, 3).tolist()]
    return "\n".join(rows) + "\n"


# ------------------------------------------------------------------ 1. the rule header against the restatement, word for word
@pytest.mark.parametrize("S,L", [(2, 2), (3, 2), (5, 3), (8, 4), (33, 3)])
def test_rule_header_prefilters_word_for_word(S, L, tmp_path):
    levels = I.nasty(I.random_levels(S, L, seed=S * 10 + L))
    got = run("prefilter", case_text(S, L, levels), tmp_path)
    want = I.prefilter(levels)
    at = 0
    for k in range(L):
        count = want[k].shape[0] * want[k].shape[1] * want[k].shape[2]
        words = np.array([[int(v) for v in ln.split()] for ln in got[at:at + count]], dtype=np.uint32)
        at += count
        assert np.array_equal(words, E.bits(want[k]).reshape(-1, 4)), (S, L, k)
        if k:
            assert not np.isnan(want[k]).any(), "a corrupt texel must not produce a NaN"
    sk = I.sh_level(S, L)
    assert int(got[at]) == sk and I.level_extent(S, sk) <= 32
    sh = np.array([int(v) for v in got[at + 1:at + 28]], dtype=np.uint32).reshape(9, 3)
    assert np.array_equal(sh, E.bits(I.sh9(levels[sk])))
    assert at + 28 == len(got)
    # level 0 is the source itself, not sanitised
    assert np.array_equal(E.bits(want[0][..., :3]), E.bits(levels[0])) and np.all(want[0][..., 3] == 1)


def test_rule_header_refuses_what_has_no_second_level(tmp_path):
    assert run("prefilter", "1 2\n", tmp_path) == ["refused"]  # L >= 2 needs S >= 2
    assert run("prefilter", "5 4\n", tmp_path) == ["refused"]  # extent 5 has levels 5, 2, 1
    assert run("prefilter", "8 1\n", tmp_path) == ["refused"]
    assert I.max_levels(1, 16) == 1 and I.max_levels(5, 16) == 3 and I.max_levels(256, 16) == 9 and I.max_levels(256, 4) == 4
    assert [I.sh_level(S, L) for S, L in ((2, 2), (32, 6), (33, 3), (64, 7), (256, 9), (256, 2), (256, 3))] == [0, 0, 1, 1, 3, 1, 2]


def test_rule_header_irradiance_word_for_word(tmp_path):
    rng = np.random.default_rng(5)
    sh = rng.normal(0, 1, (9, 3)).astype(f32)
    n = rng.normal(0, 1, (64, 3)).astype(f32)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    n[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=f32)
    text = "\n".join(map(str, E.bits(sh).reshape(-1).tolist())) + f"\n{len(n)}\n" + "\n".join(" ".join(map(str, r)) for r in E.bits(n).tolist()) + "\n"
    got = np.array([[int(v) for v in ln.split()] for ln in run("irradiance", text, tmp_path)], dtype=np.uint32)
    assert np.array_equal(got, E.bits(I.irradiance(sh, n)))


# ------------------------------------------------------------------ 2. the restatement against float64, within the header's bound
def test_bounds_are_the_headers():
    rule = open(RULES[0]).read()
    assert "(double)(2u * (2u * n + 6u) + 25u) * 5.9604644775390625e-8" in rule and "(double)(2u * n + 6u + 5u) * 5.9604644775390625e-8" in rule
    assert 5.9604644775390625e-8 == EPS


def prefilter_bound(n):
    return (2 * (2 * n + 6) + 25) * EPS  # ibl_rule::prefilter_bound


def sh_bound(n):
    return (2 * n + 6 + 5) * EPS  # ibl_rule::sh_bound


@pytest.mark.parametrize("n,k,L", [(8, 1, 4), (8, 3, 4), (16, 1, 11), (16, 10, 11), (32, 2, 11), (32, 1, 6)])
def test_f32_stays_within_the_bound_of_float64(n, k, L):
    rgb = I.random_levels(n, 1, seed=n + k)[0]
    got = I.prefilter_level(rgb, k, L)[..., :3].astype(np.float64)
    want = I.prefilter_level(rgb, k, L, dtype=np.float64)[..., :3]
    err = float(np.max(np.abs(got - want) / want))
    print(f"n={n} k={k} L={L}: worst relative error {err:.3g}, bound {prefilter_bound(n):.3g}")
    assert err <= prefilter_bound(n)


def test_f32_stays_within_the_bound_of_float64_at_extent_64():
    """n = 64 on every 61st output texel (403 of 24 576, spread over all faces and rows: 61 is prime to 64); each integrates the
    whole level, so the trees are the full 2 n + 6 additions deep"""
    n, L = 64, 11
    rgb = I.random_levels(n, 1, seed=64)[0]
    pick = np.arange(0, 6 * n * n, 61)
    for k in (1, 4):
        got = I.prefilter_level(rgb, k, L, pick=pick, chunk=64)[:, :3].astype(np.float64)
        want = I.prefilter_level(rgb, k, L, dtype=np.float64, pick=pick, chunk=64)[:, :3]
        err = float(np.max(np.abs(got - want) / want))
        print(f"n={n} k={k} L={L}: worst relative error {err:.3g}, bound {prefilter_bound(n):.3g}")
        assert err <= prefilter_bound(n)


@pytest.mark.parametrize("n", [5, 16, 32])
def test_sh_stays_within_the_bound_of_float64(n):
    rgb = I.random_levels(n, 1, seed=n)[0]
    got, want = I.sh9(rgb).astype(np.float64), I.sh9(rgb, dtype=np.float64)
    scale = I.sh9(rgb, dtype=np.float64, absolute=True)
    err = float(np.max(np.abs(got - want) / scale))
    print(f"n={n}: worst error relative to sum |term| {err:.3g}, bound {sh_bound(n):.3g}")
    assert err <= sh_bound(n)


# ------------------------------------------------------------------ 3. properties
@pytest.mark.parametrize("value", [0.25, 1.0, 8.0])
def test_a_constant_power_of_two_survives_exactly(value):
    S, L = 8, 4
    levels = [np.full((6, I.level_extent(S, k), I.level_extent(S, k), 3), value, dtype=f32) for k in range(L)]
    for k, lv in enumerate(I.prefilter(levels)):
        assert np.all(lv[..., :3] == f32(value)) and np.all(lv[..., 3] == 1), k  # wt * 2^e is exact, so num = 2^e den to the bit


@pytest.mark.parametrize("fill", [0.0, np.nan])
def test_an_empty_environment_gives_zeros(fill):
    S, L = 5, 3
    levels = [np.full((6, I.level_extent(S, k), I.level_extent(S, k), 3), fill, dtype=f32) for k in range(L)]
    out = I.prefilter(levels)
    for lv in out[1:]:
        assert np.all(lv[..., :3] == 0) and not np.isnan(lv).any()
    assert np.all(I.sh9(levels[I.sh_level(S, L)]) == 0)


def quadratic_environment(n):
    """a radiance that is a polynomial of degree <= 2 in the direction, positive everywhere"""
    u, _ = E.geometry(n)
    x, y, z = (u[..., k].astype(np.float64) for k in range(3))
    r = 1.0 + 0.5 * x - 0.25 * y + 0.3 * x * y + 0.2 * (3 * z * z - 1)
    g = 0.8 + 0.4 * z + 0.25 * (x * x - y * y) - 0.2 * y * z
    b = 1.2 - 0.3 * x + 0.35 * x * z + 0.1 * y
    return np.stack([r, g, b], axis=-1).astype(f32)


def test_the_roughest_level_is_the_irradiance_of_its_own_sh():
    """At a = 1 the weight is (N.L) dw: the level IS the cosine-weighted mean, which for a radiance of degree <= 2 the nine
    coefficients reproduce exactly in the continuum.  On the grid both are quadratures.  Measured with this reference alone at
    n = 32, in float64: worst relative difference 2.97e-4 (the texel-grid quadrature of the clamped cosine, whose kink at the
    horizon the 6 * 32^2 texels resolve to about 1 / n^2 = 9.8e-4 of the integral at worst); the float32 evaluations change no
    digit of that figure (their own error is below 1e-5, section 2).  Tolerance: 6e-4 = twice the measured quadrature error, the
    margin being for the float32 evaluations and for nothing else: the grid and the polynomial are fixed."""
    n = 32
    rgb = quadratic_environment(n)
    u, _ = E.geometry(n)
    N = u.reshape(-1, 3)
    L = 3  # k = L - 1: r = 1, a2 = 1, oma = 0
    assert I.roughness(L - 1, L) == (f32(1), f32(0))
    rough64 = I.prefilter_level(rgb, L - 1, L, dtype=np.float64)[..., :3].reshape(-1, 3)
    irr64 = I.irradiance(I.sh9(rgb, dtype=np.float64), N, dtype=np.float64)
    quadrature = float(np.max(np.abs(rough64 - irr64) / irr64))
    rough = I.prefilter_level(rgb, L - 1, L)[..., :3].reshape(-1, 3).astype(np.float64)
    irr = I.irradiance(I.sh9(rgb), N).astype(np.float64)
    worst = float(np.max(np.abs(rough - irr) / irr64))
    print(f"quadrature error in float64: {quadrature:.3g}; float32 level against float32 irradiance: {worst:.3g}")
    assert quadrature <= 6e-4 and worst <= 6e-4


# ------------------------------------------------------------------ 4. the lookups
def test_lookup_is_the_skybox_bilinear_on_whole_levels_and_its_mix_between():
    S, L = 8, 4
    out = I.prefilter(I.random_levels(S, L, seed=3))
    rng = np.random.default_rng(9)
    d = rng.normal(0, 1, (200, 3)).astype(f32)
    d[:8] = np.array([[1, 1, 1], [1, -1, 1], [-1, 1, -1], [1, 1, 0], [0, 1, 1], [1, 0, -1], [1, 0, 0], [0, 0, -1]], dtype=f32)  # corners, edges, centres
    for k in range(L):
        got, level, frac = I.specular(out, d, np.full(len(d), k / (L - 1), dtype=f32))
        if k in (0, L - 1):
            assert np.all(level == k) and np.all(frac == 0)
        whole = (level == k) & (frac == 0)  # (k / (L - 1)) * (L - 1) may round off k for the levels between
        assert np.array_equal(E.bits(got[whole]), E.bits(lodref.bilinear(out[k], lodref._AsStored(), d[whole])[:, :3]))
    level, frac = I.lod_of(np.array([0.0, 1.0, 0.5, 2.0, -1.0, np.nan, 1 / 3], dtype=f32), 4)
    assert level.tolist() == [0, 3, 1, 3, 0, 0, 1] and frac[:6].tolist() == [0, 0, 0.5, 0, 0, 0]
    assert frac[6] == f32(f32(1 / 3) * f32(3)) - f32(1)
    got, level, frac = I.specular(out, d, np.full(len(d), 0.5, dtype=f32))
    lo, hi = lodref.bilinear(out[1], lodref._AsStored(), d)[:, :3], lodref.bilinear(out[2], lodref._AsStored(), d)[:, :3]
    assert np.all(level == 1) and np.all(frac == f32(0.5))
    assert np.array_equal(E.bits(got), E.bits((lo * (f32(1) - f32(0.5)) + hi * f32(0.5)).astype(f32)))


# ------------------------------------------------------------------ 5. the ABI is declared everywhere
def test_abi_is_declared_in_every_layer():
    from rend3_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    assert re.search(r"int r3n_environment_prefilter\(r3n_ctx \*ctx, const r3n_env_prefilter_params \*params, r3n_env_prefilter_result \*out\);", hdr)
    assert "int r3n_environment_probe(r3n_ctx *ctx, uint32_t cube, const float sh[9][4], const r3n_env_query32 *queries, uint32_t n, r3n_env_sample32 *out);" in hdr
    assert "int r3n_skybox_set_level(r3n_ctx *ctx, float level);" in hdr
    assert _ffi.SIGNATURES["r3n_environment_prefilter"] == (_ffi.cint, [_ffi.vp, _ffi.vp, _ffi.vp])
    assert _ffi.SIGNATURES["r3n_skybox_set_level"] == (_ffi.cint, [_ffi.vp, _ffi.cfloat])
    assert [(n, getattr(_ffi.EnvPrefilterResult, n).offset) for n, _ in _ffi.EnvPrefilterResult._fields_] == \
        [("cube_id", 0), ("extent", 4), ("levels", 8), ("sh_level", 12), ("sh", 16)]
    assert ctypes.sizeof(_ffi.EnvPrefilterParams) == 12 and ctypes.sizeof(_ffi.EnvPrefilterResult) == 160
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert "pub fn r3n_environment_prefilter(ctx: *mut r3n_ctx, params: *const r3n_env_prefilter_params, out: *mut r3n_env_prefilter_result) -> c_int;" in rs
    assert "pub fn r3n_environment_probe(ctx: *mut r3n_ctx, cube: u32, sh: *const f32, queries: *const r3n_env_query32, n: u32, out: *mut r3n_env_sample32) -> c_int;" in rs
    assert "pub fn r3n_skybox_set_level(ctx: *mut r3n_ctx, level: f32) -> c_int;" in rs and "pub sh: [[f32; 4]; 9]," in rs
    assert set(build.UNITS["ibl.hip"]) >= {"ibl.h", "ibl_rule.h", "ibl_lookup.h", "cube_sample.h", "envlight_rule.h", "equirect_rule.h"}
    assert {"ibl.h", "ibl_rule.h", "ibl_lookup.h", "cube_sample.h"} <= set(build.UNITS["r3n.hip"]) and "cube_sample.h" in build.UNITS["skybox.hip"]
    hip = open(os.path.join(CSRC, "r3n.hip")).read()
    assert '{"ibl_tile", &ibl_tile, 0, R3N_IBL_TILE_MAX, 1}' in hip and '{"ibl_block", &ibl_block, 64, 256, 64}' in hip
    rule = open(RULES[0]).read()
    assert f"MAX_EXTENT = {I.MAX_EXTENT}u, MAX_LEVELS = {I.MAX_LEVELS}u, SH_EXTENT = {I.SH_EXTENT}u;" in rule
    assert "Y00 = 0.282095f, Y1 = 0.488603f, Y2A = 1.092548f, Y20 = 0.315392f, Y22 = 0.546274f;" in rule and "0.6666667f" in rule
    sky = open(os.path.join(CSRC, "skybox.hip")).read()
    sample = open(os.path.join(CSRC, "cube_sample.h")).read()
    for moved in ("R3N_DEV void sky_project(", "R3N_DEV void sky_fetch(", "R3N_DEV void sky_texel_any(", "R3N_DEV void sky_bilinear("):
        assert moved in sample and moved not in sky
    assert '#include "cube_sample.h"' in sky and "R3N_DEV void cube_sample_level(" in sample
    lib = _ffi.lib()
    assert all(hasattr(lib, s) for s in ("r3n_environment_prefilter", "r3n_environment_probe", "r3n_skybox_set_level"))
    assert lib.r3n_environment_prefilter(None, None, None) == -1  # (no context: refused before anything is touched)
    assert lib.r3n_skybox_set_level(None, 1.0) == -1


# ------------------------------------------------------------------ 6. the Python layer and the viewer
def test_python_layer_refusals_and_viewer_flag():
    from rend3_amd import renderer as R
    from rend3_amd import scene_viewer as V
    assert all(hasattr(R.Renderer, m) for m in ("prefilter_environment", "environment_probe", "set_skybox_level"))
    assert R.ENV_QUERY.itemsize == 32 and R.ENV_SAMPLE.itemsize == 32 and (R.IBL_MAX_EXTENT, R.IBL_MAX_LEVELS) == (I.MAX_EXTENT, I.MAX_LEVELS)

    class Stub:  # the checks in front of the library call need no context
        cubes = [(np.zeros((6, 4, 4, 4), dtype=np.uint8), True), R._EquirectCube(0, 8, 4, b"", 4096, 2)]
        _cube_extent_and_mips = R.Renderer._cube_extent_and_mips

        def _flush_cubes(self):
            pass

    for kw, match in ((dict(cube=2), "no such cube"), (dict(cube=-1), "no such cube"), (dict(cube=0, level=1), "no such level"),
                      (dict(cube=1), "no level of extent <= 256")):
        with pytest.raises(ValueError, match=match):
            R.Renderer.prefilter_environment(Stub(), **kw)
    with pytest.raises(ValueError, match="no such cube"):
        R.Renderer.environment_probe(Stub(), 2, np.zeros((9, 3)), [])
    with pytest.raises(ValueError, match="float32\\[9, 3\\]"):
        R.Renderer.environment_probe(Stub(), 0, np.zeros((3, 3)), [])
    s = Stub()
    with pytest.raises(ValueError, match="NaN"):
        R.Renderer.set_skybox_level(s, float("nan"))
    R.Renderer.set_skybox_level(s, None)
    assert s._skybox_level == -1.0
    R.Renderer.set_skybox_level(s, 2.5)
    assert s._skybox_level == 2.5

    class Host(Stub):  # a derived cube leaves the list when the array is re-sent
        def __init__(self):
            self.cubes = [(np.zeros((6, 4, 4, 4), dtype=np.uint8), True), R._DerivedCube(4, 3, 0, 0)]
            self._background, self._cubes_dirty = 1, False

        _drop_derived_cubes = R.Renderer._drop_derived_cubes

    h = Host()
    assert R.Renderer.add_texture_cube(h, np.zeros((6, 2, 2, 4), dtype=np.uint8)) == 1
    assert len(h.cubes) == 2 and h._background is None and h._cubes_dirty

    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(["--skybox", "sky.hdr", "--skybox-blur", "0.5"]))
    assert s["skybox_blur"] == 0.5 and V.default_settings()["skybox_blur"] is None

    class NoSky:
        handedness = V.RIGHT

    with pytest.raises(ValueError, match="--skybox-blur needs a skybox"):
        V.build(NoSky(), None, None, V.default_settings(skybox_blur=0.5))
