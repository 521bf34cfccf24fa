"""CPU-only: the exposure / tonemapping-operator contract (include/r3n.h r3n_tonemap_set).  The numpy
restatement (tests/tonemap_reference.py) is tied to the oracle's blit, to a brute-force metering and to a float64 evaluation of its
tables; the rule header the kernels share with the host (rend3_amd/csrc/exposure_rule.h) is compiled into a stand-alone program
under the address and undefined-behaviour sanitizers and must print the reference's words; the ABI is present in the header, the
ctypes layer and the Rust crates.  The GPU side is tests/test_tonemap_ops_gpu.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import host_check
import tonemap_reference as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "exposure_rule_check.cpp")
RULE = os.path.join(ROOT, "rend3_amd", "csrc", "exposure_rule.h")
f32 = np.float32
ALL_HALVES = np.arange(65536, dtype=np.uint16)


def every_half_image():
    """256 x 256: every half in every colour channel (NaN, +-inf, -0, subnormals, negatives), the channels permuted"""
    return np.stack([ALL_HALVES, ALL_HALVES[::-1], np.roll(ALL_HALVES, 12345), ALL_HALVES], axis=1).copy()


# ------------------------------------------------------------------ 1, 2: the reference against the oracle's blit
@pytest.mark.parametrize("output_format", [0, 1, 2, 3])
def test_blit_at_zero_ev_is_the_oracles_blit(output_format):
    hdr = every_half_image()
    assert T.exp2_lin(0.0) == f32(1.0)
    got8, gotf = T.tonemap(hdr, T.exp2_lin(0.0), T.OPS["blit"], output_format)
    exp8, expf = T.transfer(hdr, output_format)
    assert np.array_equal(got8, exp8)
    assert np.array_equal(gotf.view(np.uint32), expf.view(np.uint32))


@pytest.mark.parametrize("output_format", [0, 3])
def test_integer_stops_scale_exactly(output_format):
    """2^k for k = -3..3 is exact, so on every half whose product is a half again the result is the oracle's blit of that half"""
    x = ALL_HALVES.view(np.float16).astype(np.float64)
    for k in range(-3, 4):
        scale = T.exp2_lin(float(k))
        assert scale == f32(2.0 ** k)
        with np.errstate(all="ignore"):
            prod = x * 2.0 ** k
            as_half = prod.astype(np.float16)
            exact = np.isfinite(x) & (x > 0) & (as_half.astype(np.float64) == prod) & (prod <= 65504.0)
        assert exact.sum() > 25000
        src = ALL_HALVES[exact]
        hdr = np.stack([src, src, src, np.full_like(src, 0x3C00)], axis=1).copy()
        scaled = as_half[exact].view(np.uint16)
        host = np.stack([scaled, scaled, scaled, np.full_like(src, 0x3C00)], axis=1).copy()
        got8, gotf = T.tonemap(hdr, scale, T.OPS["blit"], output_format)
        exp8, expf = T.transfer(host, output_format)
        assert np.array_equal(got8, exp8), k
        assert np.array_equal(gotf.view(np.uint32), expf.view(np.uint32)), k


# ------------------------------------------------------------------ 3, 4: bins and tables
def test_bin_edges():
    for o in range(-16, 16):
        for s in range(8):
            edge = f32(2.0 ** o * (1 + s / 8))
            j = (o + 16) * 8 + s
            assert T.bins_of(np.array([edge]))[0] == j
            below = np.nextafter(edge, f32(0), dtype=f32)
            assert T.bins_of(np.array([below]))[0] == max(j - 1, 0)
    lum = np.array([0.0, -0.0, -1.0, np.nan, -np.inf, np.inf, 2.0 ** 16, 2.0 ** -17, 1e-45, 65504.0], dtype=f32)
    assert list(T.bins_of(lum)) == [-1, -1, -1, -1, -1, 255, 255, 0, 0, 255]


def test_bin_values_against_float64():
    assert len(T.LQ) == 256
    for j, q in enumerate(T.LQ):
        lo, hi = 2.0 ** ((j >> 3) - 16) * (1 + (j & 7) / 8), 2.0 ** ((j >> 3) - 16) * (1 + ((j & 7) + 1) / 8)
        assert abs(q - np.log2(np.float64((lo + hi) / 2)) * 65536.0) <= 1.0, j
    assert T.E[0] == 1 and T.E[256] == 2 and np.all(np.diff(T.E) > 0)
    assert np.max(np.abs(T.E.astype(np.float64) / np.exp2(np.arange(257) / 256.0) - 1)) < 2.0 ** -24


def test_exp2_lin_is_close_and_exact_on_integers():
    rng = np.random.default_rng(5)
    for e in list(rng.uniform(-32, 32, 400).astype(f32)) + [f32(-1e-9), f32(31.999998), f32(-32), f32(32), f32(-2.5), f32(1.37)]:
        got = float(T.exp2_lin(e))
        assert abs(got / 2.0 ** float(e) - 1) < 2e-6, e  # the chord's error is (ln 2 / 256)^2 / 8 = 9.2e-7
    for k in range(-32, 33):
        assert T.exp2_lin(k) == f32(2.0 ** k)


# ------------------------------------------------------------------ 5: the integer metering against brute force
def random_image(rng, n, spread):
    lum = np.exp2(rng.uniform(-spread, spread, n)).astype(np.float16)
    hdr = np.zeros((n, 4), dtype=np.uint16)
    hdr[:, :3] = (lum[:, None] * rng.uniform(0.2, 1.0, (n, 3))).astype(np.float16).view(np.uint16)
    hdr[rng.random(n) < 0.1] = 0  # black: excluded
    hdr[:, 3] = 0x3C00
    return hdr


def brute_force(hdr, o):
    b = T.bins_of(T.luminance(hdr))
    b = np.sort(b[b >= 0])
    lo, hi = len(b) * o["low_permille"] // 1000, len(b) * o["high_permille"] // 1000
    return sum(T.LQ[j] for j in b[lo:hi]), hi - lo


METER_CASES = [(1, 500, 950), (2, 0, 1000), (7, 500, 950), (64, 0, 1), (333, 999, 1000), (1000, 250, 750), (4097, 500, 950), (50, 0, 1000)]


def test_metering_equals_brute_force():
    rng = np.random.default_rng(17)
    for n, lo, hi in METER_CASES:
        for spread in (1.0, 12.0):
            hdr = random_image(rng, n, spread)
            o = T.default_opts(low_permille=lo, high_permille=hi)
            hist, excluded = T.histogram(hdr)
            assert int(hist.sum()) + excluded == n
            assert T.meter(hist, o) == brute_force(hdr, o), (n, lo, hi)


# ------------------------------------------------------------------ 6: the operators
@pytest.mark.parametrize("op", ["reinhard", "aces"])
def test_operators_are_monotone_and_finite(op):
    pos = ALL_HALVES[(ALL_HALVES <= 0x7C00)]  # +0 .. +inf in rising order
    x = T.halves_f32(pos)
    for scale in (2.0 ** -14, 0.17, 1.0, T.exp2_lin(1.37), 64.0, 2.0 ** 20):
        y = T.operate(x, scale, T.OPS[op], white=4.0)
        assert np.all(np.isfinite(y)) and np.all(y >= 0)
        assert np.all(np.diff(y) >= -np.abs(y[1:]) * f32(2.0 ** -22))  # rises, to within the roundings of the rational form (2 ulp)
        h = y.astype(np.float16)
        assert np.all(np.isfinite(h)) and np.all(np.diff(h.astype(f32)) >= 0)  # what is stored (half) is monotone outright
    every = T.operate(T.halves_f32(ALL_HALVES), 1.0, T.OPS[op])
    assert np.all(np.isfinite(every))  # NaN, -inf, negatives: 0


# ------------------------------------------------------------------ 7: the shared rule header, sanitized, stand-alone
def program():
    return host_check.program(SRC, [RULE], fp_contract_off=True)


def run(cmd, text=""):
    res = subprocess.run([program(), cmd], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]  # a sanitizer report goes to stderr
    return res.stdout.split("\n")[:-1]


def bits(x):
    return int(np.asarray(x, dtype=f32).view(np.uint32))


def test_rule_header_tables_bins_and_scale():
    lines = [int(v) for v in run("tables")]
    assert lines[:256] == T.LQ
    assert lines[256:] == [int(v) for v in T.E.view(np.uint32)]
    rng = np.random.default_rng(3)
    lum = np.concatenate([rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32),
                          np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x37800000, 0x377FFFFF, 0x47800000, 0x477FFFFF], dtype=np.uint32)])
    got = [int(v) for v in run("bins", "\n".join(str(int(u)) for u in lum))]
    assert got == [int(b) for b in T.bins_of(lum.view(f32))]
    evs = np.concatenate([rng.uniform(-32, 32, 3000).astype(f32), np.arange(-32, 33).astype(f32),
                          np.array([-1e-9, -1e-30, 31.999998, -2.5, 1.37], dtype=f32)])
    got = [int(v) for v in run("exp2", "\n".join(str(bits(e)) for e in evs))]
    assert got == [bits(T.exp2_lin(e)) for e in evs]


SEQUENCES = [dict(adapt=1.0), dict(adapt=0.5), dict(adapt=0.05, low_permille=0, high_permille=1000, exposure_ev=1.25),
             dict(adapt=0.5, min_ev=-0.5, max_ev=0.75)]


def test_rule_header_steps_equal_the_reference():
    rng = np.random.default_rng(29)
    for over in SEQUENCES:
        o = T.default_opts(exposure_mode=1, **over)
        hists = [T.histogram(random_image(rng, n, spread))[0] for n, spread in ((700, 2.0), (64, 10.0), (2000, 0.5), (1, 1.0), (900, 14.0))]
        hists.insert(2, np.zeros(256, dtype=np.uint32))  # nothing to meter: the state is carried over
        hists.insert(0, np.zeros(256, dtype=np.uint32))  # ... and before anything was metered: clamp(exposure_ev), invalid
        head = " ".join(str(bits(o[k])) for k in ("exposure_ev",)) + f" {bits(f32(o['white']) * f32(o['white']))} " + \
            " ".join(str(bits(o[k])) for k in ("key_log2", "min_ev", "max_ev", "adapt")) + f" {o['low_permille']} {o['high_permille']}"
        lines = run("steps", head + "\n" + "\n".join(" ".join(str(int(v)) for v in h) for h in hists) + "\n")
        assert len(lines) == len(hists)
        st = dict(T.INVALID)
        for k, (h, line) in enumerate(zip(hists, lines)):
            st = T.step(st, h, o)
            s, n = T.meter(h, o)
            assert [int(v) for v in line.split()] == [s, n] + T.state_words(st), (over, k)
        assert st["valid"] == 1


# ------------------------------------------------------------------ 8: the ABI is declared everywhere
def test_abi_is_declared_in_every_layer():
    from rend3_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    for name, value in (("R3N_TONEMAP_OP_BLIT", 0), ("R3N_TONEMAP_OP_REINHARD", 1), ("R3N_TONEMAP_OP_ACES", 2), ("R3N_EXPOSURE_MANUAL", 0), ("R3N_EXPOSURE_AUTO", 1)):
        assert re.search(rf"#define {name} {value}u\b", hdr), name
    assert "int r3n_tonemap_set(r3n_ctx *ctx, const r3n_tonemap_opts *opts);" in hdr
    assert "int r3n_readback_exposure(r3n_ctx *ctx, r3n_exposure_state *out);" in hdr
    assert hdr.count("tonemapping.rs:1-10") >= 7  # every entry cites what it completes
    assert _ffi.SIGNATURES["r3n_tonemap_set"] == (_ffi.cint, [_ffi.vp, _ffi.vp])
    assert _ffi.SIGNATURES["r3n_readback_exposure"] == (_ffi.cint, [_ffi.vp, _ffi.vp])
    o, s = _ffi.TonemapOpts, _ffi.ExposureState
    assert ctypes.sizeof(o) == 48
    assert [(n, getattr(o, n).offset) for n, _ in o._fields_] == [("op", 0), ("exposure_mode", 4), ("exposure_ev", 8), ("white", 12), ("key_log2", 16),
        ("min_ev", 20), ("max_ev", 24), ("adapt", 28), ("low_permille", 32), ("high_permille", 36), ("_pad", 40)]
    assert ctypes.sizeof(s) == 1056
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [("histogram", 0), ("excluded", 1024), ("valid", 1028), ("mean_log2", 1032),
        ("target_ev", 1036), ("current_ev", 1040), ("scale", 1044), ("_pad", 1048)]
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert "pub fn r3n_tonemap_set(ctx: *mut r3n_ctx, opts: *const r3n_tonemap_opts) -> c_int;" in rs
    assert "pub fn r3n_readback_exposure(ctx: *mut r3n_ctx, out: *mut r3n_exposure_state) -> c_int;" in rs
    assert "pub struct r3n_tonemap_opts {" in rs and "pub histogram: [u32; 256]," in rs and "pub const R3N_EXPOSURE_AUTO: u32 = 1;" in rs
    routine = open(os.path.join(ROOT, "bindings", "rend3-routine-amd", "src", "tonemapping.rs")).read()
    assert "sys::r3n_tonemap_set(" in routine and "pub fn set_tonemapping(" in routine
    assert "exposure_rule.h" in build.UNITS["exposure.hip"] and "exposure.h" in build.UNITS["r3n.hip"]
    lib = _ffi.lib()
    assert hasattr(lib, "r3n_tonemap_set") and hasattr(lib, "r3n_readback_exposure")
    assert lib.r3n_tonemap_set(None, None) == -1  # (no context: refused before anything is touched)


# ------------------------------------------------------------------ 9: what the Python layer refuses
def test_python_refusals_and_defaults():
    import rend3_amd
    from rend3_amd import renderer as R
    o = R.tonemap_opts()
    assert (o.op, o.exposure_mode, o.exposure_ev, o.white) == (0, 0, 0.0, 4.0)
    assert abs(o.key_log2 - math.log2(0.18)) < 1e-6 and (o.low_permille, o.high_permille) == (500, 950) and 0 < o.adapt <= 1
    a = R.tonemap_opts("aces", 0.5, auto_exposure=rend3_amd.AutoExposure(speed=2.0), dt=0.25)
    assert (a.op, a.exposure_mode) == (2, 1) and abs(a.adapt - (1 - math.exp(-0.5))) < 1e-6
    assert R.tonemap_opts(auto_exposure=R.AutoExposure(speed=math.inf)).adapt == 1.0
    assert 0 < R.tonemap_opts(auto_exposure=R.AutoExposure(speed=1e-12)).adapt  # never rounds to "no adaptation"
    with pytest.raises(ValueError):
        R.tonemap_opts("filmic")
    with pytest.raises(TypeError):
        R.tonemap_opts(auto_exposure=dict(key=0.18))
    for bad in (dict(key=0.0), dict(key=-1.0), dict(key=math.nan), dict(speed=0.0), dict(low=0.95, high=0.5), dict(high=1.5), dict(low=-0.1)):
        with pytest.raises(ValueError):
            R.tonemap_opts(auto_exposure=R.AutoExposure(**bad))
    with pytest.raises(ValueError):
        R.tonemap_opts(auto_exposure=R.AutoExposure(), dt=0.0)
    from rend3_amd import scene_viewer as V
    import argparse
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(["--tonemap", "aces", "--exposure", "-1.5", "--auto-exposure"]))
    assert (s["tonemap"], s["exposure"], s["auto_exposure"]) == ("aces", -1.5, True)
    d = V.default_settings()
    assert (d["tonemap"], d["exposure"], d["auto_exposure"]) == ("blit", 0.0, False)

    class BlitOnly:
        handedness = V.RIGHT

    with pytest.raises(ValueError):
        V.build(BlitOnly(), None, None, V.default_settings(tonemap="aces"))
