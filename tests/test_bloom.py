"""CPU-only: the bloom contract (DESIGN.md section 2 "Bloom", include/r3n.h r3n_bloom_set).  The numpy restatement
(tests/bloom_reference.py) is tied to tests/tonemap_reference.py (a zero pyramid changes no byte), to the two consequences DESIGN.md
derives (constant images, images below the knee), to clamping and energy properties, and to an independent float64 evaluation of
the filters; the rule header the kernels share with the host (rend3_amd/csrc/bloom_rule.h) is compiled into a stand-alone program
under the address and undefined-behaviour sanitizers and must print the reference's words; the ABI is present in the header, the
ctypes layer and the Rust crates.  The GPU side is tests/test_bloom_gpu.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bloom_reference as B
import host_check
import tonemap_reference as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "bloom_rule_check.cpp")
RULES = [os.path.join(ROOT, "rend3_amd", "csrc", f) for f in ("bloom_rule.h", "exposure_rule.h")]
f32 = np.float32
ONE = 0x3C00


def half_bits(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)


def grey_image(w, h, value):
    img = np.empty((h, w, 4), dtype=np.uint16)
    img[..., :3] = half_bits(value)
    img[..., 3] = ONE
    return img


def random_image(rng, w, h, octaves=14.0, zeros=0.05):
    img = np.empty((h, w, 4), dtype=np.uint16)
    img[..., :3] = (np.exp2(rng.uniform(-octaves, octaves, (h, w, 1))) * rng.uniform(0.1, 1.0, (h, w, 3))).astype(np.float16).view(np.uint16)
    img[..., 3] = ONE
    img[rng.random((h, w)) < zeros, :3] = 0
    return img


# ------------------------------------------------------------------ 1. tied to tonemap_reference
def test_levels():
    assert B.levels(3840, 2160, 16) == [(1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17), (15, 9), (8, 5), (4, 3),
                                        (2, 2), (1, 1)]
    assert B.levels(3840, 2160, 8)[-1] == (15, 9)
    assert B.levels(1, 1, 16) == [(1, 1)] and B.levels(2, 1, 16) == [(1, 1)] and B.levels(2, 2, 16) == [(1, 1)]
    assert B.levels(3, 5, 16) == [(2, 3), (1, 2), (1, 1)] and B.levels(17, 9, 2) == [(9, 5), (5, 3)]
    assert len(B.levels(1 << 20, 1, 16)) == 16


@pytest.mark.parametrize("output_format", [0, 1, 2, 3])
def test_zero_pyramid_is_the_tonemap_reference(output_format):
    """with a zero pyramid (an image wholly below threshold - knee), with bloom off and with intensity 0 the bytes and the float
    view are tonemap_reference's for the same options"""
    rng = np.random.default_rng(3)
    w, h = 37, 21
    img = random_image(rng, w, h, octaves=3.0)
    o = B.default_opts(threshold=40.0, knee=10.0, intensity=0.5)  # lo = 30 > 2^3
    for op, white, ev in ((0, 4.0, 0.0), (1, 0.75, 1.37), (2, 4.0, -2.5)):
        scale = T.exp2_lin(ev)
        want8, wantf = T.tonemap(img.reshape(-1, 4), scale, op, output_format, white)
        for opts in (o, None, B.default_opts(intensity=0.0)):
            got8, gotf, pyr = B.render(img, scale, op, output_format, opts, white)
            assert np.array_equal(got8, want8) and np.array_equal(gotf.view(np.uint32), wantf.view(np.uint32))
            if opts is o:
                assert all(not lvl.any() for chain in pyr for lvl in chain), "every level of d and a is zero"
    # the same image does bloom at the default threshold
    got8, _, pyr = B.render(img, 1.0, 2, output_format, B.default_opts(intensity=0.5))
    assert pyr[1][0].any() and not np.array_equal(got8, T.tonemap(img.reshape(-1, 4), 1.0, 2, output_format)[0])


# ------------------------------------------------------------------ 2. properties on the reference alone
def scalar_bright(value, o):
    """the bright pass of a grey pixel, on scalars"""
    lo, k2, inv = B.constants(o)
    m = f32(value)
    s = min(max(f32(m - lo), f32(0)), k2)
    q = f32(f32(s * s) * inv)
    e = max(q, f32(m - f32(o["threshold"])))
    w = f32(e / max(m, f32(2.0 ** -14)))
    return np.float16(f32(m * w))


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (17, 9)])
@pytest.mark.parametrize("value", [0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 3.0, 1000.0])
def test_constant_images_keep_a_constant_pyramid(size, value):
    """halves times small integers, normalised by powers of two -- d_k == p exactly for every k, and a_k follows the
    scalar recursion a_k = half(p + scatter * a_{k+1}).  (lo = 0.5: 0.25 lies below it, 0.5 on it, 0.75 .. 1.25 inside the knee.)"""
    w, h = size
    o = B.default_opts(max_levels=16, scatter=0.7)
    value = float(np.float16(value))
    p = scalar_bright(value, o)
    if value <= 0.5:
        assert p == 0
    else:
        assert p > 0
    d, a = B.pyramid(grey_image(w, h, value), 1.0, o)
    assert len(d) == len(B.levels(w, h, 16))
    for lvl in d:
        assert np.all(lvl == p.view(np.uint16)), (size, value)
    ak = p
    for k in range(len(d) - 1, -1, -1):
        if k < len(d) - 1:
            u = f32(f32(f32(3) * f32(f32(3) * f32(ak) + f32(ak)) + f32(f32(3) * f32(ak) + f32(ak))) * f32(1 / 16))
            assert u == f32(ak), "the tent of a constant is the constant"
            ak = np.float16(f32(f32(p) + f32(f32(o["scatter"]) * u)))
        assert np.all(a[k] == ak.view(np.uint16)), (size, value, k)


def impulse_image(w, h, x, y, value=64.0):
    img = grey_image(w, h, 0.0)
    img[y, x, :3] = half_bits(value)
    return img


def impulse_positions(w, h):
    """each corner, and the middle of each edge"""
    return [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]


def test_impulses_at_corners_and_edges_spread_through_clamped_taps():
    """an impulse in a corner or on an edge of an odd-sized target: the first level holds exactly the weights the clamped taps give
    it, nothing anywhere else, and the weight a clamped tap gathers is the sum of the taps that fell outside"""
    w, h = 17, 9
    o = B.default_opts(threshold=0.0, knee=0.0, max_levels=3)  # the bright pass is the identity on a grey pixel: w = m / m
    wts = np.array([1, 3, 3, 1], dtype=np.int64)
    for (x, y) in impulse_positions(w, h):
        d, a = B.pyramid(impulse_image(w, h, x, y, 64.0), 1.0, o)
        dw, dh = B.levels(w, h, 3)[0]
        want = np.zeros((dh, dw), dtype=np.float64)
        for dy in range(dh):
            for dx in range(dw):
                wx = sum(wts[i] for i in range(4) if min(max(2 * dx - 1 + i, 0), w - 1) == x)
                wy = sum(wts[i] for i in range(4) if min(max(2 * dy - 1 + i, 0), h - 1) == y)
                want[dy, dx] = 64.0 * wx * wy / 64.0  # exact in half: small integers
        got = B.halves(d[0])
        for c in range(3):
            assert np.array_equal(got[..., c].astype(np.float64), want), (x, y)
        assert (want > 0).sum() <= 4
        if (x, y) == (0, 0):
            assert want[0, 0] == 16.0 and want.sum() == 16.0  # column -1 clamps onto column 0: weights (1 + 3) each way, no other texel
        if (x, y) == (w - 1, h - 1):  # the last column / row of an odd size: the two taps past the edge clamp onto it, 3 + 3 + 1
            assert want[-1, -1] == 49.0 and want[-1, -2] == 7.0 and want[-2, -2] == 1.0 and want.sum() == 64.0
        # the up chain stays inside the hull of what the down chain touched plus one texel per level, and is finite
        assert all(np.isfinite(B.halves(lvl)).all() for lvl in a)


def test_interior_impulse_energy_quarters_per_level():
    """the 4x4 tent sums to 64 over the taps of one destination and every source texel is gathered with total weight 16 = 64 / 4
    by the destinations around it (away from the edges): sum(d_{k+1}) = sum(d_k) / 4, to within the half rounding of the stored
    texels -- at most 16 non-zero texels per level hold the impulse, each within 2^-11 relative of its exact value"""
    w = h = 129
    o = B.default_opts(threshold=0.0, knee=0.0, max_levels=4)
    img = impulse_image(w, h, 64, 66, 1000.0)
    d, _ = B.pyramid(img, 1.0, o)
    prev = float(B.halves(B.bright_pass(img, 1.0, o))[..., 0].astype(np.float64).sum())
    assert prev == 1000.0
    for k, lvl in enumerate(d):
        x = B.halves(lvl)[..., 0].astype(np.float64)
        assert lvl[0].max() == 0 and lvl[-1].max() == 0 and lvl[:, 0].max() == 0 and lvl[:, -1].max() == 0, "the impulse stays interior"
        s = float(x.sum())
        assert abs(s - prev / 4) <= (prev / 4) * ((1 + 2.0 ** -11) * (1 + 2.0 ** -24) ** 7 - 1) * 1.0000001, (k, s, prev / 4)
        prev = s


def test_sanitising_is_exposure_rules():
    """NaN, +-inf, negative and zero pixels enter as exposure_rule::exposed defines: 0, capped at 65504"""
    px = np.array([[0x7E00, 0x3C00, 0x3C00, ONE], [0xFC00, 0x4000, 0, ONE], [0x7C00, 0, 0, ONE], [0xBC00, 0xC000, 0x8000, ONE], [0x7BFF, 0x7BFF, 0x7BFF, ONE],
                   [0, 0, 0, ONE], [0x0001, 0x0001, 0x0001, ONE]], dtype=np.uint16).reshape(1, -1, 4)
    v = B.exposed(px, 2.0)
    assert np.array_equal(v[0], np.array([[0, 2, 2], [0, 4, 0], [65504, 0, 0], [0, 0, 0], [65504, 65504, 65504], [0, 0, 0], [2.0 ** -23] * 3], dtype=f32))
    o = B.default_opts(threshold=1.0, knee=0.0)
    p = B.halves(B.bright_pass(px, 2.0, o))
    assert np.isfinite(p).all() and (p >= 0).all() and not np.signbit(p).any()
    assert p[0, 0, 0] == 0 and p[0, 0, 1] == 1.0  # m = 2: w = 1 / 2
    assert p[0, 3].max() == 0 and p[0, 5].max() == 0 and p[0, 6].max() == 0
    assert np.all(p[0, 4] == np.float16(f32(65504) * f32(f32(65503) / f32(65504))))
    d, a = B.pyramid(px, 2.0, o)
    assert all(np.isfinite(B.halves(lvl)).all() for lvl in d)


# ------------------------------------------------------------------ 3. an independent float64 evaluation of the filters
def filters_f64(p_bits, n_levels, scatter):
    """the down and the up chain of the bright-pass image in float64 with no intermediate rounding, written tap by tap (not
    separably): d_k(x, y) = sum_ij wx_i wy_j s(clamp(2x-1+i), clamp(2y-1+j)) / 64, weights (1, 3, 3, 1)"""
    wt = (1.0, 3.0, 3.0, 1.0)
    src = p_bits.view(np.float16).astype(np.float64)
    d = []
    for _ in range(n_levels):
        h, w = src.shape[:2]
        dw, dh = (w + 1) // 2, (h + 1) // 2
        out = np.zeros((dh, dw, 3))
        for y in range(dh):
            for x in range(dw):
                acc = np.zeros(3)
                for j in range(4):
                    for i in range(4):
                        acc += wt[i] * wt[j] * src[min(max(2 * y - 1 + j, 0), h - 1), min(max(2 * x - 1 + i, 0), w - 1)]
                out[y, x] = acc / 64.0
        d.append(out)
        src = out
    a = [None] * n_levels
    a[-1] = d[-1]
    for k in range(n_levels - 2, -1, -1):
        h, w = d[k].shape[:2]
        ch, cw = a[k + 1].shape[:2]
        out = np.zeros_like(d[k])
        for y in range(h):
            for x in range(w):
                xn, yn = x // 2, y // 2
                xf = min(max(xn + (1 if x % 2 else -1), 0), cw - 1)
                yf = min(max(yn + (1 if y % 2 else -1), 0), ch - 1)
                u = (9.0 * a[k + 1][yn, xn] + 3.0 * a[k + 1][yn, xf] + 3.0 * a[k + 1][yf, xn] + a[k + 1][yf, xf]) / 16.0
                out[y, x] = d[k][y, x] + scatter * u
        a[k] = out
    return d, a


@pytest.mark.parametrize("size", [(17, 9), (33, 32)])
def test_reference_against_float64(size):
    """The bound, derived and not tuned.  Every value is non-negative, so relative errors never grow through a sum: a sum of terms
    each within (1 + e) of its exact value is within (1 + e) of the exact sum.  One down step is, along its longest path, a
    product, two sums (the row), a product, two sums and the product by 1/64 (the column): 7 f32 operations, each within
    (1 + 2^-24), and one half store within (1 + 2^-11).  One up step is 2 operations for the row term, 3 for the column, the
    product by scatter and the sum with d_k: 7 operations and one store, applied to the worse of its two inputs.  The longest path
    to a_0 runs down L levels and up L - 1: the bound is ((1 + 2^-24)^7 (1 + 2^-11))^(2L - 1) - 1, and ^(k + 1) for d_k.
    The (1 + 2^-11) of a half store holds for normal halves only, so the image is strictly positive (>= 2^-6: every texel of
    every level is a convex combination of such values, or larger) and small enough never to overflow."""
    w, h = size
    rng = np.random.default_rng(11)
    img = np.empty((h, w, 4), dtype=np.uint16)
    img[..., :3] = np.exp2(rng.uniform(-6, 6, (h, w, 3))).astype(np.float16).view(np.uint16)
    img[..., 3] = ONE
    o = B.default_opts(threshold=0.0, knee=0.0, scatter=0.7, max_levels=16)
    d, a = B.pyramid(img, 1.0, o)
    L = len(d)
    assert L == len(B.levels(w, h, 16)) >= 5
    p = B.bright_pass(img, 1.0, o)
    assert B.halves(p).min() >= 2.0 ** -6
    d64, a64 = filters_f64(p, L, float(f32(o["scatter"])))
    step = (1 + 2.0 ** -24) ** 7 * (1 + 2.0 ** -11)
    for k in range(L):
        got = B.halves(d[k]).astype(np.float64)
        assert got.min() >= 2.0 ** -6
        assert np.all(np.abs(got - d64[k]) <= d64[k] * (step ** (k + 1) - 1)), ("d", k)
        got = B.halves(a[k]).astype(np.float64)
        assert np.all(np.abs(got - a64[k]) <= a64[k] * (step ** (L + (L - 1 - k)) - 1)), ("a", k)


# ------------------------------------------------------------------ 4. the shared rule header, sanitized, stand-alone
def program():
    return host_check.program(SRC, RULES, fp_contract_off=True)


def run(cmd, text=""):
    res = subprocess.run([program(), cmd], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]  # a sanitizer report goes to stderr
    return res.stdout.split("\n")[:-1]


def bits(x):
    return int(np.asarray(x, dtype=f32).view(np.uint32))


def texel_lines(img):
    return "\n".join(" ".join(str(int(v)) for v in t) for t in np.asarray(img).reshape(-1, img.shape[-1])[:, :3])


def parse_texels(lines, w, h):
    return np.array([[int(v) for v in ln.split()] for ln in lines], dtype=np.uint16).reshape(h, w, 3)


def test_rule_header_levels():
    cases = [(1, 1, 16), (2, 1, 16), (2, 2, 1), (3, 5, 16), (17, 9, 2), (257, 131, 16), (1024, 600, 16), (3840, 2160, 16), (3840, 2160, 8), (1 << 20, 1, 16)]
    lines = run("levels", "\n".join(f"{w} {h} {m}" for w, h, m in cases))
    for (w, h, m), line in zip(cases, lines):
        want = B.levels(w, h, m)
        assert [int(v) for v in line.split()] == [len(want)] + [v for wh in want for v in wh], (w, h, m)


SPECIAL = np.array([[0x7E00, ONE, ONE, ONE], [0xFC00, 0x4000, 0, ONE], [0x7C00, 0, 0, ONE], [0xBC00, 0xC000, 0x8000, ONE], [0x7BFF, 0x7BFF, 0x7BFF, ONE],
                    [0, 0, 0, ONE], [1, 1, 1, ONE], [0x3800, 0x3800, 0x3800, ONE], [0x3C00, 0x3A00, 0x3555, ONE], [0x3E00, 0, 0x0400, ONE],
                    [28172, 29170, 29170, ONE]], dtype=np.uint16)  # (the last: at 1.37 EV v * w is 16004.0003 -> f32 16004, a tie of the half grid -> 16000)


@pytest.mark.parametrize("opts", [dict(), dict(threshold=0.0, knee=0.0), dict(threshold=2.0, knee=2.0), dict(threshold=65504.0, knee=1.0),
                                  dict(threshold=0.5, knee=0.0), dict(threshold=1.0, knee=1e-3)])
def test_rule_header_bright_pass(opts):
    rng = np.random.default_rng(19)
    o = B.default_opts(**opts)
    img = np.concatenate([random_image(rng, 64, 32, 14.0).reshape(-1, 4), random_image(rng, 64, 32, 1.5).reshape(-1, 4), SPECIAL]).reshape(1, -1, 4)
    for scale in (f32(1.0), T.exp2_lin(1.37), f32(2.0 ** -9), f32(4096.0)):
        head = f"{bits(scale)} {bits(o['intensity'])} {bits(o['threshold'])} {bits(o['knee'])} {bits(o['scatter'])} {o['max_levels']}\n"
        got = parse_texels(run("bright", head + texel_lines(img[0]) + "\n"), img.shape[1], 1)
        assert np.array_equal(got, B.bright_pass(img, scale, o)), (opts, scale)


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (2, 2), (3, 3), (5, 3), (17, 9), (64, 33)])
def test_rule_header_down_and_up_steps(size):
    w, h = size
    rng = np.random.default_rng(23)
    src = random_image(rng, w, h, 14.0)[..., :3]
    want = B.down(src)
    dh, dw = want.shape[:2]
    got = parse_texels(run("down", f"{w} {h}\n" + texel_lines(src) + "\n"), dw, dh)
    assert np.array_equal(got, want)
    for scatter in (0.7, 1.0, 0.0):
        a = B.up(src, want, scatter)
        got = parse_texels(run("up", f"{dw} {dh} {w} {h} {bits(scatter)}\n" + texel_lines(want) + "\n" + texel_lines(src) + "\n"), w, h)
        assert np.array_equal(got, a), scatter
    # a store that overflows the half range saturates to +inf in both
    big = np.full((h, w, 3), 0x7BFF, dtype=np.uint16)
    a = B.up(big, B.down(big), 1.0)
    assert np.all(a == 0x7C00)
    got = parse_texels(run("up", f"{dw} {dh} {w} {h} {bits(1.0)}\n" + texel_lines(B.down(big)) + "\n" + texel_lines(big) + "\n"), w, h)
    assert np.array_equal(got, a)


def test_rule_header_composite():
    rng = np.random.default_rng(31)
    v = np.concatenate([np.exp2(rng.uniform(-14, 16, 500)).astype(f32), np.array([0, 65504, 65504, 1.0, 0.0], dtype=f32)])
    b = np.concatenate([np.exp2(rng.uniform(-14, 16, 500)).astype(f32), np.array([0, 65504, np.inf, np.inf, 0.0], dtype=f32)])
    for intensity in (0.04, 1.0, 1024.0):
        got = [int(x) for x in run("composite", "\n".join(f"{bits(x)} {bits(y)} {bits(intensity)}" for x, y in zip(v, b)) + "\n")]
        with np.errstate(all="ignore"):
            want = np.minimum(v + f32(intensity) * b, B.MAX_HALF).astype(f32)
        assert got == [int(x) for x in want.view(np.uint32)]
        assert np.isfinite(want).all()


# ------------------------------------------------------------------ 5. the ABI is declared everywhere
def test_abi_is_declared_in_every_layer():
    from rend3_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    assert re.search(r"#define R3N_BLOOM_MAX_LEVELS 16u\b", hdr)
    assert "int r3n_bloom_set(r3n_ctx *ctx, const r3n_bloom_opts *opts);" in hdr
    assert re.search(r"int r3n_readback_bloom\(r3n_ctx \*ctx, uint32_t level, uint16_t \*rgb16f, uint64_t capacity_texels,\s+uint32_t \*width, "
                     r"uint32_t \*height, uint32_t \*levels\);", hdr)
    assert hdr.count("tonemapping.rs:1-10") >= 11  # the seven of the operators, and every bloom entry cites it too
    assert _ffi.SIGNATURES["r3n_bloom_set"] == (_ffi.cint, [_ffi.vp, _ffi.vp])
    assert _ffi.SIGNATURES["r3n_readback_bloom"] == (_ffi.cint, [_ffi.vp, _ffi.u32, _ffi.vp, _ffi.u64, _ffi.vp, _ffi.vp, _ffi.vp])
    o = _ffi.BloomOpts
    assert ctypes.sizeof(o) == 32 and ctypes.sizeof(_ffi.TonemapOpts) == 48
    assert [(n, getattr(o, n).offset) for n, _ in o._fields_] == [("intensity", 0), ("threshold", 4), ("knee", 8), ("scatter", 12), ("max_levels", 16),
                                                                  ("_pad", 20)]
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert "pub fn r3n_bloom_set(ctx: *mut r3n_ctx, opts: *const r3n_bloom_opts) -> c_int;" in rs
    assert "pub fn r3n_readback_bloom(ctx: *mut r3n_ctx, level: u32, rgb16f: *mut u16, capacity_texels: u64, width: *mut u32, height: *mut u32, " \
           "levels: *mut u32) -> c_int;" in rs
    assert "pub struct r3n_bloom_opts {" in rs and "pub max_levels: u32," in rs and "pub const R3N_BLOOM_MAX_LEVELS: u32 = 16;" in rs
    routine = open(os.path.join(ROOT, "bindings", "rend3-routine-amd", "src", "tonemapping.rs")).read()
    assert "sys::r3n_bloom_set(" in routine and "pub fn set_bloom(" in routine
    assert set(build.UNITS["bloom.hip"]) >= {"bloom.h", "bloom_rule.h"}
    assert {"bloom.h", "bloom_rule.h"} <= set(build.UNITS["r3n.hip"]) and "bloom_rule.h" in build.UNITS["exposure.hip"]
    hip = open(os.path.join(ROOT, "rend3_amd", "csrc", "r3n.hip")).read()
    assert '{"bloom_tail", &t.bloom_tail, 0, 1u << 24, 1}' in hip and '{"bloom_keep_down", &t.bloom_keep_down, 0, 1, 1}' in hip
    assert "#define R3N_STAGE_COUNT 25" in hdr or re.search(r"R3N_STAGE_COUNT\s*=?\s*25", hdr), "bloom is timed under R3N_STAGE_TONEMAP: no new stage"
    lib = _ffi.lib()
    assert hasattr(lib, "r3n_bloom_set") and hasattr(lib, "r3n_readback_bloom")
    assert lib.r3n_bloom_set(None, None) == -1  # (no context: refused before anything is touched)
    assert lib.r3n_readback_bloom(None, 0, None, 0, None, None, None) == -1


# ------------------------------------------------------------------ 6. what the Python layer refuses
def test_python_refusals_and_defaults():
    import argparse
    import rend3_amd
    from rend3_amd import renderer as R
    from rend3_amd import scene_viewer as V
    o = R.bloom_opts()
    assert (round(o.intensity, 6), o.threshold, o.knee, round(o.scatter, 6), o.max_levels) == (0.04, 1.0, 0.5, 0.7, 8)
    assert rend3_amd.bloom_opts is R.bloom_opts
    z = R.bloom_opts(intensity=0.0, threshold=0.0, knee=0.0, scatter=0.0, max_levels=1)
    assert (z.intensity, z.threshold, z.knee, z.scatter, z.max_levels) == (0, 0, 0, 0, 1)
    R.bloom_opts(intensity=1024.0, threshold=65504.0, knee=65504.0, scatter=1.0, max_levels=16)
    nan = math.nan
    for bad in (dict(intensity=-0.1), dict(intensity=1024.5), dict(intensity=nan), dict(threshold=-1.0), dict(threshold=65505.0), dict(threshold=nan),
                dict(knee=-0.1), dict(knee=1.5), dict(knee=nan), dict(scatter=-0.1), dict(scatter=1.1), dict(scatter=nan), dict(max_levels=0),
                dict(max_levels=17), dict(max_levels=2.5), dict(intensity="1"), dict(intensity=math.inf), dict(threshold=math.inf)):
        with pytest.raises(ValueError):
            R.bloom_opts(**bad)
    assert hasattr(R.Renderer, "set_bloom") and hasattr(R.Renderer, "readback_bloom") and hasattr(R.TonemappingRoutine, "set_bloom")
    flags = ["--bloom", "0.1", "--bloom-threshold", "1.5", "--bloom-knee", "0.25", "--bloom-scatter", "0.5", "--bloom-levels", "6"]
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(flags))
    assert (s["bloom"], s["bloom_threshold"], s["bloom_knee"], s["bloom_scatter"], s["bloom_levels"]) == (0.1, 1.5, 0.25, 0.5, 6)
    d = V.default_settings()
    assert (d["bloom"], d["bloom_threshold"], d["bloom_knee"], d["bloom_scatter"], d["bloom_levels"]) == (0.0, 1.0, 0.5, 0.7, 8), "off by default"

    class BlitOnly:  # the oracle-side and blit-only renderers have no set_bloom, as they have no set_tonemapping
        handedness = V.RIGHT

    with pytest.raises(ValueError, match="--bloom"):
        V.build(BlitOnly(), None, None, V.default_settings(bloom=0.1))
    from oracle import world as ow
    assert not hasattr(ow.OracleRenderer, "set_bloom") and not hasattr(ow.OracleRenderer, "set_tonemapping")
