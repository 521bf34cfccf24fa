"""CPU-only: cubes from equirectangular panoramas (DESIGN.md section 2 "Cubes from panoramas", include/r3n.h
r3n_texture_cubes_write_sources).  The rule header the kernels share with the host (rend3_amd/csrc/equirect_rule.h) is compiled into
a stand-alone program under the address and undefined-behaviour sanitizers and must print the words of the numpy restatement
(tests/equirect_reference.py); the restatement is held to an independent float64 evaluation and to the geometry that must hold
exactly; containers.parse_hdr reads what a small writer here writes; the ABI is present in every layer.  The GPU side is
tests/test_equirect_gpu.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import equirect_reference as Q
import host_check
import skybox_reference as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "equirect_rule_check.cpp")
RULE = os.path.join(ROOT, "rend3_amd", "csrc", "equirect_rule.h")
f32 = np.float32
SOURCES = [(1, 1), (2, 1), (4, 2), (7, 5), (64, 32)]
EXTENTS = [1, 2, 3, 5, 8]


def program():
    return host_check.program(SRC, [RULE], fp_contract_off=True)


def run(cmd, text=""):
    res = subprocess.run([program(), cmd], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stdout[-2000:] + res.stderr[-4000:]  # a sanitizer report goes to stderr
    return res.stdout.split("\n")[:-1]


def words(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


def lines_of(a):
    return "\n".join(" ".join(str(int(v)) for v in row) for row in words(a).reshape(-1, 4)) + "\n"


def parse(lines, shape, dtype=np.uint32):
    return np.array([[int(v) for v in ln.split()] for ln in lines], dtype=np.int64).astype(dtype).reshape(shape)


def random_panorama(rng, W, H):
    src = np.empty((H, W, 4), dtype=f32)
    src[..., :3] = (np.exp2(rng.uniform(-8, 8, (H, W, 1))) * rng.uniform(0.1, 1.0, (H, W, 3))).astype(f32)
    src[..., 3] = rng.uniform(0, 1, (H, W)).astype(f32)
    return src


# ------------------------------------------------------------------ 1. the rule header against the restatement, word for word
def test_rule_header_rgbe_decode():
    cases = np.array([(b, (b * 7 + 1) % 256 if b else 0, 255 - b if b != 1 else 1, e) for e in range(256) for b in (0, 1, 128, 255)], dtype=np.uint8)
    got = parse(run("rgbe", "\n".join(" ".join(str(int(v)) for v in c) for c in cases) + "\n"), (-1, 4))
    want = Q.rgbe_decode(cases)
    assert np.array_equal(got, words(want))
    # the definition itself, in exact arithmetic: byte * 2^(e - 136); e == 0 is black; alpha is 1
    for c, w in zip(cases, want):
        for k in range(3):
            assert float(w[k]) == (0.0 if c[3] == 0 else math.ldexp(int(c[k]), int(c[3]) - 136)), c
        assert w[3] == 1.0
    assert float(Q.rgbe_decode(np.array([255, 255, 255, 255], dtype=np.uint8))[0]) == 255 * 2.0 ** 119
    assert float(Q.rgbe_decode(np.array([1, 0, 0, 1], dtype=np.uint8))[0]) == 2.0 ** -135  # a subnormal


def atan2_grid():
    v = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 1e-30, -1e-30, 1e30, -1e30, 0.41421357, 2.4142137, 1.0000001, 0.99999994]
    rng = np.random.default_rng(5)
    v += list(rng.normal(size=24))
    ys, xs = np.meshgrid(np.array(v, dtype=f32), np.array(v, dtype=f32))
    return ys.reshape(-1), xs.reshape(-1)


def test_rule_header_atan2_turns():
    ys, xs = atan2_grid()
    got = parse(run("atan2", "\n".join(f"{a} {b}" for a, b in zip(words(ys), words(xs))) + "\n"), (-1,))
    want = Q.atan2_turns(ys, xs)
    assert np.array_equal(got, words(want))
    at = {(float(y), float(x), bool(np.signbit(y)), bool(np.signbit(x))): float(w) for y, x, w in zip(ys, xs, want)}
    for sy in (False, True):
        for sx in (False, True):
            assert at[(0.0, 0.0, sy, sx)] == 0.0, "atan2_turns(0, 0) = 0 for either sign of either zero"
    assert at[(0.0, 1.0, False, False)] == 0.0 and at[(1.0, 0.0, False, False)] == 0.25 and at[(0.0, -1.0, False, True)] == 0.5
    assert at[(-1.0, 0.0, True, False)] == -0.25
    for (y, x), turns in (((1.0, 1.0), 0.125), ((1.0, -1.0), 0.375), ((-1.0, -1.0), -0.375), ((-1.0, 1.0), -0.125)):
        assert abs(at[(y, x, y < 0, x < 0)] - turns) <= Q.E
    finite = np.isfinite(want)
    exact = np.arctan2(ys.astype(np.float64), xs.astype(np.float64)) / (2 * math.pi)
    err = np.abs(want.astype(np.float64) - exact)[finite & ((ys != 0) | (xs != 0))]
    assert np.all(np.minimum(err, 1 - err) <= Q.E)


@pytest.mark.parametrize("source", SOURCES)
def test_rule_header_taps(source):
    W, H = source
    cases = [(f, n) for n in EXTENTS for f in range(6)]
    got = run("taps", "\n".join(f"{f} {n} {W} {H}" for f, n in cases) + "\n")
    at = 0
    for f, n in cases:
        c0, c1, r0, r1, fx, fy = Q.face_taps(f, n, W, H)
        g = parse(got[at:at + n * n], (n, n, 6))
        at += n * n
        for k, w in enumerate((c0, c1, r0, r1, words(fx), words(fy))):
            assert np.array_equal(g[..., k], w), (f, n, k)
        assert c0.min() >= 0 and c1.min() >= 0 and max(c0.max(), c1.max()) < W and r0.min() >= 0 and max(r0.max(), r1.max()) < H
        assert fx.min() >= 0 and fx.max() < 1 and fy.min() >= 0 and fy.max() < 1
    assert at == len(got)


@pytest.mark.parametrize("source", [(1, 1), (7, 5), (64, 32)])
def test_rule_header_faces(source):
    W, H = source
    src = random_panorama(np.random.default_rng(W), W, H)
    for n in (1, 3, 8):
        got = parse(run("faces", f"{n} {W} {H}\n" + lines_of(src)), (6, n, n, 4))
        assert np.array_equal(got, words(Q.faces(src, n)))


def test_rule_header_chain_steps():
    rng = np.random.default_rng(9)
    for s in range(1, 10):
        face = random_panorama(rng, s, s)
        want = Q.chain_step(face)
        d = max(1, s >> 1)
        assert want.shape == (d, d, 4)
        assert np.array_equal(parse(run("chain", f"{s}\n" + lines_of(face)), (d, d, 4)), words(want)), s
        if s % 2 == 0 and s & (s - 1) == 0:  # (a power of two: the taps are exactly the 2 x 2 block, the weights exactly 1 / 2)
            mean = ((face[0::2, 0::2] * f32(0.5) + face[0::2, 1::2] * f32(0.5)) * f32(0.5) + (face[1::2, 0::2] * f32(0.5) + face[1::2, 1::2] * f32(0.5)) * f32(0.5))
            assert np.array_equal(words(want), words(mean))


def test_rule_header_plans():
    cases = [(T, [(n, n.bit_length())]) for n in (1, 2, 33, 64, 65, 1024) for T in (0, 1, 32, 64)]
    cases += [(T, [(65, 7), (5, 3), (1024, 4), (64, 1)]) for T in (0, 1, 4, 32, 64)] + [(4, [])]
    got = run("plan", "\n".join(f"{T} {len(c)} " + " ".join(f"{n} {m}" for n, m in c) for T, c in cases) + "\n")
    for (T, c), line in zip(cases, got):
        p = Q.plan([n for n, _ in c], [m for _, m in c], T)
        want = [p["faces"], p["levels"], p["tail"], Q.plan_launches(p)] + [Q.tail_from(n, m, T) for n, m in c]
        assert [int(v) for v in line.split()] == want, (T, c)
    # what the plan means, on examples
    assert Q.plan([1024], [11], 0) == {"faces": 1, "levels": 10, "tail": 0}, "threshold 0: a launch per level"
    assert Q.plan([1024], [11], 64) == {"faces": 1, "levels": 4, "tail": 1}, "1024 -> 64 level by level, 32 .. 1 in the tail"
    assert Q.plan([64], [7], 64) == {"faces": 1, "levels": 0, "tail": 1} and Q.plan([65], [7], 64) == {"faces": 1, "levels": 1, "tail": 1}
    assert Q.plan([1], [1], 64) == {"faces": 1, "levels": 0, "tail": 0} and Q.plan([2], [2], 1) == {"faces": 1, "levels": 1, "tail": 0}
    assert Q.plan([], [], 64) == {"faces": 0, "levels": 0, "tail": 0}


# ------------------------------------------------------------------ 2. the restatement against float64
def test_polynomial_keeps_to_the_stated_error():
    e_bits, worst_poly, worst_atan2 = run("sweep")[0].split()
    assert int(e_bits) == int(words(f32(Q.E)).reshape(-1)[0]) and Q.E == 2.0 ** -22
    header = open(RULE).read()
    assert "constexpr float ATAN2_TURNS_E = 0x1p-22f;" in header and "E = 2^-22 turns" in header
    assert float(worst_poly) <= 2.0 ** -24, "the header derives E from a polynomial error below 2^-24 turns"
    assert float(worst_atan2) <= Q.E


@pytest.mark.parametrize("source", [(7, 5), (64, 32), (65535, 3)])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 33])
def test_coordinates_against_float64(source, n):
    """|x_rule - x_f64| <= W (E + 4 * 2^-24) and the same in y with H: E bounds the angle (in turns), and behind it u = 0.5 + phi is
    one rounding of a value <= 1 (2^-25), u * W one of a value <= W (W 2^-25 ... W 2^-24) and the - 0.5 another; v carries the
    latitude twice, which the derivation of E in the header allows for."""
    W, H = source
    j, i = np.mgrid[0:n, 0:n]
    for f in range(6):
        u, v = Q.panorama_uv(Q.face_direction(f, i, j, n))
        x, y = (u * f32(W) - f32(0.5)).astype(np.float64), (v * f32(H) - f32(0.5)).astype(np.float64)
        sc, tc = (2.0 * i + 1.0 - n) / n, (2.0 * j + 1.0 - n) / n
        d = S._face_point(np.full(sc.shape, f), sc, tc)  # the project's own convention, in float64
        phi = np.arctan2(d[..., 2], d[..., 0])
        theta = np.arctan2(d[..., 1], np.hypot(d[..., 0], d[..., 2]))
        x64, y64 = (0.5 + phi / (2 * math.pi)) * W - 0.5, (0.5 - theta / math.pi) * H - 0.5
        dx = np.abs(x - x64)
        dx = np.minimum(dx, W - dx)  # (columns wrap: u = 0 and u = 1 are one meridian)
        assert np.all(dx <= W * (Q.E + 4 * 2.0 ** -24)), (f, float(dx.max()))
        assert np.all(np.abs(y - y64) <= H * (Q.E + 4 * 2.0 ** -24)), (f, float(np.abs(y - y64).max()))


# ------------------------------------------------------------------ 3. geometry that must hold exactly
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("source", SOURCES)
def test_centre_texels_land_on_the_seam_and_the_poles(source, n):
    W, H = source
    m = n // 2
    c0, c1, r0, r1, fx, fy = Q.face_taps(1, n, W, H)  # -X looks along the seam of the panorama
    assert (c0[m, m], c1[m, m]) == (W - 1, 0) and fx[m, m] == 0.5
    c0, c1, r0, r1, fx, fy = Q.face_taps(0, n, W, H)  # +X at its centre column(s)
    assert float(Q.panorama_uv(Q.face_direction(0, m, m, n))[0]) == 0.5
    for f, row in ((2, 0), (3, H - 1)):
        c0, c1, r0, r1, fx, fy = Q.face_taps(f, n, W, H)
        assert (r0[m, m], r1[m, m]) == (row, row), "the pole reads one row only"


@pytest.mark.parametrize("n", EXTENTS)
def test_a_constant_panorama_gives_constant_faces_and_chain(n):
    for W, H in SOURCES:
        rgbe = np.tile(np.array([200, 17, 96, 131], dtype=np.uint8), (H, W, 1))
        src = Q.rgbe_decode(rgbe)
        levels = Q.cube(src, n)
        assert len(levels) == n.bit_length()
        for lvl in levels:
            assert np.all(words(lvl).reshape(-1, 4) == words(src[0, 0])), (W, H, n)


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_rows_only_panorama_is_symmetric_under_a_quarter_turn(n):
    """a panorama that is a function of the row alone: the faces +Y and -Y are unchanged by a quarter turn about Y, bit for bit (the
    direction grid is exactly antisymmetric and x^2 + z^2 commutes), and the four side faces are equal, on every level.  (The
    chain of +Y / -Y is symmetric only to rounding: the blit filters along x first, and a quarter turn swaps the axes.)"""
    H, W = 32, 64
    rng = np.random.default_rng(n)
    src = np.repeat(random_panorama(rng, 1, H), W, axis=1)
    lv = Q.cube(src, n)
    for f in (2, 3):
        assert np.array_equal(words(lv[0][f]), words(np.rot90(lv[0][f])))
    for lvl in lv:
        for f in (1, 4, 5):
            assert np.array_equal(words(lvl[f]), words(lvl[0]))


# ------------------------------------------------------------------ 4. containers.parse_hdr
def hdr_file(rgbe, rle=None, magic=b"#?RADIANCE", fmt=b"32-bit_rle_rgbe", res=None, extra=b"EXPOSURE=1.0\n"):
    """rle: None = flat scanlines; else a list of (kind, length) ops ("run" | "lit") that tile the width, used for every channel"""
    h, w = rgbe.shape[:2]
    out = magic + b"\n# written by the test\n" + extra + b"FORMAT=" + fmt + b"\n\n" + (res or f"-Y {h} +X {w}".encode()) + b"\n"
    for y in range(h):
        if rle is None:
            out += rgbe[y].tobytes()
            continue
        out += bytes([2, 2, w >> 8, w & 255])
        for ch in range(4):
            x = 0
            for kind, n in rle:
                if kind == "run":
                    out += bytes([128 + n, int(rgbe[y, x, ch])])
                else:
                    out += bytes([n]) + rgbe[y, x:x + n, ch].tobytes()
                x += n
            assert x == w
    return out


def runs_image(rng, h, ops):
    """an image whose "run" stretches are constant per channel, so that the run-length file stores it exactly"""
    w = sum(n for _, n in ops)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    x = 0
    for kind, n in ops:
        if kind == "run":
            img[:, x:x + n] = img[:, x:x + 1]
        x += n
    return img


def test_parse_hdr_reads_flat_and_run_length_scanlines():
    from rend3_amd import containers as C
    rng = np.random.default_rng(2)
    for w in (7, 8, 32768):  # below the run-length limit, the lowest and one above the highest width it can encode
        img = rng.integers(0, 256, (2, w, 4), dtype=np.uint8)
        for magic in (b"#?RADIANCE", b"#?RGBE"):
            p = C.parse_hdr(hdr_file(img, magic=magic))
            assert (p["width"], p["height"]) == (w, 2) and p["rgbe"].dtype == np.uint8 and np.array_equal(p["rgbe"], img)
    ops = [("run", 1), ("lit", 1), ("run", 127), ("lit", 127), ("lit", 128), ("run", 127), ("run", 2), ("lit", 3)]
    img = runs_image(rng, 3, ops)
    assert np.array_equal(C.parse_hdr(hdr_file(img, rle=ops))["rgbe"], img)
    for w in (8, 32767):
        ops = [("run", 127)] * (w // 127) + ([("lit", w % 127)] if w % 127 else [])
        img = runs_image(rng, 1, ops)
        assert np.array_equal(C.parse_hdr(hdr_file(img, rle=ops))["rgbe"], img)
    # a flat scanline that begins 2 2 in a picture too narrow for run lengths is pixels
    img = rng.integers(0, 256, (1, 7, 4), dtype=np.uint8)
    img[0, 0] = (2, 2, 0, 7)
    assert np.array_equal(C.parse_hdr(hdr_file(img))["rgbe"], img)
    assert C.parse_hdr(b"\xabKTX 20\xbb\r\n\x1a\n" + bytes(80)) is None and C.parse_hdr(b"") is None


def test_parse_hdr_refusals():
    from rend3_amd import containers as C
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (2, 16, 4), dtype=np.uint8)
    for res in (b"+Y 2 +X 16", b"-Y 2 -X 16", b"+X 16 -Y 2", b"-X 16 +Y 2"):
        with pytest.raises(C.TextureUnsupported):
            C.parse_hdr(hdr_file(img, res=res))
    with pytest.raises(C.TextureUnsupported):
        C.parse_hdr(hdr_file(img, fmt=b"32-bit_rle_xyze"))
    for bad in (hdr_file(img, fmt=b"8-bit"), hdr_file(img, res=b"2 16"), hdr_file(img, res=b"-Y two +X 16"), hdr_file(img, res=b"-Y 0 +X 16"),
                b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", hdr_file(img)[:-1]):
        with pytest.raises(C.TextureLoadError) as info:
            C.parse_hdr(bad)
        assert not isinstance(info.value, C.TextureUnsupported)
    ops = [("run", 10), ("lit", 6)]
    img = runs_image(rng, 2, ops)
    good = hdr_file(img, rle=ops)
    assert np.array_equal(C.parse_hdr(good)["rgbe"], img)
    head = len(good) - 2 * (4 + 4 * (2 + 7))
    for bad in (good[:-1], good[:-7], good[:head + 5]):  # truncated inside a literal, inside a run, behind a scanline's header
        with pytest.raises(C.TextureLoadError):
            C.parse_hdr(bad)
    overlong = bytearray(good)
    overlong[head + 4] = 128 + 17  # the first run of the first channel: 17 > 16
    with pytest.raises(C.TextureLoadError, match="passes its end"):
        C.parse_hdr(bytes(overlong))
    overlong[head + 4] = 128 + 10
    overlong[head + 6] = 7  # the literals behind it: 10 + 7 > 16
    with pytest.raises(C.TextureLoadError, match="passes its end"):
        C.parse_hdr(bytes(overlong))
    wrong_width = bytearray(good)
    wrong_width[head + 3] = 15
    with pytest.raises(C.TextureLoadError):
        C.parse_hdr(bytes(wrong_width))


# ------------------------------------------------------------------ 5. the ABI is declared everywhere
def test_abi_is_declared_in_every_layer():
    from rend3_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    assert re.search(r"int r3n_texture_cubes_write_sources\(r3n_ctx \*ctx, const r3n_cube_source \*sources, uint32_t n_cubes, const void \*payload,\s+"
                     r"uint64_t payload_bytes\);", hdr)
    assert "#define R3N_CUBE_SOURCE_CUBE 0u" in hdr and "#define R3N_CUBE_SOURCE_EQUIRECT 1u" in hdr and "#define R3N_CUBE_ENCODING_RGBE8 0x100u" in hdr
    assert "#define R3N_TEXTURE_FORMAT_COUNT 34u" in hdr, "RGBE8 is a source encoding of this entry, not a 35th texture format"
    assert _ffi.SIGNATURES["r3n_texture_cubes_write_sources"] == (_ffi.cint, [_ffi.vp, _ffi.vp, _ffi.u32, _ffi.vp, _ffi.u64])
    s = _ffi.CubeSource
    assert ctypes.sizeof(s) == 32
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [("kind", 0), ("format", 4), ("width", 8), ("height", 12), ("face_extent", 16),
                                                                  ("mips", 20), ("offset", 24)]
    assert (_ffi.CUBE_SOURCE_CUBE, _ffi.CUBE_SOURCE_EQUIRECT, _ffi.CUBE_ENCODING_RGBE8) == (0, 1, 0x100)
    rs = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    assert "pub fn r3n_texture_cubes_write_sources(ctx: *mut r3n_ctx, sources: *const r3n_cube_source, n_cubes: u32, payload: *const c_void, " \
           "payload_bytes: u64) -> c_int;" in rs
    assert "pub struct r3n_cube_source {" in rs and "pub face_extent: u32," in rs and "pub offset: u64," in rs
    assert "pub const R3N_CUBE_SOURCE_EQUIRECT: u32 = 1;" in rs and "pub const R3N_CUBE_ENCODING_RGBE8: u32 = 0x100;" in rs.replace("256", "0x100")
    assert set(build.UNITS["equirect.hip"]) >= {"equirect.h", "equirect_rule.h", "vertex_gather.h"}
    assert {"equirect.h", "equirect_rule.h"} <= set(build.UNITS["r3n.hip"])
    hip = open(os.path.join(ROOT, "rend3_amd", "csrc", "r3n.hip")).read()
    assert '{"equirect_tail", &equirect_tail, 0, equirect_rule::TAIL_CAP, 1}' in hip
    assert f"#define R3N_EQUIRECT_TAIL_DEFAULT {Q.TAIL_DEFAULT}u" in open(os.path.join(ROOT, "rend3_amd", "csrc", "equirect.h")).read()
    lib = _ffi.lib()
    assert hasattr(lib, "r3n_texture_cubes_write_sources")
    assert lib.r3n_texture_cubes_write_sources(None, None, 0, None, 0) == -1  # (no context: refused before anything is touched)


def test_python_layer_refusals_and_viewer_flags(tmp_path):
    import argparse
    from rend3_amd import renderer as R
    from rend3_amd import scene_viewer as V
    assert all(hasattr(R.Renderer, m) for m in ("add_texture_cube_equirect", "environment_mean"))
    flags = ["--skybox", "sky.hdr", "--skybox-extent", "256", "--ambient-from-skybox", "0.5"]
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(flags))
    assert (s["skybox"], s["skybox_extent"], s["skybox_equirect"], s["ambient_from_skybox"]) == ("sky.hdr", 256, None, 0.5)
    d = V.default_settings()
    assert (d["skybox"], d["skybox_extent"], d["skybox_equirect"], d["ambient_from_skybox"]) == (None, None, None, None)
    s = V.settings_from(V.add_arguments(argparse.ArgumentParser()).parse_args(["--skybox-equirect", "pano.ktx2"]))
    assert s["skybox_equirect"] == "pano.ktx2"
    img = np.random.default_rng(1).integers(0, 256, (4, 8, 4), dtype=np.uint8)
    path = tmp_path / "sky.hdr"
    path.write_bytes(hdr_file(img))
    data, w, h, fmt = V.load_panorama(str(path))
    assert (w, h, fmt) == (8, 4, "rgbe8") and np.array_equal(data, img)

    class Recorder:  # what add_skybox asks of a renderer for a panorama
        handedness = V.RIGHT

        def add_texture_cube_equirect(self, data, width, height, fmt="rgbe8", face_extent=None, mips="maximum"):
            self.got = (np.asarray(data).copy(), width, height, fmt, face_extent, mips)
            return 3

        def set_background_texture(self, handle):
            self.background = handle

    r = Recorder()
    assert V.add_skybox(r, str(path), extent=16) == 3 and r.background == 3
    assert np.array_equal(r.got[0], img) and r.got[1:] == (8, 4, "rgbe8", 16, "maximum")

    class FacesOnly:
        handedness = V.RIGHT

    with pytest.raises(ValueError, match="panorama"):
        V.add_skybox(FacesOnly(), str(path))
    with pytest.raises(ValueError, match="one background"):
        V.build(FacesOnly(), None, None, V.default_settings(skybox=str(path), skybox_equirect=str(path)))
    with pytest.raises(ValueError, match="--ambient-from-skybox"):
        V.build(FacesOnly(), None, None, V.default_settings(ambient_from_skybox=1.0))
