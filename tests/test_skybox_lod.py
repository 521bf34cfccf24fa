"""Cubes with mip chains and float texels without a GPU: the numpy reference of the contract (tests/skybox_lod_reference.py)
against the one-level reference and against hand-written expectations, the coverage of the GPU file's cases, the KTX2 / DDS cube
readers, add_texture_cube_encoded's validation, the ABI tables, and csrc/cube_faces.h through tests/cube_faces_check.cpp -- a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process.  The GPU side is
tests/test_skybox_lod_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import host_check
import skybox_lod_cases as cases
import skybox_lod_reference as lodref
import skybox_reference as sky
from rend3_amd import containers as C

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")


# ------------------------------------------------------------------ the reference against the one-level reference
@pytest.mark.parametrize("n,srgb", [(1, True), (2, False), (5, True), (16, False)])
def test_one_level_equals_the_level_0_reference(n, srgb):
    rng = np.random.default_rng(40 + n)
    texels = rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8)
    fmt = C.RGBA8_SRGB if srgb else C.RGBA8
    levels = lodref.decode_cube(fmt, n, [[texels[f].tobytes()] for f in range(6)])
    assert np.array_equal(levels[0], texels)
    d = rng.normal(size=(4000, 3)).astype(f32)
    d[:8] = [(1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, -1)]  # the corners
    zero = np.zeros(len(d), dtype=np.int64)
    got = lodref.sample(levels, fmt, d, zero, np.zeros(len(d), dtype=f32))
    assert np.array_equal(got.view(np.uint32), sky.sample(texels, srgb, d).view(np.uint32))
    # and as a frame: select_level gives level 0 for a one-level cube whatever the camera is
    name, _, _, (w, h), hand, view, proj = cases.frame_cases()[4]
    inv = cases.inverse_matrix(hand, view, proj, w, h)
    assert np.array_equal(lodref.sky_frame(levels, fmt, inv, w, h), sky.sky_frame(texels, srgb, inv, w, h)), name


# ------------------------------------------------------------------ hand-written expectations
def flat_matrix(a):
    """inv_origin_view_proj that sends clip (cx, cy, 1, 1) to the world point (a * cx, a * cy, 1): the +Z face, s = 0.5 * a * cx + 0.5,
    so one pixel of a W-wide target is a / W of the face -- N * a / W texels (column-major, like the frame uniforms)"""
    m = np.zeros(16, dtype=f32)
    m[0], m[5], m[8 + 2], m[12 + 3] = a, a, 1.0, 1.0
    return m


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_constant_levels_identify_level_and_fraction(k):
    """level k of the cube is the colour (k, 0, 0): the sampled red IS level + frac.  A footprint of 1.5 * 2^k texels per pixel
    must give level k and frac 0.5 -- away from the powers of two, where rounding would decide the level"""
    n, w = 128, 4
    faces = cases.constant_level_cube(n, 7, lambda level: float(level))
    levels = lodref.decode_cube(C.RGBA16F, n, faces)
    a = 1.5 * 2.0 ** k * w / n
    assert a * (1.0 + 1.0 / w) < 1.0, "the neighbours of every pixel (clip x, y up to 1 + 1 / w) stay on the +Z face"
    inv = flat_matrix(a)
    ys, xs = np.mgrid[0:w, 0:w]
    d, level, frac, unbounded, rho = lodref.select_level(inv, w, w, xs.reshape(-1), ys.reshape(-1), n, 7)
    assert (sky.select_face(d)[0] == 4).all() and not unbounded.any()
    assert (level == k).all()
    assert np.abs(frac - 0.5).max() < 1e-3 and np.abs(rho - 1.5 * 2.0 ** k).max() < 1e-3 * 2.0 ** k
    frame = lodref.sky_frame(levels, C.RGBA16F, inv, w, w).view(np.float16).astype(f32)
    assert np.abs(frame[..., 0] - (k + 0.5)).max() < 2e-3  # (1e-3 of the fraction, and the rounding to half of a value below 8)
    assert (frame[..., 1] == 0).all() and (frame[..., 3] == 1).all()


def test_clamp_unbounded_and_one_level():
    n, w = 64, 4
    faces = cases.constant_level_cube(n, 3, lambda level: float(level))  # a partial chain: levels 0 .. 2
    levels = lodref.decode_cube(C.RGBA16F, n, faces)
    ys, xs = np.mgrid[0:w, 0:w]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    # 12 texels per pixel asks for level 3.58: clamped at level 2, frac 0
    inv = flat_matrix(12.0 * w / n)
    _, level, frac, unbounded, _ = lodref.select_level(inv, w, w, xs, ys, n, 3)
    assert (level == 2).all() and (frac == 0).all() and not unbounded.any()
    assert (lodref.sky_frame(levels, C.RGBA16F, inv, w, w)[..., 0] == np.float16(2.0).view(np.uint16)).all()
    # a matrix that turns the +x neighbour of the last column behind +Z's axis: z = 1 - 0.9 * cx, cx = 1.25 there
    m = flat_matrix(0.1)
    m[2] = -0.9
    d, level, frac, unbounded, _ = lodref.select_level(m, w, w, xs, ys, n, 3)
    assert (sky.select_face(d)[0] == 4).all()
    assert np.array_equal(unbounded, xs == w - 1)
    assert (level[unbounded] == 2).all() and (frac[unbounded] == 0).all()
    # one level: level 0 whatever the gradients are
    _, level, frac, unbounded, _ = lodref.select_level(m, w, w, xs, ys, n, 1)
    assert not level.any() and not frac.any() and not unbounded.any()


# ------------------------------------------------------------------ the GPU file's cases reach every path
def test_frame_cases_reach_every_path():
    reached = {p: [] for p in lodref.PATHS}
    for name, n, mips, (w, h), hand, view, proj in cases.frame_cases():
        mips = mips or cases.full_chain(n)
        paths = lodref.classify(cases.inverse_matrix(hand, view, proj, w, h), w, h, n, mips)
        for p, m in paths.items():
            if m.any():
                reached[p].append(name)
    assert all(reached[p] for p in lodref.PATHS), {p: v for p, v in reached.items() if not v}
    # the cases the issue names
    by_name = {c[0]: c for c in cases.frame_cases()}
    name, n, mips, (w, h), hand, view, proj = by_name["behind the axis"]
    assert (w, h) == (2, 2)
    assert lodref.classify(cases.inverse_matrix(hand, view, proj, w, h), w, h, n, cases.full_chain(n))["unbounded"].any()
    assert by_name["N 64 on 8 x 8"][1:4] == (64, 0, (8, 8))
    assert {c[1] for c in cases.frame_cases()} >= {1, 2, 3, 4, 5, 8, 16, 64}
    sizes = [c[3] for c in cases.frame_cases()]
    assert min(sizes) == (2, 2) and max(sizes) == (64, 48)


# ------------------------------------------------------------------ the cube readers
def small_cube(fmt, n=5, mips=3, seed=9):
    return cases.random_cube(fmt, n, mips, seed)


@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_cube_files_round_trip(fmt):
    faces = small_cube(fmt)
    srgb = fmt in lodref.SRGB_FORMATS
    for data, parse, other in ((cases.write_ktx2_cube(fmt, 5, faces), C.parse_ktx2_cube, C.parse_dds_cube),
                               (cases.write_dds_cube(fmt, 5, faces), C.parse_dds_cube, C.parse_ktx2_cube)):
        got = parse(data, srgb)
        assert got["format"] == fmt and got["width"] == 5
        assert got["faces"] == faces
        assert other(data, srgb) is None  # not that container
    # the 2D readers keep refusing cubes: a material cannot use one
    with pytest.raises(C.TextureUnsupported):
        C.parse_ktx2(cases.write_ktx2_cube(fmt, 5, faces), srgb)
    with pytest.raises(C.TextureUnsupported):
        C.parse_dds(cases.write_dds_cube(fmt, 5, faces), srgb)


def test_legacy_dds_cube_and_srgb_flag():
    for fmt in (C.RGBA8_SRGB, C.BC1):
        faces = small_cube(fmt, 4, 2)
        got = C.parse_dds_cube(cases.write_dds_cube(fmt, 4, faces, dx10=False), fmt == C.RGBA8_SRGB)
        assert got == {"format": fmt, "width": 4, "faces": faces}
    # sRGB-ness follows the use, not the file: the same bytes read as the linear format
    faces = small_cube(C.RGBA8_SRGB, 4, 1)
    assert C.parse_ktx2_cube(cases.write_ktx2_cube(C.RGBA8_SRGB, 4, faces), False)["format"] == C.RGBA8
    assert C.parse_dds_cube(cases.write_dds_cube(C.RGBA8_SRGB, 4, faces), False)["format"] == C.RGBA8


def test_cube_file_refusals():
    fmt = C.BC6H_UF
    faces = small_cube(fmt, 4, 2)
    ktx = lambda **kw: cases.write_ktx2_cube(fmt, 4, faces, **kw)  # noqa: E731
    dds = lambda **kw: cases.write_dds_cube(fmt, 4, faces, **kw)   # noqa: E731
    unsupported = [
        (C.parse_ktx2_cube, cases.write_ktx2_cube(fmt, 4, faces[:1], face_count=1)),   # a 2D texture
        (C.parse_ktx2_cube, cases.write_ktx2_cube(fmt, 4, faces[:3], face_count=3)),   # a partial cube
        (C.parse_ktx2_cube, ktx(layers=2)),                                            # an array of cubes
        (C.parse_ktx2_cube, ktx(scheme=2)),                                            # supercompression
        (C.parse_ktx2_cube, ktx(height=8)),                                            # not square
        (C.parse_dds_cube, dds(caps2=0x200 | 0x400 | 0x800)),                          # a partial cube
        (C.parse_dds_cube, dds(array_size=2)),                                         # an array of cubes
        (C.parse_dds_cube, dds(misc=0, caps2=0)),                                      # no cube flag
        (C.parse_dds_cube, dds(height=8)),                                             # not square
        (C.parse_dds_cube, cases.write_dds_cube(C.RGBA8, 4, small_cube(C.RGBA8, 4, 1), dx10=False, caps2=0)),  # legacy, no cube caps
    ]
    for parse, data in unsupported:
        with pytest.raises(C.TextureUnsupported):
            parse(data, False)
    # the error kinds of the 2D readers
    bad = bytearray(ktx())
    bad[12:16] = (0x7FFFFFF0).to_bytes(4, "little")
    with pytest.raises(C.TextureLoadError) as e:
        C.parse_ktx2_cube(bytes(bad), False)
    assert e.value.kind == "TextureBadKxt2Format"
    bad = bytearray(ktx())
    bad[12:16] = (152).to_bytes(4, "little")  # an ETC2 format
    with pytest.raises(C.TextureUnsupported):
        C.parse_ktx2_cube(bytes(bad), False)
    bad = bytearray(ktx())
    bad[12 + 7 * 4:12 + 8 * 4] = (0).to_bytes(4, "little")
    with pytest.raises(C.TextureLoadError) as e:
        C.parse_ktx2_cube(bytes(bad), False)
    assert e.value.kind == "TextureZeroLevels"
    bad = bytearray(ktx())
    bad[80 + 8:80 + 16] = (17).to_bytes(8, "little")  # level 0's byte length
    with pytest.raises(C.TextureLoadError) as e:
        C.parse_ktx2_cube(bytes(bad), False)
    assert e.value.kind == "TextureDecode"
    assert C.parse_ktx2_cube(ktx()[:-1], False) is None  # truncated: the reader fails
    bad = bytearray(dds())
    bad[128:132] = (200).to_bytes(4, "little")
    with pytest.raises(C.TextureLoadError) as e:
        C.parse_dds_cube(bytes(bad), False)
    assert e.value.kind == "TextureBadDxgiFormat"
    with pytest.raises(C.TextureLoadError) as e:
        C.parse_dds_cube(dds()[:-1], False)
    assert e.value.kind == "TextureTooManyLayers"
    assert C.parse_dds_cube(b"nothing", False) is None and C.parse_ktx2_cube(b"nothing", False) is None


# ------------------------------------------------------------------ the host API without a context
def test_add_texture_cube_encoded_validates():
    from rend3_amd.renderer import Renderer, _EncodedCube
    r = Renderer.__new__(Renderer)  # no context: the method only edits the host-side array
    r.cubes, r._cubes_dirty, r._background = [], False, None
    faces = small_cube(C.BC7_SRGB, 5, 3)
    assert r.add_texture_cube_encoded(C.BC7_SRGB, 5, faces) == 0
    assert r.add_texture_cube(np.zeros((6, 2, 2, 4), dtype=np.uint8)) == 1
    assert isinstance(r.cubes[0], _EncodedCube) and r.cubes[0].mips == 3 and r._cubes_dirty
    bad = [
        (C.FORMAT_COUNT, 5, faces),                                   # an unknown format
        (C.BC7_SRGB, 0, faces), (C.BC7_SRGB, 16385, faces),           # the extent
        (C.BC7_SRGB, 5, faces[:5]),                                   # five faces
        (C.BC7_SRGB, 5, [f[:2] for f in faces[:5]] + [faces[5]]),     # faces with different level counts
        (C.BC7_SRGB, 5, [f + [f[2]] for f in faces]),                 # more levels than 5 has
        (C.BC7_SRGB, 5, [[] for _ in range(6)]),                      # no level
        (C.BC7_SRGB, 5, [[f[0][:-1]] + f[1:] for f in faces]),        # a short level
        (C.RGBA8, 5, faces),                                          # the byte counts of another format
    ]
    for fmt, width, fs in bad:
        with pytest.raises(ValueError):
            r.add_texture_cube_encoded(fmt, width, fs)
    assert len(r.cubes) == 2


def test_abi_tables_name_the_new_entries():
    from rend3_amd import _ffi
    header = open(os.path.join(ROOT, "include", "r3n.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rend3-amd-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("r3n_texture_cubes_write_encoded", "r3n_readback_cube_face"):
        assert f"int {name}(" in header and f"pub fn {name}(" in rust and name in integration
        assert f'"{name}"' in open(_ffi.__file__).read()


# ------------------------------------------------------------------ csrc/cube_faces.h alone, under the sanitizers
SRC = os.path.join(HERE, "cube_faces_check.cpp")
HEADER = os.path.join(ROOT, "rend3_amd", "csrc", "cube_faces.h")
# Every entry's borders come from this table (k_cube_assemble), so this comparison is the one tie between it and resolve_texel:
# every extent a test sends through the plain entry -- 4 (test_skybox.py's constant cubes, the viewer's PNG faces,
# test_equirect_gpu.py, test_resources_gpu.py), 1, 2, 7, 8, 16, 64 (test_skybox.py), 7, 2 and 1, 3, 4, 5 (test_skybox_lod_gpu.py)
# -- beside the smallest ones and one above 64 that is no power of two
EXTENTS = (1, 2, 3, 4, 5, 7, 8, 16, 64, 100)


def expected_sources(n):
    """per face, per position of the bordered face: the id of the texel resolve_texel names, -1 at the corners"""
    out = []
    for f in range(6):
        ids = np.arange(6 * n * n, dtype=np.int64).reshape(6, n, n, 1)
        face, corner = lodref.bordered_face(ids, f)
        out.append(np.where(corner, -1, face[..., 0]).reshape(-1))
    return np.concatenate(out)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = host_check.program(SRC, [HEADER])
    table = tmp_path_factory.mktemp("cube_faces") / "table.txt"
    with open(table, "w") as f:
        for n in EXTENTS:
            f.write(f"n {n}\n" + " ".join(str(int(v)) for v in expected_sources(n)) + "\n")
    res = subprocess.run([exe, str(table)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # a sanitizer report goes there
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(" ")
        assert name not in lines and name != "FAIL", line
        lines[name] = rest
    return lines


def test_faces_assemble_as_the_reference_resolves_them(printed):
    for n in EXTENTS:
        assert printed[f"extent_{n}"] == "0"
    # the table is not vacuous: every face borrows from four other faces, reversed runs included
    ids = expected_sources(5).reshape(6, 7, 7)
    for f in range(6):
        others = {int(v) // 25 for v in np.concatenate([ids[f, 0, 1:-1], ids[f, -1, 1:-1], ids[f, 1:-1, 0], ids[f, 1:-1, -1]])}
        assert len(others) == 4 and f not in others and (f ^ 1) not in others
    assert (ids[:, [0, 0, -1, -1], [0, -1, 0, -1]] == -1).all()


def test_pool_layout(printed):
    """level k's six bordered faces behind level k - 1's, every level on a 4-word boundary (skybox.h)"""
    for n, mips, per in ((1, 1, 1), (1, 1, 4), (3, 2, 1), (5, 3, 4), (8, 4, 1), (64, 7, 4), (16384, 15, 1)):
        want, at = [], 0
        for k in range(mips + 1):
            want.append(at)
            at += (6 * (max(1, n >> k) + 2) ** 2 * per + 3) & ~3
        assert [int(v) for v in printed[f"layout_{n}_{mips}_{per}"].split()] == want


# ------------------------------------------------------------------ the viewer's flag
def test_viewer_skybox_takes_a_cube_file(tmp_path):
    """--skybox FILE.ktx2 | FILE.dds: build() reads the file with the cube readers and hands format, width and faces over; a file
    that is neither container is an error, not a skipped sky"""
    from rend3_amd import scene_viewer as sv
    faces = cases.random_cube(C.BC6H_UF, 8, 4, 3)
    calls = []

    class Stop(Exception):
        pass

    class R:
        handedness = sv.RIGHT

        def add_texture_cube_encoded(self, fmt, width, fs):
            calls.append((fmt, width, fs == faces))
            return 2

        def set_background_texture(self, handle):
            calls.append(("bind", handle))
            raise Stop

    for name, data in (("a.ktx2", cases.write_ktx2_cube(C.BC6H_UF, 8, faces)), ("b.dds", cases.write_dds_cube(C.BC6H_UF, 8, faces))):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(Stop):
            sv.build(R(), None, None, sv.default_settings(file="unused.glb", skybox=str(tmp_path / name)))
    assert calls == [(C.BC6H_UF, 8, True), ("bind", 2)] * 2
    (tmp_path / "c.bin").write_bytes(b"neither")
    with pytest.raises(ValueError):
        sv.build(R(), None, None, sv.default_settings(file="unused.glb", skybox=str(tmp_path / "c.bin")))
