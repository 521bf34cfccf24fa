"""GPU: cubes built from equirectangular panoramas by r3n_texture_cubes_write_sources (rend3_amd/csrc/equirect.hip: k_equirect_faces,
the chain kernels; k_cube_assemble behind them) against tests/equirect_reference.py -- every level of every face word for word,
under every launch plan, from RGBE8 and from decoded sources; arrays that mix stored cubes and panoramas; frames over a built cube
against frames over the same texels uploaded as Rgba32Float; refusals; the ambient helper.  The reference itself is tied down in
tests/test_equirect.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

import cube_refusals
import equirect_reference as Q
import skybox_lod_cases as cases
import skybox_lod_reference as lodref
import skybox_reference as S
from oracle import host as oh
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ERR_INVALID_ARG, ERR_STATE, ERR_CAPACITY = -1, -4, -6
RGBE8 = 0x100
EXTENTS = (1, 2, 3, 5, 64, 65)  # 64: the whole chain in the tail launch at the cap; 65: one level launch in front of it
SOURCES = [(1, 1), (2, 1), (7, 5), (130, 65)]


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def tune(r, kv):
    fn = r.lib.r3n_internal_set_tuning
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    assert fn(r.ctx, kv.encode()) == 0, r.lib.r3n_last_error(r.ctx)


def launches_of(r):
    fn = r.lib.r3n_internal_cube_source_launches  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_uint64
    return int(fn(r.ctx))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rgbe_source(W, H):
    """random RGBE bytes; where there is room, texels with exponent bytes 0, 1 and 255 and with zero mantissas"""
    rng = np.random.default_rng(W * 1000 + H)
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(100, 160, (H, W))
    flat = img.reshape(-1, 4)
    if len(flat) >= 16:
        flat[3, 3], flat[7, 3], flat[11, 3] = 0, 1, 255
        flat[5] = (0, 0, 0, 140)
        flat[13] = (255, 255, 255, 255)
        flat[-1, 3], flat[-2, 3] = 1, 0
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def f32_source(W, H):
    rng = np.random.default_rng(W * 77 + H)
    src = np.empty((H, W, 4), dtype=f32)
    src[..., :3] = (np.exp2(rng.uniform(-10, 10, (H, W, 1))) * rng.uniform(-0.2, 1.0, (H, W, 3))).astype(f32)
    src[..., 3] = rng.uniform(0, 1, (H, W)).astype(f32)
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def reference(kind, W, H, n, mips=None):
    src = Q.rgbe_decode(rgbe_source(W, H)) if kind == "rgbe" else f32_source(W, H)
    levels = Q.cube(src, n, mips)
    for lvl in levels:
        lvl.setflags(write=False)
    return levels


def check_cube(p, ci, levels, what):
    """every level and face of cube ci as the device holds it: the interior word for word, the border the texel across the edge"""
    for k, level in enumerate(levels):
        for f in range(6):
            got = p.readback_cube_face(ci, k, f)
            want, corner = lodref.bordered_face(level, f)
            assert got.dtype == np.float32 and got.shape == want.shape, (what, k, f)
            bad = (words(got) != words(want)).any(axis=2) & ~corner
            assert not bad.any(), f"{what} level {k} face {f}: {bad.sum()} texels differ, first {np.argwhere(bad)[0]}: " \
                                  f"got {got[tuple(np.argwhere(bad)[0])]}, want {want[tuple(np.argwhere(bad)[0])]}"
            assert not words(got)[corner].any(), "corner words are written as zero"


# ------------------------------------------------------------------ 1. every level and face, word for word
@pytest.mark.parametrize("source", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["rgbe", "rgba32f"])
def test_every_level_and_face(r3, kind, source):
    """six cubes in ONE call, N = 1, 2, 3, 5, 64, 65 with their full chains, from one panorama each"""
    W, H = source
    p = r3.Renderer(oh.LEFT, f32(1.0))
    for n in EXTENTS:
        if kind == "rgbe":
            p.add_texture_cube_equirect(rgbe_source(W, H), W, H, face_extent=n)
        else:
            p.add_texture_cube_equirect(f32_source(W, H), W, H, fmt=C.RGBA32F, face_extent=n)
    for ci, n in enumerate(EXTENTS):
        check_cube(p, ci, reference(kind, W, H, n), (kind, source, n))
    p.close()


def decode_level(fmt, w, h, data):
    from oracle import lib as olib
    c = olib.get().c
    src = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
    assert c.r3o_texture_level_bytes(fmt, w, h) == len(src)
    if lodref.is_float(fmt):
        out = np.zeros((h, w, 4), dtype=f32)
        assert c.r3o_texture_decode_level_f32(fmt, w, h, src.ctypes.data, out.ctypes.data) == 0
        return out
    out = np.zeros((h, w, 4), dtype=np.uint8)
    assert c.r3o_texture_decode_level(fmt, w, h, src.ctypes.data, out.ctypes.data) == 0
    srgb = fmt in (C.RGBA8_SRGB, C.BGRA8_SRGB, C.BC1_SRGB, C.BC2_SRGB, C.BC3_SRGB, C.BC7_SRGB)
    texels = np.empty((h, w, 4), dtype=f32)
    texels[..., :3] = np.asarray(S.decode_table(srgb), dtype=f32)[out[..., :3]]
    texels[..., 3] = out[..., 3].astype(f32) / f32(255.0)
    return texels


def decoded_sources():
    rng = np.random.default_rng(0xE9)
    gold = np.load(os.path.join(HERE, "golden", "bcn_float_blocks.npz"))["bc6h_uf_data"].reshape(-1, 16)
    half = (np.exp2(rng.uniform(-8, 8, (5, 7, 1))) * rng.uniform(-1.0, 1.0, (5, 7, 4))).astype(np.float16)
    return [(C.RGBA16F, 7, 5, half.tobytes()),
            (C.RGB9E5, 7, 5, rng.integers(0, 1 << 32, 35, dtype=np.uint64).astype(np.uint32).tobytes()),
            (C.BC6H_UF, 14, 7, gold[40:48].tobytes()),  # 4 x 2 blocks, both extents leave partial blocks
            (C.RGBA8_SRGB, 6, 3, rng.integers(0, 256, 72, dtype=np.uint8).tobytes()),
            (C.RGBA8, 6, 3, rng.integers(0, 256, 72, dtype=np.uint8).tobytes())]


def test_sources_through_the_decode_tables(r3):
    """one panorama each of Rgba16Float, Rgb9e5Ufloat and Bc6hRgbUfloat (an extent that is no multiple of 4), decoded by the job
    tables of the 2D path into the call's scratch block; and the two RGBA8 classes, which land in the f32 class too"""
    p = r3.Renderer(oh.LEFT, f32(1.0))
    want = []
    for fmt, w, h, data in decoded_sources():
        src = decode_level(fmt, w, h, data)
        for n in (5, 8):
            p.add_texture_cube_equirect(data, w, h, fmt=fmt, face_extent=n)
            want.append((C.FORMAT_NAMES[fmt], n, Q.cube(src, n)))
    for ci, (name, n, levels) in enumerate(want):
        check_cube(p, ci, levels, (name, n))
    assert launches_of(p) == 3 + 1 + 0 + 1 + 1, "three decode families (f32 texels, f32 blocks, RGBA8 texels), the faces, no level launch, the tail, the assemble"
    p.close()


# ------------------------------------------------------------------ 2. the same words under every plan
def test_same_words_under_every_plan(r3):
    W, H = 130, 65
    shapes = [(65, 7), (5, 3), (64, 7), (33, 2), (2, 1)]  # (N, mips): chains that end before, at and behind every threshold
    for T in (0, 1, 4, None, 64):
        p = r3.Renderer(oh.LEFT, f32(1.0))  # (a fresh context: None leaves its default)
        if T is not None:
            tune(p, f"equirect_tail={T}")
        for n, mips in shapes:
            p.add_texture_cube_equirect(rgbe_source(W, H), W, H, face_extent=n, mips=mips)
        for ci, (n, mips) in enumerate(shapes):
            check_cube(p, ci, reference("rgbe", W, H, n, mips), (T, n, mips))
        plan = Q.plan([n for n, _ in shapes], [m for _, m in shapes], Q.TAIL_DEFAULT if T is None else T)
        assert launches_of(p) == Q.plan_launches(plan) + 1, (T, plan)  # (+ k_cube_assemble; RGBE needs no decode launch)
        if T == 0:
            assert plan == {"faces": 1, "levels": 6, "tail": 0}
        if T == 64:
            assert plan == {"faces": 1, "levels": 1, "tail": 1}
        p.close()
    p = r3.Renderer(oh.LEFT, f32(1.0))
    fn = p.lib.r3n_internal_set_tuning
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    assert fn(p.ctx, b"equirect_tail=65") == ERR_INVALID_ARG, "the cap is 64: what the tail's LDS block holds"
    p.close()


# ------------------------------------------------------------------ 3. arrays that mix kinds
def all_faces(p, ci, n, mips):
    return [p.readback_cube_face(ci, k, f).copy() for k in range(mips) for f in range(6)]


def test_an_array_that_mixes_kinds(r3):
    W, H = 7, 5
    stored = [(C.BC6H_UF, 8, 4, cases.random_cube(C.BC6H_UF, 8, 4, 11)), (C.RGBA8_SRGB, 5, 3, cases.random_cube(C.RGBA8_SRGB, 5, 3, 12))]
    p = r3.Renderer(oh.LEFT, f32(1.0))
    a = p.add_texture_cube_encoded(*stored[0][:2], stored[0][3])
    b = p.add_texture_cube_equirect(rgbe_source(W, H), W, H, face_extent=5)
    c = p.add_texture_cube_encoded(*stored[1][:2], stored[1][3])
    d = p.add_texture_cube_equirect(rgbe_source(130, 65), 130, 65, face_extent=65, mips=3)
    e = p.add_texture_cube(np.random.default_rng(3).integers(0, 256, (6, 4, 4, 4), dtype=np.uint8), srgb=True)
    check_cube(p, b, reference("rgbe", W, H, 5), "N 5 between stored cubes")
    check_cube(p, d, reference("rgbe", 130, 65, 65, 3), "N 65, three levels")
    mixed = [all_faces(p, a, 8, 4), all_faces(p, c, 5, 3), all_faces(p, e, 4, 1)]
    # the stored cubes alone, through r3n_texture_cubes_write_encoded
    q = r3.Renderer(oh.LEFT, f32(1.0))
    q.add_texture_cube_encoded(*stored[0][:2], stored[0][3])
    q.add_texture_cube_encoded(*stored[1][:2], stored[1][3])
    q.add_texture_cube(p.cubes[e][0], srgb=True)
    alone = [all_faces(q, 0, 8, 4), all_faces(q, 1, 5, 3), all_faces(q, 2, 4, 1)]
    for m, o in zip(mixed, alone):
        assert all(x.dtype == y.dtype and np.array_equal(words(x), words(y)) for x, y in zip(m, o))
    # and an array of stored cubes only gives the same words and descriptors through either entry
    q._flush_cubes_sources()
    again = [all_faces(q, 0, 8, 4), all_faces(q, 1, 5, 3), all_faces(q, 2, 4, 1)]
    for m, o in zip(again, alone):
        assert all(x.dtype == y.dtype and np.array_equal(words(x), words(y)) for x, y in zip(m, o))
    assert launches_of(q) == 2 + 1, "two decode families and the assemble: nothing of the equirect path is launched"
    p.close()
    q.close()


# ------------------------------------------------------------------ 4. frames
@pytest.mark.parametrize("hand", [oh.LEFT, oh.RIGHT], ids=["left", "right"])
def test_frames_equal_those_over_the_uploaded_texels(r3, hand):
    """a skybox frame over the built cube is the frame over the reference's faces and chain uploaded as Rgba32Float through
    r3n_texture_cubes_write_encoded, bit for bit: a camera that minifies (several levels of the chain) and one that magnifies"""
    W, H, n = 130, 65, 64
    w, h = 64, 48
    levels = reference("rgbe", W, H, n)
    a, b = r3.Renderer(hand, f32(w) / f32(h)), r3.Renderer(hand, f32(w) / f32(h))
    a.set_background_texture(a.add_texture_cube_equirect(rgbe_source(W, H), W, H, face_extent=n))
    b.set_background_texture(b.add_texture_cube_encoded(C.RGBA32F, n, [[np.ascontiguousarray(lvl[f]).tobytes() for lvl in levels] for f in range(6)]))
    for fa, fb in zip(all_faces(a, 0, n, len(levels)), all_faces(b, 0, n, len(levels))):
        assert np.array_equal(words(fa), words(fb))
    look = oh.look_at_lh if hand == oh.LEFT else oh.look_at_rh
    differ = []
    for target, fov in (((-1.0, 0.4, -0.7), 170.0), ((0.3, 1.0, 0.2), 100.0), ((1.0, -0.2, 0.9), 12.0)):
        for r in (a, b):
            r.set_camera_data(look((0, 0, 0), target, (0, 1, 0)), ("perspective", fov, 0.1))
        for samples in (1, 4):
            fa, fb = a.render(w, h, samples=samples), b.render(w, h, samples=samples)
            assert np.array_equal(fa["hdr16"], fb["hdr16"]) and np.array_equal(fa["rgba8"], fb["rgba8"]), (target, fov, samples)
            differ.append(len(np.unique(fa["hdr16"].reshape(-1, 4), axis=0)))
    assert min(differ) > 100, "the frames show the panorama"
    a.close()
    b.close()


def test_refusals_leave_everything_unchanged(r3):
    from rend3_amd import _ffi
    from rend3_amd.renderer import BaseRenderGraph, BaseRenderGraphInputs, BaseRenderGraphSettings, RenderGraph
    w, h = 16, 12
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    lib, ctx = p.lib, p.ctx
    p.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
    p.add_texture_cube_encoded(C.RGBA8_SRGB, 4, cases.random_cube(C.RGBA8_SRGB, 4, 3, 2))
    p.set_background_texture(p.add_texture_cube_equirect(rgbe_source(7, 5), 7, 5, face_extent=8))
    base = p.render(w, h)
    kept = [(0, 0), (0, 2), (1, 0), (1, 3)]
    before = [p.readback_cube_face(ci, k, 3).copy() for ci, k in kept]
    payload = np.zeros(cube_refusals.PAYLOAD_BYTES, dtype=np.uint8)

    def write(kind=1, fmt=RGBE8, width=8, height=4, extent=4, mips=1, offset=0, payload_bytes=len(payload), n=1, null=False):
        src = (_ffi.CubeSource * n)(*[_ffi.CubeSource(kind, fmt, width, height, extent, mips, offset)] * n)
        return lib.r3n_texture_cubes_write_sources(ctx, None if null else ctypes.addressof(src), n, _ffi.ptr(payload), payload_bytes)

    # the rows of tests/cube_refusals.py, which tests/test_cube_plan.py sends to the planner on the CPU: code AND message
    refusals = []
    for row in cube_refusals.SOURCES:
        cubes = cube_refusals.source_cubes(row)
        src = (_ffi.CubeSource * len(cubes))(*[_ffi.CubeSource(*cube) for cube in cubes])
        code = lib.r3n_texture_cubes_write_sources(ctx, ctypes.addressof(src), len(cubes), _ffi.ptr(payload), row[2])
        assert lib.r3n_last_error(ctx).decode() == "texture cubes write (sources): " + row[4], row[0]
        refusals.append((row[0], code, row[3]))
    refusals.append(("null", write(null=True), ERR_INVALID_ARG))
    assert len(refusals) >= 20
    for what, code, want in refusals:
        assert code == want, f"{what}: {code}"
    assert all(np.array_equal(words(x), words(p.readback_cube_face(ci, k, 3))) for x, (ci, k) in zip(before, kept))
    after = p.render(w, h)
    assert np.array_equal(base["hdr16"], after["hdr16"]) and np.array_equal(base["rgba8"], after["rgba8"]), "the array and the binding are what they were"

    # inside a frame: R3N_ERR_STATE
    codes = {}
    ev = p.evaluate_instructions()
    graph_base = BaseRenderGraph(p)
    graph = RenderGraph()
    graph_base.add_to_graph(graph, BaseRenderGraphInputs(ev, graph_base.default_routines(), (w, h), 1), BaseRenderGraphSettings((0, 0, 0, 0), (0, 0, 1, 1)))
    names = [name for name, _ in graph.nodes]
    graph.nodes.insert(names.index("Skybox"), ("probe", lambda r, _ev: codes.__setitem__("in frame", write())))
    graph.execute(p, ev)
    assert codes == {"in frame": ERR_STATE}
    assert np.array_equal(p.readback_frame(ev, w, h)["hdr16"], base["hdr16"])

    # replacing the array unbinds a cube that left it: cube 1 is bound, the new array has one cube
    assert write() == 0
    assert lib.r3n_skybox_set(ctx, 2) == ERR_INVALID_ARG
    clear = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (clear["hdr16"] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all(), "the vanished cube was unbound"
    p.close()


# ------------------------------------------------------------------ 5. the ambient helper and the viewer's way in
def test_environment_mean_and_the_viewer(r3, tmp_path):
    from rend3_amd import scene_viewer as V
    from test_equirect import hdr_file
    W, H = 130, 65
    p = r3.Renderer(oh.RIGHT, f32(1.0))
    path = tmp_path / "sky.hdr"
    path.write_bytes(hdr_file(np.array(rgbe_source(W, H))))
    sky = V.add_skybox(p, str(path))  # the default extent: half the panorama's height
    assert p.cubes[sky].width == 32 and p.cubes[sky].mips == 6
    levels = reference("rgbe", W, H, 32)
    check_cube(p, sky, levels, "through the viewer")
    mean = p.environment_mean(sky)
    assert mean.dtype == np.float32 and np.array_equal(words(mean), words(Q.environment_mean(levels)))
    finite = p.add_texture_cube_equirect(f32_source(7, 5), 7, 5, fmt=C.RGBA32F, face_extent=5)
    assert np.array_equal(words(p.environment_mean(finite)), words(Q.environment_mean(reference("rgba32f", 7, 5, 5))))
    short = p.add_texture_cube_equirect(rgbe_source(7, 5), 7, 5, face_extent=8, mips=2)
    with pytest.raises(ValueError):
        p.environment_mean(short)
    p.close()
