"""Cube textures of any format with their mip chains on the GPU: r3n_texture_cubes_write_encoded (decode jobs + k_cube_assemble,
rend3_amd/csrc/cube_faces.hip), r3n_readback_cube_face, and the skybox node's level selection and trilinear filter
(rend3_amd/csrc/skybox.hip).  The judge is tests/skybox_lod_reference.py -- texels from the oracle's decoders, the contract of
DESIGN.md section 2 in numpy -- and, where geometry is in the frame, the oracle through the identity of tests/test_skybox.py: at
pixel p a frame with a skybox equals the oracle's frame with clear_color = sky(p).  The cases and their coverage of every path of
the sampler are shared with, and proven by, tests/test_skybox_lod.py."""
import numpy as np
import pytest

import cube_refusals
import scenes
import skybox_lod_cases as cases
import skybox_lod_reference as lodref
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
AMBIENT = (0.1, 0.1, 0.1, 1.0)
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, ERR_CAPACITY = -1, -4, -5, -6


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def fmt_id(fmt):
    return C.FORMAT_NAMES[fmt]


# ------------------------------------------------------------------ 1. bordered faces
@pytest.mark.parametrize("fmt", cases.FORMATS, ids=fmt_id)
def test_bordered_faces(r3, fmt):
    """seven cubes in ONE call -- N = 1, 2, 3, 4, 5, 8, 16 with their full chains (3 and 5 leave partial blocks) -- and every level
    of every face word for word: the interior from the oracle's decoder, the border from resolve_texel.  Corner words excluded."""
    p = r3.Renderer(oh.LEFT, f32(1.0))
    cubes = []
    for n in (1, 2, 3, 4, 5, 8, 16):
        faces = cases.random_cube(fmt, n, cases.full_chain(n), 100 * fmt + n)
        assert p.add_texture_cube_encoded(fmt, n, faces) == len(cubes)
        cubes.append((n, lodref.decode_cube(fmt, n, faces)))
    for ci, (n, levels) in enumerate(cubes):
        for k, level in enumerate(levels):
            for f in range(6):
                got = p.readback_cube_face(ci, k, f)
                want, corner = lodref.bordered_face(level, f)
                if lodref.is_float(fmt):
                    assert got.dtype == np.float32 and got.shape == want.shape
                    g, w = got.view(np.uint32), want.view(np.uint32)
                else:
                    assert got.dtype == np.uint32 and got.shape == corner.shape
                    g, w = got, np.ascontiguousarray(want).view(np.uint32)[..., 0]
                bad = (g != w).reshape(corner.shape + (-1,)).any(axis=2) & ~corner
                assert not bad.any(), f"{fmt_id(fmt)} N {n} level {k} face {f}: {bad.sum()} texels differ, first {np.argwhere(bad)[0]}"
                assert not g.reshape(corner.shape + (-1,))[corner].any(), "corner words are written as zero"
    p.close()


# ------------------------------------------------------------------ 2. frames over an empty world
def render_cases(r3, fmt, nonfinite=False):
    """every frame case, one and four samples, against the reference: all cubes of a handedness in one array, bound in turn"""
    all_cases = cases.frame_cases()
    cubes = []
    for k, (name, n, mips, size, hand, view, proj) in enumerate(all_cases):
        mips = mips or cases.full_chain(n)
        faces = cases.random_cube(fmt, n, mips, 7000 + 10 * fmt + k, nonfinite)
        cubes.append((faces, lodref.decode_cube(fmt, n, faces)))
    nan_pixels = 0
    for hand in (oh.LEFT, oh.RIGHT):
        p = r3.Renderer(hand, f32(1.0))
        for (name, n, mips, size, *_), (faces, _) in zip(all_cases, cubes):
            p.add_texture_cube_encoded(fmt, n, faces)
        for k, (name, n, mips, (w, h), case_hand, view, proj) in enumerate(all_cases):
            if case_hand != hand:
                continue
            levels = cubes[k][1]
            p.aspect_ratio = f32(w) / f32(h)
            p.set_background_texture(k)
            p.set_camera_data(view, proj)
            inv = cases.inverse_matrix(hand, view, proj, w, h)
            want = lodref.sky_frame(levels, fmt, inv, w, h)
            nan_ok = lodref.may_be_nan(levels, fmt, inv, w, h) if nonfinite else np.zeros((h, w), dtype=bool)
            for samples in (1, 4):
                got = p.render(w, h, samples=samples, clear_color=(0.3, 0.3, 0.3, 1.0))["hdr16"]
                both_nan = np.isnan(want.view(np.float16)) & np.isnan(got.view(np.float16)) & nan_ok[..., None]
                bad = ((want != got) & ~both_nan).any(axis=2)
                assert not bad.any(), (f"{fmt_id(fmt)} '{name}' samples {samples}: {bad.sum()} of {w * h} px differ, first {np.argwhere(bad)[0]}: "
                                       f"want {want[tuple(np.argwhere(bad)[0])]}, got {got[tuple(np.argwhere(bad)[0])]}")
            nan_pixels += int(np.isnan(want.view(np.float16)).any(axis=2).sum())
        p.close()
    return nan_pixels


@pytest.mark.parametrize("fmt", cases.FORMATS, ids=fmt_id)
def test_frames_over_an_empty_world(r3, fmt):
    """nothing but sky: hdr16 equals the reference bit for bit at every pixel of every case -- level 0, two levels, the clamp, the
    unbounded footprint of the 2 x 2 target, edges and corners above level 0, levels of extent 1, N = 64 on 8 x 8"""
    render_cases(r3, fmt)


def test_frames_of_a_cube_that_holds_inf_and_nan(r3):
    """an Rgba16Float cube with +-inf and NaN texels: NaN-for-NaN equality where the REFERENCE says a pixel may be NaN (a footprint
    texel that is not finite), bit equality everywhere else"""
    assert render_cases(r3, C.RGBA16F, nonfinite=True) > 0, "the case needs NaN pixels"


# ------------------------------------------------------------------ 3. geometry and blend objects in front of a mipped float cube
@pytest.mark.parametrize("samples,hand", [(1, oh.LEFT), (4, oh.RIGHT)])
def test_mipped_float_cube_with_geometry(r3, samples, hand):
    """no sample on the sky -> the oracle's frame; sky alone, nothing blended over it -> the reference; shared with geometry or
    blended over -> the oracle rendered with clear_color = sky(p) (a sample of such pixels)"""
    w, h, n = 160, 96, 256
    aspect = f32(w) / f32(h)
    mips = cases.full_chain(n)
    rng = np.random.default_rng(31 + samples)
    faces = [[(rng.random((max(1, n >> k) ** 2, 4)) * 4.0).astype(np.float16).tobytes() for k in range(mips)] for _ in range(6)]
    levels = lodref.decode_cube(C.RGBA16F, n, faces)
    o, p = OracleRenderer(hand, aspect), r3.Renderer(hand, aspect)
    zs = 1.0 if hand == oh.LEFT else -1.0
    look = oh.look_at_lh if hand == oh.LEFT else oh.look_at_rh
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 80, 0xC0FFEE, handedness=hand, lights=1, with_cutout=True)
        hs = scenes.add_blend_objects(r, oh, mk, 0xB1E2D)
        if hand == oh.RIGHT:  # the blend objects are laid out in front of a camera that looks down +z
            for k, hnd in enumerate(hs):
                r.set_object_transform(hnd, oh.mat4_mul(oh.translation((-5.0 + k, 0.5 + 0.2 * k, zs * (4.0 + k))), oh.scale((1.5, 1.5, 0.3))))
        r.set_camera_data(look((-1.0, 1.5, zs * -3.0), (1.0, 1.0, zs * 8.0), (0, 1, 0)), ("perspective", 75.0, 0.1))
    p.set_background_texture(p.add_texture_cube_encoded(C.RGBA16F, n, faces))
    base_clear = (0.25, 0.5, 0.75, 1.0)
    fo = o.render(w, h, samples=samples, ambient=AMBIENT, clear_color=base_clear)
    fp = p.render(w, h, samples=samples, ambient=AMBIENT, clear_color=base_clear)
    assert np.array_equal(fo["vis"], fp["vis"])
    assert len(fo["blend_list"][0]) > 0
    depth = (fp["vis"] >> np.uint64(32)).astype(np.uint32).view(f32)
    takes = f32(0.0) >= depth
    n_sky = takes.astype(int) if takes.ndim == 2 else takes.sum(axis=2)
    inv = oh.mat4_inverse(o.camera.origin_view_proj)
    want = lodref.sky_frame(levels, C.RGBA16F, inv, w, h)
    paths = lodref.classify(inv, w, h, n, mips)
    none = n_sky == 0
    unblended = (fo["hdr16"] == np.array(base_clear, dtype=np.float16).view(np.uint16)).all(axis=2)
    alone = (n_sky == samples) & unblended
    rest = ~none & ~alone
    assert none.sum() > 500 and alone.sum() > 500 and rest.sum() >= 16, (none.sum(), alone.sum(), rest.sum())
    assert (paths["two levels"] & alone).sum() > 200, "the sky of this case must blend two levels"
    assert np.array_equal(fo["hdr16"][none], fp["hdr16"][none]), "pixels without sky differ from the oracle"
    bad = (want != fp["hdr16"]).any(axis=2) & alone
    assert not bad.any(), f"{bad.sum()} of {alone.sum()} sky px differ from the reference, first {np.argwhere(bad)[0]}"
    pick = np.argwhere(rest)
    pick = pick[np.random.default_rng(5).permutation(len(pick))[:16]]
    shared = 0
    for y, x in pick:
        sp = want[y, x].view(np.float16).astype(f32)
        fq = o.render(w, h, samples=samples, ambient=AMBIENT, clear_color=tuple(float(v) for v in sp))
        shared += 0 < n_sky[y, x] < samples
        assert np.array_equal(fq["hdr16"][y, x], fp["hdr16"][y, x]), f"pixel ({x}, {y}), {n_sky[y, x]} sky samples: {fq['hdr16'][y, x]} != {fp['hdr16'][y, x]}"
        assert np.abs(fq["rgba8"][y, x].astype(int) - fp["rgba8"][y, x].astype(int)).max() <= 1
    if samples == 4:
        assert shared > 0, "no pixel shared by sky and geometry among the sampled ones"
    p.close()


# ------------------------------------------------------------------ 4. a one-level RGBA8 cube through either entry
def test_one_level_rgba8_cube_through_either_entry(r3):
    """the same device words and the same frames from r3n_texture_cubes_write and r3n_texture_cubes_write_encoded"""
    w, h = 48, 32
    rng = np.random.default_rng(12)
    plain = [(rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8), srgb) for n, srgb in ((7, True), (2, False))]
    a, b = r3.Renderer(oh.LEFT, f32(w) / f32(h)), r3.Renderer(oh.LEFT, f32(w) / f32(h))
    for faces, srgb in plain:
        a.add_texture_cube(faces, srgb=srgb)
        b.add_texture_cube_encoded(C.RGBA8_SRGB if srgb else C.RGBA8, faces.shape[1], [[faces[f].tobytes()] for f in range(6)])
    for ci, (faces, _) in enumerate(plain):
        n = faces.shape[1]
        for f in range(6):
            wa, wb = a.readback_cube_face(ci, 0, f), b.readback_cube_face(ci, 0, f)
            inner = np.ones((n + 2, n + 2), dtype=bool)
            inner[[0, 0, -1, -1], [0, -1, 0, -1]] = False
            assert wa.dtype == wb.dtype == np.uint32 and np.array_equal(wa[inner], wb[inner]), f"cube {ci} face {f}"
            assert np.array_equal(wa[1:-1, 1:-1], faces[f].view(np.uint32)[..., 0])
        for r in (a, b):
            r.set_background_texture(ci)
            r.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
        for samples in (1, 4):
            fa, fb = a.render(w, h, samples=samples), b.render(w, h, samples=samples)
            assert np.array_equal(fa["hdr16"], fb["hdr16"]) and np.array_equal(fa["rgba8"], fb["rgba8"]), f"cube {ci} samples {samples}"
    a.close()
    b.close()


def test_plain_entry_word_for_word(r3):
    """r3n_texture_cubes_write is the encoded entry's path: cubes of N = 1, 3, 4, 5 in ONE call (the second sRGB), every bordered
    face word for word -- the interior, all four edges from resolve_texel, zero corners.  N = 1 makes every border texel another
    face's only texel; the odd extents in front of other cubes need the 4-word padding of levels and cubes.  Two launches: one
    decode family and the assemble."""
    import ctypes
    rng = np.random.default_rng(21)
    p = r3.Renderer(oh.LEFT, f32(1.0))
    cubes = [(rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8), srgb) for n, srgb in ((1, False), (3, True), (4, False), (5, False))]
    for ci, (faces, srgb) in enumerate(cubes):
        assert p.add_texture_cube(faces, srgb=srgb) == ci
    for ci, (faces, srgb) in enumerate(cubes):
        for f in range(6):
            got = p.readback_cube_face(ci, 0, f)
            want, corner = lodref.bordered_face(faces, f)
            want = np.ascontiguousarray(want).view(np.uint32)[..., 0]
            assert got.dtype == np.uint32 and got.shape == corner.shape
            bad = (got != want) & ~corner
            assert not bad.any(), f"N {faces.shape[1]} face {f}: {bad.sum()} texels differ, first {np.argwhere(bad)[0]}"
            assert not got[corner].any(), "corner words are written as zero"
        out, cls = np.zeros(4 * (faces.shape[1] + 2) ** 2, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        assert p.lib.r3n_readback_cube_face(p.ctx, ci, 0, 0, r3._ffi.ptr(out), out.size, r3._ffi.ptr(cls)) == 0 and cls[0] == (1 if srgb else 0)
    fn = p.lib.r3n_internal_cube_source_launches  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_uint64
    assert int(fn(p.ctx)) == 2
    p.close()


# ------------------------------------------------------------------ 5. refusals and state
def test_plain_entry_refuses_a_pool_past_2_32_words(r3):
    """three 16384^2 cubes through r3n_texture_cubes_write: 6 * 16386^2 words each, the third passes 2^32 -> R3N_ERR_CAPACITY before
    anything is read (n_texels claims room the small buffer does not have) or changed: the array, the binding, the next frame"""
    from rend3_amd import _ffi
    w, h = 16, 12
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    p.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
    rng = np.random.default_rng(22)
    p.add_texture_cube(rng.integers(0, 256, (6, 3, 3, 4), dtype=np.uint8), srgb=False)
    p.set_background_texture(p.add_texture_cube(rng.integers(0, 256, (6, 4, 4, 4), dtype=np.uint8), srgb=True))
    base = p.render(w, h)
    words = [p.readback_cube_face(ci, 0, f).copy() for ci, f in ((0, 0), (0, 5), (1, 2))]
    texels = np.zeros(1024, dtype=np.uint32)
    desc = np.array([[0, 16384, 16384, 1, C.RGBA8, 0, 0, 0]] * 3, dtype=np.uint32)
    assert p.lib.r3n_texture_cubes_write(p.ctx, _ffi.ptr(desc), 3, _ffi.ptr(texels), 1 << 40) == ERR_CAPACITY
    assert p.lib.r3n_last_error(p.ctx).decode() == "texture cubes write: the cube pool exceeds 2^32 words"
    assert all(np.array_equal(a, p.readback_cube_face(ci, 0, f)) for a, (ci, f) in zip(words, ((0, 0), (0, 5), (1, 2))))
    after = p.render(w, h)
    assert np.array_equal(base["hdr16"], after["hdr16"]) and np.array_equal(base["rgba8"], after["rgba8"])
    assert len(np.unique(base["hdr16"].reshape(-1, 4), axis=0)) > 4, "the frame shows the bound cube"
    p.close()


def test_refusals_leave_everything_unchanged(r3):
    from rend3_amd import _ffi
    from rend3_amd.renderer import BaseRenderGraph, BaseRenderGraphInputs, BaseRenderGraphSettings, RenderGraph
    w, h = 16, 12
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    lib, ctx = p.lib, p.ctx
    p.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
    first = cases.random_cube(C.BC6H_UF, 8, 4, 1)
    second = cases.random_cube(C.RGBA8_SRGB, 4, 3, 2)
    p.add_texture_cube_encoded(C.BC6H_UF, 8, first)
    p.set_background_texture(p.add_texture_cube_encoded(C.RGBA8_SRGB, 4, second))
    base = p.render(w, h)
    words = [p.readback_cube_face(ci, k, 3).copy() for ci, k in ((0, 0), (0, 3), (1, 2))]

    payload = np.zeros(cube_refusals.PAYLOAD_BYTES, dtype=np.uint8)

    def write(width, height, mips, fmt, offset=0, stored=0, payload_bytes=len(payload), n=1):
        desc = np.array([[offset, width, height, mips, fmt, stored, 0, 0]] * n, dtype=np.uint32)
        return lib.r3n_texture_cubes_write_encoded(ctx, _ffi.ptr(desc), n, _ffi.ptr(payload), payload_bytes)

    # the rows of tests/cube_refusals.py, which tests/test_cube_plan.py sends to the planner on the CPU: code AND message
    refusals = []
    for row in cube_refusals.ENCODED:
        desc = np.array(cube_refusals.encoded_cubes(row), dtype=np.uint32)
        code = lib.r3n_texture_cubes_write_encoded(ctx, _ffi.ptr(desc), len(desc), _ffi.ptr(payload), row[2])
        assert lib.r3n_last_error(ctx).decode() == "texture cubes write (encoded): " + row[4], row[0]
        refusals.append((row[0], code, row[3]))
    refusals.append(("null", lib.r3n_texture_cubes_write_encoded(ctx, None, 1, _ffi.ptr(payload), 16), ERR_INVALID_ARG))
    assert len(refusals) >= 14
    # (a job family past 2^31 wave slots cannot be reached: a wave slot takes 64 texels or blocks and the pool's 2^32 words hold at
    # most 2^26 wave slots of them -- the pool is refused first; the check stands for a change of either constant)
    for what, code, want in refusals:
        assert code == want, f"{what}: {code}"
    assert write(4, 4, 3, C.RGBA8, stored=3) == 0  # stored_mips == mips is the same as 0 ...
    p._cubes_dirty = True                         # ... and replaced the array: send the renderer's own again
    p._flush_cubes()
    # the array, the binding and the next frame are what they were
    assert all(np.array_equal(a.view(np.uint32), p.readback_cube_face(ci, k, 3).view(np.uint32)) for a, (ci, k) in zip(words, ((0, 0), (0, 3), (1, 2))))
    after = p.render(w, h)
    assert np.array_equal(base["hdr16"], after["hdr16"]) and np.array_equal(base["rgba8"], after["rgba8"])
    # each refusal on its own, frame by frame (the renderer does not re-send: the library's state alone)
    for args in (dict(width=4, height=2, mips=1, fmt=C.RGBA8), dict(width=4, height=4, mips=3, fmt=C.RGBA8, stored=1),
                 dict(width=16384, height=16384, mips=1, fmt=C.R8_SNORM, payload_bytes=1 << 40)):
        assert write(**args) < 0
        again = p.render(w, h)
        assert np.array_equal(base["hdr16"], again["hdr16"])
    for bad in ((2, 0, 0), (0, 4, 0), (0, 0, 6), (1, 3, 0)):  # the read-back's own refusals
        out = np.zeros(400, dtype=np.uint32)
        assert lib.r3n_readback_cube_face(ctx, *bad, _ffi.ptr(out), out.size, None) == ERR_INVALID_ARG
    out = np.zeros(400, dtype=np.uint32)
    assert lib.r3n_readback_cube_face(ctx, 0, 0, 0, _ffi.ptr(out), 10 * 10 * 4 - 1, None) == ERR_INVALID_ARG  # a short dst
    assert lib.r3n_readback_cube_face(ctx, 0, 0, 0, _ffi.ptr(out), 10 * 10 * 4, None) == 0

    # inside a frame: R3N_ERR_STATE
    codes = {}
    ev = p.evaluate_instructions()
    graph_base = BaseRenderGraph(p)
    graph = RenderGraph()
    graph_base.add_to_graph(graph, BaseRenderGraphInputs(ev, graph_base.default_routines(), (w, h), 1), BaseRenderGraphSettings((0, 0, 0, 0), (0, 0, 1, 1)))
    names = [name for name, _ in graph.nodes]
    graph.nodes.insert(names.index("Skybox"), ("probe", lambda r, _ev: codes.__setitem__("in frame", write(4, 4, 1, C.RGBA8))))
    graph.execute(p, ev)
    assert codes == {"in frame": ERR_STATE}
    assert np.array_equal(p.readback_frame(ev, w, h)["hdr16"], base["hdr16"])

    # replacing the array unbinds a cube that left it: cube 1 is bound, the new array has one cube.  The call goes to the library
    # directly, so the renderer sends no binding of its own and the library's unbinding is what the frame shows
    assert write(4, 4, 1, C.RGBA8) == 0
    assert lib.r3n_skybox_set(ctx, 2) == ERR_INVALID_ARG
    clear = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (clear["hdr16"] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all(), "the vanished cube was unbound"
    p.close()


# ------------------------------------------------------------------ 6. containers
@pytest.mark.parametrize("fmt", [C.BC6H_UF, C.RGBA8_SRGB], ids=fmt_id)
def test_cube_files_through_the_viewer(r3, tmp_path, fmt):
    """a KTX2 and a DDS cube file through scene_viewer's --skybox path give the frame of the same faces handed over directly"""
    from rend3_amd import scene_viewer as sv
    w, h, n = 24, 16, 8
    faces = cases.random_cube(fmt, n, 4, 55)
    files = {"sky.ktx2": cases.write_ktx2_cube(fmt, n, faces), "sky.dds": cases.write_dds_cube(fmt, n, faces)}
    frames = []
    for name in (None, "sky.ktx2", "sky.dds"):
        p = r3.Renderer(oh.RIGHT, f32(w) / f32(h))
        if name is None:
            p.set_background_texture(p.add_texture_cube_encoded(fmt, n, faces))
        else:
            (tmp_path / name).write_bytes(files[name])
            assert sv.add_skybox(p, str(tmp_path / name)) == 0
        p.set_camera_data(oh.look_at_rh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
        frames.append(p.render(w, h))
        p.close()
    assert len(np.unique(frames[0]["hdr16"].reshape(-1, 4), axis=0)) > 50
    for fr in frames[1:]:
        assert np.array_equal(fr["hdr16"], frames[0]["hdr16"]) and np.array_equal(fr["rgba8"], frames[0]["rgba8"])
