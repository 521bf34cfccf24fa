"""The skybox node (r3n_texture_cubes_write / r3n_skybox_set / r3n_skybox, rend3_amd/csrc/skybox.hip) on the GPU.

The oracle has no cube sampler, and needs none, through one identity: AT PIXEL p, A FRAME WITH A SKYBOX EQUALS THE FRAME WITHOUT
ONE RENDERED WITH clear_color = (sky(p), 1) -- the oracle rounds the clear colour to half where the sky is rounded to half, and
resolves and blends over it in the same way.  Where the sky is one colour (cubes whose bytes are all 0 or 255: the bilinear
blend c * (1 - f) + c * f is exact for 0.0 and 1.0) that is a whole-frame, bit-for-bit comparison with the existing oracle; where
it is not, the numpy restatement of the contract (tests/skybox_reference.py) gives sky(p)."""
import math

import numpy as np
import pytest

import scenes
import skybox_reference as sky
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 320, 192
AMBIENT = (0.1, 0.1, 0.1, 1.0)
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def constant_cube(colour, n=4):
    faces = np.zeros((6, n, n, 4), dtype=np.uint8)
    faces[..., :3] = colour
    faces[..., 3] = 93  # a cube's alpha is not sampled: the sky's alpha is 1
    return faces


def random_cube(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (6, n, n, 4), dtype=np.uint8)


def inv_origin_view_proj(o):
    return oh.mat4_inverse(o.camera.origin_view_proj)


def sky_mask(frame):
    """per pixel: how many of its samples take the sky (the depth half of the visibility keys through the reference's test)"""
    depth = (frame["vis"] >> np.uint64(32)).astype(np.uint32).view(f32)
    t = sky.takes_sky(depth)
    return t.astype(int) if t.ndim == 2 else t.sum(axis=2)


def build_world(r, mk, blend, n_objects=120):
    scenes.build_random_scene(r, oh, mk, n_objects, 0xC0FFEE, lights=2, with_cutout=True)
    if blend:
        scenes.add_blend_objects(r, oh, mk, 0xB1E2D)


def move_camera(rs, f):
    eye = (-2.0 + 1.5 * f, 1.0 + 0.3 * f, -3.0 + 0.5 * f)
    for r in rs:
        r.set_camera_data(oh.look_at_lh(eye, (0.5 * f, 0.5, 8.0), (0, 1, 0)), ("perspective", 60.0, 0.1))


# ------------------------------------------------------------------ 1. constant cube == clear colour, whole frame, on the oracle alone
# samples, R3N_FRAME_NODES, blend objects, R3N_EDGE_CAPACITY, colour, sRGB.  Without blend objects the four-sample frames take the
# split resolve (with 8 entries per edge sub-list almost every edge pixel overflows it) and the resolve and the sky run on the
# resolve's own stream while the next frame starts; with them every sample is kept and the transparent pass blends over the sky.
CONSTANT_CASES = [
    (1, False, True, None, (255, 0, 0), True),
    (1, True, True, None, (0, 255, 255), False),
    (1, False, False, None, (255, 255, 0), True),
    (4, False, True, None, (0, 0, 255), True),
    (4, True, True, None, (255, 255, 255), False),
    (4, False, False, None, (255, 0, 255), False),
    (4, True, False, None, (0, 255, 0), True),
    (4, False, False, 8, (0, 255, 255), True),
    (4, True, False, 8, (255, 0, 0), False),
]


@pytest.mark.parametrize("samples,nodes,blend,edge_capacity,colour,srgb", CONSTANT_CASES)
def test_constant_cube_equals_clear_colour(r3, monkeypatch, samples, nodes, blend, edge_capacity, colour, srgb):
    monkeypatch.setenv("R3N_FRAME_NODES", "1" if nodes else "0")
    if edge_capacity is not None:
        monkeypatch.setenv("R3N_EDGE_CAPACITY", str(edge_capacity))
    aspect = f32(W) / f32(H)
    o, p = OracleRenderer(oh.LEFT, aspect), r3.Renderer(oh.LEFT, aspect)
    build_world(o, omk, blend)
    build_world(p, r3.material_record, blend)
    p.set_background_texture(p.add_texture_cube(constant_cube(colour), srgb=srgb))
    clear = tuple(c / 255 for c in colour) + (1.0,)
    for f in range(3):
        move_camera((o, p), f)
        fo = o.render(W, H, samples=samples, ambient=AMBIENT, clear_color=clear)
        # the product's clear colour is another one: whatever of it stays visible is a pixel the sky missed
        fp = p.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0.5, 0.25, 0.125, 0.5))
        if blend:
            assert len(fo["blend_list"][0]) > 0
        n_sky = sky_mask(fp)
        assert (n_sky > 0).sum() > 500 and (n_sky == 0).sum() > 500, "the case needs sky and geometry"
        if samples == 4:
            assert ((n_sky > 0) & (n_sky < 4)).sum() > 50, "the case needs pixels shared by sky and geometry"
        compare_frames(fo, fp, f"constant cube {colour} frame {f}")
    assert p.stage_times()["skybox"][1] == 3
    p.close()


@pytest.mark.parametrize("samples", [1, 4])
def test_frames_in_flight_wait_for_the_sky(r3, monkeypatch, samples):
    """three frames enqueued without a read-back in between: the resolve and the sky of frame N run on the resolve's stream
    while the main stream works on frame N + 1; the read-back of the last frame must wait for its sky"""
    monkeypatch.setenv("R3N_FRAME_NODES", "0")
    aspect = f32(W) / f32(H)
    o, p = OracleRenderer(oh.LEFT, aspect), r3.Renderer(oh.LEFT, aspect)
    build_world(o, omk, False)
    build_world(p, r3.material_record, False)
    p.set_background_texture(p.add_texture_cube(constant_cube((255, 255, 0)), srgb=True))
    for f in range(3):
        move_camera((o, p), f)
        fo = o.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(1.0, 1.0, 0.0, 1.0))
        fp = p.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0, 0, 0, 0), readback=(f == 2))
    compare_frames(fo, fp, "frames in flight, last frame")
    p.close()


# ------------------------------------------------------------------ 2. one colour per face
FACE_COLOURS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]


@pytest.mark.parametrize("samples", [1, 4])
def test_six_colour_cube(r3, samples):
    n = 8
    faces = np.zeros((6, n, n, 4), dtype=np.uint8)
    for k, col in enumerate(FACE_COLOURS):
        faces[k, ..., :3] = col
    faces[..., 3] = 255
    aspect = f32(W) / f32(H)
    o, p = OracleRenderer(oh.LEFT, aspect), r3.Renderer(oh.LEFT, aspect)
    build_world(o, omk, True, 60)
    build_world(p, r3.material_record, True, 60)
    p.set_background_texture(p.add_texture_cube(faces, srgb=True))
    # from inside the box of objects towards a corner of the cube: three faces, three edges and the corner on screen
    view = oh.look_at_lh((0.0, 1.0, 0.0), (6.0, 6.5, 7.0), (0, 1, 0))
    for r in (o, p):
        r.set_camera_data(view, ("perspective", 75.0, 0.1))
    fp = p.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0.5, 0.5, 0.5, 1.0))
    ys, xs = np.mgrid[0:H, 0:W]
    d = sky.pixel_directions(inv_origin_view_proj(o), W, H, xs.reshape(-1), ys.reshape(-1))
    face, i0, j0, _, _ = sky.footprint(d, n)
    inside = ((i0 >= 0) & (i0 <= n - 2) & (j0 >= 0) & (j0 <= n - 2)).reshape(H, W)
    face = face.reshape(H, W)
    seen = [k for k in range(6) if (inside & (face == k)).sum() > 200]
    assert len(seen) >= 3, "the camera must see three faces"
    n_sky = None
    for k in seen:
        # (the oracle's frame index advances; the scene and the camera are still, so its image does not change)
        fo = o.render(W, H, samples=samples, ambient=AMBIENT, clear_color=tuple(c / 255 for c in FACE_COLOURS[k]) + (1.0,))
        if n_sky is None:
            assert np.array_equal(fo["vis"], fp["vis"])
            n_sky = sky_mask(fp)
            assert (n_sky == samples).sum() > 2000 and (n_sky == 0).sum() > 2000
        m = inside & (face == k)
        # footprint inside face k: the sky there is exactly the face's colour -- sky, geometry, shared and blended-over pixels alike
        assert np.array_equal(fo["hdr16"][m], fp["hdr16"][m]), f"face {sky.FACES[k]}: {(fo['hdr16'][m] != fp['hdr16'][m]).any(axis=1).sum()} px differ"
        assert np.abs(fo["rgba8"][m].astype(int) - fp["rgba8"][m].astype(int)).max() <= 1
    # the rest (footprints across an edge): where the pixel is sky alone and nothing blends over it, the numpy reference
    fo = o.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0.25, 0.5, 0.75, 1.0))
    unblended = (fo["hdr16"] == np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float16).view(np.uint16)).all(axis=2)
    m = ~inside & (n_sky == samples) & unblended
    assert m.sum() > 100
    want = sky.sky_frame(faces, True, inv_origin_view_proj(o), W, H)
    assert np.array_equal(want[m], fp["hdr16"][m]), f"{(want[m] != fp['hdr16'][m]).any(axis=1).sum()} of {m.sum()} edge px differ"
    p.close()


# ------------------------------------------------------------------ 3. random cubes against the numpy reference
def cameras():
    """(name, handedness, view, projection): looking at a face, along an edge, into a corner; perspective and orthographic"""
    out = []
    for hand, look in ((oh.LEFT, oh.look_at_lh), (oh.RIGHT, oh.look_at_rh)):
        tag = "lh" if hand == oh.LEFT else "rh"
        out.append((f"face {tag}", hand, look((0, 0, 0), (0.2, -0.1, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1)))
        out.append((f"edge {tag}", hand, look((1, 2, 3), (1 + 1.0, 2.0, 3 + 1.0), (0, 1, 0)), ("perspective", 90.0, 0.5)))
        out.append((f"corner {tag}", hand, look((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1)))
        out.append((f"down {tag}", hand, look((0, 5, 0), (0.3, -1.0, 0.2), (0, 0, 1)), ("perspective", 120.0, 0.1)))
        out.append((f"ortho {tag}", hand, look((0, 0, 0), (1.0, 0.4, 1.0), (0, 1, 0)), ("orthographic", (3.0, 2.0, 4.0))))
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_random_cubes_empty_world(r3, n):
    """nothing but sky: every pixel's half bits equal the reference's, every camera, sRGB and unorm, one and four samples"""
    w, h = 96, 64
    renderers = {}
    for k, (name, hand, view, proj) in enumerate(cameras()):
        for srgb in (True, False):
            faces = random_cube(n, 1000 * n + k)
            if hand not in renderers:
                renderers[hand] = r3.Renderer(hand, f32(w) / f32(h))
            p = renderers[hand]
            p.replace_texture_cubes([(faces, srgb)])
            p.set_background_texture(0)
            p.set_camera_data(view, proj)
            cam = oh.CameraState(view, proj, hand, f32(w) / f32(h))
            want = sky.sky_frame(faces, srgb, oh.mat4_inverse(cam.origin_view_proj), w, h)
            for samples in (1, 4):
                fp = p.render(w, h, samples=samples, clear_color=(0.3, 0.3, 0.3, 1.0))
                bad = (want != fp["hdr16"]).any(axis=2)
                assert not bad.any(), f"N {n} {name} srgb {srgb} samples {samples}: {bad.sum()} px differ, first {np.argwhere(bad)[0]}"
    for p in renderers.values():
        p.close()


GEOMETRY_CASES = [
    (7, True, 1, oh.LEFT, ("perspective", 60.0, 0.1)),
    (64, False, 4, oh.LEFT, ("perspective", 75.0, 0.1)),
    (2, True, 4, oh.RIGHT, ("orthographic", (40.0, 24.0, 80.0))),
    (64, True, 1, oh.RIGHT, ("perspective", 90.0, 0.1)),
]


@pytest.mark.parametrize("n,srgb,samples,hand,proj", GEOMETRY_CASES)
def test_random_cubes_with_geometry(r3, n, srgb, samples, hand, proj):
    """every pixel belongs to one of three classes and is judged in it: no sample on the sky -> the oracle's frame; sky alone
    with nothing blended over it -> the reference; shared with geometry or blended over -> (a sample of at least 16 of them)
    the oracle rendered with clear_color = sky(p)"""
    w, h = 160, 96
    aspect = f32(w) / f32(h)
    faces = random_cube(n, 77 + n)
    o, p = OracleRenderer(hand, aspect), r3.Renderer(hand, aspect)
    zs = 1.0 if hand == oh.LEFT else -1.0
    look = oh.look_at_lh if hand == oh.LEFT else oh.look_at_rh
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 80, 0xC0FFEE, handedness=hand, lights=1, with_cutout=True)
        hs = scenes.add_blend_objects(r, oh, mk, 0xB1E2D)
        if hand == oh.RIGHT:  # the blend objects are laid out in front of a camera that looks down +z
            for k, hnd in enumerate(hs):
                r.set_object_transform(hnd, oh.mat4_mul(oh.translation((-5.0 + k, 0.5 + 0.2 * k, zs * (4.0 + k))), oh.scale((1.5, 1.5, 0.3))))
        r.set_camera_data(look((-1.0, 1.5, zs * -3.0), (1.0, 1.0, zs * 8.0), (0, 1, 0)), proj)
    p.set_background_texture(p.add_texture_cube(faces, srgb=srgb))
    base_clear = (0.25, 0.5, 0.75, 1.0)
    fo = o.render(w, h, samples=samples, ambient=AMBIENT, clear_color=base_clear)
    fp = p.render(w, h, samples=samples, ambient=AMBIENT, clear_color=base_clear)
    assert np.array_equal(fo["vis"], fp["vis"])
    assert len(fo["blend_list"][0]) > 0
    n_sky = sky_mask(fp)
    want = sky.sky_frame(faces, srgb, inv_origin_view_proj(o), w, h)
    none = n_sky == 0
    unblended = (fo["hdr16"] == np.array(base_clear, dtype=np.float16).view(np.uint16)).all(axis=2)
    alone = (n_sky == samples) & unblended
    rest = ~none & ~alone
    assert none.sum() > 500 and alone.sum() > 500 and rest.sum() >= 16, (none.sum(), alone.sum(), rest.sum())
    assert np.array_equal(fo["hdr16"][none], fp["hdr16"][none]), "pixels without sky differ from the oracle"
    bad = (want != fp["hdr16"]).any(axis=2) & alone
    assert not bad.any(), f"{bad.sum()} of {alone.sum()} sky px differ from the reference, first {np.argwhere(bad)[0]}"
    pick = np.argwhere(rest)
    pick = pick[np.random.default_rng(5).permutation(len(pick))[:24]]
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


# ------------------------------------------------------------------ 4. row ranges
@pytest.mark.parametrize("samples", [1, 4])
def test_row_ranges_add_up(r3, samples):
    w, h = 160, 96
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    scenes.build_random_scene(p, oh, r3.material_record, 60, 0xC0FFEE, lights=1, with_cutout=True)
    p.set_camera_data(oh.look_at_lh((0, 1, -3), (1, 1, 8), (0, 1, 0)), ("perspective", 60.0, 0.1))
    cube = p.add_texture_cube(random_cube(16, 3), srgb=True)

    def frame(background, rows):
        p.set_background_texture(background)
        p._check(p.lib.r3n_set_row_range(p.ctx, rows[0], rows[1]), "r3n_set_row_range")
        return p.render(w, h, samples=samples, ambient=AMBIENT, clear_color=(1.0, 0.0, 1.0, 1.0))

    whole = frame(cube, (0, 0xFFFFFFFF))
    half = h // 2
    for rows, mine, other in (((0, half), slice(0, half), slice(half, h)), ((half, 0xFFFFFFFF), slice(half, h), slice(0, half))):
        plain = frame(None, (0, 0xFFFFFFFF))  # every row back to the clear colour
        assert (plain["hdr16"] != whole["hdr16"]).any(axis=2).sum() > 500
        part = frame(cube, rows)
        for key in ("hdr16", "rgba8"):
            assert np.array_equal(part[key][mine], whole[key][mine]), f"rows {rows}: {key} of the band"
            assert np.array_equal(part[key][other], plain[key][other]), f"rows {rows}: {key} outside the band was touched"
    p._check(p.lib.r3n_set_row_range(p.ctx, 0, 0xFFFFFFFF), "r3n_set_row_range")
    p.close()


# ------------------------------------------------------------------ 5. state and errors
def test_state_and_errors(r3, monkeypatch):
    from rend3_amd import _ffi
    from rend3_amd.renderer import BaseRenderGraph, BaseRenderGraphInputs, BaseRenderGraphSettings, RenderGraph
    w, h = 64, 48
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    lib, ctx = p.lib, p.ctx
    p.add_object(scenes.cube_mesh(p), p.add_material(r3.material_record(albedo=(0.5, 0.5, 0.5, 1.0), albedo_mode="value"), 0), oh.translation((0, 0, 4)))
    p.set_camera_data(oh.identity(), ("perspective", 60.0, 0.1))
    red = p.add_texture_cube(constant_cube((255, 0, 0)), srgb=True)
    p.set_background_texture(red)
    assert lib.r3n_skybox(ctx) == ERR_STATE  # outside a frame

    # the node outside its window: probes between the nodes of the graph mirror
    codes = {}
    ev = p.evaluate_instructions()
    base = BaseRenderGraph(p)
    graph = RenderGraph()
    base.add_to_graph(graph, BaseRenderGraphInputs(ev, base.default_routines(), (w, h), 1), BaseRenderGraphSettings((0, 0, 0, 0), (0, 0, 1, 1)))
    names = [name for name, _ in graph.nodes]
    assert names.index("Resolve Opaque") + 1 == names.index("Skybox") == names.index("PBR Forward Transparent") - 1
    for after in ("Frame Uniforms", "Primary Culling", "Skybox", "PBR Forward Transparent", "Tonemapping"):
        at = names.index(after) + 1
        graph.nodes.insert(at, ("probe " + after, lambda r, _ev, key=after: codes.__setitem__(key, r.lib.r3n_skybox(r.ctx))))
        names.insert(at, "probe " + after)
    graph.execute(p, ev)
    assert codes == {"Frame Uniforms": ERR_STATE, "Primary Culling": ERR_STATE, "Skybox": 0, "PBR Forward Transparent": ERR_STATE,
                     "Tonemapping": ERR_STATE}
    assert lib.r3n_skybox_set(ctx, 1) == 0
    fr = p.readback_frame(ev, w, h)
    one = np.array([1.0, 0.0, 0.0, 1.0], dtype=np.float16).view(np.uint16)
    assert (fr["hdr16"][0, 0] == one).all()  # (drawn twice: the probe behind the node repeats it)

    # binding and upload errors
    assert lib.r3n_skybox_set(ctx, 2) == ERR_INVALID_ARG
    assert lib.r3n_skybox_set(ctx, 0xFFFFFFFF) == ERR_INVALID_ARG
    texels = np.zeros(6 * 16 + 64, dtype=np.uint32)

    def write(width, height, mips, fmt, n_texels=len(texels)):
        desc = np.array([[0, width, height, mips, fmt, 0, 0, 0]], dtype=np.uint32)
        return lib.r3n_texture_cubes_write(ctx, _ffi.ptr(desc), 1, _ffi.ptr(texels), n_texels)

    assert write(4, 2, 1, 1) == ERR_INVALID_ARG      # not square
    assert write(0, 0, 1, 1) == ERR_INVALID_ARG
    assert write(4, 4, 1, 1, 6 * 16 - 1) == ERR_INVALID_ARG  # faces outside the texel array
    assert write(4, 4, 2, 1) == ERR_UNSUPPORTED      # a mip chain
    assert write(4, 4, 1, 14) == ERR_UNSUPPORTED     # R3N_TEXTURE_BC7_RGBA_UNORM
    assert write(4, 4, 1, 21) == ERR_UNSUPPORTED     # R3N_TEXTURE_RGBA16_FLOAT
    # (a refused upload leaves the array as it was)
    fr = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (fr["hdr16"][0, 0] == one).all()

    # replacing the cube array between frames takes effect
    p.replace_texture_cubes([(constant_cube((0, 255, 0)), False)])
    fr = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (fr["hdr16"][0, 0] == np.array([0.0, 1.0, 0.0, 1.0], dtype=np.float16).view(np.uint16)).all()
    assert (fr["rgba8"][0, 0] == (0, 255, 0, 255)).all()
    centre = fr["hdr16"][h // 2, w // 2].copy()  # the cube object
    # set(0) after a sky frame: the clear colour is back, the geometry unchanged
    p.set_background_texture(None)
    fr = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (fr["hdr16"][0, 0] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all()
    assert (fr["hdr16"][h // 2, w // 2] == centre).all()
    # an emptied array unbinds the skybox
    p.set_background_texture(0)
    p.render(w, h, clear_color=(0, 0, 1, 1))
    p.replace_texture_cubes([])
    fr = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (fr["hdr16"][0, 0] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all()
    p.close()


@pytest.mark.parametrize("samples", [1, 4])
def test_triangle_at_depth_zero_loses_to_the_sky(r3, samples):
    """GreaterEqual: the sky's depth 0.0 passes against a stored 0.0, so a triangle lying exactly on the far plane of an
    orthographic camera is overdrawn by the sky (skybox.hip sky_passes, skybox_reference.takes_sky) -- the frame is the one
    without that triangle, cleared to the sky's colour"""
    w = h = 64
    quad = (np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], dtype=f32), np.array([0, 2, 1, 0, 3, 2], dtype=np.uint32))
    normals = np.array([(0, 0, -1)] * 4, dtype=f32)
    o, p = OracleRenderer(oh.LEFT, f32(1.0)), r3.Renderer(oh.LEFT, f32(1.0))
    for r, mk, far in ((o, omk, False), (p, r3.material_record, True)):
        mesh = r.add_mesh(quad[0], quad[1], normals=normals)
        mat = r.add_material(mk(albedo=(0.5, 0.25, 1.0, 1.0), albedo_mode="value", unlit=True), 0)
        r.add_object(mesh, mat, oh.mat4_mul(oh.translation((1.0, 0.3, 2.0)), oh.scale((0.5, 0.5, 1.0))))
        if far:
            r.add_object(mesh, mat, oh.translation((0.0, 0.0, 5.0)))  # z = 5 is the far plane: depth (5 * -0.1) + 0.5 == 0.0
        r.set_camera_data(oh.identity(), ("orthographic", (4.0, 4.0, 10.0)))
    p.set_background_texture(p.add_texture_cube(constant_cube((255, 255, 0)), srgb=False))
    fo = o.render(w, h, samples=samples, clear_color=(1.0, 1.0, 0.0, 1.0))
    fp = p.render(w, h, samples=samples, clear_color=(0.0, 0.0, 1.0, 1.0))
    ids, depth = fp["vis"] & np.uint64(0xFFFFFFFF), (fp["vis"] >> np.uint64(32)).astype(np.uint32)
    assert ((ids != 0) & (depth == 0)).sum() > 500 * samples, "the far quad must be in the visibility buffer at depth 0.0"
    assert ((ids != 0) & (depth != 0)).sum() > 100 * samples
    assert np.array_equal(fo["hdr16"], fp["hdr16"]), f"{(fo['hdr16'] != fp['hdr16']).any(axis=2).sum()} px differ"
    assert np.abs(fo["rgba8"].astype(int) - fp["rgba8"].astype(int)).max() <= 1
    p.close()


# ------------------------------------------------------------------ 6. nothing moved
@pytest.mark.parametrize("samples", [1, 4])
def test_no_skybox_no_launch(r3, samples):
    """with no skybox bound the node launches nothing (the frame itself is held to the oracle by the parity suite, unchanged);
    with one bound it launches once per frame"""
    aspect = f32(W) / f32(H)
    o, p = OracleRenderer(oh.LEFT, aspect), r3.Renderer(oh.LEFT, aspect)
    build_world(o, omk, True, 60)
    build_world(p, r3.material_record, True, 60)
    p.add_texture_cube(constant_cube((255, 0, 0)))  # uploaded, never bound
    p.stage_times()
    for f in range(2):
        move_camera((o, p), f)
        fo = o.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(W, H, samples=samples, ambient=AMBIENT, clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"no skybox frame {f}")
    assert p.stage_times()["skybox"] == (0.0, 0)
    p.set_background_texture(0)
    p.render(W, H, samples=samples, ambient=AMBIENT)
    assert p.stage_times()["skybox"][1] == 1
    p.close()
