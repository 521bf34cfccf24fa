"""GPU parity tests: the HIP path (through the C ABI, include/r3n.h) against the CPU oracle on the same inputs.

Bar (task statement, BASELINE.json north_star):
  * visible-object set (L1), per-triangle pass/residual sets (L2), indirect-call counts, baked matrices,
    visibility/depth keys, shadow atlas: BIT-EXACT;
  * framebuffer after tonemap: |delta| <= 1e-3 in float (north_star tolerance); the tests additionally
    require the Rgba16Float HDR buffer to be bit-identical and the 8-bit image to be within 1 LSB.
Also re-runs the reference's golden-image scenes through the HIP path (pixel-exact where the reference's
own threshold is Mean(0.0)).
"""
import math
import os

import numpy as np
import pytest

import scenes
import test_oracle_goldens as G
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def compare_frames(o, p, tag=""):
    """o: oracle frame dict, p: product frame dict."""
    cap = o["capacity"]
    assert p["capacity"] == cap
    if "visible" in p:
        # the matrices any kernel reads: r3n_render_frame bakes the slots that pass the frustum test (or were batched last
        # frame), not the whole buffer (kernels_cull.h k_object_pass_chained); the per-node path bakes every enabled slot
        baked_slots = (o["objects"][:, 29] != 0) & o["visible"].astype(bool)
        assert np.array_equal(o["baked"].view(np.uint32)[baked_slots], p["baked"].view(np.uint32)[baked_slots]), tag + " baked"
        assert np.array_equal(o["visible"], p["visible"]), tag + " L1 visible objects"
        n = len(o["pass"])
        assert np.array_equal(o["pass"], p["pass"][:n]), tag + f" L2 pass set ({(o['pass'] != p['pass'][:n]).sum()} differ)"
        assert np.array_equal(o["residual"], p["residual"][:n]), tag + " L2 residual set"
        # IndirectCall.vertex_count = 3 * triangles appended (cull.wgsl:63-73), per material key
        tri_obj = np.searchsorted(o["tri_base"], np.arange(n), side="right") - 1
        keys = o["material_keys"][o["objects"][tri_obj, 22]] if n else np.zeros(0, dtype=np.uint8)
        for k in range(3):
            assert p["draw_calls"][k][0] == 3 * int((o["pass"].astype(bool) & (keys == k)).sum()), tag + f" predicted call {k}"
            assert p["draw_calls"][3 + k][0] == 3 * int((o["residual"].astype(bool) & (keys == k)).sum()), tag + f" residual call {k}"
            assert p["draw_calls"][k][1] == 1 and p["draw_calls"][k][3] == 0 and p["draw_calls"][k][4] == 0
        for so, sp in zip(o["shadows"], p["shadows"]):
            assert np.array_equal(so["visible"], sp["visible"]), tag + " shadow L1"
            assert np.array_equal(so["pass"], sp["pass"][: len(so["pass"])]), tag + " shadow L2"
    assert np.array_equal(o["vis"], p["vis"]), tag + f" visibility keys ({(o['vis'] != p['vis']).sum()} px differ)"
    assert np.array_equal(o["atlas"].view(np.uint32), p["atlas"].view(np.uint32)), tag + " shadow atlas"
    hd = (o["hdr16"] != p["hdr16"]).any(axis=2).sum()
    assert hd == 0, tag + f" HDR f16 differs in {hd} px"
    assert np.abs(o["rgba_f32"] - p["rgba_f32"]).max() <= 1e-3, tag + " framebuffer > 1e-3"
    assert np.abs(o["rgba8"].astype(int) - p["rgba8"].astype(int)).max() <= 1, tag + " rgba8 > 1 LSB"


def both(r3, handedness=oh.LEFT, aspect=None):
    return OracleRenderer(handedness, aspect), r3.Renderer(handedness, aspect)


# ------------------------------------------------------------------ reference golden scenes through the HIP path
def test_golden_empty(r3):
    r = r3.Renderer(oh.LEFT)
    r.set_camera_data(oh.identity(), ("raw", oh.identity()))
    out = r.render(64, 64)
    assert np.array_equal(out["rgba8"], G.load("rend3-test/simple/empty.png"))


@pytest.mark.parametrize("handedness,winding_ccw,visible",
                         [(oh.LEFT, False, True), (oh.LEFT, True, False), (oh.RIGHT, False, False), (oh.RIGHT, True, True)])
def test_golden_triangle(r3, handedness, winding_ccw, visible):
    """rend3-test/tests/simple.rs:28-84"""
    o, p = both(r3, handedness)
    for r, mk in ((o, omk), (p, r3.material_record)):
        pos = [(0.5, -0.5, 0.0), (0.0, 0.5, 0.0), (-0.5, -0.5, 0.0)] if winding_ccw else [(0.5, -0.5, 0.0), (-0.5, -0.5, 0.0), (0.0, 0.5, 0.0)]
        mesh = r.add_mesh(pos, mesh_handedness=oh.RIGHT if winding_ccw else oh.LEFT)
        r.add_object(mesh, scenes.unlit(r, mk, (0.25, 0.5, 0.75, 1.0)), oh.identity())
        r.set_camera_data(oh.identity(), ("raw", oh.identity()))
    fo, fp = o.render(64, 64), p.render(64, 64)
    compare_frames(fo, fp)
    name = "triangle.png" if visible else "triangle-backface.png"
    assert np.array_equal(fp["rgba8"], G.load("rend3-test/simple/" + name))


def test_golden_coordinate_space(r3):
    """rend3-test/tests/simple.rs:86-141 (six frames on one renderer: exercises the temporal two-pass state)"""
    o, p = both(r3)
    for r, mk in ((o, omk), (p, r3.material_record)):
        for _n, right, up, camv in G.COORD_TESTS:
            right, up, camv = (np.array(v, dtype=f32) for v in (right, up, camv))
            pos = [f32(0.5) * right + f32(-0.5) * up, f32(-0.5) * right + f32(-0.5) * up, f32(0.0) * right + f32(0.5) * up]
            color = camv * f32(-0.25) if bool((camv < 0).any()) else camv
            r.add_object(r.add_mesh(pos, mesh_handedness=oh.LEFT), scenes.unlit(r, mk, (color[0], color[1], color[2], 1.0)), oh.identity())
    for name, _right, up, camv in G.COORD_TESTS:
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh(camv, (0, 0, 0), up), ("raw", oh.identity()))
        fo, fp = o.render(64, 64), p.render(64, 64)
        compare_frames(fo, fp, name)
        assert np.array_equal(fp["rgba8"], G.load(f"rend3-test/simple/coordinate-space-{name}.png")), name


def test_golden_duplicate_object_retain(r3):
    """rend3-test/tests/object.rs:9-59"""
    o, p = both(r3)
    hs = []
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.set_camera_data(oh.identity(), ("raw", oh.identity()))
        mat = scenes.unlit(r, mk, (1, 1, 1, 1))
        mesh = scenes.plane_mesh(r)
        hs.append((mesh, mat, r.add_object(mesh, mat, G.srt((-0.25, 0.25, 0.25), (-0.5, 0, 0)))))
    fo, fp = o.render(64, 64), p.render(64, 64)
    compare_frames(fo, fp, "left")
    assert np.array_equal(fp["rgba8"], G.load("rend3-test/object/duplicate-object-retain-left.png"))
    for r, (mesh, mat, h) in zip((o, p), hs):
        r.add_object(mesh, mat, G.srt((-0.25, 0.25, 0.25), (0.5, 0, 0)))
        r.remove_object(h)
    fo, fp = o.render(64, 64), p.render(64, 64)
    compare_frames(fo, fp, "right")
    assert np.array_equal(fp["rgba8"], G.load("rend3-test/object/duplicate-object-retain-right.png"))
    # third frame: the removed slot is really gone, the history still lines up
    compare_frames(o.render(64, 64), p.render(64, 64), "after removal")


def test_golden_multi_frame_add(r3):
    """rend3-test/tests/object.rs:61-109: object buffer grows 16 -> 32"""
    o, p = both(r3)
    ms = []
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.set_camera_data(oh.identity(), ("raw", oh.orthographic_lh(0.0, 2.0, 16.0, 0.0, 0.0, 1.0)))
        ms.append((scenes.unlit(r, mk, (1, 1, 1, 1)), scenes.plane_mesh(r)))
    base = oh.mat4_mul(oh.translation((0.5, 0.5, 0.0)), oh.scale((0.5, 1.0, 1.0)))
    for x in range(2):
        for r, (mat, mesh) in zip((o, p), ms):
            for y in range(16):
                r.add_object(mesh, mat, oh.mat4_mul(oh.translation((x, y, 0.0)), base))
        fo, fp = o.render(64, 64), p.render(64, 64)
        compare_frames(fo, fp, f"col{x}")
        assert np.array_equal(fp["rgba8"], G.load(f"rend3-test/object/multi-frame-add-{x}.png")), x


def test_golden_sample_coverage_1(r3):
    """rend3-test/tests/msaa.rs:41-82 at 1 spp: 4096 objects, sub-pixel cull vs raster consistency"""
    o, p = both(r3)
    base = oh.mat4_mul(oh.translation((0.5, 0.5, 0.0)), oh.scale((0.5, 0.5, 1.0)))
    for r, mk in ((o, omk), (p, r3.material_record)):
        mat = scenes.unlit(r, mk, (1, 1, 1, 1))
        mesh = scenes.plane_mesh(r)
        for x in range(64):
            for y in range(64):
                sx, sy = f32(1.0) - (f32(x) / f32(63.0)), f32(1.0) - (f32(y) / f32(63.0))
                r.add_object(mesh, mat, oh.mat4_mul(oh.mat4_mul(oh.translation((x, y, 0.0)), oh.scale((sx, sy, 1.0))), base))
        r.set_camera_data(oh.identity(), ("raw", oh.orthographic_lh(0.0, 64.0, 64.0, 0.0, 0.0, 1.0)))
    fo, fp = o.render(64, 64), p.render(64, 64)
    compare_frames(fo, fp)
    assert np.array_equal(fp["rgba8"], G.load("rend3-test/msaa/sample-coverage-1.png"))


def test_golden_shadow_plane_and_cube(r3):
    """rend3-test/tests/shadow.rs:9-54"""
    o, p = both(r3)
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.add_directional_light(color=(1, 1, 1), intensity=1.0, direction=(-1.0, -1.0, 1.0), distance=5.0, resolution=256)
        r.add_object(scenes.plane_mesh(r), scenes.lit(r, mk, (0.25, 0.5, 0.75, 1.0)), oh.rotation_x(-math.pi / 2))
        r.set_camera_data(oh.look_at_lh((0.0, 1.0, -1.0), (0, 0, 0), (0, 1, 0)), ("orthographic", (2.5, 2.5, 5.0)))
    fo, fp = o.render(256, 256), p.render(256, 256)
    compare_frames(fo, fp, "plane")
    gold = G.load("rend3-test/shadow/plane.png")
    assert np.array_equal(gold[..., :3].any(axis=2), fp["rgba8"][..., :3].any(axis=2))
    assert np.abs(fp["rgba8"].astype(int) - gold.astype(int)).max() <= 1
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.add_object(scenes.cube_mesh(r), scenes.lit(r, mk, (0.75, 0.5, 0.25, 1.0)), G.srt((0.25, 0.25, 0.25), (0.25, 0.25, -0.25)))
    fo, fp = o.render(256, 256), p.render(256, 256)
    compare_frames(fo, fp, "cube")
    gold = G.load("rend3-test/shadow/cube.png")
    assert (np.abs(fp["rgba8"].astype(int) - gold.astype(int)).max(axis=2) <= 2).mean() >= 0.99


def test_golden_cube_example(r3):
    """examples/src/cube/mod.rs (BASELINE.json configs[0], at the golden's 1280x720)"""
    w, h = 1280, 720
    o, p = both(r3, oh.LEFT, f32(w) / f32(h))
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.add_object(scenes.cube_mesh(r), r.add_material(mk(albedo=(0.5, 0.5, 0.5, 1.0), albedo_mode="value"), scenes.OPAQUE), oh.identity())
        r.set_camera_data(oh.mat4_mul(oh.from_euler_xyz(-0.55, 0.5, 0.0), oh.translation((-3.0, -3.0, 5.0))), ("perspective", 60.0, 0.1))
        r.add_directional_light(color=(1, 1, 1), intensity=1.0, direction=(-1.0, -4.0, 2.0), distance=400.0, resolution=2048)
        r.add_point_light((0.1, 1.2, -1.5), (1.0, 0.0, 0.0), 4.0, 2.0)
        r.add_point_light((1.5, 1.2, -0.1), (0.0, 1.0, 0.0), 4.0, 2.0)
    fo = o.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
    fp = p.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
    compare_frames(fo, fp)
    from PIL import Image
    gold = np.array(Image.open(os.path.join(G.GOLD, "cube-screenshot.png")).convert("RGBA"))
    diff = np.abs(fp["rgba8"].astype(int) - gold.astype(int)).max(axis=2)
    assert diff.mean() <= 1.0 and (diff <= 3).mean() >= 0.995


def test_golden_static_gltf_example(r3):
    """examples/src/static_gltf/mod.rs at 1280x720: real asset through the GLB reader (row N1), HIP == oracle, and the
    HIP image against the reference's screenshot."""
    w, h = 1280, 720
    o, p = both(r3, oh.LEFT, f32(w) / f32(h))
    G.build_static_gltf(o, oh, omk)
    G.build_static_gltf(p, r3.host, r3.material_record)
    for f in range(2):
        fo = o.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        fp = p.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        compare_frames(fo, fp, f"static_gltf frame {f}")
    _gold, diff = G.golden_stats(fp["rgba8"], "static_gltf-screenshot.png")
    assert diff.mean() <= 0.1 and (diff <= 1).mean() >= 0.998


def test_golden_skinning_example(r3):
    """examples/src/skinning/mod.rs at 1280x720, three animation times: GLB skin -> k_skinning -> every pass; HIP ==
    oracle bit for bit, and the t = 0 HIP image against the reference's screenshot (bounds: test_oracle_goldens)."""
    w, h = 1280, 720
    o, p = both(r3, oh.LEFT, f32(w) / f32(h))
    io = G.build_skinning_example(o, oh, omk)
    ip = G.build_skinning_example(p, r3.host, r3.material_record)
    for f, t in enumerate((0.0, 0.11, 0.31)):
        G.set_skinning_pose(o, oh, io, t)
        G.set_skinning_pose(p, r3.host, ip, t)
        fo = o.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        fp = p.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        compare_frames(fo, fp, f"skinning example t={t}")
        if f == 0:
            _gold, diff = G.golden_stats(fp["rgba8"], "skinning-screenshot.png")
            assert diff.mean() <= 0.6 and (diff <= 1).mean() >= 0.97


# ------------------------------------------------------------------ synthetic scenes: multi-frame temporal parity
@pytest.mark.parametrize("handedness", [oh.LEFT, oh.RIGHT])
def test_random_scene_multi_frame(r3, handedness):
    """'scifi-like' synthetic scene (SURVEY section 8d cfg 2 shape, reduced to oracle-in-seconds size): camera
    orbits over 4 frames so predicted/residual/Hi-Z occlusion all engage; one object moves, one is removed."""
    o, p = both(r3, handedness, f32(320) / f32(192))
    ho = scenes.build_random_scene(o, oh, omk, 300, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    hp = scenes.build_random_scene(p, oh, r3.material_record, 300, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    look = oh.look_at_lh if handedness == oh.LEFT else oh.look_at_rh
    for f in range(4):
        ang = 0.35 * f
        eye = (3.0 * math.sin(ang), 1.0 + 0.5 * f, -3.0 * math.cos(ang))
        for r in (o, p):
            r.set_camera_data(look(eye, (10 * math.sin(ang + 0.3), 0, 10 * math.cos(ang + 0.3)), (0, 1, 0)), ("perspective", 60.0, 0.1))
        if f == 2:
            for r, hs in ((o, ho), (p, hp)):
                r.set_object_transform(hs[5], oh.mat4_mul(oh.translation((2.0, 0.5, 6.0)), oh.scale((2, 2, 2))))
                r.remove_object(hs[7])
        fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"frame {f}")
        if f >= 1:
            assert fo["pass"].sum() > 0 and fo["visible"].sum() > 0
    # occlusion culling engaged: some frustum-visible, front-facing triangles were rejected by Hi-Z at least once
    assert fo["residual"].sum() < fo["pass"].sum()


@pytest.mark.parametrize("n_objects", [16, 32, 128])
def test_object_added_past_a_full_buffer(r3, n_objects):
    """The object buffer is exactly full (a power of two: freelist/buffer.rs:48-52), two frames of history exist, then an object is
    added: its handle is the old capacity, the buffer doubles, and the triangle cull looks the new object up in LAST frame's table
    of result-bit bases, which was sized for the old capacity.  It must read 'not batched last frame' (batching.rs:226) -- every
    passing triangle residual, drawn by pass 2 in its first frame.  (tools/fuzz_parity.py found the read running past the
    allocation: the object's first frame was drawn by neither pass.)"""
    o, p = both(r3, oh.LEFT, f32(200) / f32(120))
    ho = scenes.build_random_scene(o, oh, omk, n_objects, 11, lights=1, shadow_res=128)
    hp = scenes.build_random_scene(p, oh, r3.material_record, n_objects, 11, lights=1, shadow_res=128)
    assert ho == hp and max(ho) == n_objects - 1
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((0, 2, -8), (0, 0, 0), (0, 1, 0)), ("perspective", 70.0, 0.1))
    for f in range(2):
        compare_frames(o.render(200, 120), p.render(200, 120), f"frame {f}")
    added = [r.add_object(scenes.cube_mesh(r), scenes.lit(r, mk, (0.8, 0.7, 0.2, 1.0)), oh.translation((0.0, 1.0, -3.0)))
             for r, mk in ((o, omk), (p, r3.material_record))]
    assert added == [n_objects, n_objects]
    fo, fp = o.render(200, 120), p.render(200, 120)
    assert fo["capacity"] == 2 * n_objects
    first = int(fo["tri_base"][n_objects])
    assert fo["residual"][first:first + 12].sum() > 0, "the new cube is in view: its front faces are newly visible"
    compare_frames(fo, fp, "the frame the buffer grew in")
    compare_frames(o.render(200, 120), p.render(200, 120), "the frame after")


def test_target_resize_keeps_the_temporal_history(r3):
    """The target changes size (and sample count) between frames.  The reference keeps a camera's culling buffers across that --
    CullingBufferMap is keyed by the camera alone (culler.rs:53-80) -- so the frame after the change still draws last frame's
    predicted triangles first and only the newly visible ones are residual.  (Rounds 1-5 reset the history on a size change;
    tools/fuzz_parity.py --mutate found the difference against the oracle.)"""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    scenes.build_random_scene(o, oh, omk, 200, 0xC0FFEE, lights=1, with_cutout=True)
    scenes.build_random_scene(p, oh, r3.material_record, 200, 0xC0FFEE, lights=1, with_cutout=True)
    for f, (w, h, s) in enumerate(((320, 192, 1), (320, 192, 1), (211, 140, 1), (211, 140, 4), (400, 90, 4), (64, 64, 1))):
        ang = 0.2 * f
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh((3.0 * math.sin(ang), 1.0, -3.0 * math.cos(ang)), (10 * math.sin(ang + 0.3), 0, 10 * math.cos(ang + 0.3)), (0, 1, 0)),
                              ("perspective", 60.0, 0.1))
        fo = o.render(w, h, samples=s, ambient=(0.1, 0.1, 0.1, 1.0))
        fp = p.render(w, h, samples=s, ambient=(0.1, 0.1, 0.1, 1.0))
        compare_frames(fo, fp, f"frame {f} at {w}x{h} s{s}")
        if f >= 1:
            assert 0 < fo["residual"].sum() < fo["pass"].sum(), "history engaged: most passing triangles were predicted"


def test_hiz_pyramid_matches_oracle(r3):
    """hi_z.wgsl: non-power-of-two target (odd mip dimensions take the 3-wide path)."""
    o, p = both(r3, oh.LEFT, f32(200) / f32(120))
    scenes.build_random_scene(o, oh, omk, 120, 7, lights=0)
    scenes.build_random_scene(p, oh, r3.material_record, 120, 7, lights=0)
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((0, 2, -8), (0, 0, 0), (0, 1, 0)), ("perspective", 70.0, 0.1))
    o.render(200, 120); p.render(200, 120, readback=False)  # frame 0: everything residual
    fo = o.render(200, 120)
    p.render(200, 120, readback=False)                       # frame 1: pass 1 draws -> non-trivial pyramid
    pyr = p.readback_hiz(200, 120)
    assert np.array_equal(fo["hiz"].view(np.uint32), pyr.view(np.uint32))
    assert fo["hiz"].max() > 0


def test_near_plane_crossing_geometry(r3):
    """A large ground grid passing under/behind the camera: triangles with w <= 0 vertices (App. D.1 quirk in the
    cull shader, homogeneous rasterisation without clipping in the draw)."""
    o, p = both(r3, oh.LEFT, f32(256) / f32(160))
    for r, mk in ((o, omk), (p, r3.material_record)):
        pos, idx, nrm = scenes.grid_plane(6, 40.0)
        r.add_object(r.add_mesh(pos, idx, normals=nrm), scenes.lit(r, mk, (0.6, 0.6, 0.6, 1.0)), oh.identity())
        pos, idx, nrm = scenes.box(1, 3, 1)
        r.add_object(r.add_mesh(pos, idx, normals=nrm), scenes.lit(r, mk, (0.9, 0.3, 0.2, 1.0)), oh.translation((1.5, 3.0, 6.0)))
        r.add_directional_light(color=(1, 1, 1), intensity=2.0, direction=(0.4, -1.0, 0.3), distance=40.0, resolution=512)
        r.set_camera_data(oh.look_at_lh((0, 1.5, -2), (0.5, 1.0, 6), (0, 1, 0)), ("perspective", 75.0, 0.1))
    for f in range(2):
        compare_frames(o.render(256, 160), p.render(256, 160), f"frame {f}")


def test_empty_and_degenerate_inputs(r3):
    """Edge cases: no objects; object with < 1 triangle; zero-area triangles; everything outside the frustum."""
    o, p = both(r3)
    for r, mk in ((o, omk), (p, r3.material_record)):
        r.set_camera_data(oh.look_at_lh((0, 0, -5), (0, 0, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    compare_frames(o.render(64, 48), p.render(64, 48), "empty")
    for r, mk in ((o, omk), (p, r3.material_record)):
        mat = scenes.unlit(r, mk, (1, 0, 0, 1))
        r.add_object(r.add_mesh([(0, 0, 0), (1, 0, 0)], [0, 1], normals=[(0, 0, 1)] * 2), mat, oh.identity())        # 0 triangles
        r.add_object(r.add_mesh([(0, 0, 0), (1, 1, 0), (2, 2, 0)], normals=[(0, 0, 1)] * 3), mat, oh.identity())     # zero area
        r.add_object(r.add_mesh([(0, 0, 0), (0, 1, 0), (1, 0, 0)], normals=[(0, 0, -1)] * 3), mat, oh.translation((500, 0, 0)))  # outside
        r.add_object(r.add_mesh([(0, 0, 0), (0, 1, 0), (1, 0, 0)], normals=[(0, 0, -1)] * 3), mat, oh.identity())    # visible
    for f in range(2):
        fo, fp = o.render(64, 48), p.render(64, 48)
        compare_frames(fo, fp, f"degenerate {f}")
    assert fo["rgba8"][..., 0].max() == 255


# ------------------------------------------------------------------ full-size properties (oracle too slow there)
def _large(r3):
    p = r3.Renderer(oh.LEFT, f32(3840) / f32(2160))
    scenes.build_random_scene(p, r3.host, r3.material_record, 20000, 0xB157, extent=(120.0, 20.0, 120.0), lights=1,
                              shadow_res=1024, shadow_distance=200.0)
    p.set_camera_data(oh.look_at_lh((0, 3, -10), (0, 0, 40), (0, 1, 0)), ("perspective", 60.0, 0.1))
    return p


def test_large_scene_properties(r3):
    """4K, 20k objects (oracle too slow): size-independent properties.
    (a) frame 0 has no history: residual == pass; a static camera reaches residual == 0;
    (b) the whole pipeline is deterministic: a second context fed the same inputs produces bit-identical sets,
        visibility keys and image on every frame (the compaction ORDER may differ, the sets may not);
    (c) occlusion only removes triangles: pass(f1) is a subset of pass(f0);
    (d) predicted IndirectCall counts == 3 * popcount(pass);
    (e) every pixel's nearest fragment in frame 2 comes from a triangle of pass(f1) + residual(f2)."""
    p, q = _large(r3), _large(r3)
    fp = [p.render(3840, 2160, ambient=(0.1, 0.1, 0.1, 1)) for _ in range(3)]
    fq = [q.render(3840, 2160, ambient=(0.1, 0.1, 0.1, 1)) for _ in range(3)]
    f0, f1, f2 = fp
    assert f0["residual"].sum() == f0["pass"].sum() > 0
    assert f2["residual"].sum() == 0
    for a, b in zip(fp, fq):
        for k in ("visible", "pass", "residual", "vis", "rgba8", "hdr16"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["atlas"].view(np.uint32), b["atlas"].view(np.uint32))
    assert not (f1["pass"].astype(bool) & ~f0["pass"].astype(bool)).any()
    assert f1["pass"].sum() < f0["pass"].sum()
    assert sum(int(f2["draw_calls"][k][0]) for k in range(3)) == 3 * int(f2["pass"].sum())
    ids = (f2["vis"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = ids[ids > 0] - 1
    assert (f1["pass"][ids].astype(bool) | f2["residual"][ids].astype(bool)).all()
    p.close(); q.close()


def test_config2_scifi_full_size(r3):
    """BASELINE.json configs[1] at FULL size: 20 000 objects / 19 M triangles, 1920x1080, right-handed, cull + compact:
    visible-object set, per-triangle pass/residual sets and indirect-call counts bit-exact vs the oracle over three
    frames (first frame without history, then a turning camera so predicted/residual/Hi-Z all engage)."""
    import rend3_amd.scenes as S
    o = OracleRenderer(oh.RIGHT, f32(1920) / f32(1080))
    p = r3.Renderer(oh.RIGHT, f32(1920) / f32(1080))
    io = S.scifi_like(o, oh, omk)
    ip = S.scifi_like(p, r3.host, r3.material_record)
    assert io["triangles"] == ip["triangles"] > 15_000_000
    for f, yaw in enumerate((0.0, 0.1, 0.25)):
        for r, hm in ((o, oh), (p, r3.host)):
            r.set_camera_data(hm.rotation_y(yaw), io["camera"][1])
        fo, fp = o.render(1920, 1080), p.render(1920, 1080)
        compare_frames(fo, fp, f"cfg2 frame {f}")
        assert fo["visible"].sum() > 1000 and fo["pass"].sum() > 1000
    p.close()


def test_config4_full_size(r3):
    """BASELINE.json configs[3] at FULL size -- 1 048 576 objects / 55 M triangles, 3840x2160 -- against the oracle (its
    cull and rasterisers are OpenMP loops: seconds per frame at this size): three frames with a turning camera, so the first
    has no history, the second culls against the Hi-Z of the first's predicted set and the third draws a non-empty
    residual.  Everything compare_frames checks is required: L1 set over the 2^20 slots, L2 pass / residual sets over all
    triangles, IndirectCall counts, baked matrices, visibility keys, HDR, framebuffer (culler.rs:531-659, cull.wgsl)."""
    import rend3_amd.scenes as S
    w, h = 3840, 2160
    o = OracleRenderer(oh.LEFT, f32(w) / f32(h))
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    io = S.emerald_like(o, oh, omk)
    ip = S.emerald_like(p, r3.host, r3.material_record)
    assert io["objects"] == ip["objects"] == 1 << 20 and io["triangles"] == ip["triangles"] > 50_000_000
    view0, proj = io["camera"]
    for f, yaw in enumerate((0.0, 0.03, 0.08)):
        for r, hm in ((o, oh), (p, r3.host)):
            r.set_camera_data(hm.mat4_mul(hm.rotation_y(yaw), view0), proj)
        fo, fp = o.render(w, h, ambient=(0.1, 0.1, 0.1, 1)), p.render(w, h, ambient=(0.1, 0.1, 0.1, 1))
        compare_frames(fo, fp, f"cfg4 full size, frame {f}")
        assert fo["visible"].sum() > 100_000 and fo["pass"].sum() > 50_000
        if f == 0:
            assert fo["residual"].sum() == fo["pass"].sum()
    assert 0 < fo["residual"].sum() < fo["pass"].sum()
    p.close()


def test_config4_full_size_four_shadow_views(r3):
    """BASELINE.json configs[3] as bench.py --config 4 times it: the full-size world WITH the four directional lights and their
    2048^2 shadow views (1 M objects through five cameras' culls, four shadow depth draws, the lit resolve): two frames against the
    oracle, everything compare_frames checks -- also the four views' L1 / L2 sets and the 4096^2 atlas."""
    import rend3_amd.scenes as S
    w, h = 3840, 2160
    o = OracleRenderer(oh.LEFT, f32(w) / f32(h))
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    io = S.emerald_like(o, oh, omk, n_lights=4)
    ip = S.emerald_like(p, r3.host, r3.material_record, n_lights=4)
    assert io["objects"] == ip["objects"] == 1 << 20
    view0, proj = io["camera"]
    for f, yaw in enumerate((0.0, 0.05)):
        for r, hm in ((o, oh), (p, r3.host)):
            r.set_camera_data(hm.mat4_mul(hm.rotation_y(yaw), view0), proj)
        fo, fp = o.render(w, h, ambient=(0.1, 0.1, 0.1, 1)), p.render(w, h, ambient=(0.1, 0.1, 0.1, 1))
        compare_frames(fo, fp, f"cfg4 full size with four shadow views, frame {f}")
    assert len(fo["shadows"]) == 4 and all(s["pass"].sum() > 10_000 for s in fo["shadows"]) and (fo["atlas"] != 0).mean() > 0.05
    assert 0 < fo["residual"].sum() < fo["pass"].sum()
    p.close()


def test_config4_million_objects_properties(r3):
    """BASELINE.json configs[3] shape: 1 048 576 objects (oracle too slow): properties only -- determinism across
    contexts, residual(frame 0) == pass(frame 0), call counts == popcounts, every nearest fragment from a drawn triangle,
    and object-range sharding: two half-range contexts produce L1/L2 sets whose union is the unsharded result."""
    import rend3_amd.scenes as S
    w, h = 1280, 720

    def make(rng=None):
        r = r3.Renderer(oh.LEFT, f32(w) / f32(h))
        info = S.emerald_like(r, r3.host, r3.material_record)
        if rng is not None:
            r.evaluate_instructions()
            r.set_object_range(*rng)
        return r, info

    a, info = make()
    assert info["objects"] == 1 << 20
    fa = [a.render(w, h) for _ in range(2)]
    assert fa[0]["residual"].sum() == fa[0]["pass"].sum() > 0
    assert sum(int(fa[1]["draw_calls"][k][0]) for k in range(3)) == 3 * int(fa[1]["pass"].sum())
    ids = (fa[1]["vis"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = ids[ids > 0] - 1
    assert (fa[0]["pass"][ids].astype(bool) | fa[1]["residual"][ids].astype(bool)).all()
    cap = a.capacity
    a.close()
    lo, _ = make((0, cap // 2))
    flo = lo.render(w, h)
    lo.close()
    hi, _ = make((cap // 2, cap))
    fhi = hi.render(w, h)
    hi.close()
    # frame 0 has no Hi-Z history, so sharded culling needs no exchange to be exact
    assert np.array_equal(flo["visible"] | fhi["visible"], fa[0]["visible"])
    assert not (flo["visible"] & fhi["visible"]).any()
    assert np.array_equal(flo["pass"] | fhi["pass"], fa[0]["pass"])
    assert np.array_equal(np.maximum(flo["vis"], fhi["vis"]), fa[0]["vis"])


def test_vertex_colour_and_cutout_alpha_paths(r3):
    """Material paths of opaque.wgsl:213-235 / depth.wgsl:112-125 that the golden scenes do not reach: vertex-colour
    albedo (linear and sRGB-decoded), cutout against an interpolated vertex alpha (forward and shadow passes).
    The sRGB decode uses pow(), so the HDR buffer is compared to 2 f16 ulps instead of bit-exactly."""
    o, p = both(r3, oh.LEFT, f32(1.5))
    rng = scenes.Pcg32(11)
    for r, mk in ((o, omk), (p, r3.material_record)):
        rng = scenes.Pcg32(11)
        pos, idx, nrm = scenes.grid_plane(8, 2.0)
        cols = np.array([[rng.randint(256), rng.randint(256), rng.randint(256), rng.randint(256)] for _ in range(len(pos))], dtype=np.uint8)
        mesh = r.add_mesh(pos, idx, normals=nrm, colors=cols)
        m_lin = r.add_material(mk(albedo=(1, 1, 1, 1), albedo_mode="vertex", vertex_srgb=False, roughness=0.4), scenes.OPAQUE)
        m_srgb = r.add_material(mk(albedo=(0.9, 0.8, 0.7, 1), albedo_mode="value_vertex", vertex_srgb=True, roughness=0.6), scenes.OPAQUE)
        m_cut = r.add_material(mk(albedo=(0.2, 0.9, 0.3, 1.0), albedo_mode="value_vertex", vertex_srgb=False, roughness=0.5, cutout=0.5), scenes.CUTOUT)
        m_cut_const = r.add_material(mk(albedo=(0.9, 0.2, 0.3, 0.3), albedo_mode="value", roughness=0.5, cutout=0.5), scenes.CUTOUT)
        tilt = oh.rotation_x(-0.9)
        r.add_object(mesh, m_lin, oh.mat4_mul(oh.translation((-2.2, 0.0, 5.0)), tilt))
        r.add_object(mesh, m_srgb, oh.mat4_mul(oh.translation((2.2, 0.0, 5.0)), tilt))
        r.add_object(mesh, m_cut, oh.mat4_mul(oh.translation((0.0, 1.5, 4.0)), tilt))       # holes where alpha < 0.5
        r.add_object(mesh, m_cut_const, oh.mat4_mul(oh.translation((0.0, 3.0, 4.5)), tilt))  # alpha 0.3 < 0.5: fully discarded
        floor = r.add_mesh(*scenes.grid_plane(2, 8.0)[:2], normals=scenes.grid_plane(2, 8.0)[2])
        r.add_object(floor, scenes.lit(r, mk, (0.7, 0.7, 0.7, 1.0)), oh.translation((0.0, -1.5, 5.0)))
        r.add_directional_light(color=(1, 1, 1), intensity=2.5, direction=(0.2, -1.0, 0.3), distance=20.0, resolution=512)
        r.set_camera_data(oh.look_at_lh((0, 2.5, -3), (0, 0.5, 5), (0, 1, 0)), ("perspective", 60.0, 0.1))
    for f in range(2):
        fo = o.render(240, 160, ambient=(0.05, 0.05, 0.05, 1), clear_color=(0.1, 0.1, 0.2, 1))
        fp = p.render(240, 160, ambient=(0.05, 0.05, 0.05, 1), clear_color=(0.1, 0.1, 0.2, 1))
        for k in ("visible", "pass", "residual", "vis"):
            assert np.array_equal(fo[k], fp[k][: len(fo[k])] if fo[k].ndim == 1 else fp[k]), k
        assert np.array_equal(fo["atlas"].view(np.uint32), fp["atlas"].view(np.uint32))  # cutout holes in the shadow map too
        ho, hp = fo["hdr16"].astype(np.int32), fp["hdr16"].astype(np.int32)
        assert np.abs(ho - hp).max() <= 2, np.abs(ho - hp).max()
        assert np.abs(fo["rgba_f32"] - fp["rgba_f32"]).max() <= 1e-3
    # the cutout object has holes: some of its bounding region shows what is behind it, and the constant-alpha one is gone
    ids = (fo["vis"] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    tri_obj = np.searchsorted(fo["tri_base"], ids[ids >= 0], side="right") - 1
    assert (tri_obj == 2).any() and not (tri_obj == 3).any()


def test_abi_error_behaviour(r3):
    """Error convention of include/r3n.h: negative codes + message, never a crash; 'nothing to draw' is a silent success."""
    from rend3_amd import _ffi
    lib = _ffi.lib()
    r = r3.Renderer(oh.LEFT)
    ctx = r.ctx
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (64, 64))
    clear = np.zeros(4, dtype=f32)
    # outside a frame
    assert lib.r3n_cull(ctx, _ffi.CAMERA_VIEWPORT) == -4 and b"baked" in lib.r3n_last_error(ctx)
    assert lib.r3n_hi_z(ctx) == -4
    assert lib.r3n_frame_end(ctx) == -4
    # unsupported rows fail loudly
    assert lib.r3n_frame_begin(ctx, _ffi.ptr(fu), 64, 64, 2, _ffi.ptr(clear), 32, 32) == -1 and b"samples" in lib.r3n_last_error(ctx)
    assert lib.r3n_frame_begin(ctx, _ffi.ptr(fu), 0, 64, 1, _ffi.ptr(clear), 32, 32) == -1
    assert lib.r3n_frame_begin(ctx, _ffi.ptr(fu), 64, 64, 1, _ffi.ptr(clear), 32, 32) == 0
    assert lib.r3n_forward(ctx, _ffi.CAMERA_VIEWPORT, _ffi.PASS_FORWARD, _ffi.SOURCE_PREDICTED, _ffi.KEY_BLEND) in (0, -1)
    assert lib.r3n_forward(ctx, _ffi.CAMERA_VIEWPORT, 7, 0, 0) == -1
    # header / capacity mismatches
    hdr = r3.host.camera_header(r.camera, None, (64, 64), 1, r.capacity + 1)
    assert lib.r3n_uniform_bake(ctx, _ffi.CAMERA_VIEWPORT, _ffi.ptr(hdr)) == -1
    hdr = r3.host.camera_header(r.camera, 3, (64, 64), 1, r.capacity)
    assert lib.r3n_uniform_bake(ctx, _ffi.CAMERA_VIEWPORT, _ffi.ptr(hdr)) == -1
    # empty world: every node is a silent no-op (culler.rs:449-451,705-707; forward.rs:214-242)
    hdr = r3.host.camera_header(r.camera, None, (64, 64), 1, r.capacity)
    assert lib.r3n_uniform_bake(ctx, _ffi.CAMERA_VIEWPORT, _ffi.ptr(hdr)) == 0
    assert lib.r3n_forward(ctx, _ffi.CAMERA_VIEWPORT, _ffi.PASS_FORWARD, _ffi.SOURCE_PREDICTED, _ffi.KEY_OPAQUE) == 0
    assert lib.r3n_hi_z(ctx) == 0 and lib.r3n_cull(ctx, _ffi.CAMERA_VIEWPORT) == 0
    assert lib.r3n_resolve_opaque(ctx) == 0 and lib.r3n_tonemap(ctx, None, 0) == 0 and lib.r3n_frame_end(ctx) == 0
    # too many lights for the LDS light list
    big = np.zeros(16 + 128 * 17, dtype=np.uint8)
    big[:4] = np.array([17], dtype=np.uint32).view(np.uint8)
    assert lib.r3n_lights_write(ctx, _ffi.ptr(big), big.nbytes, None, 0) == -5
    # object slot beyond capacity, shrinking capacity
    rec = np.zeros((1, 32), dtype=np.uint32)
    slot = np.array([r.capacity], dtype=np.uint32)
    assert lib.r3n_objects_write(ctx, _ffi.ptr(slot), _ffi.ptr(rec), 1, r.capacity) == -1
    assert lib.r3n_objects_write(ctx, None, None, 0, 1) == -1
    # Material::key() is 0 .. 2.  Beyond it the object pass's three launch plans would part (kernels_cull.h: the fused plan indexes
    # its three per-key totals by the key, the three-launch plan tests key == 2, the chained plan key >= 2): no such key gets in
    mrec, mslot = np.zeros((1, 52), dtype=f32), np.zeros(1, dtype=np.uint32)
    for bad in (3, 255):
        assert lib.r3n_materials_write(ctx, _ffi.ptr(mslot), _ffi.ptr(mrec), _ffi.ptr(np.array([bad], dtype=np.uint8)), 1) == -1
        assert b"bad key" in lib.r3n_last_error(ctx)
    assert lib.r3n_materials_write(ctx, _ffi.ptr(mslot), _ffi.ptr(mrec), _ffi.ptr(np.array([2], dtype=np.uint8)), 1) == 0
    # encoded textures: formats outside the built set, levels outside the payload, misaligned level 0
    payload = np.zeros(256, dtype=np.uint8)
    desc = np.array([[0, 8, 8, 1, 34, 0, 0, 0]], dtype=np.uint32)
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 256) == -5 and b"format" in lib.r3n_last_error(ctx)
    desc[0, 3:6] = (4, 24, 1)   # Rgba32Float with a generated chain: not a filterable format, the loader never asks for it
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 256) == -5 and b"float" in lib.r3n_last_error(ctx)
    desc[0, 3:6] = (1, 34, 0)
    desc[0, 4] = 14
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 32) == -1   # 4 BC7 blocks need 64 B
    desc[0, 0] = 2
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 256) == -1
    desc[0, 0], desc[0, 3] = 0, 5
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 256) == -1   # an 8 x 8 image has 4 levels
    desc[0, 3] = 4
    assert lib.r3n_textures_write_encoded(ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), 256) == 0
    # animation tables: parent / depth consistency, rig size, clip and key ranges; poses and skinning without matrices
    rig = np.zeros(1, dtype=[("first", np.uint32), ("n", np.uint32), ("depth", np.uint32), ("pad", np.uint32)])
    jt = np.zeros(2, dtype=[("parent", np.int32), ("depth", np.uint32), ("pad", np.uint32, 2), ("ibm", np.float32, 16)])
    clip = np.zeros(1, dtype=[("rig", np.uint32), ("track", np.uint32), ("dur", np.float32), ("pad", np.uint32)])
    trk = np.zeros(2, dtype=np.dtype([("animated", np.uint32), ("kf", np.uint32, 3), ("kc", np.uint32, 3), ("vf", np.uint32, 3),
                                      ("bt", np.float32, 3), ("br", np.float32, 4), ("bs", np.float32, 3)]))
    tv = np.zeros(8, dtype=f32)

    def write():
        return lib.r3n_animation_write(ctx, _ffi.ptr(rig), 1, _ffi.ptr(jt), 2, _ffi.ptr(clip), 1, _ffi.ptr(trk), 2, _ffi.ptr(tv), 8, _ffi.ptr(tv), 8)
    rig[0] = (0, 2, 1, 0)
    jt["parent"], jt["depth"] = [-1, 0], [0, 1]
    assert write() == 0
    jt["depth"] = [0, 0]
    assert write() == -1 and b"depth" in lib.r3n_last_error(ctx)
    jt["depth"], jt["parent"] = [0, 1], [-1, 2]
    assert write() == -1
    jt["parent"] = [-1, 0]
    rig[0] = (0, 600, 1, 0)
    assert write() == -6
    rig[0] = (0, 2, 1, 0)
    trk["kc"][1] = [0, 3, 0]   # 3 quaternion keys need 12 values, the pool has 8
    assert write() == -1
    trk["kc"][1] = [0, 2, 0]
    assert write() == 0
    rq = np.zeros(1, dtype=[("clip", np.uint32), ("time", np.float32), ("base", np.uint32), ("pad", np.uint32)])
    rq["clip"] = 1
    assert lib.r3n_pose_skeletons(ctx, _ffi.ptr(rq), 1) == -1
    sk = np.zeros((1, 10), dtype=np.uint32)
    assert lib.r3n_skinning(ctx, _ffi.ptr(sk), 1, None, 2) == -1 and b"no joint matrices" in lib.r3n_last_error(ctx)
    r.close()


def test_msaa_goldens(r3):
    """rend3-test/tests/msaa.rs (row N4): SampleCount::Four on the reference's two MSAA scenes -- HIP == oracle bit for
    bit (per-sample keys included) and the HIP image against the goldens (RGB exact; see test_oracle_goldens for alpha)."""
    for build, name in ((G.build_msaa_triangle, "four"), (G.build_sample_coverage, "sample-coverage-4")):
        o, p = both(r3, oh.LEFT)
        build(o, oh, omk)
        build(p, r3.host, r3.material_record)
        for f in range(2):
            fo = o.render(64, 64, samples=4)
            fp = p.render(64, 64, samples=4)
            compare_frames(fo, fp, f"msaa {name} frame {f}")
        gold = G.load(f"rend3-test/msaa/{name}.png")
        assert np.array_equal(fp["rgba8"][..., :3], gold[..., :3]), name


@pytest.mark.parametrize("handedness", [oh.LEFT, oh.RIGHT])
def test_msaa_random_scene_multi_frame(r3, handedness):
    """SampleCount::Four on the lit multi-frame scene of test_random_scene_multi_frame: per-sample keys, depth-min
    Hi-Z, temporal predicted / residual sets (no sub-pixel rejection under the multisample flag), cutout alpha per
    pixel, shaded samples and their box resolve -- all bit-identical to the oracle."""
    o, p = both(r3, handedness, f32(320) / f32(192))
    scenes.build_random_scene(o, oh, omk, 300, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    scenes.build_random_scene(p, oh, r3.material_record, 300, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    look = oh.look_at_lh if handedness == oh.LEFT else oh.look_at_rh
    for f in range(3):
        ang = 0.35 * f
        eye = (3.0 * math.sin(ang), 1.0 + 0.5 * f, -3.0 * math.cos(ang))
        for r in (o, p):
            r.set_camera_data(look(eye, (10 * math.sin(ang + 0.3), 0, 10 * math.cos(ang + 0.3)), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, samples=4, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=4, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"msaa random scene frame {f}")


def test_msaa_edge_queue_overflow(r3, monkeypatch):
    """The split MSAA resolve queues the extra triangles of edge pixels; with the queues shrunk to 8 entries per
    sub-list (R3N_EDGE_CAPACITY) almost every edge pixel overflows and shades itself in the first pass: same frame."""
    monkeypatch.setenv("R3N_EDGE_CAPACITY", "8")
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    scenes.build_random_scene(o, oh, omk, 200, 0xED6E, lights=1, with_cutout=True)
    scenes.build_random_scene(p, oh, r3.material_record, 200, 0xED6E, lights=1, with_cutout=True)
    for f in range(2):
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh((3.0 + f, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, samples=4, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=4, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"edge queue overflow frame {f}")


def test_exchange_path_single_rank(r3):
    """The multi-GPU exchange plumbing on one GPU: a one-rank RCCL process group, the context's buffers wrapped as torch
    tensors on the context's own stream (rend3_amd/parallel.py Exchange), MAX all-reduces of the shadow atlas and the pass-1
    keys, the reduce-scatter of the pass-2 keys, row range + row gather: the frames still equal the oracle's.  (World
    size 2 is covered on the CPU with gloo, tests/test_multi_rank_gloo.py.)"""
    import torch
    import torch.distributed as dist
    from rend3_amd import parallel
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        o, p = both(r3, oh.LEFT, f32(320) / f32(192))
        scenes.build_random_scene(o, oh, omk, 150, 0xE8C4, lights=2, with_cutout=True)
        scenes.build_random_scene(p, oh, r3.material_record, 150, 0xE8C4, lights=2, with_cutout=True)
        ex = parallel.Exchange(p, torch.device("cuda", 0))
        ex.rows_equal = True
        p.set_object_range(0, p.capacity)
        p._check(p.lib.r3n_set_row_range(p.ctx, 0, 192), "r3n_set_row_range")
        for f in range(3):
            for r in (o, p):
                r.set_camera_data(oh.look_at_lh((3.0 + f, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
            fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
            fp = p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0), exchange=ex)
            ex.gather_rows(320, 192, 1)
            compare_frames(fo, fp, f"exchange path frame {f}")
        # frames in flight: nothing read back between the frames, the row gather enqueued on the resolve's stream
        # (r3n_output_buffer_async / r3n_output_work_enqueued) while the next frame's culling is already being enqueued
        for f in range(3, 6):
            for r in (o, p):
                r.set_camera_data(oh.look_at_lh((3.0 + f, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
            fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
            assert p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0), exchange=ex, readback=False) is None
            ex.gather_rows(320, 192, 1)
        fp = p.readback_frame(p.evaluate_instructions(), 320, 192)
        compare_frames(fo, fp, "exchange path, frames in flight, last frame")
        p.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("samples,height", [(1, 192), (4, 192)])
def test_native_comm_single_rank(r3, samples, height):
    """r3n_comm_init: the sort-first exchanges issued by the library itself over RCCL (loaded at run time) inside
    r3n_render_frame -- shadow rectangles packed / broadcast / unpacked on the shadow lane's stream, the depth bands (keys under
    MSAA) gathered in place in front of Hi-Z, the Rgba8 rows gathered behind the resolve -- with a one-rank communicator set,
    which runs every call of the path except the per-band broadcasts of a ragged row split (one rank always divides the
    height): the frames equal the oracle's, also with frames in flight.
    World size 2 of the same scheme: tests/test_zzz_multi_process_gpu.py[rows] and test_two_rank_gloo_rows_exact (Python exchange)."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(height))
    scenes.build_random_scene(o, oh, omk, 150, 0xE8C5, lights=2, with_cutout=True)
    scenes.build_random_scene(p, oh, r3.material_record, 150, 0xE8C5, lights=2, with_cutout=True)
    p.comm_init(0, 1, lambda ids: ids)
    kw = dict(samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
    for f in range(3):
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh((3.0 + f, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, height, **kw)
        fp = p.render(320, height, **kw)
        compare_frames(fo, fp, f"native comm frame {f}")
    for f in range(3, 6):  # frames in flight
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh((3.0 + f, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, height, **kw)
        assert p.render(320, height, readback=False, **kw) is None
    fp = p.readback_frame(p.evaluate_instructions(), 320, height, samples)
    compare_frames(fo, fp, "native comm, frames in flight, last frame")
    st = p.stage_times()
    assert st["exchange_shadow"][1] > 0 and st["exchange_depth"][1] > 0 and st["exchange_rows"][1] > 0
    with pytest.raises(RuntimeError):
        p.render(320, height, exchange=lambda *a, **k: None, **kw)
    p.comm_destroy()
    fo = o.render(320, height, **kw)
    fp = p.render(320, height, **kw)  # back to a single-rank context
    compare_frames(fo, fp, "after comm_destroy")
    p.close()


def test_target_size_limits_fail_loudly(r3):
    """The rasteriser addresses its targets with 32-bit byte offsets: r3n_frame_begin refuses a target of 2^29 samples or more
    (and a side above 65 535) instead of rendering garbage -- before anything is allocated -- and the context stays usable."""
    p = r3.Renderer(oh.LEFT, f32(1.0))
    scenes.build_random_scene(p, r3.host, r3.material_record, 20, 0xE8C6, lights=1)
    p.set_camera_data(oh.look_at_lh((3.0, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
    for w, h, samples in ((32768, 16384, 1), (16384, 8192, 4), (70000, 16, 1)):
        with pytest.raises(RuntimeError) as e:
            p.render(w, h, samples=samples, readback=False)
        assert "target" in str(e.value)
    out = p.render(64, 48)
    assert out["rgba8"].shape == (48, 64, 4)
    p.close()


def test_golden_textured_quad_example(r3):
    """examples/src/textured_quad/mod.rs at 1280x720 (row N2): albedo texture, nearest sampler, sRGB decode -- HIP ==
    oracle bit for bit, and the HIP image against the reference's screenshot (Threshold::Mean(0.0): RGB exact)."""
    w, h = 1280, 720
    o, p = both(r3, oh.LEFT, f32(w) / f32(h))
    G.build_textured_quad(o, oh, omk)
    G.build_textured_quad(p, r3.host, r3.material_record)
    for f in range(2):
        fo = o.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        fp = p.render(w, h, clear_color=(0.10, 0.05, 0.10, 1.0))
        compare_frames(fo, fp, f"textured_quad frame {f}")
    assert np.array_equal(fp["rgba8"][..., :3], G.load("textured_quad-screenshot.png")[..., :3])


@pytest.mark.parametrize("handedness,samples", [(oh.LEFT, 1), (oh.RIGHT, 1), (oh.LEFT, 4)])
def test_textured_scene_multi_frame(r3, handedness, samples):
    """Row N2 on a lit multi-frame scene: five textures (sRGB / linear, odd extents, 1x1, generated mip chains), linear
    and nearest samplers over magnified and heavily minified surfaces, uv transform, texture x value / vertex, unlit,
    and cutout materials whose alpha is the texture's (forward pass and shadow views, each with its own derivative
    rules): visible sets, keys, atlas and HDR bit-identical to the oracle, also under MSAA x4."""
    o, p = both(r3, handedness, f32(320) / f32(192))
    scenes.build_textured_scene(o, oh, omk, 200, 0xBEEF, handedness=handedness, lights=2)
    scenes.build_textured_scene(p, oh, r3.material_record, 200, 0xBEEF, handedness=handedness, lights=2)
    look = oh.look_at_lh if handedness == oh.LEFT else oh.look_at_rh
    for f in range(3):
        eye = (-14.0 + 3.0 * f, 3.0 + f, -14.0 + 2.0 * f)
        for r in (o, p):
            r.set_camera_data(look(eye, (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"textured scene frame {f}")


def test_pbr_class_map_extents(r3):
    """The PBR class's batched three-map sampler (texture.h tex_sample3_batched: base colour + normal + AO / roughness / metallic
    maps, plain flags) over every relation of the maps' extents it distinguishes -- the same extents, half the extents with one
    level less (the level of detail of the largest map shifted by one; at level 0 the smaller map's footprint is the larger's
    level 1), a map missing, the SMALLER map first in slot order -- and over extents it declines (a quarter, a rectangle against a
    square, a short mip chain: the whole wavefront then samples one map at a time); one map per surface is magnified, the far ones
    minified down to their last levels.  Keys, atlas and HDR bit-identical to the oracle, two frames."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    rng = np.random.default_rng(0x3A7)

    def build(r, mk):
        def tex(w, h, srgb, mips="maximum"):
            img = np.random.default_rng(w * 131 + h * 7 + int(srgb)).integers(0, 256, (h, w, 4), dtype=np.uint8)
            return r.add_texture_2d(img, srgb=srgb, mip_count=mips, mip_source="generated")
        a64, n64, o64 = tex(64, 64, True), tex(64, 64, False), tex(64, 64, False)
        o32, n32, o16 = tex(32, 32, False), tex(32, 32, False), tex(16, 16, False)
        a128x32, a64short = tex(128, 32, True), tex(64, 64, True, mips=3)
        combos = [(a64, n64, o64), (a64, n64, o32), (a64, n32, o32), (a64, n64, None), (None, n64, o32), (a64, None, o32),
                  (a64, n64, o16), (a128x32, n64, o32), (a64short, n64, o32), (a64, n32, o64)]
        mats = []
        for (ta, tn, to) in combos:
            kw = dict(roughness=0.6, metallic=0.3)
            if ta is not None:
                kw.update(albedo_mode="texture", albedo_texture=ta)
            else:
                kw.update(albedo=(0.8, 0.7, 0.6, 1.0), albedo_mode="value")
            if tn is not None:
                kw.update(normal_texture=tn)
            if to is not None:
                kw.update(aomr=("combined", to))
            mats.append(r.add_material(mk(**kw)))
        pq = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=f32)
        iq = np.array([0, 2, 1, 0, 3, 2], dtype=np.uint32)
        nq = np.tile(np.array([[0, 1, 0]], dtype=f32), (4, 1))
        uv = np.array([[0, 0], [3, 0], [3, 3], [0, 3]], dtype=f32)
        quad = r.add_mesh(pq, iq, normals=nq, uv0=uv, tangents=scenes._tangents(nq))
        for k, m in enumerate(mats):  # a row of long strips running away from the camera: magnified near, minified far
            r.add_object(quad, m, oh.mat4_mul(oh.translation((-9.0 + 2.0 * k, 0.0, 30.0)), oh.scale((0.95, 1.0, 32.0))))
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -2.0, 0.4), distance=60.0, resolution=256)

    build(o, omk)
    build(p, r3.material_record)
    for f in range(2):
        eye = (0.5 * f, 1.2 + 0.8 * f, -2.5)
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 20.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"pbr class extents frame {f}")
    assert (fo["vis"] != 0).mean() > 0.3  # the strips fill a good part of the frame


def test_generated_mip_chains_match_oracle(r3):
    """MipmapSource::Generated (rend3/src/util/mipmap.rs:139-236 + mipmap.wgsl, K11): the chain the library builds on the
    GPU at upload (Linear / ClampToEdge blit per level in the texture's own format; sRGB levels decoded, filtered and
    re-encoded through the threshold table) against the oracle's, every level byte for byte: sRGB and linear formats,
    even / odd / degenerate extents, and R8 / RG8 / BGRA8 sources expanded first."""
    import test_texture_formats as T
    o, p = both(r3)
    rng = np.random.default_rng(5)
    want = []
    for (w, h, srgb) in [(64, 64, True), (37, 19, True), (128, 40, False), (1, 7, True), (5, 1, False), (256, 256, True)]:
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if (w, h) == (256, 256):  # every code next to every other: exercises the encode thresholds densely
            img[..., 0] = np.arange(256, dtype=np.uint8)[None, :]
            img[..., 1] = np.arange(256, dtype=np.uint8)[:, None]
        p.add_texture_2d(img, srgb=srgb, mip_count="maximum", mip_source="generated")
        t = o.add_texture_2d(img, srgb=srgb, mip_count="maximum", mip_source="generated")
        d = o.tex_descs[t]
        n = sum(max(1, w >> k) * max(1, h >> k) for k in range(int(d[3])))
        want.append(o.tex_pool[int(d[0]): int(d[0]) + n].view(np.uint8).reshape(-1, 4))
    for fmt, width in ((T.C.R8, 1), (T.C.RG8, 2), (T.C.BGRA8_SRGB, 4)):
        w, h = 23, 10
        raw = rng.integers(0, 256, (h, w, width), dtype=np.uint8)
        p.add_texture_2d_encoded(fmt, w, h, [raw.tobytes()], generate_mips=True)
        t = o.add_texture_2d_encoded(fmt, w, h, [raw.tobytes()], generate_mips=True)
        d = o.tex_descs[t]
        n = sum(max(1, w >> k) * max(1, h >> k) for k in range(int(d[3])))
        want.append(o.tex_pool[int(d[0]): int(d[0]) + n].view(np.uint8).reshape(-1, 4))
    got = p.readback_texels()
    want = np.concatenate(want)
    assert got.shape == want.shape
    bad = (got != want).any(axis=1)
    assert not bad.any(), f"{bad.sum()} of {len(bad)} texels differ, first at {np.nonzero(bad)[0][:4]}: {got[bad][:4].tolist()} vs {want[bad][:4].tolist()}"


def test_texture_decode_matches_oracle(r3):
    """Row N2, formats: every source format r3n_textures_write_encoded accepts, decoded / expanded on the GPU
    (csrc/texture_decode.hip) against the oracle's decoders (oracle/bcn.c, pinned on an independent decoder's output):
    the committed block vectors (every BC7 mode x partition, punch-through BC1, both endpoint orders), random blocks with
    extents that are not multiples of the block and stored mip chains down to 1 x 1, and the uncompressed expansions.
    Byte work: bit-exact."""
    import test_texture_formats as T
    o, p = both(r3)
    rng = np.random.default_rng(0xDEC0DE)
    expect = []
    for case in T.CASES:
        fmt, w, h = (int(v) for v in T.GOLD[case + "_meta"])
        data = T.GOLD[case + "_data"].tobytes()
        p.add_texture_2d_encoded(fmt, w, h, [data])
        expect.append(T.oracle_decode(fmt, w, h, data).reshape(-1, 4))
    for fmt in range(2, 16):
        w, h = (37, 21) if fmt >= 6 else (13, 7)
        levels = []
        for k in range(int(max(w, h)).bit_length()):
            lw, lh = max(1, w >> k), max(1, h >> k)
            data = rng.integers(0, 256, T.C.level_bytes(fmt, lw, lh), dtype=np.uint8).tobytes()
            levels.append(data)
            expect.append(T.oracle_decode(fmt, lw, lh, data).reshape(-1, 4))
        p.add_texture_2d_encoded(fmt, w, h, levels)
    got = p.readback_texels()
    want = np.concatenate(expect)
    assert got.shape == want.shape
    bad = (got != want).any(axis=1)
    assert not bad.any(), f"{bad.sum()} of {len(bad)} texels differ, first at {np.nonzero(bad)[0][:4]}"
    del o


def test_float_texture_decode_matches_oracle(r3):
    """Row N2, the formats whose texels are not 8-bit unorm (snorm, 16-bit, float, packed float, BC4 / BC5 snorm, BC6H):
    decoded on the GPU into four f32 per texel against the oracle's decoders (oracle/bcn.c r3o_texture_decode_level_f32,
    pinned on numpy restatements and an independent block decoder): the committed BC6H / BC5-snorm vectors (every BC6H mode),
    random data with the special encodings planted, extents that are not block multiples, stored chains down to 1 x 1, mixed
    with RGBA8 textures in the same array.  Bit patterns must agree, NaN payloads and signed zeros included."""
    import test_texture_formats as T
    o, p = both(r3)
    rng = np.random.default_rng(0xF10A7)
    expect = []
    for name in ("bc6h_uf", "bc6h_sf", "bc5s"):
        fmt, w, h = (int(v) for v in T.FLOAT_GOLD[name + "_meta"])
        data = T.FLOAT_GOLD[name + "_data"].tobytes()
        p.add_texture_2d_encoded(fmt, w, h, [data])
        expect.append(T.oracle_decode_f32(fmt, w, h, data).reshape(-1, 4))
    rgba = rng.integers(0, 256, (5, 9, 4), dtype=np.uint8)
    p.add_texture_2d(rgba, srgb=True)  # an RGBA8 texture between the float ones: both kinds share the pool
    expect.append(rgba.reshape(-1, 4))
    for fmt in range(16, 34):
        w, h = (37, 21) if fmt >= 30 else (37, 23)
        levels = []
        for k in range(int(max(w, h)).bit_length()):
            lw, lh = max(1, w >> k), max(1, h >> k)
            data = T.float_format_level(fmt, lw, lh, rng) if fmt < 30 and k == 0 else rng.integers(0, 256, T.C.level_bytes(fmt, lw, lh), dtype=np.uint8).tobytes()
            levels.append(data)
            expect.append(T.oracle_decode_f32(fmt, lw, lh, data).reshape(-1, 4))
        p.add_texture_2d_encoded(fmt, w, h, levels)
    got = p.readback_texels(per_texture=True)
    assert len(got) == 4 + 18
    at = 0
    for t, g in enumerate(got):
        want = np.concatenate(expect[at:at + (1 if t < 4 else int(37).bit_length())])
        at += 1 if t < 4 else int(37).bit_length()
        assert g.shape == want.shape and g.dtype == want.dtype, (t, g.shape, want.shape)
        gb, wb = (g.view(np.uint32), want.view(np.uint32)) if g.dtype == np.float32 else (g, want)
        bad = (gb != wb).any(axis=1)
        assert not bad.any(), f"texture {t}: {bad.sum()} of {len(bad)} texels differ, first at {np.nonzero(bad)[0][:4]}: {g[bad][:2].tolist()} vs {want[bad][:2].tolist()}"
    with pytest.raises(ValueError):
        p.add_texture_2d_encoded(24, 8, 8, [bytes(8 * 8 * 16)], generate_mips=True)  # Rgba32Float is not filterable: no generated chains
    del o


def test_generated_float_mip_chains_match_oracle(r3):
    """MipmapSource::Generated for the float-decoded formats the loader generates chains for (single-level R16Float / Rg16Float /
    Rgba16Float / Rgb10a2Unorm files): level 0 decoded and every further level blitted and rounded to the format on the GPU,
    against the oracle's chain (oracle/bcn.c r3o_generate_mips_f32; binary16 rounding pinned on numpy), bit patterns equal (NaNs:
    as NaNs) -- power-of-two, odd and 1-wide extents, values with infinities / NaNs / subnormals in level 0."""
    import test_texture_formats as T
    o, p = both(r3)
    rng = np.random.default_rng(0x3170)
    handles = []
    for fmt in (T.C.R16F, T.C.RG16F, T.C.RGBA16F, T.C.RGB10A2):
        for (w, h) in ((64, 32), (37, 19), (1, 9), (5, 1)):
            data = T.float_format_level(fmt, w, h, rng) if w * h >= 64 else rng.integers(0, 256, T.C.level_bytes(fmt, w, h), dtype=np.uint8).tobytes()
            if fmt != T.C.RGB10A2 and (w, h) == (64, 32):
                # mostly finite mid-range values so that the rounding of sums is exercised, the special encodings stay in front
                a = np.frombuffer(data, dtype=np.uint16).copy()
                a[64:] = (rng.random(len(a) - 64) * 4.0 - 2.0).astype(np.float16).view(np.uint16)
                data = a.tobytes()
            hp = p.add_texture_2d_encoded(fmt, w, h, [data], generate_mips=True)
            ho = o.add_texture_2d_encoded(fmt, w, h, [data], generate_mips=True)
            assert hp == ho
            handles.append((fmt, w, h))
    got = p.readback_texels(per_texture=True)
    assert len(got) == len(handles)
    for t, (fmt, w, h) in enumerate(handles):
        d = o.tex_descs[t]
        mips = int(max(w, h)).bit_length()
        assert int(d[3]) == mips and int(d[4]) == 2
        n = sum(max(1, w >> k) * max(1, h >> k) for k in range(mips))
        want = o.tex_pool[int(d[0]): int(d[0]) + 4 * n].reshape(-1, 4)
        g = got[t].view(np.uint32)
        assert g.shape == want.shape, (t, g.shape, want.shape)
        # a NaN produced by the blit's arithmetic (inf * 0, inf - inf) has no defined sign / payload: x86 and the GPU differ there;
        # NaN-ness itself must agree
        both_nan = np.isnan(g.view(np.float32)) & np.isnan(want.view(np.float32))
        bad = ((g != want) & ~both_nan).any(axis=1)
        assert not bad.any(), f"{T.C.FORMAT_NAMES[fmt]} {w}x{h}: {bad.sum()} of {len(bad)} texels differ, first at {np.nonzero(bad)[0][:4]}"


@pytest.mark.parametrize("samples", [1, 4])
def test_float_textures_in_a_scene(r3, samples):
    """The textured multi-frame scene over float-decoded textures in every material slot (HDR albedo above 1, snorm normal
    map, BC6H emissive, cutout alpha from an Rgba16Float texture): the sampler's float-texel path against the oracle's --
    visible sets, keys, atlas and HDR bit-identical."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    scenes.build_textured_scene(o, oh, omk, 200, 0xF16, lights=2, encoded="float")
    scenes.build_textured_scene(p, oh, r3.material_record, 200, 0xF16, lights=2, encoded="float")
    for f in range(2):
        eye = (-14.0 + 4.0 * f, 3.0 + f, -14.0 + 3.0 * f)
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"float textures frame {f}")


@pytest.mark.parametrize("samples", [1, 4])
def test_encoded_textures_in_a_scene(r3, samples):
    """The textured multi-frame scene over block-compressed / BGRA / RG / R textures (stored and generated chains):
    what the sampler reads is the decoded pool, so visible sets, keys, atlas and HDR stay bit-identical to the oracle."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    scenes.build_textured_scene(o, oh, omk, 200, 0xBC7, lights=2, encoded=True)
    scenes.build_textured_scene(p, oh, r3.material_record, 200, 0xBC7, lights=2, encoded=True)
    for f in range(2):
        eye = (-14.0 + 4.0 * f, 3.0 + f, -14.0 + 3.0 * f)
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fo = o.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"encoded textures frame {f}")


def test_frames_in_flight_world_mutation(r3):
    """Frames in flight: six frames submitted back to back with no read-back and no host
    synchronisation between them, so the resolve of frame N runs on the shade stream while frame N + 1 is culled and
    rasterised -- and the world changes before EVERY frame: object transforms, a removal, a new object (which moves
    the per-object triangle bases the resolve reads), a material rewrite.  Each world write has to order itself after
    the resolve still in flight.  The last frame must be bit-identical to the oracle that rendered the same sequence
    (the oracle needs every frame for the temporal state: previous-frame masks, predicted / residual sets)."""
    W, H = 960, 540
    o, p = both(r3, oh.LEFT, f32(W) / f32(H))
    ho = scenes.build_textured_scene(o, oh, omk, 200, 0xF1F0, handedness=oh.LEFT, lights=2)
    hp = scenes.build_textured_scene(p, oh, r3.material_record, 200, 0xF1F0, handedness=oh.LEFT, lights=2)
    extra = {}
    for r, mk in ((o, omk), (p, r3.material_record)):
        pos, idx, nrm = scenes.box()
        extra[id(r)] = (r.add_mesh(pos, idx, normals=nrm), r.add_material(mk(albedo=(0.9, 0.2, 0.1, 1.0), roughness=0.4)))
    frames = 6
    fo = fp = None
    for f in range(frames):
        eye = (-14.0 + 2.0 * f, 3.0 + 0.5 * f, -14.0 + 1.5 * f)
        for r, hs in ((o, ho), (p, hp)):
            r.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
            for k in range(0, 40, 3):  # moving objects, every frame
                r.set_object_transform(hs[k], oh.mat4_mul(oh.translation((0.4 * f - 6.0 + 0.3 * k, 0.5 + 0.1 * k, 0.25 * f * (k % 5) - 2.0)),
                                                          oh.scale((1.0 + 0.05 * f,) * 3)))
            if f == 2:
                r.remove_object(hs[50])
                r.remove_object(hs[51])
            if f == 3:
                mesh, mat = extra[id(r)]
                r.add_object(mesh, mat, oh.mat4_mul(oh.translation((0.0, 1.0, 0.0)), oh.scale((3.0, 0.5, 3.0))))
            if f == 4:
                mesh, mat = extra[id(r)]
                r.add_object(mesh, mat, oh.translation((-3.0, 2.0, 1.0)))
                mk = omk if r is o else r3.material_record
                r.update_material(mat, mk(albedo=(0.1, 0.8, 0.3, 1.0), roughness=0.7, metallic=1.0))
            if f == 5:
                r.update_directional_light(0, intensity=5.0, direction=(0.4, -1.0, 0.3))
        last = f == frames - 1
        fo = o.render(W, H, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(W, H, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0), readback=last)
    compare_frames(fo, fp, "frames in flight, last frame")
    assert fo["visible"].sum() > 0 and fo["pass"].sum() > 0


@pytest.mark.parametrize("handedness,samples,textured", [(oh.LEFT, 1, False), (oh.RIGHT, 1, True), (oh.LEFT, 4, True)])
def test_transparent_pass_multi_frame(r3, handedness, samples, textured):
    """Row N3: translucent (TransparencyType::Blend) objects over the lit random scene, four frames with the camera
    moving (the back-to-front order changes) and one translucent object moved (its sorting location switches from the
    bounding-sphere centre to the translation, object.rs:273,313): ordered ALPHA_BLENDING against the opaque depth,
    also per sample under MSAA x4 and with a textured translucent material -- HDR bit-identical to the oracle."""
    o, p = both(r3, handedness, f32(320) / f32(192))
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 120, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    ho = scenes.add_blend_objects(o, oh, omk, 0xB1E2D, textured=textured)
    hp = scenes.add_blend_objects(p, oh, r3.material_record, 0xB1E2D, textured=textured)
    look = oh.look_at_lh if handedness == oh.LEFT else oh.look_at_rh
    zs = 1.0 if handedness == oh.LEFT else -1.0
    for f in range(4):
        eye = (-2.0 + 1.5 * f, 1.0 + 0.3 * f, zs * (-3.0 + 0.5 * f))
        for r in (o, p):
            r.set_camera_data(look(eye, (0.5 * f, 0.5, zs * 8.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        if f == 2:
            for r, hs in ((o, ho), (p, hp)):
                r.set_object_transform(hs[1], oh.mat4_mul(oh.translation((0.5, 1.0, zs * 5.0)), oh.scale((2.0, 2.0, 0.2))))
        if handedness == oh.RIGHT and f == 0:
            pass
        fo = o.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        assert len(fo["blend_list"][0]) > 0
        compare_frames(fo, fp, f"transparent frame {f}")


def test_material_key_flip_between_frames(r3):
    """A material's transparency key rewritten between frames through the raw material write (the reference fixes a material's
    archetype, this ABI does not): BLEND -> OPAQUE -> BLEND.  The host mirror's cached blend-object list must follow, else the
    objects of that material are drawn by no pass at all (or by two).  The frame of the flip itself is outside the reference's
    domain (last frame's predicted triangles sit in the draw range of the OLD key), so camera and scene stand still and the
    third frame after every flip is compared: by then the temporal state has converged to the same fixed point on both sides."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 80, 0xF11B, lights=1)
    scenes.add_blend_objects(o, oh, omk, 0xB1E2E)
    scenes.add_blend_objects(p, oh, r3.material_record, 0xB1E2E)
    blend_mats = [i for i, (_rec, key) in enumerate(o.materials) if key == scenes.BLEND]
    assert blend_mats
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((-2.0, 1.0, -3.0), (0.0, 0.5, 8.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    sizes = []
    for key in (scenes.BLEND, scenes.OPAQUE, scenes.BLEND):
        for r in (o, p):
            for m in blend_mats[:3]:
                r.update_material(m, r.materials[m][0], key=key)
        for f in range(3):
            fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
            fp = p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0), readback=(f == 2))
        compare_frames(fo, fp, f"third frame after the flip to key {key}")
        sizes.append(len(fo["blend_list"][0]))
    assert sizes[1] < sizes[0] and sizes[2] == sizes[0]


@pytest.mark.parametrize("output_format", [0, 1, 2, 3])
def test_tonemap_every_half_value(r3, output_format):
    """blit.wgsl + the 8-bit store over EVERY Rgba16Float bit pattern (all 65536 halves in every channel, NaN / inf /
    negative / denormal included), for the four output formats of TonemappingRoutine (Rgba8 / Bgra8, *Srgb targets with
    the exact OETF, plain unorm targets with the shader's srgb_scene_to_display, exponent 0.4166): the device's table and
    the stand-alone blit kernel against the oracle's direct evaluation, byte for byte; the float view within 1 ulp-scale
    tolerance of the same formula."""
    from rend3_amd import _ffi
    from oracle import lib as olib
    lib = _ffi.lib()
    r = r3.Renderer(oh.LEFT)
    assert lib.r3n_set_output_format(r.ctx, 4) == -1
    r.set_output_format(output_format)
    w = h = 256
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (w, h))
    clear = np.zeros(4, dtype=f32)
    assert lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), w, h, 1, _ffi.ptr(clear), 32, 32) == 0
    halves = np.arange(65536, dtype=np.uint16)
    hdr = np.stack([halves, halves[::-1], np.roll(halves, 12345), halves], axis=1).copy()
    assert lib.r3n_hdr_write(r.ctx, _ffi.ptr(hdr), 0, w * h) == 0
    assert lib.r3n_hdr_write(r.ctx, _ffi.ptr(hdr), 1, w * h) == -1  # range check
    assert lib.r3n_tonemap(r.ctx, None, 0) == 0
    got8 = np.zeros((w * h, 4), dtype=np.uint8)
    gotf = np.zeros((w * h, 4), dtype=f32)
    assert lib.r3n_readback_output(r.ctx, _ffi.ptr(got8), _ffi.ptr(gotf)) == 0
    assert lib.r3n_frame_end(r.ctx) == 0
    o = olib.get()
    exp8 = np.zeros((w * h, 4), dtype=np.uint8)
    expf = np.zeros((w * h, 4), dtype=f32)
    o.r3o_tonemap_format(o.ptr(hdr), w * h, o.ptr(expf), o.ptr(exp8), output_format)
    bad = np.nonzero((got8 != exp8).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), hdr[bad[:5]], got8[bad[:5]], exp8[bad[:5]])
    assert np.allclose(gotf, expf, rtol=0, atol=2e-7 if output_format < 2 else 1e-6, equal_nan=True)
    r.close()


def test_output_formats_on_a_frame(r3):
    """A lit frame into a Bgra8Unorm target (the fused blit of the resolve: swizzle + manual transfer function), then
    back to the default: both equal the oracle's tonemap of the same HDR buffer."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    scenes.build_random_scene(o, oh, omk, 120, 0xF0F0, lights=1)
    scenes.build_random_scene(p, oh, r3.material_record, 120, 0xF0F0, lights=1)
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((3.0, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
    for fmt in (3, 0):
        o.output_format = fmt
        p.set_output_format(fmt)
        fo = o.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        compare_frames(fo, fp, f"output format {fmt}")
    assert (fo["rgba8"][..., :3].max(axis=2) > 40).mean() > 0.05


# ------------------------------------------------------------------ the benchmarked workload (BASELINE.json configs[2])
def _config3_pair(r3, w, h, **kw):
    """bench.py's scene on both sides: rend3_amd/scenes.py::bistro_like with every object owning its geometry."""
    import rend3_amd.scenes as S
    o, p = both(r3, oh.RIGHT, f32(w) / f32(h))
    io = S.bistro_like(o, oh, omk, unique=True, **kw)
    ip = S.bistro_like(p, r3.host, r3.material_record, unique=True, **kw)
    assert io["triangles"] == ip["triangles"] == io["unique_triangles"]
    return o, p, io


def test_config3_bistro_like(r3):
    """The benchmarked frame at a size the oracle finishes in seconds: bench.py's scene generator (street canyon, unique
    geometry per object), textured (base colour + normal + AO/roughness/metallic maps, trilinear), 4 directional lights
    with their shadow views, bench.py's camera dolly over three frames (so the predicted pass, the Hi-Z cull against it
    and the residual pass all carry history), 1920x1080 -- every frame bit-exact like the small scenes: L1 / L2 sets of
    the five cameras, keys, atlas, HDR; framebuffer within 1e-3.  Reference: examples/src/scene_viewer/mod.rs:727-751
    (camera, light, resolution of the Bistro test)."""
    import bench
    w, h = 1920, 1080
    o, p, info = _config3_pair(r3, w, h, n_objects=1200, target_tris=300_000, textured=True, tex_size=256, shadow_res=1024)
    assert info["triangles"] > 400_000
    view0, proj = info["camera"]
    for k in range(3):
        o.set_camera_data(bench.camera_path(oh, view0, k), proj)
        p.set_camera_data(bench.camera_path(r3.host, view0, k), proj)
        fo = o.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        fp = p.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        compare_frames(fo, fp, f"config 3 frame {k}")
        assert len(fo["shadows"]) == 4 and all(s["pass"].sum() > 1000 for s in fo["shadows"])
    assert fo["residual"].sum() > 0 and fo["pass"].sum() > 10_000  # the dolly keeps the residual pass busy
    assert (fo["vis"] != 0).mean() > 0.9


def test_config3_bistro_v2(r3):
    """The Bistro-faithful variant of the bench scene (bench.py --bistro-v2) at a size the oracle finishes in
    seconds: the maps arrive as BC7 with stored mip chains (decoded at upload on both sides), a fifth of the triangles are
    alpha-tested foliage cards on the CUTOUT key whose alpha comes from a leaf atlas (opaque.wgsl:231-235 in the viewport,
    depth.wgsl:100-127 in the four shadow views), a third of the props are instances of shared meshes; two resolve classes
    (base colour only / the three PBR maps) share the frame.  Three frames of the camera dolly, bit-exact like the other scenes."""
    import bench
    import rend3_amd.scenes as S
    w, h = 1280, 720
    o, p = both(r3, oh.RIGHT, f32(w) / f32(h))
    kw = dict(n_objects=900, target_tris=200_000, unique=True, v2=True, v2_tex_size=256, shadow_res=1024)
    io = S.bistro_like(o, oh, omk, **kw)
    ip = S.bistro_like(p, r3.host, r3.material_record, **kw)
    assert io["triangles"] == ip["triangles"] and io["objects"] == ip["objects"]
    assert io["unique_triangles"] < io["triangles"]  # instanced props and foliage clumps
    view0, proj = io["camera"]
    for k in range(3):
        o.set_camera_data(bench.camera_path(oh, view0, k), proj)
        p.set_camera_data(bench.camera_path(r3.host, view0, k), proj)
        fo = o.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        fp = p.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        compare_frames(fo, fp, f"bistro v2 frame {k}")
    keys = fo["material_keys"][fo["objects"][:, 22]]
    ntri = (fo["objects"][:, 21] // 3) * (fo["objects"][:, 29] != 0)
    assert ntri[keys == 1].sum() >= 0.19 * ntri.sum(), "a fifth of the triangles on the cutout key"
    # the cutout key drew in the viewport and in every shadow view
    tri_obj = np.searchsorted(fo["tri_base"], np.arange(len(fo["pass"])), side="right") - 1
    cut = keys[tri_obj] == 1
    assert (fo["pass"].astype(bool) & cut).sum() > 1000 and all((s["pass"][: len(cut)].astype(bool) & cut).sum() > 1000 for s in fo["shadows"])
    assert fo["residual"].sum() > 0 and (fo["vis"] != 0).mean() > 0.9


def test_config3_4k_frame(r3):
    """bench.py's workload at its full size -- 3840x2160, ~3 000 objects / ~2.8 M unique triangles, 4 shadow views of
    2048^2 -- with factor-only materials (the textured fragment stage is covered above at 1080p; at 4K it would only
    add oracle time): camera steps 0 and 1, both bit-exact.  Exercises what only the full size reaches: the 13-level
    Hi-Z pyramid with its odd-dimension tail, work items from > 32 px triangles in coarse mode, the 2 Mi-entry work
    queue under the ground tiles that cross the near plane, 4096^2 atlas."""
    import bench
    w, h = bench.WIDTH, bench.HEIGHT
    o, p, info = _config3_pair(r3, w, h, textured=False)
    assert info["triangles"] > 2_500_000 and info["mesh_bytes"] > 100_000_000
    view0, proj = info["camera"]
    for k in range(2):
        o.set_camera_data(bench.camera_path(oh, view0, k), proj)
        p.set_camera_data(bench.camera_path(r3.host, view0, k), proj)
        fo = o.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        fp = p.render(w, h, ambient=bench.AMBIENT, clear_color=bench.CLEAR)
        compare_frames(fo, fp, f"config 3 at 4K, frame {k}")
    assert fo["hiz"].size > w * h and fo["residual"].sum() > 0


# ------------------------------------------------------------------ runtime switches: every shipped code path is in the suite
_ORACLE_FRAMES = {}


def _scenario_frames(r3, name, make_renderer):
    """Three small multi-frame scenarios (cutout + two lights + world edits; textured right-handed; the benchmarked scene
    generator with four shadow views).  The oracle's frames are rendered once per scenario and kept; `make_renderer(handedness,
    aspect)` supplies the HIP renderer under test."""
    if name == "random":
        hand, w, h = oh.LEFT, 320, 192
        build = lambda r, hm, mk: scenes.build_random_scene(r, oh, mk, 300, 0xC0FFEE, handedness=hand, lights=2, with_cutout=True)

        def step(f, r, hm, handles):
            ang = 0.35 * f
            eye = (3.0 * math.sin(ang), 1.0 + 0.5 * f, -3.0 * math.cos(ang))
            r.set_camera_data(oh.look_at_lh(eye, (10 * math.sin(ang + 0.3), 0, 10 * math.cos(ang + 0.3)), (0, 1, 0)), ("perspective", 60.0, 0.1))
            if f == 2:
                r.set_object_transform(handles[5], oh.mat4_mul(oh.translation((2.0, 0.5, 6.0)), oh.scale((2, 2, 2))))
                r.remove_object(handles[7])
        frames, kw = 4, dict(ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
    elif name == "textured":
        hand, w, h = oh.RIGHT, 320, 192
        build = lambda r, hm, mk: scenes.build_textured_scene(r, oh, mk, 200, 0xBEEF, handedness=hand, lights=2)

        def step(f, r, hm, handles):
            r.set_camera_data(oh.look_at_rh((-14.0 + 3.0 * f, 3.0 + f, -14.0 + 2.0 * f), (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        frames, kw = 3, dict(ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
    else:  # "bistro": bench.py's generator, four 512^2 shadow views, bench.py's camera dolly
        import bench
        import rend3_amd.scenes as S
        hand, w, h = oh.RIGHT, 960, 540
        build = lambda r, hm, mk: S.bistro_like(r, hm, mk, unique=True, n_objects=600, target_tris=120_000, textured=True, tex_size=128, shadow_res=512)

        def step(f, r, hm, info):
            r.set_camera_data(bench.camera_path(hm, info["camera"][0], f), info["camera"][1])
        frames, kw = 3, dict(ambient=bench.AMBIENT, clear_color=bench.CLEAR)
    if name not in _ORACLE_FRAMES:
        o = OracleRenderer(hand, f32(w) / f32(h))
        ho = build(o, oh, omk)
        out = []
        for f in range(frames):
            step(f, o, oh, ho)
            out.append(o.render(w, h, **kw))
        _ORACLE_FRAMES[name] = out
    p = make_renderer(hand, f32(w) / f32(h))
    hp = build(p, r3.host, r3.material_record)
    for f, fo in enumerate(_ORACLE_FRAMES[name]):
        step(f, p, r3.host, hp)
        yield f, fo, p.render(w, h, **kw)
    p.close()


RUNTIME_SWITCHES = [
    {},                              # the defaults (reference for the others: same scenarios, same oracle frames)
    {"R3N_PIPELINE": "0"},           # no frames in flight: the resolve on the main stream
    {"R3N_SINGLE_STREAM": "1"},      # every camera on the main stream
    {"R3N_FRAME_NODES": "1"},        # the host mirror issues the frame node by node (one C call per reference node) instead of r3n_render_frame
    {"R3N_ALWAYS_FORK": "1"},        # the shadow lanes wait for the main stream at every fork (no epoch gate): a main-stream producer that forgot its epoch bump would differ from the default run
    {"R3N_RESOLVE_CLASSES": "0"},    # the general resolve kernel for every tile instead of one kernel per material class (kernels_shade.h R3N_CLS_*)
    {"R3N_BIG_CAPACITY": "1"},       # one entry per raster work sub-queue: the producers scan what does not fit themselves (kernels_raster.h raster_small_body)
    # launch parameters (r3n.hip Tune: dynamic-LDS occupancy caps and grid sizes; tools/tune_caps.py searches them): results never depend on them
    {"R3N_TUNE": "big_lds=16384 vp_big_lds=0 small_lds=0 vp_small_lds=32768 cut_big_lds=49152 vp_cut_big_lds=32768 cut_small_lds=8192 "
                 "vp_cut_small_lds=16384 cull_lds=32768 vp_cull_lds=16384 resolve_lds=8192 big_grid=1024 small_grid=512"},
]


@pytest.mark.parametrize("scenario", ["random", "textured", "bistro"])
@pytest.mark.parametrize("env", RUNTIME_SWITCHES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "defaults")
def test_runtime_switches(r3, monkeypatch, env, scenario):
    """Every opt-in path the library ships (r3n_create reads the environment, r3n.hip) renders the same frames as the default
    path: all of compare_frames -- sets of every camera, keys, shadow atlas, HDR bit-identical to the oracle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    made = []
    for f, fo, fp in _scenario_frames(r3, scenario, lambda hand, aspect: made.append(r3.Renderer(hand, aspect)) or made[-1]):
        compare_frames(fo, fp, f"{scenario} {env} frame {f}")
        if "R3N_BIG_CAPACITY" in env:  # the queue-full path ran: a call queued more items than the 32 sub-queues hold
            assert made[0].raster_stats().max() > 32 * int(env["R3N_BIG_CAPACITY"]), f"{scenario} frame {f}: no sub-queue overflowed"
            made[0].sync()  # (a capacity report would raise here)
    if scenario == "bistro":
        assert len(fo["shadows"]) == 4 and all(s["pass"].sum() > 200 for s in fo["shadows"]) and (fo["atlas"] != 0).mean() > 0.05


def test_tuning_rejects_what_it_does_not_know(r3):
    """r3n_internal_set_tuning: an unknown key, a value out of range or a malformed pair fails with R3N_ERR_ARG and changes nothing."""
    import ctypes
    p = r3.Renderer(oh.LEFT, f32(1.0))
    fn = p.lib.r3n_internal_set_tuning
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]
    assert fn(p.ctx, b"big_lds=32768 small_grid=1024") == 0
    for bad in (b"big_ldz=1", b"big_lds=1000000", b"big_grid=0", b"big_lds", b"big_lds=abc"):
        assert fn(p.ctx, bad) != 0, bad
    p.close()


def compare_frames_fast(o, p, tag=""):
    """R3N_SHADE_FAST against the oracle: everything in front of the fragment stage stays bit-exact (sets, keys, atlas); the
    shaded image is held to the north-star tolerance: |delta| <= 1e-3 on the tonemapped framebuffer, <= 1 LSB in 8 bit."""
    n = len(o["pass"])
    assert np.array_equal(o["visible"], p["visible"]) and np.array_equal(o["pass"], p["pass"][:n]) and np.array_equal(o["residual"], p["residual"][:n]), tag
    assert np.array_equal(o["vis"], p["vis"]), tag + " visibility keys"
    assert np.array_equal(o["atlas"].view(np.uint32), p["atlas"].view(np.uint32)), tag + " shadow atlas"
    d = np.abs(o["rgba_f32"] - p["rgba_f32"])
    assert d.max() <= 1e-3, tag + f" framebuffer max |delta| {d.max():.2e} at {np.unravel_index(d.argmax(), d.shape)}"
    assert np.abs(o["rgba8"].astype(int) - p["rgba8"].astype(int)).max() <= 1, tag + " rgba8 > 1 LSB"
    return float(d.max()), float((o["hdr16"] != p["hdr16"]).any(axis=2).mean())


def test_shade_mode_fast_within_tolerance(r3):
    """The opt-in fast fragment-stage arithmetic (r3n_set_shade_mode(R3N_SHADE_FAST): fused multiply-add, v_rcp / v_rsq) on
    the lit random scene (point + directional lights, cutouts), the textured scene using every material variant, and the
    benchmarked street scene: framebuffer within 1e-3 of the oracle after tonemap on every frame, everything upstream of
    the fragment stage still bit-exact.  Switching back to EXACT restores bit-identical HDR."""
    import bench
    import rend3_amd.scenes as S
    worst = 0.0
    for name in ("random", "textured", "street"):
        if name == "street":
            w, h = 1280, 720
            o, p = both(r3, oh.RIGHT, f32(w) / f32(h))
            kw = dict(n_objects=600, target_tris=100_000, textured=True, tex_size=128, shadow_res=512)
            info = S.bistro_like(o, oh, omk, **kw)
            S.bistro_like(p, r3.host, r3.material_record, **kw)
            cams = [(bench.camera_path(oh, info["camera"][0], k), info["camera"][1]) for k in range(3)]
            amb, clear = bench.AMBIENT, bench.CLEAR
        else:
            w, h = 320, 192
            o, p = both(r3, oh.LEFT, f32(w) / f32(h))
            for r, mk in ((o, omk), (p, r3.material_record)):
                if name == "random":
                    scenes.build_random_scene(r, oh, mk, 150, 0xFA57, lights=2, with_cutout=True)
                    r.add_point_light((0.0, 3.0, 4.0), (1.0, 0.8, 0.6), 30.0, 12.0)
                else:
                    scenes.build_textured_scene(r, oh, mk, 200, 0xFA58, lights=2)
            cams = [(oh.look_at_lh((-14.0 + 4.0 * f, 3.0 + f, -14.0 + 3.0 * f), (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1)) for f in range(3)]
            amb, clear = (0.1, 0.1, 0.1, 1.0), (0.02, 0.03, 0.05, 1.0)
        p.set_shade_mode(1)
        differing = 0.0
        for f, (view, proj) in enumerate(cams):
            for r in (o, p):
                r.set_camera_data(view, proj)
            fo = o.render(w, h, ambient=amb, clear_color=clear)
            fp = p.render(w, h, ambient=amb, clear_color=clear)
            mx, frac = compare_frames_fast(fo, fp, f"fast {name} frame {f}")
            worst, differing = max(worst, mx), max(differing, frac)
        assert differing > 0.0, "the fast mode produced bit-identical HDR everywhere: is it wired up?"
        p.set_shade_mode(0)
        fo = o.render(w, h, ambient=amb, clear_color=clear)
        fp = p.render(w, h, ambient=amb, clear_color=clear)
        compare_frames(fo, fp, f"back to exact, {name}")
    assert worst <= 1e-3


# ------------------------------------------------------------------ multi-GPU sharding on the HIP path, two contexts on one device
def test_sharded_two_contexts_multi_frame(r3):
    """The sharded product path over several frames with camera motion, without a second GPU: two contexts on this device
    play rank 0 and rank 1 of rend3_amd/parallel.py's scheme -- viewport objects split by slot range, shadow views split by
    view -- and their frames advance in lockstep, node by node; at every exchange point a local stand-in for the collectives
    merges their buffers with torch (shadow rectangles copied from their owner, MAX of the pass-1 depth planes through
    r3n_exchange_depth, MAX of the pass-2 keys).  Every frame: keys, atlas and image of BOTH contexts equal the unsharded
    context's, each rank's L1 / L2 sets are the unsharded sets restricted to its range and their union is the whole set --
    which only holds from frame 1 on if the Hi-Z each rank culls against is the global one."""
    import ctypes
    import torch
    from rend3_amd import parallel
    from rend3_amd.renderer import BaseRenderGraph, BaseRenderGraphInputs, BaseRenderGraphSettings, RenderGraph
    w, h, frames = 640, 360, 4
    ref, a, b = (r3.Renderer(oh.LEFT, f32(w) / f32(h)) for _ in range(3))
    for r in (ref, a, b):
        scenes.build_textured_scene(r, oh, r3.material_record, 300, 0x5AAD, lights=2)
    counts = np.zeros(ref.capacity, dtype=np.int64)
    for hd, m in ref.object_meta.items():
        counts[hd] = ref.meshes[m["mesh"]].index_count // 3
    ranges = parallel.partition_objects(counts, 2)
    dev = torch.device("cuda", 0)

    class Rank:
        def __init__(self, r, rank):
            self.r, self.rank, self.pending = r, rank, None
            r.set_object_range(*ranges[rank])
            for v in range(2):
                if parallel.shadow_view_owner(v, 2) == rank:
                    r.set_camera_object_range(v, 0, 0xFFFFFFFE)

        def owns_shadow_view(self, v):
            return parallel.shadow_view_owner(v, 2) == self.rank

        def __call__(self, what, r, ev=None, samples=1):
            self.pending = (what, ev)

        def buffers(self):
            vis, vis_n, atlas, atlas_n = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()
            self.r._check(self.r.lib.r3n_exchange_buffers(self.r.ctx, ctypes.byref(vis), ctypes.byref(vis_n), ctypes.byref(atlas), ctypes.byref(atlas_n)), "exchange_buffers")
            return (parallel.device_tensor(vis.value, vis_n.value, "<i8", dev), parallel.device_tensor(atlas.value, atlas_n.value, "<f4", dev))

        def depth_plane(self):
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            self.r._check(self.r.lib.r3n_exchange_depth(self.r.ctx, ctypes.byref(p), ctypes.byref(n)), "exchange_depth")
            return parallel.device_tensor(p.value, n.value, "<f4", dev)

    ranks = [Rank(a, 0), Rank(b, 1)]

    def merge(what, ev):
        if what == "pass1":
            planes = [rk.depth_plane() for rk in ranks]
        else:
            bufs = [rk.buffers() for rk in ranks]
        for rk in ranks:
            rk.r.sync()
        if what == "shadow":
            aw, ah = ev.shadow_target_size
            for v, sh in enumerate(ev.shadows):
                x, y, s = sh["offset"][0], sh["offset"][1], sh["size"]
                own = parallel.shadow_view_owner(v, 2)
                src = bufs[own][1].view(ah, aw)[y:y + s, x:x + s]
                bufs[1 - own][1].view(ah, aw)[y:y + s, x:x + s].copy_(src)
        elif what == "pass1":
            m = torch.maximum(planes[0], planes[1])
            planes[0].copy_(m); planes[1].copy_(m)
        else:
            m = torch.maximum(bufs[0][0], bufs[1][0])
            bufs[0][0].copy_(m); bufs[1][0].copy_(m)
        torch.cuda.synchronize()

    amb, clear = (0.1, 0.1, 0.1, 1.0), (0.02, 0.03, 0.05, 1.0)
    for f in range(frames):
        eye = (-14.0 + 3.0 * f, 3.0 + 0.5 * f, -14.0 + 2.0 * f)
        for r in (ref, a, b):
            r.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        fr = ref.render(w, h, ambient=amb, clear_color=clear)
        graphs, evs = [], []
        for rk in ranks:
            ev = rk.r.evaluate_instructions()
            base = BaseRenderGraph(rk.r)
            g = RenderGraph()
            base.add_to_graph(g, BaseRenderGraphInputs(ev, base.default_routines(), (w, h), 1), BaseRenderGraphSettings(amb, clear), exchange=rk)
            graphs.append(g)
            evs.append(ev)
        assert len(graphs[0].nodes) == len(graphs[1].nodes)
        for (na, body_a), (nb, body_b) in zip(graphs[0].nodes, graphs[1].nodes):
            assert na.split(" S")[0] == nb.split(" S")[0]
            body_a(a, evs[0])
            body_b(b, evs[1])
            if ranks[0].pending is not None:
                assert ranks[1].pending is not None and ranks[1].pending[0] == ranks[0].pending[0]
                merge(*ranks[0].pending)
                ranks[0].pending = ranks[1].pending = None
        outs = [rk.r.readback_frame(evs[k], w, h, 1, {v for v in range(2) if rk.owns_shadow_view(v)}) for k, rk in enumerate(ranks)]
        tri_obj = np.searchsorted(np.concatenate([[0], np.cumsum(counts)])[:-1], np.arange(len(fr["pass"])), side="right") - 1
        for k, fo in enumerate(outs):
            tag = f"frame {f} rank {k}"
            assert np.array_equal(fo["vis"], fr["vis"]), tag + " keys"
            assert np.array_equal(fo["atlas"].view(np.uint32), fr["atlas"].view(np.uint32)), tag + " atlas"
            assert np.array_equal(fo["hdr16"], fr["hdr16"]) and np.array_equal(fo["rgba8"], fr["rgba8"]), tag + " image"
            lo, hi = ranges[k]
            own = np.zeros(len(fr["visible"]), dtype=bool)
            own[lo:hi] = True
            assert np.array_equal(fo["visible"].astype(bool), fr["visible"].astype(bool) & own), tag + " L1"
            town = own[tri_obj]
            n = len(fr["pass"])
            assert np.array_equal(fo["pass"][:n].astype(bool), fr["pass"].astype(bool) & town), tag + " L2 pass"
            assert np.array_equal(fo["residual"][:n].astype(bool), fr["residual"].astype(bool) & town), tag + " L2 residual"
            v = k  # the view this rank owns
            assert np.array_equal(fo["shadows"][v]["visible"], fr["shadows"][v]["visible"]) and np.array_equal(fo["shadows"][v]["pass"], fr["shadows"][v]["pass"]), tag + " shadow sets"
        n = len(fr["pass"])
        assert np.array_equal((outs[0]["pass"][:n] | outs[1]["pass"][:n]), fr["pass"]), f"frame {f} union"
    assert fr["residual"].sum() > 0 and fr["pass"].sum() > 1000
    for r in (ref, a, b):
        r.close()


def test_baked_matrices_of_last_frames_visible_slots(r3):
    """r3n_render_frame bakes the slots inside the frustum now OR in the camera's previous frame (last frame's predicted
    triangles are drawn with THIS frame's matrices, forward.rs:224-232); compare_frames checks the first set only.  The camera turns
    away between two frames: the slots that left the frustum must hold this frame's matrices all the same."""
    o, p = both(r3, oh.LEFT, f32(320) / f32(192))
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 300, 0xBA4ED, lights=1)
    kw = dict(ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
    prev = None
    left = 0
    for f, ang in enumerate((0.0, 0.9, 1.8, 0.4)):
        for r in (o, p):
            r.set_camera_data(oh.look_at_lh((0.0, 2.0, -4.0), (12.0 * math.sin(ang), 1.0, 12.0 * math.cos(ang) - 4.0), (0, 1, 0)), ("perspective", 50.0, 0.1))
        fo, fp = o.render(320, 192, **kw), p.render(320, 192, **kw)
        compare_frames(fo, fp, f"frame {f}")
        if prev is not None:
            gone = prev & ~fo["visible"].astype(bool) & (fo["objects"][:, 29] != 0)
            left += int(gone.sum())
            assert np.array_equal(fo["baked"].view(np.uint32)[gone], fp["baked"].view(np.uint32)[gone]), f"frame {f}: slots that left the frustum"
        prev = fo["visible"].astype(bool)
    assert left > 20, "the camera turned far enough for objects to leave the frustum"
