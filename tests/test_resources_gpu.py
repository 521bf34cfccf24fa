"""The ledger of live HIP resources (csrc/hip_owned.h, read through r3n_internal_live_resources) on the device: a renderer that has
driven every lazily allocating path gives back, at close(), exactly what it took -- device blocks, pinned blocks, events and
streams --, a second one in the same process does so again (nothing stays behind in statics), a refused r3n_create leaves
nothing, and the breadcrumb file's descriptor is closed.  tests/test_resources.py reads the same rule from the source."""
import ctypes
import gc
import os

import numpy as np
import pytest

import scenes
from oracle import host as oh

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("device allocations", "pinned host allocations", "events", "streams")
HBM_BYTES = 64 << 20  # the smallest size r3n_hbm_copy_rate accepts


def _live(lib):
    out = (ctypes.c_uint64 * 4)()
    fn = lib.r3n_internal_live_resources  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64)]
    assert fn(out) == 0
    return dict(zip(KINDS, (int(v) for v in out)))


def _light_and_camera(p):
    p.set_camera_data(oh.mat4_mul(oh.from_euler_xyz(-0.55, 0.5, 0.0), oh.translation((-3.0, -3.0, 5.0))), ("perspective", 60.0, 0.1))
    p.add_directional_light(color=(1, 1, 1), intensity=1.0, direction=(-1.0, -4.0, 2.0), distance=40.0, resolution=256)
    p.add_point_light((0.1, 1.2, -1.5), (1.0, 0.0, 0.0), 4.0, 2.0)


def _grey(p, r3, key=scenes.OPAQUE, alpha=1.0):
    return p.add_material(r3.material_record(albedo=(0.5, 0.5, 0.5, alpha), albedo_mode="value", roughness=0.5), key)


def _frames_and_blend(r3):
    """the frame path: shadow cameras, lanes, atlas and Hi-Z; the edge list and samples16; both frame slots; the fragment buffers and
    both sources of the blend order; the timing taps; the owner bytes; the sampler probe; the copy-rate probe"""
    p = r3.Renderer(oh.LEFT, f32(64.0 / 48.0))
    p.add_object(scenes.cube_mesh(p), _grey(p, r3), oh.identity())
    _light_and_camera(p)
    assert p.render(64, 48)["rgba8"].shape == (48, 64, 4)
    assert p.render(64, 48, samples=4)["rgba8"].shape == (48, 64, 4)
    for _ in range(2):  # consecutive frames: both frame slots and the alt_* set
        p.render(64, 48, readback=False)
    blend = _grey(p, r3, scenes.BLEND, 0.5)
    for winding in ([0, 1, 2], [0, 2, 1]):  # one blend-key triangle, facing the camera whichever way the front is
        p.add_object(p.add_mesh([(-1, -1, 1.5), (0, 1, 1.5), (1, -1, 1.5)], winding), blend, oh.identity())
    p.render(64, 48, readback=False)        # the order sorted on the host
    p.blend_sort = "gpu"
    p.render(64, 48, readback=False)        # the blend set, sorted on the device
    assert len(p.readback_blend_order()[0]) == 2
    cube = p.add_texture_cube(np.full((6, 4, 4, 4), 128, dtype=np.uint8))
    p.set_background_texture(cube)
    p.render(64, 48, readback=False)
    p.timing_enable(True)
    p.render(64, 48, readback=False)
    assert p.stage_times()["shade"][1] >= 1
    p.timing_enable(False)
    p.set_object_owners(np.zeros(p.capacity, dtype=np.uint8), 0)
    p.render(64, 48, readback=False)
    tex = p.add_texture_2d(np.full((8, 8, 4), 200, dtype=np.uint8), srgb=False)
    q = np.zeros(1, dtype=r3.renderer.SAMPLE_QUERY)
    q["id"][0, 0], q["u"], q["v"] = tex + 1, 0.5, 0.5
    assert p.sample_probe(r3.renderer.PROBE_FORMS.index("grad"), q).shape == (1,)
    assert p.hbm_copy_rate(HBM_BYTES, 1) > 0.0
    p.close()


def _streamed_textures(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0), texture_upload="stream")
    rng = np.random.default_rng(7)
    first = p.add_texture_2d(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8), mip_count=4, mip_source="generated")
    p._flush_textures()
    # 32 x 32, two stored levels (5120 bytes): past the first staging block, which retires
    levels = [rng.integers(0, 256, n * n * 4, dtype=np.uint8).tobytes() for n in (32, 16)]
    second = p.add_texture_2d_encoded(1, 32, 32, levels)
    p._flush_textures()
    tail = p.add_texture_2d_from_texture(second, 1)
    p._flush_textures()
    p.remove_texture(first)
    assert p.compact_textures()["pool_words_after"] > 0
    assert len(p.readback_texture_descs()) >= tail + 1
    p.close()


def _streamed_meshes(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream")
    mat = _grey(p, r3)
    first, second = scenes.cube_mesh(p), scenes.cube_mesh(p)
    p.add_object(second, mat, oh.identity())
    _light_and_camera(p)
    p.render(64, 48, readback=False)
    p.remove_mesh(first)
    assert p.compact_meshes()["blocks_moved"] >= 1  # the relocation kernel, between its two events
    p.render(64, 48, readback=False)
    p.close()


def _vertex_stages(r3):
    """one morph instance, one mesh with recomputed normals, one with generated (and recomputed) tangents, one skinned and posed"""
    from rend3_amd import anim, gltf
    p = r3.Renderer(oh.LEFT, f32(64.0 / 48.0))
    mat = _grey(p, r3)
    pos = np.array([(-1, -1, 0), (-1, 1, 0), (1, 1, 0), (1, -1, 0)], dtype=f32)
    idx, uv = [0, 2, 1, 0, 3, 2], (pos[:, :2] * f32(0.5) + f32(0.5)).astype(f32)
    targets = dict(positions=np.tile(np.array([0.0, 0.0, 0.25], dtype=f32), (1, 4, 1)) * pos[None, :, :1], normals=None, tangents=None)
    plain = p.add_mesh(pos, idx, normals=[(0, 0, -1)] * 4, morph_targets=targets)
    renormal = p.add_mesh(pos, idx, morph_targets=targets, morph_normals="recompute")
    retangent = p.add_mesh(pos, idx, uv0=uv, morph_targets=targets, morph_normals="recompute", build_tangents=True, morph_tangents="recompute")
    for k, mesh in enumerate((plain, renormal, retangent)):
        p.add_object(None, mat, oh.translation((2.5 * (k - 1), 0.0, 0.0)), morph=p.add_morph_instance(mesh, [0.5]))
    g = gltf.Gltf(os.path.join(GOLDEN, "skinning-RiggedSimple.glb"))
    inst = gltf.instance_scene(g, p, r3.host, r3.material_record)
    data = anim.AnimationData.from_gltf_scene(p, gltf.load_animations(g), inst)
    anim.pose_animation_frame(p, inst, data, 0, 0.3)  # one pose request
    _light_and_camera(p)
    p.render(64, 48, readback=False)
    st = p.stage_times()
    assert all(st[s][1] >= 1 for s in ("morph", "normals", "tangents", "skinning", "pose")), st
    p.close()


def _every_path(r3):
    _frames_and_blend(r3)
    _streamed_textures(r3)
    _streamed_meshes(r3)
    _vertex_stages(r3)


def test_the_ledger_returns_to_its_baseline():
    import rend3_amd as r3
    lib = r3.lib()
    gc.collect()
    base = _live(lib)
    for lap in range(2):  # the second lap: nothing of the first stayed behind in a static
        _every_path(r3)
        gc.collect()
        assert _live(lib) == base, (lap, base)


def test_a_live_context_shows_in_the_ledger():
    """the counters count: a context holds its four streams' worth of resources while it lives"""
    import rend3_amd as r3
    lib = r3.lib()
    gc.collect()
    base = _live(lib)
    p = r3.Renderer(oh.LEFT, f32(1.0))
    held = _live(lib)
    assert held["streams"] == base["streams"] + 4 and all(held[k] > base[k] for k in KINDS), (base, held)
    p.close()
    assert _live(lib) == base


def test_a_refused_create_leaves_nothing(monkeypatch):
    import rend3_amd as r3
    lib = r3.lib()
    gc.collect()
    base = _live(lib)
    assert not lib.r3n_create(1 << 20, None)
    assert lib.r3n_create_error().decode() == "hip_device out of range"
    assert _live(lib) == base
    monkeypatch.setenv("R3N_TUNE", "nonsense=1")
    assert not lib.r3n_create(0, None)
    assert lib.r3n_create_error().decode().startswith("R3N_TUNE: ")
    assert _live(lib) == base


def test_the_breadcrumb_descriptor_is_closed(monkeypatch, tmp_path):
    import rend3_amd as r3
    r3.Renderer(oh.LEFT, f32(1.0)).close()  # whatever the runtime opens at its first use is open now
    monkeypatch.setenv("R3N_BREADCRUMBS", str(tmp_path / "crumbs"))
    gc.collect()
    before = len(os.listdir("/proc/self/fd"))
    p = r3.Renderer(oh.LEFT, f32(1.0))
    assert len(os.listdir("/proc/self/fd")) > before
    p.close()
    assert len(os.listdir("/proc/self/fd")) == before
    (path,) = list(tmp_path.iterdir())
    assert path.read_text().splitlines()[-1].split()[3] == "destroy"
