"""GPU: r3n_environment_lights (rend3_amd/csrc/envlight.hip) against tests/envlight_reference.py: the whole result struct, raw
integer sums included, word for word, under both plans (R3N_TUNE envlight_plane) and three grid sizes (envlight_blocks = 1, 7,
default); every pool class; a level of a stored chain; the refusals; and a frame lit by the extracted lights.  Shapes are the
smallest that can still go wrong: fewer texels than a wave (n = 1, 2, 3), a partial last wave (n = 5), several blocks with an idle
tail and a texel exactly on each axis (n = 33), whole waves (n = 64)."""
import ctypes
import math

import numpy as np
import pytest

import envlight_reference as E
import skybox_reference as S
from oracle import host as oh
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
PLANS = [(plane, blocks) for plane in (0, 1) for blocks in (1, 7, 0)]  # (blocks 0: the default, from the level's size)
CONE6 = f32(math.cos(math.radians(6.0)))


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    assert hasattr(rend3_amd.lib(), "r3n_environment_lights")
    return rend3_amd


def tune(r, kv):
    fn = r.lib.r3n_internal_set_tuning  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    assert fn(r.ctx, kv.encode()) == 0, r.lib.r3n_last_error(r.ctx)


def launches_of(r):
    fn = r.lib.r3n_internal_envlight_launches
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_uint64
    return int(fn(r.ctx))


def call(r, cube, level, max_lights, cone_cos, min_share):
    from rend3_amd import _ffi
    params = _ffi.EnvLightsParams(cube, level, max_lights, float(f32(cone_cos)), float(f32(min_share)))
    out = _ffi.EnvLightsResult()
    code = r.lib.r3n_environment_lights(r.ctx, ctypes.addressof(params), ctypes.addressof(out))
    return code, out


def nasty(n, seed, huge):
    """random radiance over 12 octaves plus NaN, +-inf, -1, subnormals, zeros of both signs and (huge) 1e30"""
    rng = np.random.default_rng(seed)
    rgb = (np.exp2(rng.uniform(-6, 6, (6, n, n, 1))) * rng.uniform(0.05, 1.0, (6, n, n, 3))).astype(f32)
    flat = rgb.reshape(-1, 3)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 1e-45, 1e-39, 1e30 if huge else 100.0, 0.0, -0.0)):
        flat[(k * 7 + 3) % len(flat), k % 3] = v
    return rgb


def peaks(n):
    """a dim sky with more than sixteen peaks: on a face centre (n odd: exactly on the axis), on an edge (its cone spans two faces),
    on a corner (three faces), two equal ones, and a falling series of others"""
    rng = np.random.default_rng(n)
    rgb = rng.uniform(0.01, 0.02, (6, n, n, 3)).astype(f32)
    m = n // 2
    rgb[0, m, m] = (900.0, 800.0, 700.0)                 # +X centre
    rgb[2, m, 0] = rgb[1, 0, m] = (300.0, 500.0, 200.0)  # the +Y / -X edge, either side of it
    rgb[4, 0, 0] = rgb[1, 0, n - 1] = rgb[2, n - 1, 0] = (250.0, 250.0, 250.0)  # the -X +Y +Z corner
    rgb[3, m, m] = rgb[5, m, m] = (100.0, 100.0, 100.0)  # two equal peaks: -Y's comes first
    for k in range(20):
        f, j, i = int(rng.integers(6)), int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1))
        rgb[f, j, i] = f32(60.0 - 2.0 * k)
    return rgb


def rgba8_faces(n, seed):
    rng = np.random.default_rng(seed)
    faces = rng.integers(0, 40, (6, n, n, 4), dtype=np.uint8)
    for k, b in enumerate((0, 1, 254, 255)):
        faces[k, k % n, (2 * k) % n, :3] = b
        faces[5, (k + 1) % n, k % n, k % 3] = b
    return faces


def f32_levels(*levels):
    """faces[f][k] for add_texture_cube_encoded from (6, n, n, 3) radiance arrays, alpha 1"""
    out = [[] for _ in range(6)]
    for rgb in levels:
        rgba = np.concatenate([rgb, np.ones(rgb.shape[:3] + (1,), dtype=f32)], axis=-1)
        for f in range(6):
            out[f].append(np.ascontiguousarray(rgba[f]).tobytes())
    return out


class World:
    """one context with every cube of the tests, each extracted by the reference on demand (once)"""

    def __init__(self, r3):
        self.p = r3.Renderer(oh.LEFT, f32(1.0))
        self.rgb = {}
        self._want = {}

        def add_f32(key, *levels):
            h = self.p.add_texture_cube_encoded(C.RGBA32F, levels[0].shape[1], f32_levels(*levels))
            for k, rgb in enumerate(levels):
                self.rgb[(h, k)] = rgb
            self.handles[key] = h

        self.handles = {}
        for n in (1, 2, 3, 5):
            add_f32(("nasty", n), nasty(n, 40 + n, huge=False))
        add_f32("huge", nasty(5, 7, huge=True))
        add_f32("peaks", peaks(33))
        add_f32("black", np.zeros((6, 3, 3, 3), dtype=f32))
        add_f32("chain", np.zeros((6, 256, 256, 3), dtype=f32), nasty(128, 3, huge=False), E.sky(64))  # level 2 of a stored chain
        for key, n, srgb in (("unorm", 5, False), ("srgb", 33, True)):
            faces = rgba8_faces(n, n)
            h = self.p.add_texture_cube(faces, srgb=srgb)
            self.rgb[(h, 0)] = S.decode_table(srgb)[faces[..., :3]]
            self.handles[key] = h
        self.p._flush_cubes()

    def want(self, cube, level, max_lights, cone_cos, min_share):
        key = (cube, level, max_lights, float(f32(cone_cos)), float(f32(min_share)))
        if key not in self._want:
            self._want[key] = E.extract(self.rgb[(cube, level)], max_lights, f32(cone_cos), f32(min_share))
        return self._want[key]

    def check(self, name, level, max_lights, cone_cos, min_share, plans=PLANS):
        cube = self.handles[name]
        st = self.want(cube, level, max_lights, cone_cos, min_share)
        want = bytes(E.result_struct(st))
        for plane, blocks in plans:
            tune(self.p, f"envlight_plane={plane} envlight_blocks={blocks}")
            code, out = call(self.p, cube, level, max_lights, cone_cos, min_share)
            assert code == 0, self.p.lib.r3n_last_error(self.p.ctx)
            got = bytes(out)
            if got != want:
                a, b = np.frombuffer(got, dtype=np.uint32), np.frombuffer(want, dtype=np.uint32)
                bad = np.nonzero(a != b)[0]
                raise AssertionError(f"{name} level {level} plan {(plane, blocks)}: {len(bad)} words differ, first at word {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")
            assert launches_of(self.p) == 2 + (E.SHIFT_STEPS + 1) * max_lights
            words = np.frombuffer(got, dtype=np.uint32)
            floats = np.concatenate([words[4:8]] + [words[66 + 48 * k:66 + 48 * k + 7] for k in range(16)]).view(f32)
            assert not np.isnan(floats).any(), "no NaN in any output word"
        return st


@pytest.fixture(scope="module")
def world(r3):
    w = World(r3)
    yield w
    w.p.close()


# ------------------------------------------------------------------ 1. word for word, every plan
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_levels_smaller_than_a_block(world, n):
    for cone_cos in (0.5, 0.9):
        st = world.check(("nasty", n), 0, 16, cone_cos, 0.0)
        assert st["n_lights"] >= 1
    world.check(("nasty", n), 0, 0, 0.9, 0.0)
    world.check(("nasty", n), 0, 1, 0.9, 0.5)


def test_peaks_on_a_centre_an_edge_and_a_corner(world):
    n = 33
    st = world.check("peaks", 0, 16, 0.995, 0.0)
    assert st["n_lights"] == 16 and st["seed"][16] >> 32 != 0, "more than sixteen peaks are present"
    seeds = [l["seed"] for l in st["lights"]]
    m = n // 2
    assert seeds[0] == (0 * n + m) * n + m and st["lights"][0]["direction"][0] > 0.99999, "the face-centre peak, seeded exactly on the axis"
    faces_of = [set((np.nonzero(mask.reshape(6, -1).any(axis=1))[0]).tolist()) for mask in st["masks"]]
    assert faces_of[1] == {1, 2}, "the edge peak: one cone over two faces"
    assert faces_of[2] == {1, 2, 4}, "the corner peak: one cone over three faces"
    equal = [k for k, s in enumerate(seeds) if s in ((3 * n + m) * n + m, (5 * n + m) * n + m)]
    assert len(equal) == 2 and seeds[equal[0]] == (3 * n + m) * n + m, "two equal peaks: the lower index comes first"


def test_light_counts_and_the_share_test(world):
    assert world.check("peaks", 0, 0, 0.995, 0.0)["n_lights"] == 0
    assert world.check("peaks", 0, 1, 0.995, 0.0)["n_lights"] == 1
    full = world.want(world.handles["peaks"], 0, 16, 0.995, 0.0)
    share = 0.5 * (full["light"][1]["qy"] + full["light"][2]["qy"]) / full["total"]["qy"]  # between the second and the third light
    st = world.check("peaks", 0, 16, 0.995, share)
    assert st["n_lights"] == 2 and st["ran"] == 3, "stops behind the second light; the third candidate ran and was refused"
    assert st["remainder"]["qy"] == full["total"]["qy"] - full["light"][0]["qy"] - full["light"][1]["qy"]


def test_a_wide_cone_kills_a_sixth_of_the_sphere(world):
    st = world.check("peaks", 0, 16, 0.5, 0.0)
    assert st["lights"][0]["texels"] > 6 * 33 * 33 // 8
    dead = st["masks"][0].reshape(-1)
    assert all(not dead[l["seed"]] for l in st["lights"][1:]), "later seeds skip dead texels"


def test_level_two_of_a_stored_chain(world):
    st = world.check("chain", 2, 4, CONE6, 0.02)
    assert st["n"] == 64 and st["n_lights"] == 2 and st["ran"] == 3
    world.check("chain", 1, 3, 0.98, 0.0, plans=[(0, 7), (1, 0)])  # n = 128: 96 blocks by default


@pytest.mark.parametrize("name", ["unorm", "srgb"])
def test_rgba8_classes(world, name):
    st = world.check(name, 0, 16, 0.98, 0.0)
    assert st["n_lights"] >= 4
    world.check(name, 0, 3, 0.5, 0.01)


def test_black_and_corrupt_texels(world):
    st = world.check("black", 0, 16, 0.9, 0.0)
    assert st["n_lights"] == 0 and st["emax_bits"] == 0 and [float(a) for a in st["ambient"]] == [0.0, 0.0, 0.0, 1.0]
    st = world.check("huge", 0, 16, 0.9, 0.0)
    assert st["n_lights"] == 1 and float(st["lights"][0]["irradiance"][0]) > 1e28, "the 1e30 texel; everything else lies below the quantisation floor"


# ------------------------------------------------------------------ 2. refusals
def test_refusals_leave_the_context_usable(world):
    p, cube = world.p, world.handles["peaks"]
    tune(p, "envlight_plane=1 envlight_blocks=0")
    code, before = call(p, cube, 0, 4, 0.99, 0.01)
    assert code == 0
    nan = float("nan")
    for args, field in (((99, 0, 4, 0.99, 0.01), "cube"), ((cube, 1, 4, 0.99, 0.01), "level"), ((cube, 0, 17, 0.99, 0.01), "max_lights"),
                        ((cube, 0, 4, 0.49, 0.01), "cone_cos"), ((cube, 0, 4, 1.0, 0.01), "cone_cos"), ((cube, 0, 4, nan, 0.01), "cone_cos"),
                        ((cube, 0, 4, 0.99, -0.5), "min_share"), ((cube, 0, 4, 0.99, 1.0), "min_share"), ((cube, 0, 4, 0.99, nan), "min_share")):
        code, _ = call(p, *args)
        assert code == ERR_INVALID_ARG and field in p.lib.r3n_last_error(p.ctx).decode(), args
        code, after = call(p, cube, 0, 4, 0.99, 0.01)
        assert code == 0 and bytes(after) == bytes(before), args
    assert p.lib.r3n_environment_lights(p.ctx, None, None) == ERR_INVALID_ARG
    with pytest.raises(ValueError, match="no such cube"):
        p.environment_lights(99)
    lights, ambient = p.environment_lights(cube, max_lights=4, cone_degrees=math.degrees(math.acos(0.99)), min_share=0.01)
    assert len(lights) == before.n_lights and ambient.tolist() == list(before.ambient)


def test_inside_a_frame_and_above_1024(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0))
    # two stored levels, 2048 and 1024, of zero BC1 blocks (black): the finer is refused by name, the coarser runs all 6 * 1024^2 texels
    faces = [[bytes(C.level_bytes(C.BC1, 2048, 2048)), bytes(C.level_bytes(C.BC1, 1024, 1024))] for _ in range(6)]
    cube = p.add_texture_cube_encoded(C.BC1, 2048, faces)
    p._flush_cubes()
    code, _ = call(p, cube, 0, 4, 0.99, 0.01)
    msg = p.lib.r3n_last_error(p.ctx).decode()
    assert code == ERR_UNSUPPORTED and "2048" in msg and "level 1" in msg and "does not store" not in msg, msg
    for plane in (0, 1):
        tune(p, f"envlight_plane={plane}")
        code, out = call(p, cube, 1, 2, 0.99, 0.01)
        assert code == 0 and (out.extent, out.n_lights, out.emax_bits, out.total.texels) == (1024, 0, 0, 0) and list(out.ambient) == [0.0, 0.0, 0.0, 1.0]
    with pytest.raises(r3.R3nError, match="level"):
        p.environment_lights(cube, level=0)
    assert p.environment_lights(cube)[0] == [], "level=None takes level 1"
    # inside a frame
    from rend3_amd.renderer import BaseRenderGraph, BaseRenderGraphInputs, BaseRenderGraphSettings, RenderGraph
    w, h = 16, 12
    p.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
    seen = {}
    ev = p.evaluate_instructions()
    graph_base = BaseRenderGraph(p)
    graph = RenderGraph()
    graph_base.add_to_graph(graph, BaseRenderGraphInputs(ev, graph_base.default_routines(), (w, h), 1), BaseRenderGraphSettings((0, 0, 0, 0), (0, 0, 1, 1)))
    names = [name for name, _ in graph.nodes]

    def probe(r, _ev):
        seen["code"] = call(p, cube, 1, 2, 0.99, 0.01)[0]
        seen["message"] = p.lib.r3n_last_error(p.ctx).decode()

    graph.nodes.insert(names.index("Skybox"), ("probe", probe))
    graph.execute(p, ev)
    assert seen["code"] == ERR_STATE and "inside a frame" in seen["message"]
    code, _ = call(p, cube, 1, 2, 0.99, 0.01)
    assert code == 0
    p.close()


# ------------------------------------------------------------------ 3. a frame
def test_a_frame_lit_by_the_extracted_lights(r3):
    """add_environment_lights is add_directional_light + ambient by hand, bit for bit, and the frame is the oracle's under those
    lights within the suite's tolerance (compare_frames: sets and HDR bit-exact, framebuffer within 1e-3)"""
    import scenes
    from oracle.world import OracleRenderer, material_record as omk
    from test_gpu_parity import compare_frames
    w, h = 96, 96
    sky = (E.sky(32, suns=(((0.3, 0.8, 0.5), 5.0, 600.0), ((-1.0, 0.6, -0.4), 6.0, 80.0))) * f32(0.25)).astype(f32)
    a, b = r3.Renderer(oh.LEFT, f32(1.0)), r3.Renderer(oh.LEFT, f32(1.0))
    o = OracleRenderer(oh.LEFT, f32(1.0))
    for r, mk in ((o, omk), (a, r3.material_record), (b, r3.material_record)):
        mesh = scenes.cube_mesh(r)
        mat = r.add_material(mk(albedo=(0.6, 0.5, 0.4, 1.0), albedo_mode="value"), 0)
        r.add_object(mesh, mat, oh.identity())
        r.add_object(mesh, mat, oh.mat4_mul(oh.translation((0.0, -1.6, 0.0)), oh.scale((6.0, 0.5, 6.0))))
        r.set_camera_data(oh.mat4_mul(oh.from_euler_xyz(-0.55, 0.5, 0.0), oh.translation((-3.0, -3.0, 5.0))), ("perspective", 60.0, 0.1))
    cube = a.add_texture_cube_encoded(C.RGBA32F, 32, f32_levels(sky))
    ids, ambient = a.add_environment_lights(cube, max_lights=4, cone_degrees=8.0, min_share=0.02, scale=0.5, distance=40.0, resolution=512)
    lights, rest = a.environment_lights(cube, max_lights=4, cone_degrees=8.0, min_share=0.02)
    assert ids == [0, 1] and len(lights) == 2
    hand = tuple(float(v) for v in (rest[:3] * f32(0.5))) + (1.0,)
    assert tuple(float(v) for v in ambient) == hand
    for r in (b, o):
        for l in lights:
            r.add_directional_light(color=tuple(float(v) for v in l["irradiance"]), intensity=0.5, direction=tuple(-float(v) for v in l["direction"]),
                                    distance=40.0, resolution=512)
    fa = a.render(w, h, ambient=tuple(float(v) for v in ambient), clear_color=(0.1, 0.05, 0.1, 1.0))
    fb = b.render(w, h, ambient=hand, clear_color=(0.1, 0.05, 0.1, 1.0))
    fo = o.render(w, h, ambient=hand, clear_color=(0.1, 0.05, 0.1, 1.0))
    assert np.array_equal(fa["hdr16"], fb["hdr16"]) and np.array_equal(fa["rgba8"], fb["rgba8"]) and np.array_equal(fa["atlas"].view(np.uint32), fb["atlas"].view(np.uint32))
    compare_frames(fo, fa, "environment lights")
    lit = fa["rgba8"][..., :3].astype(int)
    assert lit.max() > 120 and len(np.unique(lit.reshape(-1, 3), axis=0)) > 50, "the lights light the scene"
    a.close()
    b.close()
