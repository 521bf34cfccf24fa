"""GPU: r3n_environment_prefilter, r3n_environment_probe and r3n_skybox_set_level (rend3_amd/csrc/ibl.hip, skybox.hip) against
tests/ibl_reference.py: every level of every face of the new cube and the nine SH coefficients word for word, under every launch
plan (R3N_TUNE ibl_tile x ibl_block), from sources of all three pool classes and from a base level above 0; the append semantics;
the refusals; the probe; and frames drawn at a fixed level.  Shapes are the smallest that can still go wrong (S, L):
(2, 2) fewer outputs than a wave; (3, 2) an odd extent, levels 3 and 1; (5, 3) partial waves; (8, 4) 96 outputs on level 1;
(16, 5) more than a workgroup with an idle tail; (33, 3) a texel exactly on each axis of the mirror level, several LDS tiles, tile
boundaries inside rows."""
import ctypes

import numpy as np
import pytest

import envlight_reference as E
import ibl_reference as I
import skybox_lod_cases as cases
import skybox_lod_reference as lodref
import skybox_reference as S
from oracle import host as oh
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
SHAPES = [(2, 2), (3, 2), (5, 3), (8, 4), (16, 5), (33, 3)]
PLANS = [(tile, block) for tile in (48, 64, 512) for block in (64, 256)] + [(0, 128), (256, 256)]  # (tile 0: no LDS; (256, 256): the default)


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    assert hasattr(rend3_amd.lib(), "r3n_environment_prefilter")
    return rend3_amd


def tune(r, kv):
    fn = r.lib.r3n_internal_set_tuning  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    assert fn(r.ctx, kv.encode()) == 0, r.lib.r3n_last_error(r.ctx)


def launches_of(r):
    fn = r.lib.r3n_internal_ibl_launches
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_uint64
    return int(fn(r.ctx))


def call(r, cube, level, levels):
    from rend3_amd import _ffi
    params = _ffi.EnvPrefilterParams(cube, level, levels)
    out = _ffi.EnvPrefilterResult()
    code = r.lib.r3n_environment_prefilter(r.ctx, ctypes.addressof(params), ctypes.addressof(out))
    return code, out


def message(r):
    return r.lib.r3n_last_error(r.ctx).decode()


def f32_faces(levels):
    """faces[f][k] for add_texture_cube_encoded from (6, n, n, 3) radiance arrays, alpha 1"""
    out = [[] for _ in range(6)]
    for rgb in levels:
        rgba = np.concatenate([rgb, np.ones(rgb.shape[:3] + (1,), dtype=f32)], axis=-1)
        for f in range(6):
            out[f].append(np.ascontiguousarray(rgba[f]).tobytes())
    return out


def rgba8_levels(S_, L, seed):
    rng = np.random.default_rng(seed)
    levels = [rng.integers(0, 256, (6, I.level_extent(S_, k), I.level_extent(S_, k), 4), dtype=np.uint8) for k in range(L)]
    levels[0][0, 0, 0, :3] = 0
    levels[0][1, 0, 0, :3] = 255
    return levels


def sh_of(out):
    return np.array([[out.sh[m][ch] for ch in range(4)] for m in range(9)], dtype=f32)


def check_cube(p, handle, want, what):
    """every level of every face of cube `handle`, corners excluded (they are zero), word for word"""
    for k, level in enumerate(want):
        for f in range(6):
            got = p.readback_cube_face(handle, k, f)
            exp, corner = lodref.bordered_face(level, f)
            assert got.dtype == np.float32 and got.shape == exp.shape, (what, k, f)
            g, w = got.view(np.uint32), np.ascontiguousarray(exp).view(np.uint32)
            bad = (g != w).any(axis=2) & ~corner
            assert not bad.any(), f"{what} level {k} face {f}: {bad.sum()} texels differ, first {np.argwhere(bad)[0]}: {got[tuple(np.argwhere(bad)[0])]} != {exp[tuple(np.argwhere(bad)[0])]}"
            assert not g[corner].any(), "corner words are written as zero"


class World:
    """one context with every source cube of the tests; the reference of each (cube, base level, levels) is computed once"""

    def __init__(self, r3):
        self.p = r3.Renderer(oh.LEFT, f32(1.0))
        self.levels = {}  # handle -> the decoded stored levels, (6, n, n, 3) f32
        self.handles = {}
        self._want = {}
        for S_, L in SHAPES:
            levels = I.nasty(I.random_levels(S_, L, seed=100 * S_ + L))
            self.handles[("f32", S_)] = h = self.p.add_texture_cube_encoded(C.RGBA32F, S_, f32_faces(levels))
            self.levels[h] = levels
        for key, fmt, srgb in (("unorm", C.RGBA8, False), ("srgb", C.RGBA8_SRGB, True)):
            raw = rgba8_levels(5, 3, 77 + fmt)
            self.handles[key] = h = self.p.add_texture_cube_encoded(fmt, 5, [[raw[k][f].tobytes() for k in range(3)] for f in range(6)])
            self.levels[h] = [S.decode_table(srgb)[lv[..., :3]] for lv in raw]
        levels = I.nasty(I.random_levels(16, 4, seed=9))  # a stored chain 16, 8, 4, 2: the base level may be 1
        self.handles["chain"] = h = self.p.add_texture_cube_encoded(C.RGBA32F, 16, f32_faces(levels))
        self.levels[h] = levels
        self.p._flush_cubes()

    def want(self, cube, level, L):
        key = (cube, level, L)
        if key not in self._want:
            src = self.levels[cube][level:level + L]
            self._want[key] = (I.prefilter(src), I.sh9(src[I.sh_level(src[0].shape[1], L)]))
        return self._want[key]

    def run(self, name, level, L, plans):
        cube = self.handles[name]
        levels, sh = self.want(cube, level, L)
        for tile, block in plans:
            tune(self.p, f"ibl_tile={tile} ibl_block={block}")
            count = len(self.p.cubes)
            handle, got_sh = self.p.prefilter_environment(cube, level=level, levels=L)
            assert handle == count and launches_of(self.p) == 6
            assert np.array_equal(E.bits(got_sh), E.bits(sh)), f"{name} plan {(tile, block)}: SH {got_sh} != {sh}"
            check_cube(self.p, handle, levels, f"{name} from level {level}, plan {(tile, block)}")
            for lv in levels[1:]:
                assert not np.isnan(lv).any()
        tune(self.p, "ibl_tile=256 ibl_block=256")


@pytest.fixture(scope="module")
def world(r3):
    w = World(r3)
    yield w
    w.p.close()


# ------------------------------------------------------------------ 1. word for word, every plan
@pytest.mark.parametrize("S_,L", SHAPES)
def test_every_level_and_the_sh_word_for_word_under_every_plan(world, S_, L):
    world.run(("f32", S_), 0, L, PLANS)


@pytest.mark.parametrize("name", ["unorm", "srgb"])
def test_rgba8_classes(world, name):
    world.run(name, 0, 3, [(48, 64), (256, 256)])


def test_a_base_level_above_zero_and_fewer_levels_than_stored(world):
    world.run("chain", 1, 3, [(48, 64), (0, 256)])   # S = 8 from the stored levels 8, 4, 2
    world.run("chain", 0, 2, [(64, 256)])            # two of four stored levels: r = 0, 1
    cube = world.handles["chain"]
    handle, _ = world.p.prefilter_environment(cube)  # the defaults: level 0, all four stored levels
    check_cube(world.p, handle, world.want(cube, 0, 4)[0], "defaults")


# ------------------------------------------------------------------ 2. append semantics
def test_append_keeps_the_array_and_a_whole_array_write_replaces_it(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0))
    w, h = 24, 16
    rng = np.random.default_rng(3)
    first = p.add_texture_cube(rng.integers(0, 256, (6, 3, 3, 4), dtype=np.uint8), srgb=True)
    levels = I.random_levels(8, 4, seed=2)
    src = p.add_texture_cube_encoded(C.RGBA32F, 8, f32_faces(levels))
    p.set_background_texture(first)
    p.set_camera_data(oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1))
    base = p.render(w, h)
    assert len(np.unique(base["hdr16"].reshape(-1, 4), axis=0)) > 4, "the frame shows the bound cube"
    before = [p.readback_cube_face(ci, k, f).copy() for ci, k, f in ((first, 0, 0), (src, 0, 5), (src, 3, 2))]
    a, sh_a = p.prefilter_environment(src)
    b, sh_b = p.prefilter_environment(src, levels=2)
    assert (a, b) == (2, 3) and len(p.cubes) == 4, "the returned id is the old count; two prefilters in a row"
    after = [p.readback_cube_face(ci, k, f) for ci, k, f in ((first, 0, 0), (src, 0, 5), (src, 3, 2))]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, after)), "earlier cubes read back unchanged"
    check_cube(p, a, I.prefilter(levels), "first prefilter")
    check_cube(p, b, I.prefilter(levels[:2]), "second prefilter")
    assert np.array_equal(E.bits(sh_a), E.bits(sh_b)) and np.array_equal(E.bits(sh_a), E.bits(I.sh9(levels[0])))
    again = p.render(w, h)
    assert np.array_equal(base["hdr16"], again["hdr16"]) and np.array_equal(base["rgba8"], again["rgba8"]), "a bound skybox stays bound"
    # a derived cube may feed a further prefilter: it is a stored chain like any other
    c, _ = p.prefilter_environment(a, level=1, levels=2)
    assert c == 4
    # a whole-array write replaces the array, the derived cubes included, and unbinds a skybox bound to one
    p.set_background_texture(b)
    bound = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert not (bound["hdr16"] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all()
    texels = np.zeros(6 * 4, dtype=np.uint32)
    desc = np.zeros((1, 8), dtype=np.uint32)
    desc[0, :5] = (0, 2, 2, 1, 0)
    from rend3_amd import _ffi
    assert p.lib.r3n_texture_cubes_write(p.ctx, _ffi.ptr(desc), 1, _ffi.ptr(texels), texels.size) == 0
    words = np.zeros(16 * 4, dtype=np.uint32)
    assert p.lib.r3n_readback_cube_face(p.ctx, 1, 0, 0, _ffi.ptr(words), words.size, None) == ERR_INVALID_ARG, "the derived cubes are gone"
    assert p.lib.r3n_skybox_set(p.ctx, 4) == ERR_INVALID_ARG
    # the frame after the write shows no sky: the binding to the vanished cube is gone (the renderer does not re-send: this is the
    # library's state alone)
    clear = p.render(w, h, clear_color=(0, 0, 1, 1))
    assert (clear["hdr16"] == np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float16).view(np.uint16)).all(), "the vanished cube was unbound"
    p.close()


# ------------------------------------------------------------------ 3. refusals
def test_refusals_change_nothing(world):
    p = world.p
    cube = world.handles[("f32", 5)]
    count = len(p.cubes)
    kept = p.readback_cube_face(cube, 1, 2).copy()
    for args, code, field in (((999, 0, 2), ERR_INVALID_ARG, "cube"), ((cube, 3, 2), ERR_INVALID_ARG, "level"), ((cube, 0, 0), ERR_INVALID_ARG, "levels"),
                              ((cube, 0, 1), ERR_INVALID_ARG, "levels"), ((cube, 0, 4), ERR_INVALID_ARG, "levels"), ((cube, 0, 17), ERR_INVALID_ARG, "levels"),
                              ((cube, 1, 3), ERR_INVALID_ARG, "levels"), ((cube, 2, 2), ERR_INVALID_ARG, "levels")):
        got, _ = call(p, *args)
        assert got == code and field in message(p), (args, message(p))
    # stored levels are missing: the chain of ("f32", 33) is 33, 16, 8 -- five levels fit its extent, three are stored
    got, _ = call(p, world.handles[("f32", 33)], 0, 4)
    assert got == ERR_UNSUPPORTED and "levels" in message(p) and "stores 3" in message(p), message(p)
    got, _ = call(p, world.handles[("f32", 33)], 2, 2)
    assert got == ERR_UNSUPPORTED and "stores 1" in message(p), message(p)
    assert p.lib.r3n_environment_prefilter(p.ctx, None, None) == ERR_INVALID_ARG
    words = np.zeros(64, dtype=np.uint32)
    from rend3_amd import _ffi
    assert p.lib.r3n_readback_cube_face(p.ctx, count, 0, 0, _ffi.ptr(words), words.size, None) == ERR_INVALID_ARG, "no cube was appended"
    assert np.array_equal(kept.view(np.uint32), p.readback_cube_face(cube, 1, 2).view(np.uint32))
    with pytest.raises(ValueError, match="no such cube"):
        p.prefilter_environment(999)
    assert len(p.cubes) == count


def test_extent_512_and_inside_a_frame(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0))
    # two stored levels, 1024 and 512, of zero BC1 blocks: both are refused by name, and the level the entry would take is not stored
    faces = [[bytes(C.level_bytes(C.BC1, 1024, 1024)), bytes(C.level_bytes(C.BC1, 512, 512))] for _ in range(6)]
    big = p.add_texture_cube_encoded(C.BC1, 1024, faces)
    small = p.add_texture_cube_encoded(C.RGBA32F, 4, f32_faces(I.random_levels(4, 3, seed=1)))
    p._flush_cubes()
    code, _ = call(p, big, 1, 2)
    assert code == ERR_UNSUPPORTED and "512" in message(p) and "level 2" in message(p) and "does not store" in message(p), message(p)
    code, _ = call(p, big, 0, 2)
    assert code == ERR_UNSUPPORTED and "1024" in message(p) and "level 2" in message(p), message(p)
    with pytest.raises(ValueError, match="no level of extent <= 256"):
        p.prefilter_environment(big)
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
        seen["prefilter"] = (call(p, small, 0, 3)[0], message(p))
        seen["level"] = (p.lib.r3n_skybox_set_level(p.ctx, 1.0), message(p))

    graph.nodes.insert(names.index("Skybox"), ("probe", probe))
    graph.execute(p, ev)
    assert seen["prefilter"][0] == ERR_STATE and "inside a frame" in seen["prefilter"][1]
    assert seen["level"][0] == ERR_STATE and "inside a frame" in seen["level"][1]
    assert p.lib.r3n_skybox_set_level(p.ctx, float("nan")) == ERR_INVALID_ARG
    code, out = call(p, small, 0, 3)
    assert code == 0 and (out.cube_id, out.extent, out.levels, out.sh_level) == (2, 4, 3, 0)
    p.close()


# ------------------------------------------------------------------ 4. the probe
def test_probe_word_for_word(world):
    from rend3_amd import renderer as R
    p = world.p
    cube = world.handles[("f32", 8)]
    levels, sh = world.want(cube, 0, 4)
    handle, got_sh = p.prefilter_environment(cube, level=0, levels=4)
    rng = np.random.default_rng(12)
    d = rng.normal(0, 1, (160, 3)).astype(f32)
    special = np.array([[1, 1, 1], [1, -1, 1], [-1, 1, -1], [-1, -1, -1], [1, 1, 0], [0, 1, 1], [1, 0, -1], [-1, 1, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1],
                        [1, 1, 0.999], [0.875, 1, 0.875], [-0.001, 0.002, 1]], dtype=f32)  # corners, edges, face centres, next to them
    d[:len(special)] = special
    rough = rng.uniform(0, 1, len(d)).astype(f32)
    rough[:8] = [0.0, 1.0, 1 / 3, 2 / 3, np.nan, -0.5, 1.5, 0.5]  # the ends, exactly on a level (2 / 3 * 3 = 2), NaN, outside [0, 1]
    rough[20:40] = 0.0
    rough[40:60] = 1.0
    q = np.zeros(len(d), dtype=R.ENV_QUERY)
    q["dir"], q["roughness"] = d, rough
    normals = rng.normal(0, 1, (len(d), 3)).astype(f32)
    q["n"] = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)
    got = p.environment_probe(handle, got_sh, q)
    want_spec, level, frac = I.specular(levels, d, rough)
    assert level[:8].tolist() == [0, 3, 1, 2, 0, 0, 3, 1] and frac[3] == 0 and frac[7] == f32(0.5)
    assert np.array_equal(got["level"], level.astype(np.uint32)) and np.array_equal(E.bits(got["fraction"]), E.bits(frac))
    assert np.array_equal(E.bits(got["specular"]), E.bits(want_spec))
    assert np.array_equal(E.bits(got["irradiance"]), E.bits(I.irradiance(sh, q["n"])))
    # an RGBA8 cube through the same lookup: its own decode table
    src = world.handles["srgb"]
    dec = [np.concatenate([lv, np.ones(lv.shape[:3] + (1,), dtype=f32)], axis=-1) for lv in world.levels[src]]
    got = p.environment_probe(src, got_sh, q)
    want_spec, level, frac = I.specular(dec, d, rough)
    assert np.array_equal(E.bits(got["specular"]), E.bits(want_spec)) and np.array_equal(got["level"], level.astype(np.uint32))
    from rend3_amd import _ffi
    coeff = np.zeros((9, 4), dtype=f32)
    assert p.lib.r3n_environment_probe(p.ctx, 999, _ffi.ptr(coeff), None, 0, None) == ERR_INVALID_ARG and "no such cube" in message(p)
    with pytest.raises(ValueError, match="no such cube"):
        p.environment_probe(999, got_sh, q)


# ------------------------------------------------------------------ 5. frames at a fixed level
@pytest.mark.parametrize("size", [(64, 48), (23, 17)])
def test_frames_at_a_fixed_level(r3, size):
    w, h = size
    S_, L = 8, 4
    levels = I.random_levels(S_, L, seed=21)
    a = r3.Renderer(oh.LEFT, f32(1.0))
    src = a.add_texture_cube_encoded(C.RGBA32F, S_, f32_faces(levels))
    view, proj = oh.look_at_lh((0, 0, 0), (-1.0, 1.0, -1.0), (0, 1, 0)), ("perspective", 100.0, 0.1)
    a.aspect_ratio = f32(w) / f32(h)
    a.set_camera_data(view, proj)
    handle, _ = a.prefilter_environment(src)
    a.set_background_texture(handle)
    auto = {s: a.render(w, h, samples=s) for s in (1, 4)}
    want = I.prefilter(levels)
    # whole levels: the frame of a one-level Rgba32Float cube uploaded from the read-back level
    b = r3.Renderer(oh.LEFT, f32(1.0))
    b.aspect_ratio = f32(w) / f32(h)
    b.set_camera_data(view, proj)
    last = {}
    for k in range(L):
        n = I.level_extent(S_, k)
        back = np.stack([a.readback_cube_face(handle, k, f)[1:-1, 1:-1] for f in range(6)])
        assert np.array_equal(E.bits(back), E.bits(want[k]))
        b.replace_texture_cubes([])
        b.set_background_texture(b.add_texture_cube_encoded(C.RGBA32F, n, [[np.ascontiguousarray(back[f]).tobytes()] for f in range(6)]))
        a.set_skybox_level(float(k))
        for samples in (1, 4):
            fa, fb = a.render(w, h, samples=samples), b.render(w, h, samples=samples)
            assert np.array_equal(fa["hdr16"], fb["hdr16"]) and np.array_equal(fa["rgba8"], fb["rgba8"]), f"level {k} samples {samples}"
            assert len(np.unique(fa["hdr16"].reshape(-1, 4), axis=0)) > (4 if n > 1 else 0)
            last[samples] = fb
    # a level beyond the last is the last; a fraction mixes two levels as the reference does
    a.set_skybox_level(99.0)
    assert np.array_equal(a.render(w, h)["hdr16"], last[1]["hdr16"])
    inv = cases.inverse_matrix(oh.LEFT, view, proj, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    d = S.pixel_directions(inv, w, h, xs.reshape(-1), ys.reshape(-1))
    for lod in (0.25, 1.5, 2.75):
        a.set_skybox_level(lod)
        level = np.full(len(d), int(lod), dtype=np.int64)
        frac = np.full(len(d), f32(lod) - f32(int(lod)), dtype=f32)
        mixed = lodref.sample(want, I.F32_CLASS, d, level, frac).astype(np.float16).view(np.uint16).reshape(h, w, 4)
        for samples in (1, 4):
            assert np.array_equal(a.render(w, h, samples=samples)["hdr16"], mixed), f"level {lod} samples {samples}"
    # negative: the automatic frame, bit for bit
    a.set_skybox_level(-1.0)
    for samples in (1, 4):
        again = a.render(w, h, samples=samples)
        assert np.array_equal(again["hdr16"], auto[samples]["hdr16"]) and np.array_equal(again["rgba8"], auto[samples]["rgba8"])
    # a one-level cube ignores the level
    b.set_skybox_level(2.0)
    assert np.array_equal(b.render(w, h)["hdr16"], last[1]["hdr16"])
    a.close()
    b.close()
