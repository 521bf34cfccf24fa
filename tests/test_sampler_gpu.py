"""The texture sampler (rend3_amd/csrc/texture.h) on the GPU, bit for bit against the oracle's tex_sample_grad, on every path it can
take: through r3n_sample_probe -- every instantiation the frame's kernels launch, on the query sets of tests/sampler_queries.py,
one thread per query and 64 consecutive queries a wavefront -- and through whole frames of a stage whose quads have chosen
texture coordinates and gradients.  tests/test_sampler.py holds, on the oracle alone, the conditions this file rests on: every path
name below is reached by whole waves and inside mixed ones, every reference value is finite (so equality is of the u32 words, the
sign of zero included), and the half-size rule of TexShare holds on the contract's own arithmetic.

Which query set reaches which path of sampler_queries.VOCABULARY (sets that reach it with whole waves first):
  unbound                  share_triples (a slot without a map, and the triple without any); every set under share / batched
  general                  texel_lattice, wild_coordinates, lod_edges, row_wrap (37x19, 3x5, the float textures, the nearest sampler)
  general_remainder_wrap   texel_lattice, wild_coordinates, lod_edges, row_wrap (37x19, 3x5)
  general_float_texels     texel_lattice, wild_coordinates, lod_edges, row_wrap (Rgba32Float 8x8, Rgba16Float 16x4)
  general_nearest          texel_lattice (levels up to 16 texels), wild_coordinates, lod_edges
  nearest_rounds_up        wild_coordinates (rho = 1.5 * 2^k), lod_edges (1.5 * 2^k and the f32 on either side)
  short                    every set
  short_fallback           wild_coordinates (floors of 2^24 and more, infinite, NaN; general entry only)
  total_block              wild_coordinates (the same queries through the short-path-only forms)
  one_level / two_levels   every set / all but texel_lattice
  closed_form_tail         texel_lattice, row_wrap, lod_edges, wild_coordinates (128x32, 32x128, 64x1, 1x64 past their square part)
  share_recomputed         every set; share_same: texel_lattice, row_wrap (one texture three times), share_triples;
  share_half               share_triples
  batched_accepts / batched_declines / batched_lane_misfit    share_triples (declines: whole waves of a misfit relation, and waves
                           in which only some lanes' maps do not fit); every other set is accepted
  batched_first_is_f1 / batched_half_shifted / batched_unbound_slot    share_triples (level 0 / level >= 1 / a slot unbound)
  row_pair / row_wrap      row_wrap (both table orders: the pool's last word is last16's 1x1 level, or w64x1's), texel_lattice,
                           every 1-texel-wide level
  alpha_one / alpha_zero / alpha_arithmetic    alpha_footprints (a255, a0, block interiors of a0_255; borders, 254/255, 0/1, 128)

What these tests notice (each a one-line change to a scratch copy of csrc/, built with rend3_amd.build.build(csrc=, out=, obj_dir=)
and loaded through R3N_LIB; this file run against it once; every change keeps every address inside the pool):
  tex_footprint: `frac >= 0.5f` -> `> 0.5f` (nearest, ties up)        probe: grad, grad_rgb, alpha on lod_edges and wild_coordinates (rho =
                                                                        1.5 * 2^k); the stale-id / general probes after the removal
  tex_sample_alpha: the shortcut widened to any uniform byte           probe: alpha, alpha_short on alpha_footprints, lod_edges, share_triples,
    (`all_and == all_or` -> unorm8(all_and))                            row_wrap (both orders); the probes after the removal
  tex_level_start_pow2: the tail term dropped (`false && L > m + 1`)   probe: short, short_rgb, share, alpha_short, batched on texel_lattice,
                                                                        wild_coordinates, lod_edges, share_triples, row_wrap (both orders);
                                                                        frames: class_kernels, the replaced-texture sequence (frame 0)
  tex_sample3_batched: first_is_f1 ignored for the first level's       probe: batched on share_triples (first: s64 / l32 / l64 at level 0);
    weights (`bilinear(ta[k], .., f0)`)                                 frames: class_kernels, the replaced-texture sequence (721 px)
  tex_sample3_batched: the wrap patch of the first level's 8-byte      probe: batched on every set (row_wrap under both table orders);
    row loads skipped (`false && __any(wrap_a)`)                        frames: class_kernels, the replaced-texture sequence
  commit_texture_placement (r3n_textures_update): classes_dirty        test_a_replaced_texture_moves_its_materials_between_the_kernels alone
    not raised                                                          (frame 1: HDR differs in 3537 px); every other test passes
  the same line: cutout_short_dirty not raised                         the same test alone (frame 1: 256 px of visibility keys differ: the
                                                                        SHORTA rasterisers went on sampling the 37 x 19 map)
  (first_is_f1 ignored for `two[k]`, the issue's example, was NOT tried: the second level's loads then apply the reference's level-1
  footprint to the half-size map's level 1, past the end of its chain -- and of the pool, for last16.)

Not reachable through the public texture calls: small_pool == 0 (a pool beyond 2^30 words: 4 GiB of texels, too large for a test),
so the general sampler behind a power-of-two RGBA8 texture is reached by the nearest sampler and by wild coordinates only; the
last term of tex_level_start_pow2 (`L > M + 1`: levels behind the chain's 1x1 level), because a chain has at most
floor(log2(max(w, h))) + 1 levels (texture_jobs.h chain_fault); extents whose product is beyond 2^29 (texture_is_short's guard)."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import sampler_queries as sq
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames
from test_sampler import reference

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARG = -1
OPAQUE, CUTOUT, BLEND = 0, 1, 2


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


_PRODUCTS = {}


@pytest.fixture(scope="module")
def products(r3):
    """order -> a product renderer holding the table: built once per order, shared, never changed"""
    def get(order):
        if order not in _PRODUCTS:
            p = r3.Renderer(oh.LEFT, f32(1.0))
            sq.Table(order).build(p)
            _PRODUCTS[order] = p
        return _PRODUCTS[order]
    yield get
    for p in _PRODUCTS.values():
        p.close()
    _PRODUCTS.clear()


# ------------------------------------------------------------------------------------------------------------------ probe tests
def expected_words(form, want):
    """The u32 words a form must return, from three independent oracle samples per query: a channel the form does not produce is
    +0.  (n, 3, 4) u32."""
    w = np.ascontiguousarray(want["rgba"]).view(np.uint32)
    exp = np.zeros_like(w)
    if form in ("grad", "short"):
        exp[:, 0, :] = w[:, 0, :]
    elif form in ("grad_rgb", "short_rgb"):
        exp[:, 0, :3] = w[:, 0, :3]
    elif form in ("alpha", "alpha_short"):
        exp[:, 0, 3] = w[:, 0, 3]
    else:  # share, batched: slots 0 and 1 with alpha, slot 2 without
        exp[:, :2, :] = w[:, :2, :]
        exp[:, 2, :3] = w[:, 2, :3]
    return exp


def describe(table, q, P):
    names = [table.names[i - 1] if 1 <= i <= len(table.names) else str(i) for i in q["id"]]
    taken = [k for k, v in P.items() if k != "valid" and v[0]]
    return (f"textures {names} nearest {int(q['nearest'])} u {float(q['u'])!r} v {float(q['v'])!r} ddx {q['ddx'].tolist()} "
            f"ddy {q['ddy'].tolist()} paths {taken}")


def probe_and_compare(p, ref, table, form, q, tag, sample=None):
    """Drops what the form's preconditions exclude, runs the probe and the oracle on the rest, compares words."""
    q = np.ascontiguousarray(q[sq.paths(q, form, table)["valid"]])
    assert len(q) >= 64, tag
    P = sq.paths(q, form, table)  # (of the array as it is sent: its waves are the probe's)
    got = p.sample_probe(sq.FORMS.index(form), q)
    want = (sample or ref.sample)(q)
    assert np.isfinite(want["rgba"]).all()
    exp = expected_words(form, want)
    g = np.ascontiguousarray(got["rgba"]).view(np.uint32)
    compare = np.ones(len(q), dtype=bool)
    if form == "batched":
        flags_ok = got["flags"] == P["batched_accepts"].astype(np.uint32)
        assert flags_ok.all(), f"{tag}: the batched form's flag differs from the classifier's on {int((~flags_ok).sum())} queries, first: " \
            + describe(table, q[np.argmin(flags_ok)], {k: v[np.argmin(flags_ok):][:1] for k, v in P.items()})
        compare = P["batched_accepts"]
        assert compare.any() or "share" in tag
    else:
        assert (got["flags"] == 0).all(), tag
    bad = (g != exp).reshape(len(q), -1).any(axis=1) & compare
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{tag}: {int(bad.sum())} of {int(compare.sum())} queries differ from the oracle; first, query {i}: "
                             + describe(table, q[i], {k: v[i:i + 1] for k, v in P.items()})
                             + f"\n  got  {got['rgba'][i].tolist()}\n  want {want['rgba'][i].tolist()} (channels the form produces)")
    return int(compare.sum())


CASES = [(name, "a") for name in sq.SETS] + [("row_wrap", "b")]


@pytest.mark.parametrize("form", sq.FORMS)
@pytest.mark.parametrize("set_name,order", CASES, ids=[f"{n}-{o}" for n, o in CASES])
def test_probe_equals_oracle(products, set_name, order, form):
    ref = reference(order)
    q = ref.sets[set_name][0]
    n = probe_and_compare(products(order), ref, ref.table, form, q, f"{form} on {set_name} (table order {order})")
    assert n >= 64


def test_probe_refuses_what_the_short_forms_cannot_take(products):
    """Every kind of violation returns R3N_ERR_INVALID_ARG without a launch, and the context goes on working."""
    p, ref = products("a"), reference("a")
    t = ref.table
    ok = sq.make((t.id("l32"), t.id("s64"), t.id("l64")), 0.3, 0.6, (0.05, 0.0), (0.0, 0.02))

    def code(form, q):
        q = np.ascontiguousarray(q)
        out = np.zeros(len(q), dtype=sq.RESULT)
        return p.lib.r3n_sample_probe(p.ctx, form, q.ctypes.data_as(ctypes.c_void_p), len(q), out.ctypes.data_as(ctypes.c_void_p))

    def with_id(slot, tid, nearest=0):
        q = np.concatenate([ok] * 70)  # the offender sits in the second wave
        q["id"][66, slot] = tid
        q["nearest"][66] = nearest
        return q
    short_only = [sq.FORMS.index(f) for f in sq.SHORT_ONLY_FORMS]
    for form in short_only:
        slots = (0, 1, 2) if sq.FORMS[form] in sq.THREE_MAP_FORMS else (0,)
        for slot in slots:
            for bad in (t.id("odd37x19"), t.id("odd3x5"), t.id("f32_8"), t.id("f16_16x4"), len(t.names) + 1, 0xFFFFFFFF):
                assert code(form, with_id(slot, bad)) == INVALID_ARG, (sq.FORMS[form], slot, bad)
        assert code(form, with_id(0, t.id("l32"), nearest=1)) == INVALID_ARG, sq.FORMS[form]
        assert b"sample probe" in p.lib.r3n_last_error(p.ctx)
        assert code(form, with_id(0, 0)) == 0  # an unbound slot is no violation
    for form in (len(sq.FORMS), len(sq.FORMS) + 1, 0xFFFFFFFF):
        assert code(form, ok) == INVALID_ARG, form
    # the general forms take all of it, as the product does
    for form in ("grad", "grad_rgb", "alpha"):
        for bad in (t.id("odd37x19"), len(t.names) + 1, 0xFFFFFFFF):
            assert code(sq.FORMS.index(form), with_id(0, bad, nearest=1)) == 0
    # (what an id past the table returns -- zeros, like the oracle -- is compared in test_probe_equals_oracle: wild_coordinates asks it)
    # and the context is as usable as before
    for form in ("short", "batched", "grad"):
        probe_and_compare(p, ref, t, form, ref.sets["row_wrap"][0], f"{form} after the refusals")


def _replace_in_place(p, slot, fmt, w, h, levels):
    """r3n_textures_update on a slot that holds a texture: replaced where it is, without a removal in front (the Renderer only ever
    adds and removes; its bookkeeping of the slot -- live -- stays right)."""
    from rend3_amd import _ffi
    p.sync()
    payload = np.frombuffer(b"".join(levels), dtype=np.uint8).copy()
    assert len(payload) % 4 == 0
    descs = np.array([[0, w, h, len(levels), fmt, 0, 0, 0]], dtype=np.uint32)
    slots = np.array([slot], dtype=np.uint32)
    _ffi.check(p.ctx, p.lib.r3n_textures_update(p.ctx, _ffi.ptr(slots), _ffi.ptr(descs), 1, _ffi.ptr(payload), len(payload)), "r3n_textures_update")


def _replace_in_oracle(o, slot, fmt, w, h, levels):
    """the oracle has no slots to reuse: the new texture is appended and its descriptor row moved into the slot"""
    o.add_texture_2d_encoded(fmt, w, h, levels)
    o.tex_descs[slot] = o.tex_descs[-1]
    o.tex_descs = np.ascontiguousarray(o.tex_descs[:-1])


def test_probe_after_remove_compact_and_replace(r3):
    """The probe sees the context's texture state as it is: after a removal in the middle of the table, after a compaction (every
    later texture at a new offset, the level-offset table rewritten), and after an update puts the 37 x 19 texture into a short
    texture's slot (the slot leaves the short path, and the probe's own validation must say so).  After each of the three, ids that
    stay valid are asked through every form, and the removed slot's stale id through the general forms alone, where it reads the
    1 x 1 RGBA8 entry at pool word 0 that r3n_textures_remove leaves (r3n.h).  The oracle has no removal: its removed slot is that
    entry written by hand into its descriptor table, (offset 0, 1 x 1, one level, unorm) -- pool word 0 is s64's first texel on
    both sides, before and after the compaction."""
    ref = reference("a")
    table = copy.copy(ref.table)
    o = OracleRenderer(oh.LEFT, f32(1.0))
    sq.Table("a").build(o)
    p = r3.Renderer(oh.LEFT, f32(1.0), texture_upload="stream")
    try:
        sq.Table("a").build(p)
        gone = table.names.index("c64m3")
        sets = ("share_triples", "row_wrap", "lod_edges")

        def check(tag):
            table.descs, table.pool = o.tex_descs.copy(), o.tex_pool
            for set_name in sets:
                q = ref.sets[set_name][0]
                q = q[~(q["id"] == gone + 1).any(axis=1)]
                for form in sq.FORMS:
                    probe_and_compare(p, ref, table, form, q, f"{form} on {set_name} {tag}", sample=lambda x: ref.sample(x, o))
            q = ref.sets["lod_edges"][0]
            q = q[q["id"][:, 0] == gone + 1].copy()
            assert len(q) >= 64
            for form in ("grad", "grad_rgb", "alpha"):
                probe_and_compare(p, ref, table, form, q, f"{form}, the stale id {tag}", sample=lambda x: ref.sample(x, o))

        p.remove_texture(gone)
        o.tex_descs[gone] = (0, 1, 1, 1, 0, 0, 0, 0)  # what a removed slot reads as (r3n.h r3n_textures_remove): pool word 0 -- s64's first texel
        check("after the removal")
        moved = p.compact_textures()
        assert moved["textures_moved"] >= 10
        check("after the compaction")
        slot = table.names.index("l32")
        odd = ref.table.specs[ref.table.names.index("odd37x19")]
        _replace_in_place(p, slot, odd[4], odd[1], odd[2], ref.table.levels_of("odd37x19"))
        _replace_in_oracle(o, slot, odd[4], odd[1], odd[2], ref.table.levels_of("odd37x19"))
        check("after the replacement")
        # the slot has left the short path: the classifier says so, and so does the probe's validation (h_tex_short follows the update)
        one = np.concatenate([sq.make((slot + 1, slot + 1, slot + 1), 0.5, 0.5, (0, 0), (0, 0))] * 64)
        out = np.zeros(len(one), dtype=sq.RESULT)
        for form in sq.FORMS:
            code = p.lib.r3n_sample_probe(p.ctx, sq.FORMS.index(form), one.ctypes.data_as(ctypes.c_void_p), len(one), out.ctypes.data_as(ctypes.c_void_p))
            assert code == (INVALID_ARG if form in sq.SHORT_ONLY_FORMS else 0), (form, code)
            assert sq.paths(one, form, table)["valid"].all() == (form not in sq.SHORT_ONLY_FORMS), form
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------------------------ frame tests
W, H, CELL = 128, 96, 16
AMBIENT, CLEAR = (0.05, 0.05, 0.05, 1.0), (0.1, 0.05, 0.1, 1.0)
# (samples, blend quads, environment): the resolves tests/test_lights_gpu.py names
FRAME_FORMS = {
    "class_kernels": (1, False, {}),
    "general_kernel": (1, False, {"R3N_RESOLVE_CLASSES": "0"}),
    "split": (4, False, {}),
    "unsplit_blend": (4, True, {}),
}


def quad_list(table):
    """(kind, textures, per-pixel uv span as a multiple of 1 / width of the first texture, uv origin, NaN vertex?) per grid cell"""
    t = table.names.index
    cells = [
        ("albedo", [t("s64")], 1.0, (2.0 ** 24, 0.25), False),              # offset by 2^24: floors past the short path's range
        ("albedo", [t("l64")], 2.0, (3e9, 0.5), False),                     # by 3e9: the wrap gives up
        ("albedo", [t("l32")], 1.0, (0.25, 0.25), True),                    # one NaN component at one vertex
        ("albedo", [t("l32")], 1.0, (1.0 - 8.0 / 32.0, 0.0), False),        # the row wraps at the right edge inside the quad
        ("albedo", [t("last16")], 16.0, (0.0, 0.0), False),                 # the last texture of the pool at its 1x1 level
        ("albedo", [t("last16")], 12.0, (0.125, 0.25), False),              # ... and between its last two
        ("albedo", [t("r128x32")], 128.0, (0.0, 0.0), False),               # the non-square chains at their tails
        ("albedo", [t("r128x32")], 96.0, (0.3, 0.1), False),
        ("albedo", [t("r32x128")], 24.0, (0.1, 0.3), False),
        ("albedo", [t("w64x1")], 32.0, (0.0, 0.0), False),
        ("albedo", [t("h1x64")], 48.0, (0.2, 0.2), False),
        ("nearest", [t("odd37x19")], 3.0, (0.0, 0.0), False),
    ]
    spans = (0.5, 1.5, 2.0, 3.0, 6.0)
    for k, (name, ids) in enumerate(sq.share_relations(table)):
        if any(ids):
            cells.append(("pbr", [i - 1 if i else None for i in ids], spans[k % len(spans)], (0.125 * (k % 8), 0.0625 * (k % 5)), False))
    for k, name in enumerate(sq.ALPHA_NAMES):
        cells.append(("cutout", [t(name)], 1.0, (0.0, 0.03125 * k), False))
        cells.append(("cutout", [t(name)], 1.5, (0.25, 0.5), False))
    assert len(cells) <= (W // CELL) * (H // CELL), len(cells)
    return cells


def build_stage(r, mk, table, blend):
    """A grid of axis-aligned 16 x 16 pixel quads under the identity view and a raw identity projection: clip space is the
    quads' own coordinates, a quad's uv span per pixel is what quad_list names.  One material per quad; directional lights
    with small shadow maps, so that the shadow rasteriser's cutout test samples the alpha textures too.  Returns the material
    handles by cell."""
    handles = table.build(r)
    r.set_camera_data(oh.identity(), ("raw", oh.identity()))
    # two lights: one on the quads' fronts, and one from behind -- shadow views cull FRONT faces, so that one's view draws them
    r.add_directional_light(color=(1.0, 0.9, 0.8), intensity=2.0, direction=(0.2, -0.3, 1.0), distance=4.0, resolution=128)
    r.add_directional_light(color=(0.3, 0.4, 0.5), intensity=1.0, direction=(-0.2, -0.3, -1.0), distance=4.0, resolution=128)
    mats = []
    for cell, (kind, tex, span, origin, nan) in enumerate(quad_list(table)):
        cx, cy = cell % (W // CELL), cell // (W // CELL)
        x0, x1 = -1.0 + 2.0 * CELL * cx / W, -1.0 + 2.0 * CELL * (cx + 1) / W
        y0, y1 = 1.0 - 2.0 * CELL * cy / H, 1.0 - 2.0 * CELL * (cy + 1) / H
        width = int(table.descs[tex[0] if tex[0] is not None else next(i for i in tex if i is not None)][1])
        du = span / width
        u0, v0 = origin
        #      top left       top right                 bottom left               bottom right
        pos = [(x0, y0, 0.5), (x1, y0, 0.5), (x0, y1, 0.5), (x1, y1, 0.5)]
        uv = np.array([(u0, v0), (u0 + CELL * du, v0), (u0, v0 + CELL * du), (u0 + CELL * du, v0 + CELL * du)], dtype=f32)
        if nan:
            uv[1, 0] = np.nan  # the top right vertex: one of the two triangles interpolates NaN
        mesh = r.add_mesh(pos, [3, 2, 0, 3, 0, 1], normals=[(0, 0, -1)] * 4, tangents=[(1, 0, 0)] * 4, uv0=uv)
        if kind == "albedo":
            mat = r.add_material(mk(albedo_mode="texture", albedo_texture=handles[tex[0]], roughness=0.6), OPAQUE)
        elif kind == "nearest":
            mat = r.add_material(mk(albedo_mode="texture", albedo_texture=handles[tex[0]], roughness=0.6, nearest=True), OPAQUE)
        elif kind == "cutout":
            mat = r.add_material(mk(albedo_mode="texture", albedo_texture=handles[tex[0]], roughness=0.5, cutout=0.5), CUTOUT)
        else:  # the PBR class: base colour, normal and AO / roughness / metallic maps, nothing else
            a, n, m = (None if i is None else handles[i] for i in tex)
            mat = r.add_material(mk(albedo_mode="texture" if a is not None else "value", albedo=(0.8, 0.7, 0.6, 1.0), albedo_texture=a, roughness=0.7,
                                    metallic=0.3, normal_texture=n, aomr=None if m is None else ("combined", m)), OPAQUE)
        mats.append(mat)
        r.add_object(mesh, mat, oh.identity())
    if blend:
        for z, alpha in ((0.75, 0.5), (0.25, 0.35)):  # one in front of the grid and one behind it, whichever way depth runs
            pos = [(-0.9, 0.8, z), (0.7, 0.8, z), (-0.9, -0.6, z), (0.7, -0.6, z)]
            uv = np.array([(0, 0), (3.0, 0), (0, 2.0), (3.0, 2.0)], dtype=f32)
            mesh = r.add_mesh(pos, [3, 2, 0, 3, 0, 1], normals=[(0, 0, -1)] * 4, uv0=uv)
            mat = r.add_material(mk(albedo_mode="texture_value", albedo_texture=handles[table.names.index("a0_255")],
                                    albedo=(1.0, 1.0, 1.0, alpha), roughness=0.4), BLEND)
            r.add_object(mesh, mat, oh.identity())
    return mats


def render(r, samples):
    return r.render(W, H, samples=samples, ambient=AMBIENT, clear_color=CLEAR)


@functools.lru_cache(maxsize=None)
def oracle_frames(samples, blend):
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    build_stage(o, omk, sq.Table("a"), blend)
    frames = [render(o, samples) for _ in range(2)]
    covered = (frames[0]["vis"].reshape(-1) != frames[0]["vis"].reshape(-1)[-1]).mean()
    assert covered > 0.6, f"the stage's quads cover {covered:.0%} of the frame: wrong winding or depth?"
    assert len(np.unique(frames[0]["atlas"].view(np.uint32))) > 1, "no shadow view drew a quad"
    return frames


@pytest.mark.parametrize("form", list(FRAME_FORMS))
def test_frames_of_the_sampler_stage(r3, monkeypatch, form):
    """Two frames (the second draws the predicted set) of the stage through every resolve: sets, keys, the shadow atlas as words, HDR
    f16 bit for bit."""
    samples, blend, env = FRAME_FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = oracle_frames(samples, blend)
    p = r3.Renderer(oh.LEFT, f32(W) / f32(H))
    try:
        build_stage(p, r3.material_record, sq.Table("a"), blend)
        for f, fo in enumerate(want):
            compare_frames(fo, render(p, samples), f"sampler stage, {form}, frame {f}")
    finally:
        p.close()


def test_a_replaced_texture_moves_its_materials_between_the_kernels(r3):
    """Three frames on one context.  Frame 0: every bound texture is short (the class kernels' short-path-only instantiations, the
    SHORTA rasterisers).  In front of frame 1 the albedo map of a PBR material and that of a cutout material are replaced, in their
    slots, by the 37 x 19 texture: the materials' records do not change, their classes must (R3N_FEAT_TEX_GENERAL,
    cutout_alpha_short).  In front of frame 2 they are replaced back.  All three frames equal the oracle's."""
    table = sq.Table("a")
    o = OracleRenderer(oh.LEFT, f32(W) / f32(H))
    p = r3.Renderer(oh.LEFT, f32(W) / f32(H), texture_upload="stream")
    try:
        build_stage(o, omk, table, False)
        build_stage(p, r3.material_record, sq.Table("a"), False)
        # unbind what is not short in frame 0: the nearest quad's 37 x 19 map gives way to a short one (the material is rewritten
        # on both sides; the slots replaced below are named by OTHER materials, which stay as they are)
        cells = quad_list(table)
        near = next(k for k, c in enumerate(cells) if c[0] == "nearest")
        for r, mk in ((o, omk), (p, r3.material_record)):
            r.update_material(near, mk(albedo_mode="texture", albedo_texture=table.names.index("s16"), roughness=0.6))
        slots = [table.names.index("l32"), table.names.index("a0_255")]  # albedo of PBR quads / of cutout quads (and more)
        assert any(c[0] == "pbr" and c[1][0] == slots[0] for c in cells) and any(c[0] == "cutout" and c[1][0] == slots[1] for c in cells)
        odd = table.specs[table.names.index("odd37x19")]
        saved = o.tex_descs[slots].copy()
        for f in range(3):
            if f == 1:
                for s in slots:  # r3n_textures_update alone: no removal whose own dirty flags would cover for the update's
                    _replace_in_place(p, s, odd[4], odd[1], odd[2], table.levels_of("odd37x19"))
                    _replace_in_oracle(o, s, odd[4], odd[1], odd[2], table.levels_of("odd37x19"))
            if f == 2:
                for s in slots:
                    spec = table.specs[s]
                    _replace_in_place(p, s, spec[4], spec[1], spec[2], table.levels_of(spec[0]))
                o.tex_descs[slots] = saved
            compare_frames(render(o, 1), render(p, 1), f"replaced textures, frame {f}")
    finally:
        p.close()
