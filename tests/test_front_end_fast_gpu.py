"""The geometry front end's shortcuts (R3N_TUNE front_end_fast: packed transforms, the unit-w paths of the triangle cull and of
prepare_triangle, no depth in a shadow view's cull) change no bit: every world here is rendered twice, under front_end_fast=1 and
under front_end_fast=0, on 64 x 64 targets.  Each build's pass / residual sets and both lists are compared with
tests/triangle_cull_reference.py (entry by entry per region: triangle_cull_worlds.check_list) and its whole frames with the
oracle; then the two builds with each other, bit for bit: sets, the lists' entries per region, the shadow atlas, the visibility
keys, the Hi-Z pyramid.

A world is tests/triangle_cull_worlds.py's (records over one shared index run) with two additions: the run may draw from a table
with EXTRA triangles behind triangle_cull_worlds.TABLE, and an object may carry a model matrix of its own -- so the expectation is
traced per triangle with its object's baked matrix.

  counts        objects of 1, 64, 65 and 64 * R3N_CHUNK_ITERS + 1 triangles under the orthographic shadow view (a single slot, a
                full pair, a pair whose second slot has one live lane -- the clamped lanes fetch the last triangle --, a chunk
                boundary), the affine viewport (w = 1: the unit-w path WITH depth and Hi-Z against the injected cone plane, which
                occludes some of the table and not others) and the perspective viewport (w = mesh z: the general path)
  edges         the whole table -- det == 0, smin / smax that round to the same integer through a tie -- plus triangles that
                escape the tie by one step of the clip coordinate, for both values of POSITIVE_AREA_VISIBLE (the shadow view and
                the right-handed viewport have it, the left-handed viewport has not) and, multisampled, with the rounding rule off
  non-finite    a wave slot of 63 finite triangles and one with a +inf coordinate, another with a NaN coordinate: w = 0 * inf = NaN
                is not 1, the whole slot takes the divisions and gives the oracle's bits.  The two finite vertices of each span
                several pixels, so the cull passes the triangle (fminf / fmaxf skip the NaN) and prepare_triangle meets it too:
                in the shadow view's draw of the same frame and in the viewport's first pass of the next
  disagreement  one object with a model matrix whose last row is (0, 0, 1/4, 1): w != 1 for its slots only, between neighbours
                that go unit-w in the same launch, in a shadow view and in the affine viewport"""
import numpy as np
import pytest

import object_pass_reference as op
import triangle_cull_reference as tc
import triangle_cull_worlds as tw
from oracle import host as oh
from test_gpu_parity import compare_frames
from test_hiz_gpu import Inject, oracle_hook
from test_triangle_cull_gpu import Product, check_lists, check_sets

pytestmark = pytest.mark.gpu
f32, u32, u64, i64 = np.float32, np.uint32, np.uint64, np.int64
TUNES = ("front_end_fast=1", "front_end_fast=0")
CHUNK_BOUNDARY = 64 * tc.CHUNK_ITERS + 1


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


# ------------------------------------------------------------------ tables and runs
def escape_triangles():
    """smin = 3.5 exactly (rounds to 4); smax one step of the clip coordinate above 4.5 (rounds to 5: the triangle escapes the
    rule that rejects rint_x_k_odd) -- in x and in y, both windings"""
    out = []
    for positive in (False, True):
        bx = tw.box(3.5, 10, 4.5, 20, positive=positive)
        by = tw.box(10, 7.5, 20, 8.5, positive=positive)
        top_x, top_y = f32(tw.clip64(4.5)), f32(tw.clip64(8.5))
        bx[bx[:, 0] == top_x, 0] = np.nextafter(top_x, f32(1.0))
        by[by[:, 1] == top_y, 1] = np.nextafter(top_y, f32(1.0))
        out += [bx, by]
    return np.stack(out).astype(f32)


def non_finite_triangles():
    """two finite vertices eight pixels apart in x and y, the third with a +inf / a NaN coordinate; both windings"""
    a, b = (tw.clip64(20), tw.clip64(20)), (tw.clip64(28), tw.clip64(28))
    out = []
    for bad in (f32(np.inf), f32(np.nan)):
        for order in ((0, 1, 2), (1, 0, 2)):
            v = np.array([(*a, 1.0), (*b, 1.0), (bad, tw.clip64(24), 1.0)], dtype=f32)
            out.append(v[list(order)])
    return np.stack(out).astype(f32)


ESCAPE, NON_FINITE = escape_triangles(), non_finite_triangles()
POSITIONS = np.concatenate([tw.TABLE.positions, ESCAPE, NON_FINITE]).astype(f32)
ESCAPE_IDS = len(tw.TABLE) + np.arange(len(ESCAPE))
INF_IDS = len(tw.TABLE) + len(ESCAPE) + np.arange(2)
NAN_IDS = len(tw.TABLE) + len(ESCAPE) + 2 + np.arange(2)


def special_slots():
    """(run, start of the inf slot, start of the NaN slot, start of the escape triangles): tw.RUN, then two 64-entry stretches of
    robustly passing palette triangles with one non-finite triangle each (lane 17, lane 63), then the escapes"""
    ok = np.concatenate([tw.TABLE.pal_ids("pass"), tw.TABLE.pal_ids("back")])
    fill = ok[np.arange(64) % len(ok)]
    s_inf, s_nan = fill.copy(), fill.copy()
    s_inf[17], s_nan[63] = INF_IDS[0], NAN_IDS[1]
    s_inf2, s_nan2 = fill.copy(), fill.copy()
    s_inf2[0], s_nan2[31] = INF_IDS[1], NAN_IDS[0]
    run = np.concatenate([tw.RUN, s_inf, s_nan, s_inf2, s_nan2, ESCAPE_IDS, fill]).astype(i64)
    at = len(tw.RUN)
    return run, at, at + 64, at + 128, at + 192, at + 256


RUN, AT_INF, AT_NAN, AT_INF2, AT_NAN2, AT_ESCAPE = special_slots()
INDICES = (3 * RUN[:, None] + np.arange(3)[None, :]).reshape(-1).astype(u32)
NOT_AFFINE = np.eye(4, dtype=f32).reshape(-1).copy()
NOT_AFFINE[11] = 0.25  # column-major: last row (0, 0, 1/4, 1) -- w = z / 4 + 1


MIN_CAPACITY = 16  # a context's object buffer starts at sixteen slots (FreelistDerivedBuffer::STARTING_SIZE) and never shrinks


def world(ntri, start, transforms=None, materials=None):
    """the objects given, then disabled slots up to MIN_CAPACITY"""
    live = len(ntri)
    pad = max(MIN_CAPACITY - live, 0)
    ntri, start = list(ntri) + [1] * pad, list(start) + [0] * pad
    if materials is not None:
        materials = list(materials) + [0] * pad
    n = len(ntri)
    w = dict(capacity=n, ntri=np.asarray(ntri, dtype=i64), start=np.asarray(start, dtype=i64), enabled=np.arange(n) < live,
             material=np.asarray(materials if materials is not None else [(0, 1)[i % 2] for i in range(n)], dtype=u32),
             spheres=np.tile(tw.DRAWN_SPHERE, (n, 1)), transform=np.tile(np.eye(4, dtype=f32).reshape(-1), (n, 1)))
    for slot, m in (transforms or {}).items():
        w["transform"][slot] = m
    assert (w["start"] + w["ntri"] <= len(RUN)).all()
    return w


def records(w, mesh):
    rec = tw.records(w, mesh)
    rec.view(f32)[:, 0:16] = w["transform"]
    return rec


WORLDS = {
    # the four counts, each from the run's first entry where it is long enough to hold the FORMS, and once more from the seeded part
    "counts": lambda: world([1, 64, 65, CHUNK_BOUNDARY, 1, 65, 64, CHUNK_BOUNDARY, 1], [7, 0, 64, 0, tw.RANDOM_FROM + 5, tw.RANDOM_FROM + 70, tw.RANDOM_FROM + 200, tw.RANDOM_FROM + 300, 3]),
    # every table entry (an object of 5 * 64 + len(TABLE) triangles from the run's start), the escapes, a single slot
    "edges": lambda: world([tw.RANDOM_FROM, len(ESCAPE), 1], [0, AT_ESCAPE, AT_ESCAPE + 1]),
    # the non-finite slots as objects of their own (single slots), as a pair of one object, and behind finite neighbours
    "non_finite": lambda: world([64, 64, 64, 128, 65, 64], [0, AT_INF, AT_NAN, AT_INF2, 64, AT_NAN2], materials=[0, 0, 0, 0, 0, 0]),
    # object 1's matrix is not affine: its three slots divide, objects 0 and 2 beside it do not
    "disagreement": lambda: world([65, 130, 64, 1], [0, 64, 128, 9], transforms={1: NOT_AFFINE}),
}
# world, handedness, samples, projections of the two frames (the second has history and draws the first's predicted list), the light
CASES = {
    "counts-left": dict(world="counts", hand="left", samples=1, frames=("affine", "alt"), light=True),
    "counts-perspective": dict(world="counts", hand="left", samples=1, frames=("w", "affine"), light=False),
    "edges-left": dict(world="edges", hand="left", samples=1, frames=("affine", "affine"), light=True),
    "edges-right": dict(world="edges", hand="right", samples=1, frames=("affine", "alt"), light=True),
    "edges-left-4-samples": dict(world="edges", hand="left", samples=4, frames=("affine", "affine"), light=False),
    "edges-right-4-samples": dict(world="edges", hand="right", samples=4, frames=("affine", "affine"), light=False),
    "non-finite-left": dict(world="non_finite", hand="left", samples=1, frames=("affine", "affine"), light=True),
    "non-finite-right": dict(world="non_finite", hand="right", samples=1, frames=("affine", "alt"), light=True),
    "disagreement-left": dict(world="disagreement", hand="left", samples=1, frames=("affine", "alt"), light=True),
    "disagreement-right": dict(world="disagreement", hand="right", samples=1, frames=("affine", "affine"), light=True),
}


def setup_renderer(r, mk, oracle_side=False):
    """triangle_cull_worlds.setup_renderer with this file's table and run (normals given: none is computed from a NaN)"""
    normals = np.tile(np.array([0.0, 0.0, 1.0], dtype=f32), (len(POSITIONS) * 3, 1))
    m = r.add_mesh(POSITIONS.reshape(-1, 3), INDICES, normals=normals, mesh_handedness=0)
    r.add_material(mk(albedo=(0.2, 0.6, 0.9, 1.0), albedo_mode="value", unlit=True), tc.OPAQUE)
    r.add_material(mk(albedo=(0.9, 0.5, 0.1, 0.9), albedo_mode="value", unlit=True, cutout=0.5), tc.CUTOUT)
    return r.meshes[m]


# ------------------------------------------------------------------ the expectation, traced per triangle
def frame_expectation(w, hdr, pyramid, prev):
    recs = records(w, op.NoMesh)
    hu = hdr.view(u32)
    shadow, flags, res = int(hu[32]) != tc.INVALID, int(hu[58]), (hdr[56], hdr[57])
    drawn, baked = op.oracle_inside(hdr, recs), op.oracle_baked(hdr, recs)
    ntri = np.where(w["enabled"], w["ntri"], 0)
    obj = np.repeat(np.arange(w["capacity"]), ntri)
    base = np.zeros(w["capacity"], dtype=i64)
    base[1:] = np.cumsum(ntri[:-1])
    ids = RUN[w["start"][obj] + (np.arange(len(obj)) - base[obj])]
    desc = None if shadow else tc.hiz_desc(int(res[0]), int(res[1]))
    tr = tc.trace(flags, shadow, res, baked[obj, 16:32], POSITIONS[ids], pyramid, desc)
    e = tc.expected_lists(ntri, tc.material_key(w["material"], tw.MATERIAL_KEYS), drawn, tr["visible"], shadow=shadow, prev=prev)
    e.update(trace=tr, ids=ids, baked=baked, shadow=shadow, flags=flags, start=w["start"], plan=tc.slot_plan(ntri[e["drawn"]]), header=hdr)
    return e


class Context(Product):
    """test_triangle_cull_gpu.Product on this file's mesh, records with the world's model matrices"""

    def __init__(self, r3, cfg, tune, monkeypatch):
        from rend3_amd import _ffi
        monkeypatch.setenv("R3N_FRAME_NODES", "0")
        monkeypatch.setenv("R3N_TUNE", tune)
        self.ffi, self.cfg = _ffi, cfg
        self.p = r3.Renderer(tw.handedness(cfg["hand"]), f32(1.0))
        self.mesh = setup_renderer(self.p, r3.material_record)
        if cfg["light"]:
            self.p.add_directional_light(**tw.LIGHT)
        self.inject = Inject(self.p)

    def write(self, w):
        self.p.write_object_records(np.arange(w["capacity"]), records(w, self.mesh), w["capacity"], {})


class Oracle:
    def __init__(self, cfg):
        from oracle.world import OracleRenderer, material_record
        self.cfg = cfg
        self.o = OracleRenderer(tw.handedness(cfg["hand"]), f32(1.0))
        self.mesh = setup_renderer(self.o, material_record, oracle_side=True)
        if cfg["light"]:
            self.o.add_directional_light(**tw.LIGHT)

    def frame(self, w, matrix, plane):
        o = self.o
        o.objects, o.capacity, o.object_meta = records(w, self.mesh), w["capacity"], {}
        o.set_camera_data(oh.identity(), ("raw", tw.MATRICES[matrix]))
        return o.render(64, 64, samples=self.cfg["samples"], exchange=oracle_hook(plane))


ORACLE_FRAMES = {}  # case -> the oracle's frames: computed once, shared by the two builds' runs, never changed


def oracle_frames(case):
    if case not in ORACLE_FRAMES:
        cfg = dict(CASES[case], extent=(64, 64))
        orc, w = Oracle(cfg), WORLDS[cfg["world"]]()
        ORACLE_FRAMES[case] = [orc.frame(w, m, tw.plane_of(cfg)) for m in cfg["frames"]]
    return ORACLE_FRAMES[case]


def sorted_regions(refs, counts):
    """a list's entries, each region's sorted: which entry of a sub-list a chunk's atomic reserved first is the launch's business"""
    out, at = [], 0
    for n in counts.reshape(-1).astype(i64):
        out.append(np.sort(tw.key64(refs[at:at + n])))
        at += n
    return np.concatenate(out) if out else np.zeros(0, dtype=u64)


def render_case(r3, monkeypatch, case, tune):
    """both frames of a case on a context created under `tune`, each checked against the reference and the oracle; returns what the
    two builds are compared on"""
    cfg = dict(CASES[case], extent=(64, 64))
    w = WORLDS[cfg["world"]]()
    P, prev, kept = Context(r3, cfg, tune, monkeypatch), {}, []
    try:
        P.write(w)
        for f, matrix in enumerate(cfg["frames"]):
            tag = f"{case} frame {f} ({matrix}) under {tune}"
            plane = tw.plane_of(cfg)
            P.render(matrix, plane)
            pyramid = P.p.readback_hiz(64, 64)
            if plane is not None:
                assert np.array_equal(pyramid.view(u32), tw.pyramid_of(plane).view(u32)), f"{tag}: the pyramid is not the injected plane's"
            views, out = [], dict(hiz=pyramid.view(u32).copy())
            for name, hdr, _sh in tw.view_headers(tw.MATRICES[matrix], tw.handedness(cfg["hand"]), (64, 64), cfg["samples"], w["capacity"], cfg["light"]):
                viewport = name == "viewport"
                e = prev[name] = frame_expectation(w, hdr, None if not viewport else pyramid, prev.get(name))
                cam = P.ffi.CAMERA_VIEWPORT if viewport else 0
                got = P.read_camera(cam, e["total"])
                check_sets(got, e, f"{tag} {name}", viewport)
                check_lists(P, cam, e, got, f"{tag} {name}", viewport)
                views.append((name, got))
                out[name] = dict(sets={k: got[k].copy() for k in ("pass", "residual", "visible")}, calls=got["draw_calls"].copy(),
                                 lists=[(sorted_regions(*P.p.readback_triangle_lists(cam, which)[:2]), P.p.readback_triangle_lists(cam, which)[1].copy())
                                        for which in ((0, 1) if viewport else (0,))])
            fo = oracle_frames(case)[f]
            assert np.array_equal(fo["hiz"].view(u32), pyramid.view(u32)), f"{tag}: pyramid != oracle"
            images = P.read_images(fo["atlas_size"])
            fp = dict(dict(views)["viewport"], capacity=w["capacity"], shadows=[g for n, g in views if n == "shadow"], **images)
            compare_frames(fo, fp, tag)
            out.update(atlas=images["atlas"].view(u32).copy(), vis=images["vis"].copy())
            kept.append(out)
    finally:
        P.close()
    return kept


@pytest.mark.parametrize("case", list(CASES))
def test_fast_and_plain_front_end_give_the_same_bits(r3, monkeypatch, case):
    fast, plain = (render_case(r3, monkeypatch, case, tune) for tune in TUNES)
    for f, (a, b) in enumerate(zip(fast, plain)):
        tag = f"{case} frame {f}: front_end_fast=1 against =0"
        for name in ("hiz", "atlas", "vis"):
            assert np.array_equal(a[name], b[name]), f"{tag}: {name} differs"
        for view in ("shadow", "viewport"):
            if view not in a:
                continue
            for k in ("pass", "residual", "visible"):
                assert np.array_equal(a[view]["sets"][k], b[view]["sets"][k]), f"{tag}: {view} {k} bits differ"
            assert np.array_equal(a[view]["calls"], b[view]["calls"]), f"{tag}: {view} draw calls differ"
            for which, ((ra, ca), (rb, cb)) in enumerate(zip(a[view]["lists"], b[view]["lists"])):
                assert np.array_equal(ca, cb), f"{tag}: {view} {tw.LIST_NAMES[which]} list: counts per region differ"
                assert np.array_equal(ra, rb), f"{tag}: {view} {tw.LIST_NAMES[which]} list: entries differ"


def test_the_worlds_hold_what_they_are_for():
    """(no GPU work: the shapes the cases rest on)"""
    plan = tc.slot_plan(WORLDS["counts"]()["ntri"])
    kinds = set(plan["kind"]) if "kind" in plan else None
    assert kinds is None or {tc.PAIR_FIRST, tc.PAIR_SECOND, tc.SINGLE} <= kinds
    assert CHUNK_BOUNDARY == 257
    for ids, bad in ((INF_IDS, np.isinf), (NAN_IDS, np.isnan)):
        assert all(bad(POSITIONS[i]).sum() == 1 for i in ids)
    hdr = tw.view_headers(tw.M_AFFINE, oh.LEFT, (64, 64), 1, 1, False)[0][1]
    mvp = np.eye(4, dtype=f32).reshape(-1)
    tr = tc.trace(int(hdr.view(u32)[58]) | tc.POSITIVE_AREA_VISIBLE, True, (f32(64), f32(64)), mvp, ESCAPE)
    assert (np.rint(tr["smin"]) != np.rint(tr["smax"])).all(), "the escapes leave the tie"
    assert tr["visible"][2:].all() and not tr["visible"][:2].any(), "and pass under their winding's flag"
    w = tc.trace(0, True, (f32(64), f32(64)), NOT_AFFINE, tw.TABLE.positions[:8])["clip"][:, :, 3]
    assert (w != f32(1.0)).all()
    nf = tc.trace(tc.POSITIVE_AREA_VISIBLE, True, (f32(64), f32(64)), mvp, NON_FINITE)
    assert np.isnan(nf["clip"][:, 2, 3]).all() and nf["visible"].all(), "w = NaN, and the cull passes it on to the rasteriser"
