"""The object pass (frustum test, visible-object scan, work-list scatter, first-entry table, uniform bake) on every launch plan
the host can pick for it -- k_object_pass_fused, k_object_count -> k_object_scan -> k_object_scatter, k_object_pass_chained --
at every capacity where a plan or one of its parameters changes, on both frame paths, bit for bit against
tests/object_pass_reference.py and, for the worlds small enough, against whole oracle frames.

The worlds are record arrays written with one r3n_objects_write (any capacity, spheres decoupled from the geometry); what a
camera's pass left is read through r3n_readback_visible_objects / _triangle_sets / _draw_calls / _baked.  A missing or misplaced
work-list entry, a wrong wave start or first-entry word shows as pass bits that differ (>= 90 % of the triangles pass the
triangle cull; tests/test_object_pass.py holds that and the other conditions this file rests on)."""
import numpy as np
import pytest

import object_pass_reference as op
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
T = op.TARGET


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


class Product:
    """A product context whose object buffer is written in bulk.  The host mirror's per-object bookkeeping stays empty (blend
    objects excepted: the transparent pass sorts them), its capacity follows the world's -- any number, not a power of two."""

    def __init__(self, r3, frame_nodes, monkeypatch):
        from rend3_amd import _ffi
        monkeypatch.setenv("R3N_FRAME_NODES", "1" if frame_nodes else "0")

        class Bulk(r3.Renderer):
            def _write_objects(self, items, force_capacity=False):
                if items:  # (the mirror's first, empty write would pin the capacity at 16)
                    raise AssertionError("the worlds of this file are written by Product.write")
        self.ffi = _ffi
        self.p = Bulk(oh.LEFT, f32(1.0))
        assert self.p.frame_nodes == frame_nodes
        self.meshes = op.setup_renderer(self.p, r3.material_record)
        self.recs = np.zeros((0, 32), dtype=u32)

    def write(self, world):
        """the slots the world has grown by since the last write (all of them the first time), the new capacity"""
        p, ffi = self.p, self.ffi
        first, cap = len(self.recs), world["capacity"]
        new = op.records(world, *self.meshes, first=first)
        slots = np.arange(first, cap, dtype=u32)
        p._check(p.lib.r3n_objects_write(p.ctx, ffi.ptr(slots), ffi.ptr(new), len(slots), cap), "r3n_objects_write")
        p.capacity = p._capacity_sent = cap
        self.recs = np.concatenate([self.recs, new])
        blend = np.flatnonzero((world["material"] == op.BLEND) & world["enabled"])
        p.object_meta = {int(h): dict(enabled=True, material=op.BLEND, location=world["spheres"][h, :3].copy()) for h in blend}
        p._blend_cache = None
        p.world_version += 1
        self.meta = op.meta_words(self.recs, op.MATERIAL_KEYS)

    def render(self, view, proj):
        self.p.set_camera_data(view, proj)
        self.p.render(T, T, readback=False)

    def read_camera(self, cam, want_baked=True):
        p, ffi, lib = self.p, self.ffi, self.p.lib
        cap, total = p.capacity, max(int((self.meta & op.META_NTRI_MASK).sum()), 1)
        visible, ps, rs = np.zeros(cap, dtype=np.uint8), np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        p._check(lib.r3n_readback_visible_objects(p.ctx, cam, ffi.ptr(visible), cap), "readback_visible_objects")
        p._check(lib.r3n_readback_triangle_sets(p.ctx, cam, ffi.ptr(ps), ffi.ptr(rs), total), "readback_triangle_sets")
        calls = np.zeros((6, 5), dtype=u32)
        p._check(lib.r3n_readback_draw_calls(p.ctx, cam, ffi.ptr(calls)), "readback_draw_calls")
        baked = None
        if want_baked:
            baked = np.zeros((cap, 32), dtype=f32)
            p._check(lib.r3n_readback_baked(p.ctx, cam, ffi.ptr(baked), cap), "readback_baked")
        return dict(visible=visible, residual=rs, draw_calls=calls, baked=baked, **{"pass": ps})

    def read_images(self, atlas_size):
        p, ffi, lib = self.p, self.ffi, self.p.lib
        vis = np.zeros((T, T), dtype=np.uint64)
        p._check(lib.r3n_readback_visibility(p.ctx, ffi.ptr(vis)), "readback_visibility")
        atlas = np.zeros((atlas_size[1], atlas_size[0]), dtype=f32)
        p._check(lib.r3n_readback_shadow_atlas(p.ctx, ffi.ptr(atlas)), "readback_shadow_atlas")
        hdr16 = np.zeros((T, T, 4), dtype=np.uint16)
        p._check(lib.r3n_readback_hdr(p.ctx, ffi.ptr(hdr16)), "readback_hdr")
        rgba8, rgba_f = np.zeros((T, T, 4), dtype=np.uint8), np.zeros((T, T, 4), dtype=f32)
        p._check(lib.r3n_readback_output(p.ctx, ffi.ptr(rgba8), ffi.ptr(rgba_f)), "readback_output")
        return dict(vis=vis, atlas=atlas, hdr16=hdr16, rgba8=rgba8, rgba_f32=rgba_f)

    def close(self):
        self.p.close()


def where(i, plan):
    """a slot number in the terms of the plan that handled it"""
    s = f"slot {i}: 256-slot block {i // 256}, wave {i // 64 % 4}, lane {i % 64}"
    if plan["plan"] == "chained":
        per = plan["rounds"] * 256
        s += f"; chained block {i // per} of {plan['grid']}, round {i % per // 256} of {plan['rounds']}"
    elif plan["plan"] == "three_launch":
        s += f"; scan iteration {i // 256 // 1024} of {plan['scan_iterations']} ({plan['scan_width']} threads)"
    return s


def first_diff(a, b):
    d = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return None if len(d) == 0 else (int(d[0]), len(d))


def check_camera(got, e, baked_ref, plan, tag, viewport=True):
    """the comparisons of every frame: flags over the whole capacity, both triangle sets over every canonical triangle, the six
    calls, the baked matrices as u32 words over exactly the slots where they are defined"""
    d = first_diff(got["visible"], e["flags"] & op.VIS_DRAWN)
    assert d is None, f"{tag}: drawn bits differ in {d[1]} slots, first {where(d[0], plan)}"
    for name in ("pass", "residual") if viewport else ("pass",):
        d = first_diff(got[name][: e["total"]], e[name])
        if d is not None:
            slot = int(np.searchsorted(e["tri_base"], d[0], side="right") - 1)
            raise AssertionError(f"{tag}: {name} set differs in {d[1]} triangles, first {d[0]} = triangle {d[0] - int(e['tri_base'][slot])} "
                                 f"of {int(e['ntri'][slot])} of {where(slot, plan)}")
    want_calls = e["calls"] if viewport else np.concatenate([e["calls"][:3], np.zeros(3, dtype=np.int64)])
    assert np.array_equal(got["draw_calls"][:, 0], want_calls), f"{tag}: calls {got['draw_calls'][:, 0]} != {want_calls}"
    assert (got["draw_calls"][:, 1] == 1).all() and not got["draw_calls"][:, 3:].any(), tag
    if baked_ref is not None and e["baked"].any():
        rows = np.flatnonzero(e["baked"])
        bad = (got["baked"].view(u32)[rows] != baked_ref.view(u32)[rows]).any(axis=1)
        assert not bad.any(), f"{tag}: baked matrices differ in {int(bad.sum())} of {len(rows)} defined slots, first {where(int(rows[bad][0]), plan)}"


class Run:
    """One context and, for worlds up to ORACLE_FRAME_MAX slots, one oracle beside it; frames with the cameras of the world's
    tier in turn, history kept from frame to frame."""

    def __init__(self, r3, frame_nodes, monkeypatch, tier, light=False):
        self.P = Product(r3, frame_nodes, monkeypatch)
        self.one_call, self.tier, self.light = not frame_nodes, tier, light
        self.prev, self.frame_no, self.o = None, 0, None
        if light:
            self.P.p.add_directional_light(**op.LIGHT[tier])

    def load(self, world, with_oracle):
        assert world["tier"] == self.tier
        self.world = world
        self.P.write(world)
        if with_oracle:
            assert world["capacity"] <= op.ORACLE_FRAME_MAX
            if self.o is None:
                self.o = OracleRenderer(oh.LEFT, f32(1.0))
                self.o_meshes = op.setup_renderer(self.o, omk)
                if self.light:
                    self.o.add_directional_light(**op.LIGHT[self.tier])
            op.load_oracle(self.o, world, self.o_meshes)

    def own(self, begin_end=None, owners=None, rank=0):
        cap = self.world["capacity"]
        if owners is not None:
            self.P.p.set_object_owners(owners, rank)
            self.owned = np.asarray(owners) == rank
            if self.o is not None:
                self.o.object_owners = (owners, rank)
        else:
            self.P.p.set_object_range(*begin_end)
            self.owned = (np.arange(cap) >= begin_end[0]) & (np.arange(cap) < begin_end[1])
            if self.o is not None:
                self.o.object_range = begin_end

    def flags(self, hdr, exact):
        P, cap = self.P, self.world["capacity"]
        owned = getattr(self, "owned", np.ones(cap, dtype=bool))
        owned = np.concatenate([owned, np.ones(cap - len(owned), dtype=bool)])
        if exact:
            return op.flags_exact(hdr[36:56], P.recs.view(f32)[:, 16:20], P.meta, owned)
        return op.flags_from_inside(op.oracle_inside(hdr, P.recs), P.meta, owned)

    def frame(self, tag):
        P, world, tier = self.P, self.world, self.tier
        cap, c = world["capacity"], self.frame_no % 2
        plan = op.launch_plan(cap, self.one_call)
        tag = f"{tag} frame {self.frame_no} (camera {c}) {plan}"
        view, proj = op.cameras(tier, oh)[c]
        P.p.stage_times(reset=True)
        P.render(view, proj)
        # the plan the host really took: the chained pass bakes inside its one launch, every other plan is preceded by a
        # k_uniform_bake of its own ("bake" stage scope), one per camera
        cameras = 2 if self.light else 1
        assert P.p.stage_times()["bake"][1] == (0 if plan["plan"] == "chained" else cameras), f"{tag}: the host took another plan"
        hdr = op.oracle_header(view, proj, cap)
        if tier == "exact":
            assert np.array_equal(hdr[36:56].view(u32), op.EXACT_PLANES[c].view(u32))
        e = op.expected(P.meta, self.flags(hdr, tier == "exact"), op.verdicts(tier)[c][world["pal"]], self.prev)
        if self.frame_no == 0:
            assert np.array_equal(e["residual"], e["pass"])
        got = P.read_camera(P.ffi.CAMERA_VIEWPORT, want_baked=bool(e["baked"].any()))
        check_camera(got, e, op.oracle_baked(hdr, P.recs) if e["baked"].any() else None, plan, tag)
        shadow_got = []
        if self.light:
            user = oh.CameraState(view, proj, oh.LEFT, f32(1.0))
            size, shadows, _buf = oh.evaluate_directional_lights([op.LIGHT[tier]], user)
            sh = shadows[0]
            shdr = op.oracle_header(None, None, cap, camera=sh["camera"], shadow_index=0, size=sh["size"])
            se = op.expected(P.meta, self.flags(shdr, False), op.verdicts(tier, light=True)[c][world["pal"]])
            sg = P.read_camera(0)
            check_camera(sg, se, op.oracle_baked(shdr, P.recs), op.launch_plan(cap, self.one_call), tag + " shadow view", viewport=False)
            shadow_got.append(sg)
            self.shadow_expected = se
        if self.o is not None:  # the whole frame: Hi-Z, keys, image
            self.o.set_camera_data(view, proj)
            fo = self.o.render(T, T)
            fp = dict(got, capacity=cap, shadows=shadow_got, **P.read_images(fo["atlas_size"]))
            if fp["baked"] is None:
                fp["baked"] = fo["baked"]
            compare_frames(fo, fp, tag)
            assert np.array_equal(fo["pass"], e["pass"]) and np.array_equal(fo["residual"], e["residual"]), tag + ": reference != oracle"
        self.prev, self.frame_no = e, self.frame_no + 1
        return e

    def close(self):
        self.P.close()


def worlds_of(capacity):
    """(pattern, tier, compared against whole oracle frames) of the worlds a capacity is run with.  Up to ORACLE_FRAME_MAX slots:
    "mix" (drawn / culled waves and blocks around stretches left to the tier) and "tier" on both tiers beside whole oracle
    frames, the four extreme patterns on one tier each.  Above: "mix" on both tiers and the three patterns that cost no triangles."""
    if capacity <= op.ORACLE_FRAME_MAX:
        return ([(p, t, True) for t in op.TIERS for p in ("mix", "tier")] +
                [("all", "exact", False), ("none", "random", False), ("first", "exact", False), ("last", "random", False)])
    return [("mix", "exact", False), ("mix", "random", False), ("none", "exact", False), ("first", "random", False), ("last", "exact", False)]


def run_capacity(r3, monkeypatch, capacity, frame_nodes):
    plan = op.launch_plan(capacity, not frame_nodes)
    for pattern, tier, with_oracle in worlds_of(capacity):
        run = Run(r3, frame_nodes, monkeypatch, tier)
        try:
            run.load(op.build_world(capacity, tier, pattern, big_ntri_every=op.big_ntri_every(capacity)), with_oracle)
            e0 = run.frame(f"{capacity} slots {pattern} {tier}")
            e1 = run.frame(f"{capacity} slots {pattern} {tier}")
            n_drawn = int(((e0["flags"] & op.VIS_DRAWN) != 0).sum())
            assert n_drawn == {"all": capacity, "none": 0, "first": 1, "last": 1}.get(pattern, n_drawn)
            if pattern in ("mix", "tier") and capacity >= 1024:
                assert ((e1["flags"] ^ e0["flags"]) & op.VIS_INSIDE).any(), "frame 1's use_prev set differs from its own inside set"
        finally:
            run.close()
    return plan


# ------------------------------------------------------------------ (a) every plan, both frame paths
EXPECTED_PLAN = {  # (capacity, one-call frame) -> the plan's name and the parameter that makes the capacity an edge
    **{(c, False): ("fused", None) for c in op.NODE_CAPACITIES if c <= 1024},
    (1025, False): ("three_launch", (64, 1)), (16_384, False): ("three_launch", (64, 1)), (16_385, False): ("three_launch", (1024, 1)),
    (262_144, False): ("three_launch", (1024, 1)), (262_145, False): ("three_launch", (1024, 2)),
    **{(c, True): ("chained", (1, (c + 255) // 256)) for c in op.ONE_CALL_CAPACITIES if c <= 131_072},
    (131_073, True): ("chained", (2, 257)), (262_145, True): ("chained", (3, 342)), (524_289, True): ("chained", (5, 410)),
    (1_966_081, True): ("chained", (16, 481)), (2_097_152, True): ("chained", (16, 512)), (2_097_153, True): ("three_launch", (1024, 9)),
    (131_073, False): ("three_launch", (1024, 1)), (2_097_153, False): ("three_launch", (1024, 9)), (16_385, True): ("chained", (1, 65)),
}


def assert_plan(capacity, one_call):
    plan = op.launch_plan(capacity, one_call)
    name, params = EXPECTED_PLAN[(capacity, one_call)]
    assert plan["plan"] == name
    if name == "three_launch":
        assert (plan["scan_width"], plan["scan_iterations"]) == params
    elif name == "chained":
        assert (plan["rounds"], plan["grid"]) == params


@pytest.mark.parametrize("capacity", op.NODE_CAPACITIES)
def test_per_node_frame_at_every_plan_edge(r3, monkeypatch, capacity):
    """r3n_cull -> run_object_pass: fused up to 1 024 slots (partial wave, partial block), three launches above (the
    one-wavefront scan up to 64 blocks, the 1 024-thread scan above, its carry past 1 024 blocks).  Two frames per world."""
    assert_plan(capacity, False)
    run_capacity(r3, monkeypatch, capacity, frame_nodes=True)


@pytest.mark.parametrize("capacity", op.ONE_CALL_CAPACITIES)
def test_one_call_frame_at_every_plan_edge(r3, monkeypatch, capacity):
    """r3n_render_frame -> k_object_pass_chained<true>: rounds 1, 2, 3, 5, 16, a grid of exactly 512 blocks at rounds 1 and 16,
    the use_prev bake set in frame 1 -- and the in-frame fallback to three launches at 2 097 153 slots."""
    assert_plan(capacity, True)
    run_capacity(r3, monkeypatch, capacity, frame_nodes=False)


# ------------------------------------------------------------------ (b) growth through the boundaries in one context
@pytest.mark.parametrize("tier", op.TIERS)
@pytest.mark.parametrize("frame_nodes", [True, False], ids=["per_node_frame", "one_call_frame"])
def test_one_context_grows_through_every_plan_boundary(r3, monkeypatch, frame_nodes, tier):
    """The ascending capacity list in ONE context with the frame history alive: grow, write the new tail, render.  The chain
    records of the smaller grid stay behind (stale epochs), vis_flags is regrown zero-filled with last frame's bytes kept (the
    use_prev set of the old slots), last frame's slot bases and result bits are read for the old slots only."""
    caps = op.NODE_CAPACITIES if frame_nodes else op.ONE_CALL_CAPACITIES
    run = Run(r3, frame_nodes, monkeypatch, tier)
    try:
        world = None
        for cap in caps:
            world = op.build_world(cap, tier, "mix", big_ntri_every=4096) if world is None else op.grow_world(world, cap, seed=cap)
            run.load(world, False)
            e = run.frame(f"grown to {cap} slots, {tier}")
            if run.frame_no > 1 and cap > 1024:
                assert e["residual"].sum() < e["pass"].sum(), "history: the old slots' passing triangles are not all residual"
    finally:
        run.close()


FRESH = [(c, nodes) for c in op.BOUNDARY_CAPACITIES for nodes in (True, False)
         if c not in (op.NODE_CAPACITIES if nodes else op.ONE_CALL_CAPACITIES)]


@pytest.mark.parametrize("capacity,frame_nodes", FRESH, ids=[f"{c}-{'per_node' if n else 'one_call'}" for c, n in FRESH])
def test_fresh_context_at_a_plan_boundary_of_the_other_path(r3, monkeypatch, capacity, frame_nodes):
    """Every plan-boundary capacity in a fresh context on BOTH paths: the ones a path's own list above does not hold."""
    assert sorted(FRESH) == [(16_385, False), (131_073, True), (2_097_153, True)]
    assert_plan(capacity, not frame_nodes)
    run_capacity(r3, monkeypatch, capacity, frame_nodes)


# ------------------------------------------------------------------ (c) ownership
@pytest.mark.parametrize("mode", ["range", "owners"])
@pytest.mark.parametrize("frame_nodes", [True, False], ids=["per_node_frame", "one_call_frame"])
@pytest.mark.parametrize("capacity", [1025, 131_073])
def test_drawn_bits_follow_ownership_and_inside_bits_do_not(r3, monkeypatch, capacity, frame_nodes, mode):
    """A slot range that cuts a wave in half at both ends / three ranks interleaved slot by slot, with one directional light so
    that a second camera runs its own pass.  The drawn bits (lists, sets, calls) are the owned slots'; the bake set is every
    inside slot's, of whatever rank.  At 1 025 slots the world has blend-key objects -- drawn on every rank -- and the whole frame
    is the oracle's under the same ownership."""
    tier = "exact" if mode == "range" else "random"
    small = capacity <= op.ORACLE_FRAME_MAX
    run = Run(r3, frame_nodes, monkeypatch, tier, light=True)
    try:
        world = op.build_world(capacity, tier, "tier", blend=small, big_ntri_every=op.big_ntri_every(capacity))
        run.load(world, small)
        if mode == "range":
            run.own(begin_end=(96, capacity // 128 * 64 + 32))  # both ends in the middle of a wave
        else:
            run.own(owners=(np.arange(capacity) % 3).astype(np.uint8), rank=1)
        for _f in range(2):
            e = run.frame(f"{capacity} slots, {mode}")
            inside, drawn = (e["flags"] & op.VIS_INSIDE) != 0, (e["flags"] & op.VIS_DRAWN) != 0
            blend = (run.P.meta >> 30) == op.BLEND
            assert np.array_equal(drawn, inside & (run.owned | blend)) and np.array_equal(e["baked"][inside], np.ones(inside.sum(), dtype=bool))
            assert (inside & ~drawn).sum() > 0.2 * inside.sum(), "slots of other ranks whose matrices are baked all the same"
            if small:
                assert (drawn & blend & ~run.owned).any(), "blend objects of other ranks' slots are drawn here"
            se = run.shadow_expected
            assert ((se["flags"] & op.VIS_INSIDE) != 0).sum() > ((se["flags"] & op.VIS_DRAWN) != 0).sum() > 0
    finally:
        run.close()
