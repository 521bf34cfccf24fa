"""The triangle cull (kernels_cull.h k_triangle_cull: the decision, the per-lane history, the pair path, the LDS-staged
compaction) on the GPU, bit for bit and entry by entry against tests/triangle_cull_reference.py on the worlds of
tests/triangle_cull_worlds.py -- no tolerance anywhere.  tests/test_triangle_cull.py holds, on the CPU, what this file rests on:
reference == oracle, every catalogue entry on its edge, every slot kind, ballot form, the sub-list wrap and the second loop trip.

Per run, view and frame: the pass and residual sets of r3n_readback_triangle_sets, and through r3n_readback_triangle_lists both
lists region by region -- per key exactly the reference's entries, none twice, none under another key, none in another sub-list
than its chunk's, no count above the reservation, 3 x the counts equal to the draw calls, the predicted list equal to the mask-
derived pass set -- the baked matrices of the drawn slots, and, for worlds small enough, the whole frame against the oracle (so the
next frame's first pass really consumed the list).  A failure names object, triangle, wave slot, slot kind, chunk and sub-list.

One-line mutants of kernels_cull.h (each changes a value, never an address or a bound), applied one at a time to a scratch
copy and this file run against each build.  All eight that ran failed the structure, wrap and sequence runs on both frame paths,
in check_sets; named below: the first thing that caught each.
  det <= 0 -> det < 0                  pass set, shadow view (it has the flag): det0_collinear passes
  det >= 0 -> det > 0                  pass set, viewport: det0_collinear / det0_repeated pass
  rintf -> floorf(x + 0.5f)            pass set: rint_x_k_odd(_positive) passes (3.5 and 4.5 round to 4 and 5, not 4 and 4)
  depth < occ -> depth <= occ          pass set: longest_above_2^0 .. and depth_equal (depth == occ) are rejected
  mip clamp mips - 1 -> mips - 2       pass set: longest_2^5 / longest_above_2^5, longest_64, longest_128_clamped
  hiz_sample_min -> first texel only   pass set: min_in_texel_1 .. 3 are rejected
  drop `&& triB < ntri`                residual set (a clamped lane's entry lands in the next object's triangles), vertex counts;
                                       run with every world's partly filled slots followed by real triangles of the run, so the
                                       extra entries still name fetchable triangles
  finish(.., wrel + 1, ..) -> wrel     residual set and lists: the pair's second slot repeats the first slot's triangles
NOT run on the GPU, because the lists are uninitialised memory behind what the cull writes and the same frame's rasteriser
draws whatever an entry inside the count names -- an unwritten entry there could fault:
  lane_lt | (1ull << lane)             leaves a chunk's first entry unwritten and shifts the rest by one
  run_r[k] += .. nr -> np              leaves holes inside the residual count
  region's chunk % R3N_SUBQ -> 0       writes every chunk into sub-list 0's region while the other regions' counts grow
What each leaves behind -- a duplicate, a never-written or stale entry inside the count, an entry in another sub-list's region, a
missing entry -- is instead made on the CPU and fed to the same check_list: tests/test_triangle_cull.py
test_the_list_checker_rejects_every_corruption.
  key > 2 ? 2 : key -> key             not applied: a key byte above 2 would index a fourth region (it moves an address), and no
                                       public call produces one (r3n_materials_write refuses keys above R3N_KEY_BLEND)"""
import ctypes

import numpy as np
import pytest

import triangle_cull_reference as tc
import triangle_cull_worlds as tw
from oracle import host as oh
from test_gpu_parity import compare_frames
from test_hiz_gpu import Inject

pytestmark = pytest.mark.gpu
f32, u32, u64 = np.float32, np.uint32, np.uint64
FRAME_PATHS = pytest.mark.parametrize("frame_nodes", [False, True], ids=["one_call_frame", "per_node_frame"])


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


class Product:
    """A product context whose object buffer is written in bulk from a world of tests/triangle_cull_worlds.py
    (Renderer.write_object_records: the host mirror then knows only the blend objects, which the transparent pass sorts)."""

    def __init__(self, r3, cfg, frame_nodes, monkeypatch):
        from rend3_amd import _ffi
        monkeypatch.setenv("R3N_FRAME_NODES", "1" if frame_nodes else "0")
        self.ffi, self.cfg = _ffi, cfg
        W, H = cfg["extent"]
        self.p = r3.Renderer(tw.handedness(cfg["hand"]), f32(W) / f32(H))
        assert self.p.frame_nodes == frame_nodes
        self.mesh = tw.setup_renderer(self.p, r3.material_record)
        if cfg["light"]:
            self.p.add_directional_light(**tw.LIGHT)
        self.recs = np.zeros((0, 32), dtype=u32)
        self.inject = Inject(self.p)

    def write(self, world):
        """the slots whose record changed since the last write, and the new ones"""
        recs, old = tw.records(world, self.mesh), len(self.recs)
        changed = np.ones(len(recs), dtype=bool)
        changed[:old] = (recs[:old] != self.recs).any(axis=1)
        slots = np.flatnonzero(changed)
        blend = np.flatnonzero((world["material"] == tc.BLEND) & world["enabled"])
        self.p.write_object_records(slots, recs[slots], world["capacity"], {int(h): (tc.BLEND, world["spheres"][h, :3]) for h in blend})
        self.recs = recs

    def render(self, matrix_name, plane):
        cfg = self.cfg
        self.p.set_camera_data(oh.identity(), ("raw", tw.MATRICES[matrix_name]))
        self.inject.plane = plane
        calls = self.inject.calls
        self.p.render(*cfg["extent"], samples=cfg["samples"], readback=False, exchange=self.inject)
        assert self.inject.calls == calls + (plane is not None)

    def read_camera(self, cam, total):
        p, ffi, lib = self.p, self.ffi, self.p.lib
        cap, n = p.capacity, total + 128  # (room behind the last object: an entry that names a triangle beyond it is reported, not written past the array)
        visible, ps, rs = np.zeros(cap, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        p._check(lib.r3n_readback_visible_objects(p.ctx, cam, ffi.ptr(visible), cap), "readback_visible_objects")
        p._check(lib.r3n_readback_triangle_sets(p.ctx, cam, ffi.ptr(ps), ffi.ptr(rs), n), "readback_triangle_sets")
        calls = np.zeros((6, 5), dtype=u32)
        p._check(lib.r3n_readback_draw_calls(p.ctx, cam, ffi.ptr(calls)), "readback_draw_calls")
        baked = np.zeros((cap, 32), dtype=f32)
        p._check(lib.r3n_readback_baked(p.ctx, cam, ffi.ptr(baked), cap), "readback_baked")
        return dict(visible=visible, residual=rs, draw_calls=calls, baked=baked, **{"pass": ps})

    def read_images(self, atlas_size):
        p, ffi, lib = self.p, self.ffi, self.p.lib
        W, H = self.cfg["extent"]
        s = self.cfg["samples"]
        vis = np.zeros((H, W) if s == 1 else (H, W, s), dtype=u64)
        p._check(lib.r3n_readback_visibility(p.ctx, ffi.ptr(vis)), "readback_visibility")
        atlas = np.zeros((atlas_size[1], atlas_size[0]), dtype=f32)
        p._check(lib.r3n_readback_shadow_atlas(p.ctx, ffi.ptr(atlas)), "readback_shadow_atlas")
        hdr16 = np.zeros((H, W, 4), dtype=np.uint16)
        p._check(lib.r3n_readback_hdr(p.ctx, ffi.ptr(hdr16)), "readback_hdr")
        rgba8, rgba_f = np.zeros((H, W, 4), dtype=np.uint8), np.zeros((H, W, 4), dtype=f32)
        p._check(lib.r3n_readback_output(p.ctx, ffi.ptr(rgba8), ffi.ptr(rgba_f)), "readback_output")
        return dict(vis=vis, atlas=atlas, hdr16=hdr16, rgba8=rgba8, rgba_f32=rgba_f)

    def close(self):
        self.p.close()


where = tw.where


def check_sets(got, e, tag, viewport):
    d = np.flatnonzero(got["visible"].astype(bool) != e["drawn"])
    assert len(d) == 0, f"{tag}: drawn objects differ, first slot {int(d[0])}"
    n = e["total"]
    for name in ("pass", "residual") if viewport else ("pass",):
        d = np.flatnonzero(got[name][:n] != e[name])
        assert len(d) == 0, (f"{tag}: {name} set differs in {len(d)} triangles (expected {int(e[name][d[0]])}), first "
                             f"{where(e, e['object'][d[0]], e['triangle'][d[0]])}")
    want = e["calls"] if viewport else np.concatenate([e["calls"][:3], np.zeros(3, dtype=np.int64)])
    assert np.array_equal(got["draw_calls"][:, 0], want), f"{tag}: vertex counts {got['draw_calls'][:, 0]} != {want}"
    rows = np.flatnonzero(e["drawn"])
    bad = (got["baked"].view(u32)[rows] != e["baked"].view(u32)[rows]).any(axis=1)
    assert not bad.any(), f"{tag}: baked matrices differ at slot {int(rows[bad][0])}"


def check_lists(P, cam, e, got, tag, viewport):
    """both lists of a camera (a shadow view keeps no residual list), region by region: triangle_cull_worlds.check_list"""
    for which in (0, 1) if viewport else (0,):
        refs, counts, subcap = P.p.readback_triangle_lists(cam, which)
        tw.check_list(e, which, refs, counts, subcap, P.p.capacity, got["draw_calls"][3 * which:3 * which + 3, 0], got["pass"], tag)


def run_frames(r3, monkeypatch, run, frame_nodes):
    cfg, frames = tw.run_frames(run)
    P, ex = Product(r3, cfg, frame_nodes, monkeypatch), tw.Expect(cfg)
    with_oracle = max(w["capacity"] for w, _m in frames) <= tw.ORACLE_FRAME_MAX
    orc = tw.OracleRun(cfg) if with_oracle else None
    W, H = cfg["extent"]
    try:
        for f, (world, matrix) in enumerate(frames):
            tag = f"{run} frame {f} ({matrix}, {'per-node' if frame_nodes else 'one-call'} frame)"
            plane = tw.plane_of(cfg)
            P.write(world)
            P.render(matrix, plane)
            pyramid = P.p.readback_hiz(W, H)
            if plane is not None:
                assert np.array_equal(pyramid.view(u32), tw.pyramid_of(plane).view(u32)), f"{tag}: the pyramid is not the injected plane's"
            es = ex.frame(world, matrix, pyramid)
            views = []
            for name, e in es.items():
                viewport = name == "viewport"
                cam = P.ffi.CAMERA_VIEWPORT if viewport else 0
                got = P.read_camera(cam, e["total"])
                check_sets(got, e, f"{tag} {name}", viewport)
                check_lists(P, cam, e, got, f"{tag} {name}", viewport)
                views.append((name, got))
            if orc is not None:  # the whole frame: the first pass drew last frame's predicted list, the second this frame's residual one
                fo = orc.frame(world, matrix, plane)
                assert np.array_equal(fo["hiz"].view(u32), pyramid.view(u32)), f"{tag}: pyramid != oracle"
                fp = dict(dict(views)["viewport"], capacity=world["capacity"], shadows=[g for n, g in views if n == "shadow"],
                          **P.read_images(fo["atlas_size"]))
                compare_frames(fo, fp, tag)
    finally:
        P.close()


@pytest.mark.parametrize("run", list(tw.RUNS))
def test_sets_and_lists_of_every_world(r3, monkeypatch, run):
    """the structure worlds under every view (both handednesses, one and four samples, the three targets, w = 1 and w = mesh z,
    the shadow view), the sub-list wrap and the second loop trip: two frames each (the second with history), one for the 65 700
    objects; on the one-call frame"""
    run_frames(r3, monkeypatch, run, frame_nodes=False)


@FRAME_PATHS
def test_sequence_with_history(r3, monkeypatch, frame_nodes):
    """six frames in one context: the camera alternates, slots are disabled and re-enabled, the world grows past its capacity, a
    slot is rewritten with another triangle count, a slot leaves the frustum for a frame; on both frame paths"""
    run_frames(r3, monkeypatch, "sequence", frame_nodes)


def test_per_node_frame_structure_world(r3, monkeypatch):
    run_frames(r3, monkeypatch, "structure-64x64-left", frame_nodes=True)


def test_refusals_of_the_list_readback(r3, monkeypatch):
    cfg, frames = tw.run_frames("structure-64x64-left")
    P = Product(r3, cfg, False, monkeypatch)
    p, lib, ffi = P.p, P.p.lib, P.ffi
    counts, subcap, out = np.zeros((3, 32), dtype=u32), ctypes.c_uint32(), np.zeros((16, 2), dtype=u32)

    def call(cam, which, buf, capacity):
        return lib.r3n_readback_triangle_lists(p.ctx, cam, which, ffi.ptr(buf) if buf is not None else None, capacity, ffi.ptr(counts), ctypes.byref(subcap))
    try:
        assert call(ffi.CAMERA_VIEWPORT, 0, out, 16) == -4 and b"never culled" in lib.r3n_last_error(p.ctx)  # R3N_ERR_STATE
        P.write(frames[0][0])
        P.render("affine", tw.plane_of(cfg))
        assert call(5, 0, out, 16) == -4, "a shadow view that does not exist"
        assert call(0, 1, out, 16) == -1 and b"no residual list" in lib.r3n_last_error(p.ctx)  # R3N_ERR_INVALID_ARG
        assert call(ffi.CAMERA_VIEWPORT, 2, out, 16) == -1
        assert call(ffi.CAMERA_VIEWPORT, 0, None, 0) == 0 and counts.sum() > 16, "out == NULL: the counts alone"
        total = int(counts.sum())
        out[:] = 0xABCDEF01
        assert call(ffi.CAMERA_VIEWPORT, 0, out, 16) == -1 and b"too small" in lib.r3n_last_error(p.ctx)
        assert (out == 0xABCDEF01).all(), "a short buffer is left alone"
        big = np.zeros((total + 1, 2), dtype=u32)
        big[:] = 0xABCDEF01
        assert call(ffi.CAMERA_VIEWPORT, 0, big, total) == 0 and (big[total] == 0xABCDEF01).all() and (big[:total] != 0xABCDEF01).all()
        assert lib.r3n_readback_triangle_lists(p.ctx, ffi.CAMERA_VIEWPORT, 0, ffi.ptr(big), total, None, ctypes.byref(subcap)) == -1
    finally:
        P.close()
