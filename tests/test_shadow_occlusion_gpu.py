"""GPU: the shadow views' two-phase depth draw (kernels_raster.h: k_raster_small<OCC>, k_shadow_tile_min, k_shadow_deferred;
r3n.hip shadow_occlusion_begin / _finish) changes no bit.

Every frame of every case is rendered three ways -- the default context, one created under R3N_TUNE="shadow_occlusion=0" and the
oracle -- and compared whole (test_gpu_parity.compare_frames: the views' visible / pass sets, the atlas bit for bit, the keys, the
image); the two product atlases are also compared with each other.  r3n_shadow_occlusion_stats says what the two phases did, so
that a case cannot pass because nothing was deferred.

The worlds are drawn in the window space of a light with direction (0, 0, 1) and distance 2 (shadow_occlusion_reference.py):
views of 128^2 (and 256^2, 64^2, 32^2), a few hundred triangles.  Moving the camera by k / 64 moves a 128^2 view by k texels.
"""
import numpy as np
import pytest

import shadow_occlusion_reference as so
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32 = np.float32
W = H = 32
IDENT = oh.identity()
LIGHT = dict(color=(1, 1, 1), intensity=1.0, direction=(0.0, 0.0, 1.0), distance=2.0)
NEAR, FAR = 0.75, 0.25  # depth of the occluders / of what they hide (1 is nearest the light)


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def add(r, mk, tris_px, size=128, n=0):
    pos = so.to_world(tris_px, size).reshape(-1, 3)
    normals = np.zeros_like(pos)
    normals[:, 2] = -1.0
    mat = r.add_material(mk(albedo=(0.25 + 0.25 * (n % 3), 0.5, 0.75, 1.0), albedo_mode="value", unlit=True), 0)
    return r.add_object(r.add_mesh(pos, normals=normals), mat, IDENT)


def camera(r, tx=0, ty=0):
    """camera location (tx, ty) / 64: a 128^2 view moves by whole texels"""
    r.set_camera_data(oh.translation((-tx / 64.0, -ty / 64.0, 0.0)), ("raw", IDENT))


class Trio:
    """the same world on the default context, on one with the two-phase draw off, and on the oracle"""

    def __init__(self, r3, monkeypatch, resolutions=(128,)):
        import os
        monkeypatch.setenv("R3N_FRAME_NODES", "0")
        base = os.environ.get("R3N_TUNE", "")
        self.on = r3.Renderer(oh.LEFT, f32(1.0))
        monkeypatch.setenv("R3N_TUNE", (base + " shadow_occlusion=0").strip())
        self.off = r3.Renderer(oh.LEFT, f32(1.0))
        monkeypatch.setenv("R3N_TUNE", base) if base else monkeypatch.delenv("R3N_TUNE")
        self.o = OracleRenderer(oh.LEFT, f32(1.0))
        self.all = ((self.on, r3.material_record), (self.off, r3.material_record), (self.o, omk))
        self.views = len(resolutions)
        self.lights = [[r.add_directional_light(resolution=res, **LIGHT) for res in resolutions] for r, _ in self.all]
        for r, _ in self.all:
            camera(r)
        self.n = 0

    def add(self, tris_px, size=128):
        self.n += 1
        return [add(r, mk, tris_px, size, self.n) for r, mk in self.all]

    def each(self, fn, handles=None):
        for k, (r, _) in enumerate(self.all):
            fn(r) if handles is None else fn(r, handles[k])

    def frame(self, tag):
        fo, fa, fb = self.o.render(W, H), self.on.render(W, H), self.off.render(W, H)
        compare_frames(fo, fa, tag + " (two phases)")
        compare_frames(fo, fb, tag + " (one phase)")
        assert np.array_equal(fa["atlas"].view(np.uint32), fb["atlas"].view(np.uint32)), tag
        assert fo["atlas"].any(), tag + ": empty atlas"
        for v in range(self.views):
            assert self.off.shadow_occlusion_stats(v)["active"] == 0, tag
        stats = [self.on.shadow_occlusion_stats(v) for v in range(self.views)]
        for s in stats:
            assert s["dropped"] + s["survivors"] == s["deferred"] <= s["capacity"] or not s["active"], (tag, s)
            assert s["predicted"] or s["deferred"] == 0, (tag, s)
        return stats

    def close(self):
        self.on.close()
        self.off.close()


@pytest.fixture
def trio(r3, monkeypatch):
    made = []

    def make(resolutions=(128,)):
        made.append(Trio(r3, monkeypatch, resolutions))
        return made[-1]
    yield make
    for t in made:
        t.close()


def hidden_world(t, size=128):
    """An occluder over the lower three quarters of the view (its edge on a 32-texel line, so that whole tiles of every level lie
    under it); under it a field of small triangles (in-place scan), one of work-item triangles (20 px legs) and duplicates of both
    (HIDDEN triangles of the view's winding in all); above it the same, in the open."""
    s = size / 128.0
    occluder = t.add(so.quad(-2 * s, 32 * s, 130 * s, 130 * s, NEAR), size)
    small = so.field(28 * s, 36 * s, 100 * s, 60 * s, 6 * s, 4 * s, FAR, slope=0.0005)
    big = so.field(28 * s, 64 * s, 100 * s, 100 * s, 24 * s, 20 * s, FAR + 0.05)
    t.add(np.concatenate([small, big, small[-40:], big[-3:]]), size)
    t.add(np.concatenate([so.field(2 * s, 2 * s, 126 * s, 8 * s, 6 * s, 4 * s, FAR), so.field(2 * s, 10 * s, 126 * s, 30 * s, 24 * s, 18 * s, FAR)]), size)
    return occluder


HIDDEN = 48 + 3 + 40 + 3  # 12 x 4 small and 3 large triangles drawn by the view, and the duplicates


# ------------------------------------------------------------------ static worlds
def test_first_frame_then_hidden_fields_are_dropped(trio):
    """First frame of a context: the view is drawn in two phases with nothing to predict from.  From the second frame on the
    small triangles AND the work-item triangles under the occluder are deferred and dropped; the visible ones around it are not."""
    t = trio()
    hidden_world(t)
    s0 = t.frame("frame 0")[0]
    assert s0["active"] == 1 and s0["predicted"] == 0 and s0["deferred"] == 0
    for f in (1, 2):
        s = t.frame(f"frame {f}")[0]
        assert s["active"] == 1 and s["predicted"] == 1
        assert s["dropped"] == s["deferred"] == HIDDEN and s["survivors"] == 0, s


def test_slivers_ties_and_the_depth_clip(trio):
    """Edge-on slivers under an occluder whose depth lies between their largest vertex depth (0.35) and their plane's value at the
    box corner (1 after the clamp): never dropped.  Triangles coplanar with the occluder (ties: bound == tile minimum is not
    below it).  Triangles that cross depth 0 and depth 1 of the view, under the occluder and beside it."""
    t = trio()
    t.add(so.quad(16, 16, 112, 112, 0.36))
    t.add(np.concatenate([so.slivers(20.0, 20.0, 12, 0.30, 0.35), so.slivers(60.0, 60.0, 12, 0.35, 0.30, width=9.0)]))
    t.add(np.concatenate([so.field(20, 70, 56, 106, 9, 7, 0.36), so.field(20, 70, 56, 106, 9, 7, 0.36)]))
    cross = [[(70, 20, -0.25), (110, 24, 1.25), (72, 50, 0.5)], [(2, 2, 1.5), (14, 2, -0.5), (2, 14, 0.9)], [(80, 70, 0.2), (100, 70, 1.2), (80, 100, -0.2)]]
    t.add(so.both_windings(cross))
    t.add(so.field(66, 64, 110, 110, 7, 5, 0.2))  # plainly hidden
    for f in range(3):
        s = t.frame(f"frame {f}")[0]
    assert s["dropped"] > 0, s


@pytest.mark.parametrize("hidden", [True, False], ids=["under_the_occluder", "in_the_open"])
def test_box_sizes_and_the_border(trio, hidden):
    """Scan boxes of 4, 5, 8, 9, 16, 17, 32, 33, 64 and 65 px per side -- every level of the pyramid, both sides of the in-place /
    work-item and the 64 px limits -- boxes on all four borders of the view, and two triangles just left of the view whose boxes
    the clamp leaves 1 and 2 px wide (drawn as far as the triangle cull lets them through)."""
    t = trio((256,))
    tris = [so.sided(side, x, y, FAR) for side, x, y in ((4, 40, 40), (5, 50, 40), (8, 60, 40), (9, 72, 40), (16, 84, 40), (17, 104, 40),
                                                         (32, 40, 64), (33, 76, 64), (64, 40, 104), (65, 112, 104))]
    border = [[(-3.7, 80.0, FAR), (-1.2, 84.0, FAR), (-2.5, 95.0, FAR)], [(-2.7, 100.0, FAR), (-0.2, 104.0, FAR), (-1.5, 115.0, FAR)],
              [(-6, 120, FAR), (9, 121, FAR), (-3, 140, FAR)], [(250, 120, FAR), (262, 121, FAR), (251, 150, FAR)],
              [(120, -5, FAR), (140, -4, FAR), (121, 12, FAR)], [(120, 250, FAR), (150, 251, FAR), (121, 262, FAR)], [(-4, -4, FAR), (7, -3, FAR), (-3, 6, FAR)]]
    t.add(np.concatenate(tris + [so.both_windings(border)]), 256)
    if hidden:
        t.add(so.quad(-8, -8, 264, 264, NEAR), 256)
    for f in range(2):
        s = t.frame(f"frame {f}")[0]
    # everything but the 65 px box (never deferred) is set aside when it is hidden
    assert (s["dropped"] >= 9 + 4 and s["survivors"] == 0) if hidden else s["deferred"] == 0, s


# ------------------------------------------------------------------ several views
def test_views_at_an_offset_on_one_lane_and_off_size(trio):
    """Four lights: 128^2 at the atlas origin, two more 128^2 views (view 2 shares view 0's lane and follows it there; both sit at
    non-zero atlas offsets) and a 32^2 view, below the pyramid's 64-texel tiles: drawn in one phase.  (The shadow atlas allocator
    hands out power-of-two maps only, so a view of any other size does not reach the library through a renderer; the filter
    refuses both the same way, r3n.hip occ_view_qualifies.)"""
    t = trio((128, 128, 128, 32))
    hidden_world(t)
    for f in range(3):
        stats = t.frame(f"frame {f}")
    assert [s["active"] for s in stats] == [1, 1, 1, 0]
    for s in stats[:3]:
        assert s["predicted"] == 1 and s["dropped"] == HIDDEN and s["survivors"] == 0, stats
    assert stats[3]["deferred"] == 0


def test_a_64_texel_view_beside_a_128_one(trio):
    t = trio((128, 64))
    hidden_world(t)
    for f in range(2):
        stats = t.frame(f"frame {f}")
    assert [s["active"] for s in stats] == [1, 1] and stats[0]["dropped"] > 0


# ------------------------------------------------------------------ sequences
def test_dolly_of_five_frames(trio):
    """The camera moves by (2, 0), (1, -3), (0, 0), (-4, 2) texels: the prediction is live from the second frame on and follows
    the view (the hidden fields stay hidden: dropped, no survivor beyond the few the occluder's moving edge uncovers)."""
    t = trio()
    hidden_world(t)
    path = ((0, 0), (2, 0), (3, -3), (3, -3), (-1, -1))
    for f, (tx, ty) in enumerate(path):
        t.each(lambda r: camera(r, tx, ty))
        s = t.frame(f"frame {f} camera ({tx}, {ty})")[0]
        assert s["active"] == 1 and (s["predicted"], s["deferred"] > 0, s["dropped"] > 0) == ((0, False, False) if f == 0 else (1, True, True)), (f, s)


def test_a_new_light_direction_drops_the_prediction(trio):
    """A light whose direction changes mid-sequence: no prediction in that frame, and again one in the frame after it.  (A camera
    move by a fraction of a texel never reaches the library as one: the shadow camera snaps to whole texels.)"""
    t = trio()
    hidden_world(t)
    seen = []
    for f in range(5):
        if f == 1:
            t.each(lambda r: r.set_camera_data(oh.translation((-0.5 / 64.0, 0.0, 0.0)), ("raw", IDENT)))
        if f == 3:
            for (r, _), hs in zip(t.all, t.lights):
                r.update_directional_light(hs[0], direction=(0.1, -0.05, 1.0))
        seen.append(t.frame(f"frame {f}")[0])
    assert [s["predicted"] for s in seen] == [0, 1, 1, 0, 1], seen
    assert all(s["active"] == 1 for s in seen) and seen[2]["dropped"] > 0 and seen[3]["deferred"] == 0


def test_stale_prediction_when_the_occluder_leaves_or_moves(trio):
    """The occluder is removed between frames, and a second one moves: the previous frame's minima still call the fields hidden,
    phase 1 sets them aside, phase 2 finds nothing in front of them and draws them -- survivors, and the same atlas."""
    t = trio()
    occluder = hidden_world(t)
    t.frame("frame 0")
    s = t.frame("frame 1")[0]
    assert s["dropped"] > 0 and s["survivors"] == 0
    t.each(lambda r, h: r.remove_object(h), occluder)
    s = t.frame("frame 2: occluder removed")[0]
    assert s["predicted"] == 1 and s["survivors"] == HIDDEN and s["dropped"] == 0, s
    s = t.frame("frame 3")[0]
    assert s["deferred"] == 0, s
    mover = t.add(so.quad(24, 24, 104, 104, NEAR))
    t.frame("frame 4: a new occluder")
    s = t.frame("frame 5")[0]
    assert s["dropped"] > 0 and s["survivors"] == 0
    t.each(lambda r, h: r.set_object_transform(h, oh.translation((40.0 / 64.0, 0.0, 0.0))), mover)
    s = t.frame("frame 6: it moved 40 texels")[0]
    assert s["predicted"] == 1 and s["survivors"] > 0 and s["dropped"] > 0, s
