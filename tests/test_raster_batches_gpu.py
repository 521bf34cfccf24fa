"""The batched body of the work-item rasteriser (kernels_raster.h raster_big_batched_body: one sample per pixel, opaque key, in the
shadow views and in the viewport) at the sizes where a batch can go wrong, bit for bit against tests/raster_reference.py -- in
these dyadic w = 1 worlds that integer restatement of the contract is exact.

A batch is B = R3N_BIG_BATCH consecutive entries of one work sub-queue; a wave reads all B records behind one wait, an index past
the queue's count reads the last valid record instead, and only `count` items of the batch are scanned.  What can go wrong is
therefore a matter of counts:
  queue capacity    R3N_BIG_CAPACITY in {1, B - 1, B, B + 1, 2B + 1} with more items than the queues hold: the consumer takes
                    partial batches of a queue whose counter ran past the capacity (the count is min(counter, capacity)), the
                    producer scans the rest in place
  tiny queue        three work items in all: almost every sub-queue is empty and almost every wave finds no batch
  many batches      R3N_TUNE="big_grid=256" (1 024 waves) on a 1 024 x 1 024 target with more than 1 024 * 2B items: every wave
                    takes several batches, and the sub-queue's last batch is partial
  offset view       the 32 px shadow view at x = 64 of a 128 x 64 atlas (vp_x != 0, pitch != width) beside the 64 px one
  region modes      every region an opaque producer queues is scanned in FINE blocks: its columns start on the item alignment,
                    so rx1 - (rx0 & ~15) < 32 always holds (raster_reference.plan; asserted here for every world of this file).
                    The coarse 8 x 8 mode of the shared scan is reached by the transparent pass's items only, which the batched
                    body never sees (tests/test_raster_gpu.py::test_blend_coverage covers it)
Both frame entry points run every case: r3n_render_frame and the per-node path (R3N_FRAME_NODES=1)."""
import os
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

import raster_reference as rr
from test_raster_gpu import FRAME_PATHS, IDENT, check_atlas, check_viewport, hip, queued, r3  # noqa: F401  (r3: the module's fixture)

pytestmark = pytest.mark.gpu
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch_size():
    text = open(os.path.join(ROOT, "rend3_amd", "csrc", "kernels_raster.h")).read()
    (b,) = re.findall(r"^#define\s+R3N_BIG_BATCH\s+(\d+)\b", text, flags=re.M)
    assert int(b) in (2, 3, 4)
    return int(b)


B = batch_size()
_CACHE = {}


def cover_world(N, layers):
    """`layers` right triangles over the whole N x N target (the right angle in each corner in turn, nearer from layer to layer:
    N / 32 squared work items each, all of one object: one producer wave, one sub-queue) and three smaller ones in a second object
    that make the item count odd; every triangle in both windings (the shadow view draws the other one)."""
    corner = [(Fr(-1), Fr(-1)), (Fr(1), Fr(-1)), (Fr(1), Fr(1)), (Fr(-1), Fr(1))]
    big = [rr.flat(corner[k % 4], corner[(k + 1) % 4], corner[(k + 3) % 4], Fr(k + 1, 128)) for k in range(layers)]
    assert layers < 100
    px = lambda x, y: (Fr(2 * x, N) - 1, 1 - Fr(2 * y, N))  # noqa: E731  clip position of a window position
    small = [rr.flat(px(3, 5), px(3 + w, 5), px(3, 5 + h), Fr(7, 8)) for w, h in ((40, 12), (20, 70), (9, 9))]  # 2 + 3 + 1 items
    return dict(name=f"cover {N} x {layers}", objects=[rr._object(rr.both_windings(big)), rr._object(rr.both_windings(small))])


def tiny_world():
    """three objects of one 16 px triangle each in a 64 px target: one work item per object and view"""
    px = lambda x, y: (Fr(2 * x, 64) - 1, 1 - Fr(2 * y, 64))  # noqa: E731
    tris = [rr.flat(px(x, y), px(x + 15, y), px(x, y + 15), z) for x, y, z in ((2, 3, Fr(1, 4)), (33, 5, Fr(1, 2)), (20, 40, Fr(3, 4)))]
    return dict(name="tiny 64", objects=[rr._object(rr.both_windings([t])) for t in tris])


def reference(key, world_fn, N):
    """(world, viewport view + frame, shadow view + frame of an N px light), computed once per module"""
    if key not in _CACHE:
        world = world_fn()
        vv, sv = rr.View(N, N, 1), rr.View(N, N, 1, shadow=True)
        _CACHE[key] = (world, (vv, rr.render(world, vv)), (sv, rr.render(world, sv)))
    return _CACHE[key]


def all_fine(view, ref):
    items = [it for s in ref["recs"] if s["passes"] for it in rr.plan(view, s)[1]]
    return bool(items) and all(it["fine"] for it in items)


def run(r3, monkeypatch, frame_nodes, ref, N, env, tag, overflow=None):
    """one frame of the world with one N px light under `env`: viewport keys, atlas words, items queued per call; `overflow`: the
    capacity every call must have queued more than 32 sub-queues of"""
    world, (vv, vref), (sv, sref) = ref
    assert all_fine(vv, vref) and all_fine(sv, sref), f"{tag}: an opaque producer queued a coarse region"
    p = hip(r3, monkeypatch, frame_nodes, N, N, env)
    try:
        rr.load(p, r3.material_record, world, IDENT)
        p.add_directional_light(resolution=N, **rr.LIGHT)
        fp = p.render(N, N)
        stats = queued(p.raster_stats())
        check_viewport(world, vv, vref, fp, tag)
        assert tuple(fp["atlas_size"]) == (N, N), tag
        msg = rr.describe_first_difference(world, sv, sref, np.ascontiguousarray(fp["atlas"].view(u32)))
        assert msg is None, f"{tag}, shadow view: {msg}"
        assert np.array_equal(fp["shadows"][0]["pass"][: len(sref["pass"])], sref["pass"]), f"{tag}: shadow pass set"
        want = ([rr.item_count(vv, vref["recs"])], [rr.item_count(sv, sref["recs"])])
        assert stats == want, f"{tag}: work items queued {stats}, plan() says {want}"
        if overflow is not None:
            assert min(want[0][0], want[1][0]) > 32 * overflow, f"{tag}: {want} items do not overflow 32 sub-queues of {overflow}"
        p.sync()
        assert p.capacity_reports == [], f"{tag}: {p.capacity_reports}"
        return want
    finally:
        p.close()


# ------------------------------------------------------------------ queue capacity: partial batches, the producer scans the rest
@FRAME_PATHS
@pytest.mark.parametrize("cap", sorted({1, B - 1, B, B + 1, 2 * B + 1}), ids=lambda c: f"capacity_{c}")
def test_partial_batches_of_full_queues(r3, monkeypatch, cap, frame_nodes):
    """256 px target, 64 items per covering triangle, enough layers for more than 32 * (2B + 1) items per call: at every capacity the
    queues end full (counter past the capacity), the consumer's last batch per queue holds capacity mod B records, and keys and
    atlas words are the reference's."""
    layers = (32 * (2 * B + 1)) // 64 + 2
    ref = reference(("cover", 256, layers), lambda: cover_world(256, layers), 256)
    run(r3, monkeypatch, frame_nodes, ref, 256, {"R3N_BIG_CAPACITY": cap}, f"cover 256 R3N_BIG_CAPACITY={cap}", overflow=cap)


# ------------------------------------------------------------------ tiny queue
@FRAME_PATHS
def test_three_items_in_all(r3, monkeypatch, frame_nodes):
    ref = reference("tiny", tiny_world, 64)
    want = run(r3, monkeypatch, frame_nodes, ref, 64, None, "tiny 64")
    assert want == ([3], [3])


# ------------------------------------------------------------------ many batches per wave
@FRAME_PATHS
def test_every_wave_takes_several_batches(r3, monkeypatch, frame_nodes):
    """1 024 waves (big_grid=256), 2B + 1 covering layers of 1 024 items each on a 1 024 px target plus six odd items: more than two
    batches per wave, and the count of the queue that holds them is no multiple of B."""
    layers = 2 * B + 1
    ref = reference(("cover", 1024, layers), lambda: cover_world(1024, layers), 1024)
    want = run(r3, monkeypatch, frame_nodes, ref, 1024, {"R3N_TUNE": "big_grid=256"}, "cover 1024 big_grid=256")
    for n in want[0] + want[1]:
        assert n > 1024 * 2 * B and n % B, f"{n} items"


# ------------------------------------------------------------------ a shadow view at a non-zero atlas offset
@FRAME_PATHS
@pytest.mark.parametrize("kind", ["boxes", "random"])
def test_offset_shadow_view(r3, monkeypatch, kind, frame_nodes):
    """The 64 px worlds of tests/raster_reference.py under two lights: the second view lies at x = 64 of a 128 x 64 atlas.  Nothing
    may land outside the views; every queued region is a fine one."""
    W = H = 64
    world = rr.worlds(W, H)[kind]
    vview, vref = rr.frame(kind, W, H, 1)
    assert all_fine(vview, vref)
    for size in (64, 32):
        assert all_fine(*rr.frame(kind, W, H, 1, size))
    tag = f"{kind} {W}x{H} lights (64, 32)"
    p = hip(r3, monkeypatch, frame_nodes, W, H)
    try:
        rr.load(p, r3.material_record, world, IDENT)
        for res in (64, 32):
            p.add_directional_light(resolution=res, **rr.LIGHT)
        fp = p.render(W, H)
        stats = queued(p.raster_stats())
        want = check_atlas(world, W, H, kind, fp, (64, 32), tag)
        check_viewport(world, vview, vref, fp, tag)
        assert stats == ([rr.item_count(vview, vref["recs"])], want), f"{tag}: {stats}"
    finally:
        p.close()
