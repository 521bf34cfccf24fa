"""r3n_textures_compact on the GPU (texture_compact.hip, planned by texel_compact.h): a fragmented streamed pool compacted on the
device against the whole-array write of the same textures, word for word; every pass kind and edge of the planner's list, with the
pass and launch counts the planner program gives for the same layout; the budget; the call that has nothing to do; the refusals;
the allocator afterwards; and Renderer(texture_upload="stream") frames across a compaction against "whole" and the oracle.

Pool words that belong to no texture are written by no path and are left out of the comparisons."""
import ctypes

import numpy as np
import pytest

from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_texture_compact import EDGES, planned
from test_texture_stream_gpu import (AMBIENT, CLEAR, RGBA8, RGBA8_SRGB, RGBA16F, Ctx, H, Scene, Tex, W, desc_words, identical, image,
                                     owned_words, texture_list)

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, INVALID_ARG, STATE = 0, -1, -4


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def align4(v):
    return (v + 3) & ~3


def compact(b, max_words=0, stage_words=0, null_opts=False):
    """(return code, r3n_texture_compact_result as a dict)"""
    opts = b.ffi.TextureCompactOpts(max_words=max_words, stage_words=stage_words)
    out = b.ffi.TextureCompactResult()
    code = b.lib.r3n_textures_compact(b.ctx, None if null_opts else ctypes.byref(opts), ctypes.byref(out))
    return code, {name: int(getattr(out, name)) for name, _ in b.ffi.TextureCompactResult._fields_}


def strip(words, rng):
    """An RGBA8 texture of `words` pool words: words x 1."""
    return Tex(RGBA8, words, 1, 1, 0, rng.integers(0, 256, words * 4, dtype=np.uint8))


def float_tex(rng, w=8, h=4):
    """The float class: RGBA16F, four words per texel -- 128 words at 8 x 4."""
    return Tex(RGBA16F, w, h, 1, 0, rng.uniform(-2.0, 2.0, (h, w, 4)).astype(np.float16).tobytes())


def mip_tex(rng):
    """Generated mips: RGBA8 16 x 16, one stored level of five -- 341 words."""
    return Tex(RGBA8_SRGB, 16, 16, 5, 1, rng.integers(0, 256, 1024, dtype=np.uint8))


def build(r3, items, special=None, seed=0xC0FFEE):
    """A context laid out as the planner program lays the items out: T<words> a texture, H<words> a hole -- a texture that is
    removed again -- each appended on the 4-word boundary behind the one before, one slot each.  special: item index -> a
    function of the generator that gives the Tex (of the item's word count).  The same seed gives the same texels.  Returns
    (ctx, the kept slots)."""
    b = Ctx(r3)
    rng = np.random.default_rng(seed)
    texs = [special[i](rng) if special and i in special else strip(int(it[1:]), rng) for i, it in enumerate(items)]
    cur = 0
    for slot, (it, t) in enumerate(zip(items, texs)):
        assert t.words == int(it[1:])
        b.ok(b.update([slot], [t]))
        assert int(b.descs()[slot][0]) == align4(cur), "ascending appends"
        cur = align4(cur) + t.words
    holes = [i for i, it in enumerate(items) if it[0] == "H"]
    if holes:
        b.ok(b.remove(holes))
    return b, [i for i, it in enumerate(items) if it[0] == "T"]


def snapshot(b):
    """slot -> (descriptor row, its words) of every live texture"""
    d = b.descs()
    return {slot: (row.copy(), b.words(int(row[0]), desc_words(row))) for slot, row in enumerate(d) if row[1]}


def packed_offsets(snap, prefix=None):
    """slot -> offset after a compaction of the textures in `prefix` (all when None), ascending by address"""
    out, cur = {}, 0
    for slot in sorted(snap, key=lambda s: int(snap[s][0][0])):
        if prefix is not None and slot not in prefix:
            break
        out[slot] = align4(cur)
        cur = out[slot] + len(snap[slot][1])
    return out


def assert_moved(b, before, want_offsets, tag):
    """Every texture of `before` is live with its words unchanged; `offset` is the only field that may differ, and is the wanted
    one (slots not in want_offsets: untouched)."""
    after = snapshot(b)
    assert set(after) == set(before), tag
    for slot, (row, words) in before.items():
        new_row, new_words = after[slot]
        assert new_row[1:].tolist() == row[1:].tolist(), f"{tag}: slot {slot} descriptor"
        assert int(new_row[0]) == want_offsets.get(slot, int(row[0])), f"{tag}: slot {slot} offset {int(new_row[0])}"
        bad = np.nonzero(new_words != words)[0]
        assert not len(bad), f"{tag}: slot {slot}: {len(bad)} of {len(words)} words differ, first at {bad[:4]}"
    removed = [row for row in b.descs() if not row[1]]
    assert all(int(row[0]) == 0 for row in removed), tag + ": removed slots stay entries at pool word 0"


# ------------------------------------------------------------------ 1: equals the whole-array write
def test_compaction_equals_the_whole_write(r3):
    texs = texture_list(n_small=40)
    b = Ctx(r3)
    for i, t in enumerate(texs):
        b.ok(b.update([i], [t]))
    holding = dict(enumerate(texs))
    gone = list(range(0, len(texs), 3))
    b.ok(b.remove(gone))
    for s in gone:
        del holding[s]
    rng = np.random.default_rng(11)
    extent = b.stats()["pool_words"]
    for k, t in enumerate((Tex(RGBA8, 64, 64, 1, 0, rng.integers(0, 256, 64 * 64 * 4, dtype=np.uint8)),
                           Tex(RGBA8_SRGB, 33, 31, 1, 0, rng.integers(0, 256, 33 * 31 * 4, dtype=np.uint8)), float_tex(rng, 16, 8))):
        slot = len(texs) + k
        b.ok(b.update([slot], [t]))
        holding[slot] = t
        assert int(b.descs()[slot][0]) >= extent, "it fits no hole"
    before = snapshot(b)
    st0 = b.stats()
    assert st0["free_ranges"] >= len(gone) // 2 and st0["pool_words"] > st0["live_words"] + 100
    code, res = compact(b, null_opts=True)
    b.ok(code)
    print("compaction:", res)
    order = sorted(before, key=lambda s: int(before[s][0][0]))  # B's ascending address order (compaction keeps it)
    assert_moved(b, before, packed_offsets(before), "B")
    # context A: the whole-array write of the same textures in that order
    a = Ctx(r3)
    a.ok(a.write([holding[s] for s in order]))
    da, extent_a, pool_a, mask_a = owned_words(a)
    db, extent_b, pool_b, mask_b = owned_words(b)
    live_b = sorted((row for row in db if row[1]), key=lambda row: int(row[0]))
    assert len(live_b) == len(da) == len(order)
    for k, (rb, ra) in enumerate(zip(live_b, da)):
        assert rb.tolist() == ra.tolist(), f"descriptor {k} by address"
    assert extent_a == extent_b and np.array_equal(mask_a, mask_b)
    bad = (pool_a != pool_b) & mask_a
    assert not bad.any(), f"{bad.sum()} owned pool words differ, first at {np.nonzero(bad)[0][:4]}"
    sizes = [holding[s].words for s in order]
    assert res["free_ranges_after"] == 0 and b.stats()["free_ranges"] == 0
    assert res["pool_words_after"] == sum(align4(n) for n in sizes) - (align4(sizes[-1]) - sizes[-1]) == extent_a
    assert res["pool_words_before"] == st0["pool_words"] and res["words_moved"] > 0 and res["full_syncs"] == 1
    assert res["textures_moved"] == sum(1 for s in order if packed_offsets(before)[s] != int(before[s][0][0]))
    st1 = b.stats()
    for key in ("update_calls", "kernel_launches", "bytes_staged", "full_syncs", "pool_grows", "live_words"):
        assert st1[key] == st0[key], key  # the update path's counters count none of it
    assert st1["pool_words"] == extent_a
    a.close()
    b.close()


# ------------------------------------------------------------------ 2: every pass kind and every edge
SPECIAL = ("float_and_mips", ["H4", "T128", "T341", "T1000", "H12", "T40"], 0)


@pytest.mark.parametrize("name,items,budget", EDGES + [SPECIAL], ids=[e[0] for e in EDGES + [SPECIAL]])
def test_edge_layouts(r3, name, items, budget):
    for stage in (256, 0):
        special = {1: float_tex, 2: mip_tex} if name == SPECIAL[0] else None
        b, kept = build(r3, items, special)
        before = snapshot(b)
        assert sorted(before) == kept
        want = planned(items, stage, budget, sanitize=False)  # (the sanitizer build of the planner program is the CPU test's)
        code, res = compact(b, max_words=budget, stage_words=stage)
        b.ok(code)
        print(name, "stage_words", stage, res, "planner", want)
        assert (res["passes"], res["kernel_launches"], res["words_moved"], res["textures_moved"]) == \
            (want["passes"], want["launches"], want["words_moved"], want["textures_moved"]), (name, stage)
        assert res["pool_words_after"] == want["end"] == b.stats()["pool_words"]
        order = sorted(before, key=lambda s: int(before[s][0][0]))
        moved, words = set(), 0
        for s in order:  # the budget's prefix: in-place textures cost nothing
            n = align4(len(before[s][1]))
            if packed_offsets(before)[s] != int(before[s][0][0]):
                if budget and words + n > budget:
                    break
                words += n
            moved.add(s)
        assert_moved(b, before, packed_offsets(before, moved), f"{name} stage {stage}")
        assert res["full_syncs"] == (1 if want["textures_moved"] else 0)
        b.close()


# ------------------------------------------------------------------ 3: budget
def test_budget_then_the_rest_equals_one_call(r3):
    items = ["H16", "T100", "T33", "H40", "T256", "T7", "H8", "T500", "T64", "H300", "T90"]
    b, kept = build(r3, items)
    twin, _ = build(r3, items)  # the same texels: the same seed
    before = snapshot(b)
    order = sorted(before, key=lambda s: int(before[s][0][0]))
    budget = align4(100) + align4(33) + align4(256) + 2  # ends two words into the fourth texture: three move
    code, res = compact(b, max_words=budget, stage_words=256)
    b.ok(code)
    assert res["textures_moved"] == 3 and res["words_moved"] == budget - 2
    assert_moved(b, before, packed_offsets(before, set(order[:3])), "budgeted")
    # one hole between the packed prefix and the first texture that stayed; the holes above it remain
    assert res["free_ranges_after"] == 3 and res["pool_words_after"] == res["pool_words_before"]
    code, res2 = compact(b)
    b.ok(code)
    assert res2["textures_moved"] == len(order) - 3 and res2["free_ranges_after"] == 0
    assert_moved(b, before, packed_offsets(before), "finished")
    # the twin: one unbudgeted call
    before_t = snapshot(twin)
    code, res_t = compact(twin)
    twin.ok(code)
    assert_moved(twin, before_t, packed_offsets(before_t), "twin")
    (db, extent_b, pool_b, mask_b), (dt, extent_t, pool_t, mask_t) = owned_words(b), owned_words(twin)
    assert np.array_equal(db, dt) and extent_b == extent_t and np.array_equal(mask_b, mask_t) and not ((pool_b != pool_t) & mask_b).any()
    assert res_t["pool_words_after"] == res2["pool_words_after"] and res_t["words_moved"] == res["words_moved"] + res2["words_moved"]
    b.close()
    twin.close()


# ------------------------------------------------------------------ 4: nothing to do
def test_nothing_to_do_makes_no_wait(r3):
    b, _ = build(r3, ["T16", "T7", "T64", "T300"])
    before = snapshot(b)
    st0 = b.stats()
    code, res = compact(b)
    assert code == OK and res["kernel_launches"] == res["passes"] == res["words_moved"] == res["textures_moved"] == 0
    assert res["full_syncs"] == 0 and res["pool_words_after"] == res["pool_words_before"] == st0["pool_words"]
    assert b.stats() == st0
    # a removed tail leaves the live set dense: still nothing to do, and the parked range stays parked
    b.ok(b.remove([3]))
    st1 = b.stats()
    assert st1["free_ranges"] == 1
    code, res = compact(b, null_opts=True)
    assert code == OK and res["kernel_launches"] == 0 and res["full_syncs"] == 0 and b.stats() == st1
    del before[3]
    assert_moved(b, before, {}, "dense")
    # a parked hole below a live texture: one wait for every frame in flight
    b.ok(b.remove([1]))
    code, res = compact(b)
    assert code == OK and res["full_syncs"] == 1 and res["textures_moved"] == 1 and res["free_ranges_after"] == 0
    assert b.stats()["full_syncs"] == st0["full_syncs"]  # r3n_texture_stats counts the update path alone
    del before[1]
    assert_moved(b, before, packed_offsets(before), "after the parked hole")
    b.close()


# ------------------------------------------------------------------ 5: refusals
def test_refusals_change_nothing(r3):
    b, _ = build(r3, ["H8", "T100", "T33", "H40", "T256"])

    def state(ctx):
        d, extent, pool, mask = owned_words(ctx)
        return d.copy(), extent, np.where(mask, pool, 0), ctx.stats()

    def unchanged(s0, ctx, name):
        s1 = state(ctx)
        assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1] and np.array_equal(s0[2], s1[2]) and s0[3] == s1[3], name

    s0 = state(b)
    for stage in (2, 128, 252, 258, 1023):  # not a multiple of 4, or non-zero and below 256
        code, _ = compact(b, stage_words=stage)
        assert code == INVALID_ARG and b.lib.r3n_last_error(b.ctx), stage
        unchanged(s0, b, f"stage_words {stage}")
    # inside a frame
    fu, clear = np.zeros(496, dtype=np.uint8), np.zeros(4, dtype=f32)
    b.ok(b.lib.r3n_frame_begin(b.ctx, b.ffi.ptr(fu), 16, 16, 1, b.ffi.ptr(clear), 32, 32))
    code, _ = compact(b)
    assert code == STATE and b"inside a frame" in b.lib.r3n_last_error(b.ctx)
    b.ok(b.lib.r3n_frame_end(b.ctx))
    unchanged(s0, b, "inside a frame")
    code, res = compact(b)  # the context still works
    assert code == OK and res["textures_moved"] == 3
    b.close()
    # a raw write whose ranges overlap: the slots own no words
    c = Ctx(r3)
    descs = np.array([[0, 4, 4, 1, RGBA8, 0, 0, 0], [8, 2, 2, 1, RGBA8, 0, 0, 0]], dtype=np.uint32)
    texels = np.arange(16, dtype=np.uint32)
    c.ok(c.lib.r3n_textures_write(c.ctx, c.ffi.ptr(descs), 2, c.ffi.ptr(texels), 16))
    d0, w0, st0 = c.descs(), c.words(0, 16), c.stats()
    code, _ = compact(c)
    assert code == STATE and b"owns no words" in c.lib.r3n_last_error(c.ctx)
    assert np.array_equal(c.descs(), d0) and np.array_equal(c.words(0, 16), w0) and c.stats() == st0
    c.close()


# ------------------------------------------------------------------ 6: the allocator follows
def test_allocator_follows(r3):
    b, _ = build(r3, ["H16", "T100", "H40", "T256", "T7", "H300", "T90"])
    before = snapshot(b)
    st0 = b.stats()
    code, res = compact(b)
    b.ok(code)
    freed = res["pool_words_before"] - res["pool_words_after"]
    assert freed == 16 + 40 + 300 and res["free_ranges_after"] == 0 and st0["pool_words"] == res["pool_words_before"]
    assert_moved(b, before, packed_offsets(before), "compacted")
    grows = b.stats()["pool_grows"]
    rng = np.random.default_rng(5)
    # a texture the size of the freed space goes where the mark came down to: old mark minus freed, on its 4-word boundary
    t = strip(freed, rng)
    slot = len(b.descs())
    b.ok(b.update([slot], [t]))
    at = int(b.descs()[slot][0])
    assert at == align4(res["pool_words_before"] - freed) and b.stats()["pool_grows"] == grows
    # remove, then update into the hole: the rebuilt allocator works on
    b.ok(b.remove([3]))  # the 256-word texture
    small = strip(200, rng)
    b.ok(b.update([3], [small]))
    d = b.descs()
    assert int(d[3][0]) == packed_offsets(before)[3] and int(d[3][1]) == 200
    assert b.stats()["pool_grows"] == grows
    del before[3]
    after = snapshot(b)
    for s in before:
        assert np.array_equal(after[s][1], before[s][1]), s
    b.close()


# ------------------------------------------------------------------ 7: frames
def test_frames_across_a_compaction(r3):
    from test_gpu_parity import compare_frames
    aspect = f32(W) / f32(H)
    mkp = r3.material_record
    fillers = [dict(rgba8=image(20 + k, 64, 64), srgb=True, mip_count=1) for k in range(3)]

    def scene(r, mk):
        for f in fillers:  # slots 0 .. 2, in front of everything the frames sample
            r.add_texture_2d(**f)
        return Scene(r, mk, upfront=False)

    stream = scene(r3.Renderer(oh.LEFT, aspect, texture_upload="stream"), mkp)  # texture_compact=None: only when asked
    auto = scene(r3.Renderer(oh.LEFT, aspect, texture_upload="stream", texture_compact=0.25), mkp)
    whole = scene(r3.Renderer(oh.LEFT, aspect), mkp)
    oracle = scene(OracleRenderer(oh.LEFT, aspect), omk)
    everyone = (stream, auto, whole, oracle)
    for k in range(3):  # textures arrive while frames are drawn; the third step adds a cutout material
        frames = [s.step(k) for s in everyone]
    full = stream.r.texture_stats()["pool_words"]
    assert full == auto.r.texture_stats()["pool_words"] > 3 * 4096
    for s in (stream, auto):  # churn: two of the three fillers go -- more than half of the pool becomes holes in front of every sampled texture
        s.r.remove_texture(0)
        s.r.remove_texture(1)
    dense = full - 2 * 4096

    def draw(samples, tag, in_flight=False):
        out = []
        for s in everyone:
            if in_flight and s is stream:
                # a frame in flight during the call: enqueued and not waited for, it samples the words the compaction is about to
                # move and move over -- read back only after the call (which touches none of the frame's output buffers), it is
                # the frame that shows the call waited before it moved anything
                eo = s.r.render_frame(W, H, samples, AMBIENT, CLEAR)
                res = s.r.compact_textures()
                print("compact_textures:", res)
                assert res["textures_moved"] == 5 and res["full_syncs"] == 1 and res["free_ranges_after"] == 0
                out.append(s.r.readback_frame(eo, W, H, samples))
                continue
            out.append(s.r.render(W, H, samples=samples, ambient=AMBIENT, clear_color=CLEAR))
        fs, fa, fw, fo = out
        identical(fw, fa, tag + " (texture_compact=0.25)")
        compare_frames(fo, fa, tag + " (texture_compact=0.25)")
        identical(fw, fs, tag)
        compare_frames(fo, fs, tag)
        return fs

    draw(4, "multisampled, fragmented")
    # texture_compact=0.25 compacted by itself at that flush; None never does
    assert auto.r.texture_stats()["pool_words"] == dense and auto.r.texture_stats()["free_ranges"] == 0
    assert stream.r.texture_stats()["pool_words"] == full and stream.r.texture_stats()["free_ranges"] >= 1
    draw(1, "fragmented, first single-sampled frame")
    frag = draw(1, "fragmented")
    assert stream.r.texture_stats()["pool_words"] == full
    draw(1, "in flight", in_flight=True)
    assert stream.r.texture_stats()["pool_words"] == auto.r.texture_stats()["pool_words"] == dense
    packed = draw(1, "compacted")
    identical(frag, packed, "fragmented against compacted")
    draw(4, "multisampled, compacted")
    assert (frames[3]["vis"] != 0).mean() > 0.25  # the quads cover a good part of the target
    assert np.array_equal(stream.r.readback_texture_descs()[:, 0], auto.r.readback_texture_descs()[:, 0])
    a, b = stream.r.readback_texels(per_texture=True), whole.r.readback_texels(per_texture=True)
    assert a[0] is None and a[1] is None and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
