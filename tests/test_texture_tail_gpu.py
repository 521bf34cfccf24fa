"""r3n_textures_from_texture on the GPU (texture_tail.hip, derived and laid out by texel_tail.h): a texture made of the levels
[start_mip, start_mip + mip_count) of one the pool holds, against the source's own words read back before the call and against the
same levels uploaded as an ordinary texture into a second context, word for word; every source alignment, the edges of a 16-byte
unit and of a wave slot, both pool classes, generated and block-decoded sources; the batch's launch and staging counters; when the
call waits for the frames; the derived textures after their sources are gone and the pool is compacted; the refusals; and
Renderer(texture_upload="stream") frames that sample a derived texture against an uploaded one and the oracle.

Pool words that belong to no texture are written by no path and are left out of the comparisons."""
import ctypes
import os

import numpy as np
import pytest

import scenes
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_texture_stream_gpu import (AMBIENT, BC7, CLEAR, RGBA8, RGBA8_SRGB, RGBA16F, Ctx, H, Scene, Tex, W, chain_blocks, desc_words, identical,
                                     image, owned_words)
from test_texture_tail import planned

pytestmark = pytest.mark.gpu
f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID_ARG = 0, -1
POOL_FLOAT = 2


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def align4(v):
    return (v + 3) & ~3


def from_texture(b, items, null_items=False, null_out=False):
    """(return code, r3n_texture_tail_result as a dict); items = (dst_slot, src_slot, start_mip, mip_count) each"""
    arr = (b.ffi.TextureTail16 * max(len(items), 1))(*[b.ffi.TextureTail16(*it) for it in items])
    out = b.ffi.TextureTailResult()
    code = b.lib.r3n_textures_from_texture(b.ctx, None if null_items else arr, len(items), None if null_out else ctypes.byref(out))
    return code, {name: int(getattr(out, name)) for name, _ in b.ffi.TextureTailResult._fields_}


def full_chain(w, h):
    return int(max(w, h)).bit_length()


def level_bytes(fmt, w, h):
    if fmt == BC7:
        return -(-w // 4) * -(-h // 4) * 16
    return w * h * (8 if fmt == RGBA16F else 4)


def uploaded(fmt, w, h, rng, mips=None):
    """A texture of an uncompressed format with every level of its chain stored: random texels."""
    mips = mips or full_chain(w, h)
    n = sum(level_bytes(fmt, max(1, w >> k), max(1, h >> k)) for k in range(mips))
    if fmt == RGBA16F:
        return Tex(fmt, w, h, mips, 0, rng.uniform(-2.0, 2.0, n // 2).astype(np.float16).tobytes())
    return Tex(fmt, w, h, mips, 0, rng.integers(0, 256, n, dtype=np.uint8))


def cases():
    """(name, source, start_mip, mip_count, first word of the tail in the source, its words) -- the last two are the case's point"""
    rng = np.random.default_rng(0x7A11)
    gold = np.load(os.path.join(HERE, "golden", "bcn_blocks.npz"))
    out = []
    for w in (4, 5, 6, 7):  # level 1 starts w words in: source alignments 0 .. 3
        out.append((f"strip {w}", uploaded(RGBA8, w, 1, rng), 1, 0, w, (w >> 1) + 1))
    for w, words in ((2046, 1023), (2048, 1024), (2049, 1024), (2050, 1025), (2051, 1025)):  # around one wave slot, alignments 2, 0, 1, 2, 3
        out.append((f"strip {w}", uploaded(RGBA8, w, 1, rng), 1, 1, w, words))
    t53 = uploaded(RGBA8, 5, 3, rng)  # levels at words 0, 15, 17
    out += [("5x3 from 1", t53, 1, 0, 15, 3), ("5x3 last level", t53, 2, 0, 17, 1), ("5x3 clone", t53, 0, 0, 0, 18)]
    t16 = uploaded(RGBA8, 16, 16, rng)
    out += [("16x16 levels 1-2", t16, 1, 2, 256, 64 + 16), ("16x16 last level", t16, 4, 1, 340, 1), ("16x16 clone, counted", t16, 0, 5, 0, 341)]
    out.append(("float 8x4", uploaded(RGBA16F, 8, 4, rng), 1, 0, 32 * 4, (8 + 2 + 1) * 4))
    out.append(("generated sRGB 16x16", Tex(RGBA8_SRGB, 16, 16, 5, 1, rng.integers(0, 256, 1024, dtype=np.uint8)), 1, 0, 256, 85))
    out.append(("BC7 16x8", Tex(BC7, 16, 8, 5, 0, gold["bc7_1_data"][:chain_blocks(16, 8, 5, 16)]), 1, 0, 128, 32 + 8 + 2 + 1))
    return out


CASES = cases()


def pool_class(t):
    return POOL_FLOAT if t.is_float else (1 if t.fmt == RGBA8_SRGB else 0)


def want_desc(t, start, count):
    return [max(1, t.w >> start), max(1, t.h >> start), count or t.mips - start, pool_class(t), 0, 0, 0]


def check_derived(b, dst, src, t, start, count, at, words, src_words, tag):
    """The derived entry's descriptor, its words against the source tail's (read back before the call), the source untouched."""
    d = b.descs()
    assert d[dst][1:].tolist() == want_desc(t, start, count), f"{tag}: descriptor {d[dst].tolist()}"
    assert int(d[dst][0]) % 4 == 0 and desc_words(d[dst]) == words
    got = b.words(int(d[dst][0]), words)
    bad = np.nonzero(got != src_words[at: at + words])[0]
    assert not len(bad), f"{tag}: {len(bad)} of {words} words differ, first at {bad[:4]}"
    assert d[src][1:5].tolist() == [t.w, t.h, t.mips, pool_class(t)] and np.array_equal(b.words(int(d[src][0]), t.words), src_words), tag + ": source"
    return got


# ------------------------------------------------------------------ 1: words and descriptor, one call per case
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_words_and_descriptor(r3, case):
    name, t, start, count, at, words = case
    want = planned(t.w, t.h, t.mips, 4 if t.is_float else 1, start, count, sanitize=False)  # (the sanitizer build is the CPU test's)
    assert (want["src_word"], want["words"]) == (at, words), "the case is the one its name says"
    b = Ctx(r3)
    # a 3-word texture in front: the source then starts at word 4, and a first-level-aligned tail is not at the pool's base
    b.ok(b.update([0, 1], [Tex(RGBA8, 3, 1, 1, 0, bytes(12)), t]))
    src_off = int(b.descs()[1][0])
    assert src_off == 4
    src_words = b.words(src_off, t.words)
    st0 = b.stats()
    code, res = from_texture(b, [(2, 1, start, count)])
    b.ok(code)
    print(name, res, "source alignment", (src_off + at) & 3)
    assert res["textures"] == 1 and res["kernel_launches"] == 1 and res["words_copied"] == words
    check_derived(b, 2, 1, t, start, count, at, words, src_words, name)
    st1 = b.stats()
    assert res["pool_words_after"] == st1["pool_words"] == int(b.descs()[2][0]) + words
    for key in ("update_calls", "kernel_launches", "bytes_staged", "full_syncs", "pool_grows"):
        assert st1[key] == st0[key], key  # the update path's counters count none of it
    assert st1["live_words"] == st0["live_words"] + words
    owned_words(b)  # live ranges disjoint and aligned
    b.close()


# ------------------------------------------------------------------ 2 + 3: the batch, and the same levels uploaded
@pytest.fixture(scope="module")
def batch(r3):
    """Every case in ONE call (sources that serve several cases are uploaded once).  Computed once, shared, never changed."""
    b = Ctx(r3)
    sources, slot_of = [], {}
    for _, t, *_ in CASES:
        if id(t) not in slot_of:
            slot_of[id(t)] = len(sources)
            sources.append(t)
    b.ok(b.update(range(len(sources)), sources))
    d = b.descs()
    src_words = [b.words(int(d[s][0]), t.words) for s, t in enumerate(sources)]
    st0 = b.stats()
    items = [(len(sources) + k, slot_of[id(t)], start, count) for k, (_, t, start, count, _, _) in enumerate(CASES)]
    code, res = from_texture(b, items)
    b.ok(code)
    st1 = b.stats()
    derived = []
    for (dst, src, start, count), (name, t, _, _, at, words) in zip(items, CASES):
        derived.append(check_derived(b, dst, src, t, start, count, at, words, src_words[src], "batch, " + name))
    out = dict(res=res, st0=st0, st1=st1, derived=derived, descs=b.descs(), items=items, alignments={(int(d[src][0]) + c[4]) & 3 for (_, src, _, _), c in zip(items, CASES)})
    owned_words(b)
    b.close()
    return out


def test_batch_is_one_launch_and_stages_nothing(batch):
    res, st0, st1 = batch["res"], batch["st0"], batch["st1"]
    print("batch:", res)
    assert res["kernel_launches"] == 1 and res["textures"] == len(CASES) and res["words_copied"] == sum(c[5] for c in CASES)
    assert st1["bytes_staged"] == st0["bytes_staged"] and st1["kernel_launches"] == st0["kernel_launches"] and st1["update_calls"] == st0["update_calls"]
    assert st1["live_words"] == st0["live_words"] + res["words_copied"] and res["pool_words_after"] == st1["pool_words"]
    assert batch["alignments"] == {0, 1, 2, 3}
    assert res["full_syncs"] in (0, 1) and st1["full_syncs"] == st0["full_syncs"]  # (1: the tables grow under n new slots)


def test_equals_the_upload(r3, batch):
    """Context C: the tail's levels sent through r3n_textures_update as an ordinary texture -- sliced from the host's levels, or,
    for the generated chain, the RGBA8 levels read back from the first context."""
    texs = []
    for (name, t, start, count, at, words), got in zip(CASES, batch["derived"]):
        n = count or t.mips - start
        w, h = max(1, t.w >> start), max(1, t.h >> start)
        if t.stored:  # generated: the host never had these levels
            assert start >= t.stored
            texs.append(Tex(RGBA8_SRGB if t.fmt == RGBA8_SRGB else RGBA8, w, h, n, 0, got.tobytes()))
            continue
        skip = sum(level_bytes(t.fmt, max(1, t.w >> k), max(1, t.h >> k)) for k in range(start))
        size = sum(level_bytes(t.fmt, max(1, w >> k), max(1, h >> k)) for k in range(n))
        texs.append(Tex(t.fmt, w, h, n, 0, t.data[skip: skip + size]))
    c = Ctx(r3)
    c.ok(c.update(range(len(texs)), texs))
    d = c.descs()
    for k, ((name, *_), got, (dst, *_)) in enumerate(zip(CASES, batch["derived"], batch["items"])):
        assert d[k][1:].tolist() == batch["descs"][dst][1:].tolist(), name + ": descriptor"
        up = c.words(int(d[k][0]), len(got))
        bad = np.nonzero(up != got)[0]
        assert not len(bad), f"{name}: {len(bad)} of {len(got)} words differ from the uploaded tail's, first at {bad[:4]}"
    c.close()


# ------------------------------------------------------------------ 4: waits
def test_waits_as_the_update_path_does(r3):
    """The situation of test_reuse_of_words_freed_since_the_last_wait_waits_once, with clones in place of uploads."""
    rng = np.random.default_rng(9)

    def rgba(n):
        return Tex(RGBA8, n, n, 1, 0, rng.integers(0, 256, n * n * 4, dtype=np.uint8))
    texs = [rgba(4), rgba(8), rgba(4), rgba(8)]  # words [0, 16) [16, 80) [80, 96) [96, 160)
    b = Ctx(r3)
    b.ok(b.update(range(4), texs))
    b.ok(b.remove([0]))
    b.ok(b.update([2], [rgba(4)]))  # a live slot: the full wait that ends slot 0's quarantine; it moves to word 0, [80, 96) is clean
    assert int(b.descs()[2][0]) == 0
    b.ok(b.remove([1]))  # [16, 80) is parked and slot 1 is hot; slot 0 is not
    big, small = b.words(96, 64), b.words(0, 16)
    st0 = b.stats()
    # a slot no frame in flight can name, words freed since the last wait (the clean hole is too small): one wait
    code, res = from_texture(b, [(0, 3, 0, 0)])
    b.ok(code)
    assert res["full_syncs"] == 1 and int(b.descs()[0][0]) == 16 and np.array_equal(b.words(16, 64), big)
    # that wait ended slot 1's quarantine: a fresh slot and a clean hole -- no wait
    code, res = from_texture(b, [(1, 2, 0, 1)])
    b.ok(code)
    assert res["full_syncs"] == 0 and int(b.descs()[1][0]) == 80 and np.array_equal(b.words(80, 16), small)
    # a slot that held a texture since the last wait, fresh words behind the mark: one wait
    b.ok(b.remove([1]))
    mark = b.stats()["pool_words"]
    code, res = from_texture(b, [(1, 3, 0, 0)])
    b.ok(code)
    assert res["full_syncs"] == 1 and int(b.descs()[1][0]) == mark == 160 and res["pool_words_after"] == 224
    assert np.array_equal(b.words(160, 64), big) and np.array_equal(b.words(96, 64), big)  # (the pool grew: word offsets are kept)
    st1 = b.stats()
    assert st1["full_syncs"] == st0["full_syncs"] and st1["bytes_staged"] == st0["bytes_staged"]  # r3n_texture_stats counts the update path alone
    # n == 0: no wait, no launch
    code, res = from_texture(b, [])
    assert code == OK and res["kernel_launches"] == res["full_syncs"] == res["textures"] == 0 and res["pool_words_after"] == st1["pool_words"]
    assert from_texture(b, [], null_items=True, null_out=True)[0] == OK and b.stats() == st1
    b.close()


# ------------------------------------------------------------------ 5: life after the source
def test_derived_textures_outlive_their_sources(r3):
    rng = np.random.default_rng(21)
    sources = [uploaded(RGBA8, 5, 3, rng), uploaded(RGBA8, 16, 16, rng), uploaded(RGBA16F, 8, 4, rng)]
    b = Ctx(r3)
    b.ok(b.update(range(3), sources))
    items = [(3, 0, 1, 0), (4, 1, 1, 0), (5, 1, 2, 2), (6, 2, 1, 0)]  # 3, 85, 20 and 44 words
    sizes = [3, 85, 20, 44]
    code, res = from_texture(b, items)
    b.ok(code)
    assert res["words_copied"] == sum(sizes)
    d = b.descs()
    before = [(d[dst].copy(), b.words(int(d[dst][0]), n)) for (dst, *_), n in zip(items, sizes)]
    b.ok(b.remove([0, 1, 2]))
    opts, out = b.ffi.TextureCompactOpts(), b.ffi.TextureCompactResult()
    b.ok(b.lib.r3n_textures_compact(b.ctx, ctypes.byref(opts), ctypes.byref(out)))
    assert int(out.textures_moved) == 4 and int(out.free_ranges_after) == 0
    d = b.descs()
    assert not d[:3, 1].any()
    cur = 0
    for (dst, *_), n, (row, words) in zip(items, sizes, before):
        assert d[dst][1:].tolist() == row[1:].tolist() and int(d[dst][0]) == cur
        assert np.array_equal(b.words(cur, n), words), dst
        cur += align4(n)
    st = b.stats()
    assert st["pool_words"] == sum(align4(n) for n in sizes) == int(out.pool_words_after) and st["live_words"] == sum(sizes)
    # a later update reuses what the sources gave back
    grows = st["pool_grows"]
    b.ok(b.update([0], [sources[1]]))
    assert int(b.descs()[0][0]) == st["pool_words"] and b.stats()["pool_grows"] == grows
    for (dst, *_), n, (row, words) in zip(items, sizes, before):
        assert np.array_equal(b.words(int(b.descs()[dst][0]), n), words), dst
    b.close()


# ------------------------------------------------------------------ 6: refusals leave no trace
def test_refusals_leave_no_trace(r3):
    rng = np.random.default_rng(33)
    texs = [uploaded(RGBA8, 16, 16, rng), uploaded(RGBA8, 5, 3, rng), uploaded(RGBA16F, 8, 4, rng), uploaded(RGBA8, 4, 4, rng)]
    b = Ctx(r3)
    b.ok(b.update(range(4), texs))
    b.ok(b.remove([1]))
    n = 4  # slot 1 is removed, slot 4 was never written

    def state():
        d, extent, pool, mask = owned_words(b)
        return d.copy(), extent, np.where(mask, pool, 0), b.stats()

    s0 = state()
    cases = [
        ("removed source", [(n, 1, 0, 0)]),
        ("never-written source", [(n, n, 0, 0)]),
        ("source past the table", [(n, 9, 0, 0)]),
        ("source that is a destination of the same call", [(n, 0, 1, 0), (n + 1, n, 0, 0)]),
        ("live destination", [(3, 0, 1, 0)]),
        ("destination that is its own source", [(0, 0, 1, 0)]),
        ("destination past table + n", [(n + 1, 0, 1, 0)]),
        ("destination past table + n, among good ones", [(n, 0, 1, 0), (n + 2, 0, 2, 0)]),
        ("destination named twice", [(n, 0, 1, 0), (n, 2, 1, 0)]),
        ("start_mip == mips", [(n, 0, 5, 0)]),
        ("start_mip == mips, one level asked", [(n, 0, 5, 1)]),
        ("start_mip + mip_count > mips", [(n, 0, 3, 3)]),
        ("mip_count past the chain from level 0", [(1, 2, 0, 5)]),
        ("bad second item after a good first", [(n, 0, 1, 0), (1, 0, 7, 0)]),
    ]
    for name, items in cases:
        code, _ = from_texture(b, items)
        assert code == INVALID_ARG, name
        assert b.lib.r3n_last_error(b.ctx), name
        s1 = state()
        assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1] and np.array_equal(s0[2], s1[2]) and s0[3] == s1[3], name
    out = b.ffi.TextureTailResult()
    assert b.lib.r3n_textures_from_texture(b.ctx, None, 1, ctypes.byref(out)) == INVALID_ARG  # null items with n > 0
    s1 = state()
    assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1] and np.array_equal(s0[2], s1[2]) and s0[3] == s1[3]
    # the context still works, and the allocator is where it was: the removed slot is the lowest free one, its 18 words
    # ([344, 362) behind the 341-word texture) are the first hole that takes a 3-word tail
    code, res = from_texture(b, [(1, 0, 3, 0)])  # levels 2 x 2 and 1 x 1 of the 16 x 16: 5 words
    b.ok(code)
    d = b.descs()
    assert d[1][1:5].tolist() == [2, 2, 2, 0] and int(d[1][0]) == 344 and res["full_syncs"] == 1  # (the slot was hot, the words parked)
    assert np.array_equal(b.words(344, 5), b.words(int(d[0][0]) + 256 + 64 + 16, 5))
    b.close()


# ------------------------------------------------------------------ 7: frames
def test_frames_sample_a_derived_texture(r3):
    from test_gpu_parity import compare_frames
    aspect = f32(W) / f32(H)
    rng = np.random.default_rng(64)
    levels = [rng.integers(0, 256, max(1, 64 >> k) ** 2 * 4, dtype=np.uint8).tobytes() for k in range(7)]  # 64 x 64 sRGB, every level stored

    def scene(r, mk, derive):
        # slot 0: the 64 x 64 source; slots 1 .. 3: the scene's other textures, everywhere, before slot 0 becomes free; slot 4: the
        # albedo the base quad samples -- levels 2 .. of slot 0, copied on the GPU or uploaded
        src = r.add_texture_2d_encoded(RGBA8_SRGB, 64, 64, levels)
        s = Scene(r, mk, upfront=False)
        for name in ("normal", "cutout", "other"):
            s.tex(name)
        tail = r.add_texture_2d_from_texture(src, 2) if derive else r.add_texture_2d_encoded(RGBA8_SRGB, 16, 16, levels[2:])
        assert (src, tail) == (0, 4)
        s.t["base"] = tail
        return s

    derived = scene(r3.Renderer(oh.LEFT, aspect, texture_upload="stream"), r3.material_record, True)
    direct = scene(r3.Renderer(oh.LEFT, aspect, texture_upload="stream"), r3.material_record, False)
    oracle = scene(OracleRenderer(oh.LEFT, aspect), omk, False)

    def draw(k, tag, samples=1):
        fd, fu, fo = (s.step(k, samples=samples) for s in (derived, direct, oracle))
        identical(fu, fd, tag)
        compare_frames(fo, fd, tag)
        return fd

    draw(0, "source and tail sent in one flush")
    derived.r.remove_texture(0)  # the source goes; the derived texture owns its words
    draw(1, "source removed")
    assert derived.r.readback_texture_descs()[:, 1].tolist() == [0, 32, 16, 24, 16]
    fragmented = derived.r.texture_stats()
    # removed and compacted between two frames: one in flight during the call
    eo = derived.r.render_frame(W, H, 1, AMBIENT, CLEAR)
    res = derived.r.compact_textures()
    print("compact_textures:", res)
    assert res["textures_moved"] == 4 and res["full_syncs"] == 1 and res["free_ranges_after"] == 0
    in_flight = derived.r.readback_frame(eo, W, H, 1)
    fu = direct.r.render(W, H, samples=1, ambient=AMBIENT, clear_color=CLEAR)
    identical(fu, in_flight, "in flight during the compaction")
    packed = derived.r.texture_stats()
    assert packed["pool_words"] == fragmented["pool_words"] - align4(sum(max(1, 64 >> k) ** 2 for k in range(7))) and packed["free_ranges"] == 0
    assert packed["live_words"] == fragmented["live_words"]
    f2 = draw(2, "compacted")
    assert (f2["vis"] != 0).mean() > 0.25  # the quads cover a good part of the target
    draw(4, "compacted, multisampled", samples=4)
    a, b = derived.r.readback_texels(per_texture=True), direct.r.readback_texels(per_texture=True)
    assert a[0] is None and len(a) == len(b) == 5 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ------------------------------------------------------------------ 8: the wrapper
def test_wrapper(r3, tmp_path):
    r = r3.Renderer(oh.LEFT, f32(1.0))
    r.add_texture_2d(image(7, 16, 16), srgb=True, mip_count="maximum", mip_source="generated")
    with pytest.raises(ValueError):
        r.add_texture_2d_from_texture(0, 1)
    r = r3.Renderer(oh.LEFT, f32(1.0), texture_upload="stream")
    a = r.add_texture_2d(image(7, 16, 16), srgb=True, mip_count="maximum", mip_source="generated")
    t = r.add_texture_2d_from_texture(a, 1)        # its source is queued in the same flush
    t2 = r.add_texture_2d_from_texture(t, 1, 2)    # its source is a queued tail: that one is sent first
    assert (a, t, t2) == (0, 1, 2)
    st0 = r.texture_stats()
    parts = r.readback_texels(per_texture=True)
    assert np.array_equal(parts[t], parts[a][256:]) and np.array_equal(parts[t2], parts[a][256 + 64: 256 + 64 + 16 + 4])
    d = r.readback_texture_descs()
    assert d[:, 1:5].tolist() == [[16, 16, 5, 1], [8, 8, 4, 1], [4, 4, 2, 1]]
    assert st0["update_calls"] == 1 and r.texture_stats()["update_calls"] == 1
    with pytest.raises(ValueError):
        r.add_texture_2d_from_texture(t2, 2)
    # the loader: every texture of the file with more than one level is replaced by its tail from level 1
    from rend3_amd import gltf
    path = scenes.write_textured_gltf(os.path.join(str(tmp_path), "textured.gltf"))
    full = r3.Renderer(oh.LEFT, f32(1.0), texture_upload="stream")
    gltf.instance_scene(gltf.Gltf(path), full, r3.host, r3.material_record)
    d_full = full.readback_texture_descs()
    assert len(d_full) >= 4 and (d_full[:, 3] > 1).all()
    low = r3.Renderer(oh.LEFT, f32(1.0), texture_upload="stream")
    gltf.instance_scene(gltf.Gltf(path), low, r3.host, r3.material_record, texture_skip_mips=1)
    d_low = low.readback_texture_descs()
    live = d_low[d_low[:, 1] != 0]
    assert len(d_low) == 2 * len(d_full) and len(live) == len(d_full) and not d_low[:len(d_full), 1].any()  # the originals went
    assert live[:, 1:5].tolist() == [[max(1, int(w) >> 1), max(1, int(h) >> 1), int(m) - 1, int(c)] for w, h, m, c in d_full[:, 1:5]]
    st = low.texture_stats()
    # (live_words counts a texture's own words, without the padding to its 4-word boundary; the padded sizes are what pool_words
    # is after a compaction: test_derived_textures_outlive_their_sources)
    assert st["live_words"] == sum(desc_words(row) for row in live) and st["update_calls"] == 1  # one upload call, one copy call
    whole_tex, low_tex = full.readback_texels(per_texture=True), [p for p in low.readback_texels(per_texture=True) if p is not None]
    for k, (x, y) in enumerate(zip(whole_tex, low_tex)):
        assert np.array_equal(x[int(d_full[k][1]) * int(d_full[k][2]):], y), k
    with pytest.raises(ValueError):
        gltf.instance_scene(gltf.Gltf(path), r3.Renderer(oh.LEFT, f32(1.0)), r3.host, r3.material_record, texture_skip_mips=1)
