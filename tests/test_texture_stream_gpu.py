"""The streamed texture path on the GPU: r3n_textures_update / r3n_textures_remove (single entries added, replaced and removed in a
resident texel pool; every stored level of a call decoded by one launch per kernel family, texture_decode.hip) against the whole-array
write r3n_textures_write_encoded, word for word, through the C ABI -- the two calls share their decode kernels, so the whole-array
write is itself pinned on the oracle's CPU decoders first; the launch, copy and wait structure from r3n_texture_stats; and
Renderer(texture_upload="stream") against "whole" and the oracle, frame by frame.

Pool words that belong to no texture -- the up to three words in front of a texture's 4-word boundary -- are written by neither
path and are left out of the comparisons."""
import ctypes
import os

import numpy as np
import pytest

import scenes
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk

pytestmark = pytest.mark.gpu
f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))

RGBA8, RGBA8_SRGB, R8, RG8, BGRA8_SRGB, BC1, BC3, BC4, BC5, BC7, RGBA16F, BC6H_UF = 0, 1, 2, 3, 5, 6, 10, 12, 13, 14, 21, 32
INVALID_ARG, UNSUPPORTED = -1, -5
CUTOUT = 1


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


# ------------------------------------------------------------------ textures as the C ABI takes them
class Tex:
    """One texture: extent, mips, source format, stored levels (0 = all), its levels' bytes."""

    def __init__(self, fmt, w, h, mips, stored, data):
        self.fmt, self.w, self.h, self.mips, self.stored, self.data = fmt, w, h, mips, stored, bytes(data)
        self.is_float = fmt >= 16
        self.words = sum(max(1, w >> k) * max(1, h >> k) for k in range(mips)) * (4 if self.is_float else 1)
        self.generated = mips - stored if stored else 0


def chain_blocks(w, h, mips, block_bytes):
    return sum(-(-max(1, w >> k) // 4) * -(-max(1, h >> k) // 4) for k in range(mips)) * block_bytes


def texture_list(n_small=300):
    """Every decode family and the edges of the job table: partial blocks, extents off the block size, byte sources, generated
    chains in both pool classes, and more one-texel jobs than a workgroup has wave slots."""
    gold = np.load(os.path.join(HERE, "golden", "bcn_blocks.npz"))
    fgold = np.load(os.path.join(HERE, "golden", "bcn_float_blocks.npz"))
    rng = np.random.default_rng(0x7E57)
    half = rng.uniform(-2.0, 2.0, (4, 8, 4)).astype(np.float16)
    out = [
        Tex(BC1, 8, 8, 4, 0, gold["bc1_0_data"][:chain_blocks(8, 8, 4, 8)]),        # 2x2 and 1x1 levels: single partial blocks
        Tex(BC7, 16, 8, 5, 0, gold["bc7_1_data"][:chain_blocks(16, 8, 5, 16)]),
        Tex(BC3, 5, 3, 1, 0, gold["bc3_0_data"][:32]),                               # not a multiple of 4: the scalar row path
        Tex(BC4, 4, 4, 1, 0, gold["bc4_0_data"][:8]),
        Tex(BC5, 4, 4, 1, 0, gold["bc5_0_data"][:16]),
        Tex(R8, 7, 5, 1, 0, rng.integers(0, 256, 35, dtype=np.uint8)),               # byte sources, odd sizes
        Tex(RG8, 3, 3, 1, 0, rng.integers(0, 256, 18, dtype=np.uint8)),
        Tex(BGRA8_SRGB, 4, 4, 3, 1, rng.integers(0, 256, 64, dtype=np.uint8)),       # generated mips
        Tex(RGBA8, 16, 16, 5, 1, rng.integers(0, 256, 1024, dtype=np.uint8)),        # generated mips
        Tex(BC6H_UF, 8, 8, 1, 0, fgold["bc6h_uf_data"][:64]),
        Tex(RGBA16F, 8, 4, 4, 1, half.tobytes()),                                    # a float format with generated mips
    ]
    out += [Tex(RGBA8, 1, 1, 1, 0, rng.integers(0, 256, 4, dtype=np.uint8)) for _ in range(n_small)]  # more jobs than one workgroup's
    return out


def pack(texs):
    """(descs (n, 8) u32, payload u8): levels back to back, every texture's level 0 on a 4-byte boundary."""
    descs = np.zeros((len(texs), 8), dtype=np.uint32)
    parts, at = [], 0
    for row, t in zip(descs, texs):
        row[:6] = (at, t.w, t.h, t.mips, t.fmt, t.stored)
        padded = t.data + bytes(-len(t.data) & 3)
        parts.append(padded)
        at += len(padded)
    return descs, np.frombuffer(b"".join(parts) or bytes(4), dtype=np.uint8).copy()


class Ctx:
    """A context of the C ABI."""

    def __init__(self, r3):
        from rend3_amd import _ffi
        self.ffi, self.lib = _ffi, _ffi.lib()
        self.ctx = self.lib.r3n_create(0, None)
        assert self.ctx, self.lib.r3n_create_error()

    def close(self):
        self.lib.r3n_destroy(self.ctx)

    def ok(self, code):
        assert code == 0, (code, self.lib.r3n_last_error(self.ctx))

    def write(self, texs):
        descs, payload = pack(texs)
        return self.lib.r3n_textures_write_encoded(self.ctx, self.ffi.ptr(descs), len(texs), self.ffi.ptr(payload), len(payload) if texs else 0)

    def update(self, slots, texs, payload_bytes=None, descs=None):
        d, payload = pack(texs)
        d = d if descs is None else descs
        s = np.array(slots, dtype=np.uint32)
        return self.lib.r3n_textures_update(self.ctx, self.ffi.ptr(s), self.ffi.ptr(d), len(s), self.ffi.ptr(payload),
                                            len(payload) if payload_bytes is None else payload_bytes)

    def remove(self, slots):
        s = np.array(slots, dtype=np.uint32)
        return self.lib.r3n_textures_remove(self.ctx, self.ffi.ptr(s), len(s))

    def descs(self):
        n = ctypes.c_uint32(0)
        self.lib.r3n_readback_texture_descs(self.ctx, None, 0, ctypes.byref(n))
        d = np.zeros((n.value, 8), dtype=np.uint32)
        if n.value:
            self.ok(self.lib.r3n_readback_texture_descs(self.ctx, self.ffi.ptr(d), n.value, ctypes.byref(n)))
        return d

    def words(self, first, n):
        out = np.zeros(max(n, 1), dtype=np.uint32)
        if n:
            self.ok(self.lib.r3n_readback_texels(self.ctx, first, self.ffi.ptr(out), n))
        return out[:n]

    def stats(self, reset=False):
        out = self.ffi.TextureCounters()
        self.ok(self.lib.r3n_texture_stats(self.ctx, ctypes.byref(out), 1 if reset else 0))
        return {name: int(getattr(out, name)) for name, _ in self.ffi.TextureCounters._fields_}


def desc_words(d):
    return sum(max(1, int(d[1]) >> k) * max(1, int(d[2]) >> k) for k in range(int(d[3]))) * (4 if int(d[4]) == 2 else 1)


def owned_words(ctx):
    """(descs, extent, pool words, mask of the words some live texture owns)"""
    d = ctx.descs()
    live = [r for r in d if r[1]]
    extent = max((int(r[0]) + desc_words(r) for r in live), default=0)
    pool = ctx.words(0, extent)
    mask = np.zeros(extent, dtype=bool)
    for r in live:
        assert not mask[int(r[0]): int(r[0]) + desc_words(r)].any(), "live ranges overlap"
        assert int(r[0]) % 4 == 0, "a texture starts on a 4-word boundary"
        mask[int(r[0]): int(r[0]) + desc_words(r)] = True
    return d, extent, pool, mask


@pytest.fixture(scope="module")
def whole(r3):
    """Context A: the list written once through r3n_textures_write_encoded.  Computed once, shared, never changed."""
    texs = texture_list()
    a = Ctx(r3)
    a.ok(a.write(texs))
    d, extent, pool, mask = owned_words(a)
    # the placement formula Renderer.readback_texels restates
    cur = 0
    for row, t in zip(d, texs):
        cur = (cur + 3) & ~3
        assert int(row[0]) == cur and desc_words(row) == t.words
        cur += t.words
    a.close()
    return dict(texs=texs, descs=d, extent=extent, pool=pool, mask=mask)


def test_whole_write_equals_the_oracle(whole):
    """The pin of the `whole` fixture, and through it of every comparison below: each texture of the list decoded on the CPU by
    the oracle (oracle/bcn.c, the blit chains of r3o.c) against the GPU pool range of that texture, word for word.  Per texture,
    not by pool offset: the oracle aligns only its float textures.  The list holds no NaN, so the words compare as integers."""
    o = OracleRenderer()
    c = o.lib.c
    for t in whole["texs"]:
        levels, at = [], 0
        for k in range(t.stored or t.mips):
            size = int(c.r3o_texture_level_bytes(t.fmt, max(1, t.w >> k), max(1, t.h >> k)))
            levels.append(t.data[at: at + size])
            at += size
        assert at == len(t.data), "the stored levels are the whole payload of the texture"
        o.add_texture_2d_encoded(t.fmt, t.w, t.h, levels, generate_mips=t.generated != 0)
    assert len(o.tex_descs) == len(whole["descs"]) == len(whole["texs"])
    compared = 0
    for i, (t, od, gd) in enumerate(zip(whole["texs"], o.tex_descs, whole["descs"])):
        assert od[1:5].tolist() == gd[1:5].tolist() and od[1:4].tolist() == [t.w, t.h, t.mips], f"texture {i}: extent, mips, pool class"
        assert desc_words(od) == t.words
        want = o.tex_pool[int(od[0]): int(od[0]) + t.words]
        got = whole["pool"][int(gd[0]): int(gd[0]) + t.words]
        bad = np.nonzero(want != got)[0]
        assert not len(bad), f"texture {i} (format {t.fmt}, {t.w} x {t.h}): {len(bad)} of {t.words} words differ, first at {bad[:4]}"
        compared += t.words
    assert compared == int(whole["mask"].sum()) == sum(t.words for t in whole["texs"])  # no texture and no word left out


def assert_same_as_whole(b, whole, tag):
    d, extent, pool, mask = owned_words(b)
    assert np.array_equal(d, whole["descs"]), tag + " descriptors"
    assert extent == whole["extent"] and np.array_equal(mask, whole["mask"])
    bad = (pool != whole["pool"]) & mask
    assert not bad.any(), tag + f": {bad.sum()} pool words differ, first at {np.nonzero(bad)[0][:4]}"


# ------------------------------------------------------------------ 4 + 5: append = whole, and how it got there
def test_one_update_equals_the_whole_write(r3, whole):
    texs = whole["texs"]
    b = Ctx(r3)
    b.ok(b.update(range(len(texs)), texs))
    assert_same_as_whole(b, whole, "one call")
    st = b.stats()
    generated = sum(t.generated for t in texs)
    payload_bytes = len(pack(texs)[1])
    print("one call:", st, "generated levels", generated, "payload", payload_bytes)
    assert generated == 2 + 4 + 3
    assert st["update_calls"] == 1 and st["kernel_launches"] <= 4 + generated  # all four families are in the list
    assert st["kernel_launches"] == 4 + generated
    assert st["bytes_staged"] == payload_bytes
    assert st["pool_words"] == whole["extent"] and st["live_words"] == sum(t.words for t in texs) and st["free_ranges"] == 0
    b.close()


def test_one_update_per_texture_equals_the_whole_write(r3, whole):
    texs = whole["texs"]
    b = Ctx(r3)
    grows = syncs = fresh_calls_without_wait = 0
    for i, t in enumerate(texs):
        before = b.stats()
        b.ok(b.update([i], [t]))
        after = b.stats()
        d_grow, d_sync = after["pool_grows"] - before["pool_grows"], after["full_syncs"] - before["full_syncs"]
        # every slot is new and the words are fresh: frames are waited for exactly when a buffer grows
        assert d_grow in (0, 1) and d_sync == d_grow, (i, before, after)
        grows += d_grow
        syncs += d_sync
        fresh_calls_without_wait += d_grow == 0
    assert_same_as_whole(b, whole, "one call per texture")
    st = b.stats()
    print("per texture:", st)
    assert st["update_calls"] == len(texs)
    assert st["bytes_staged"] == len(pack(texs)[1])  # every byte once: not quadratic
    assert st["kernel_launches"] == len(texs) + sum(t.generated for t in texs)  # one family per texture
    # geometric growth: each of the three resident buffers doubles at most ceil(log2(n)) + 1 times over n appends
    assert 1 <= grows <= 3 * (int(np.ceil(np.log2(len(texs)))) + 1) and fresh_calls_without_wait >= len(texs) // 2
    b.close()


def test_updates_behind_a_whole_write_equal_the_whole_write(r3, whole):
    texs = whole["texs"]
    half = len(texs) // 2
    b = Ctx(r3)
    b.ok(b.write(texs[:half]))
    b.ok(b.update(range(half, len(texs)), texs[half:]))
    assert_same_as_whole(b, whole, "whole write of the first half, then one update")
    c = Ctx(r3)
    c.ok(c.update(range(5), texs[:5]))
    c.ok(c.write(texs[:7]))  # a whole write resets the allocator to its own prefix
    c.ok(c.update(range(7, 9), texs[7:9]))
    c.ok(c.update(range(9, len(texs)), texs[9:]))
    assert_same_as_whole(c, whole, "update, whole write, updates")
    d = Ctx(r3)
    d.ok(d.write(texs))
    d.ok(d.write(texs[:7]))  # the shrinking order: table, pool extent and allocator fall back to the shorter write's prefix
    d.ok(d.update(range(7, len(texs)), texs[7:]))
    assert_same_as_whole(d, whole, "whole write, shorter whole write, update of the rest")
    b.close()
    c.close()
    d.close()


# ------------------------------------------------------------------ 6: remove, reuse, replace
@pytest.fixture(scope="module")
def single(r3):
    """The words a whole-array write of ONE texture gives it, by texture, computed on demand and kept."""
    cache = {}

    def words_of(t):
        key = (t.fmt, t.w, t.h, t.mips, t.stored, t.data)
        if key not in cache:
            a = Ctx(r3)
            a.ok(a.write([t]))
            cache[key] = a.words(0, t.words)
            a.close()
        return cache[key]
    return words_of


def check_table(b, holding, single, tag):
    """holding: slot -> Tex or None.  Ranges disjoint and aligned (owned_words), every live texture's words its own."""
    d, extent, pool, _ = owned_words(b)
    assert len(d) == len(holding)
    for slot, t in enumerate(holding):
        if t is None:
            assert d[slot][1] == 0 and d[slot][2] == 0, tag + f" slot {slot} should read as removed"
            continue
        assert (int(d[slot][1]), int(d[slot][2]), int(d[slot][3])) == (t.w, t.h, t.mips), tag
        at = int(d[slot][0])
        assert np.array_equal(pool[at: at + t.words], single(t)), tag + f" slot {slot}"
    return d, extent


def lowest_fit(d, extent, words):
    """First fit at the lowest address over the gaps between the live textures' padded ranges; the end otherwise."""
    cur = 0
    for at, n in sorted((int(r[0]), desc_words(r)) for r in d if r[1]):
        if at - cur >= ((words + 3) & ~3):
            return cur
        cur = (at + n + 3) & ~3
    return cur


def test_remove_reuse_replace(r3, single):
    texs = texture_list(n_small=13)
    b = Ctx(r3)
    b.ok(b.update(range(len(texs)), texs))
    holding = list(texs)
    d0, extent0 = check_table(b, holding, single, "before")
    # every third texture goes; the others keep their words
    gone = list(range(0, len(texs), 3))
    before = b.stats()
    b.ok(b.remove(gone))
    for s in gone:
        holding[s] = None
    d1, _ = check_table(b, holding, single, "after the removal")
    assert all(np.array_equal(d0[s], d1[s]) for s in range(len(texs)) if s not in gone)
    st = b.stats()
    assert st["full_syncs"] == before["full_syncs"] and st["free_ranges"] >= 4  # a removal waits for nothing
    assert st["live_words"] == sum(t.words for t in holding if t is not None)
    # textures that fit the holes land at the lowest fitting address; the pool does not grow; the words were freed since the last
    # full wait, so the call waits for the frames once
    rng = np.random.default_rng(3)
    for slot, t in ((0, Tex(RGBA8, 4, 4, 1, 0, rng.integers(0, 256, 64, dtype=np.uint8))),
                    (3, Tex(BC4, 4, 4, 1, 0, texs[3].data)),
                    (6, Tex(R8, 3, 3, 1, 0, rng.integers(0, 256, 9, dtype=np.uint8)))):
        d, extent = check_table(b, holding, single, "")
        want = lowest_fit(d, extent, t.words)
        assert want < extent
        before = b.stats()
        b.ok(b.update([slot], [t]))
        after = b.stats()
        holding[slot] = t
        d, _ = check_table(b, holding, single, f"hole fill into slot {slot}")
        assert int(d[slot][0]) == want, (slot, int(d[slot][0]), want)
        assert after["pool_words"] == before["pool_words"] and after["pool_grows"] == before["pool_grows"]
        if slot == 0:
            assert after["full_syncs"] == before["full_syncs"] + 1  # the slot was removed since the last wait (and so were the words)
    # larger than any hole: it goes to the end
    big = Tex(RGBA8_SRGB, 64, 64, 1, 0, rng.integers(0, 256, 64 * 64 * 4, dtype=np.uint8))
    d, extent = check_table(b, holding, single, "")
    b.ok(b.update([9], [big]))
    holding[9] = big
    d, _ = check_table(b, holding, single, "appended")
    assert int(d[9][0]) == (extent + 3) & ~3
    # a live slot replaced by another format and size (RGBA8 class <- BC7 chain, then float class)
    for t in (Tex(R8, 7, 5, 1, 0, texs[5].data), texs[10]):
        before = b.stats()
        b.ok(b.update([1], [t]))
        holding[1] = t
        check_table(b, holding, single, "replaced")
        assert b.stats()["full_syncs"] == before["full_syncs"] + 1  # the slot held a texture: a frame in flight may read it
    # removal of everything: the table stays, the pool is empty
    b.ok(b.remove([s for s, t in enumerate(holding) if t is not None]))
    d = b.descs()
    assert len(d) == len(texs) and not d[:, 1].any()
    b.ok(b.update([2], [big]))  # (waits, merges the parked ranges, starts again at word 0)
    assert int(b.descs()[2][0]) == 0 and b.stats()["live_words"] == big.words
    b.close()


def test_reuse_of_words_freed_since_the_last_wait_waits_once(r3, single):
    """The quarantine alone: a slot that no frame in flight can name (it was removed before the last full wait) takes words that
    were freed after it.  A clean hole that fits is preferred and costs no wait."""
    rng = np.random.default_rng(9)

    def rgba(n):
        return Tex(RGBA8, n, n, 1, 0, rng.integers(0, 256, n * n * 4, dtype=np.uint8))
    texs = [rgba(4), rgba(8), rgba(4), rgba(4)]  # words [0, 16) [16, 80) [80, 96) [96, 112)
    b = Ctx(r3)
    b.ok(b.update(range(4), texs))
    holding = list(texs)
    b.ok(b.remove([0]))
    holding[0] = None
    holding[2] = rgba(4)
    b.ok(b.update([2], [holding[2]]))  # a live slot: the full wait that ends slot 0's quarantine; it moves to word 0
    d, _ = check_table(b, holding, single, "replaced")
    assert int(d[2][0]) == 0
    b.ok(b.remove([1]))  # [16, 80) is parked; [80, 96) is a clean hole
    holding[1] = None
    for t, want_at, waits in ((rgba(8), 16, 1), (rgba(4), 80, 0)):
        slot = holding.index(None)
        before = b.stats()
        b.ok(b.update([slot], [t]))
        after = b.stats()
        holding[slot] = t
        d, _ = check_table(b, holding, single, f"slot {slot}")
        assert int(d[slot][0]) == want_at
        assert after["pool_grows"] == before["pool_grows"] and after["pool_words"] == before["pool_words"]
        assert after["full_syncs"] == before["full_syncs"] + waits, (slot, before, after)
    b.close()


# ------------------------------------------------------------------ 8: errors leave no trace
def test_errors_leave_no_trace(r3):
    texs = texture_list(n_small=4)
    b = Ctx(r3)
    b.ok(b.update(range(len(texs)), texs))
    b.ok(b.remove([2]))
    n = len(texs)

    def state():
        d, extent, pool, mask = owned_words(b)
        return d.copy(), extent, np.where(mask, pool, 0), b.stats()

    s0 = state()
    small = Tex(RGBA8, 2, 2, 1, 0, bytes(range(16)))
    block_generated = Tex(BC1, 8, 8, 4, 0, texs[0].data)
    block_generated.stored = 1
    cases = [
        ("duplicate slots", lambda: b.update([n, n], [small, small]), INVALID_ARG),
        ("slot past the allowed end", lambda: b.update([n + 1], [small]), INVALID_ARG),
        ("slot past the allowed end, among good ones", lambda: b.update([n, n + 2], [small, small]), INVALID_ARG),
        ("levels outside the payload", lambda: b.update([n], [small], payload_bytes=12), INVALID_ARG),
        ("level 0 off a 4-byte boundary", lambda: b.update([n], [small], descs=np.array([[2, 2, 2, 1, 0, 0, 0, 0]], dtype=np.uint32)), INVALID_ARG),
        ("a block format with stored_mips < mips", lambda: b.update([n], [block_generated]), UNSUPPORTED),
        ("bad second descriptor after a good first", lambda: b.update([0, 1], [small, block_generated]), UNSUPPORTED),
        ("removing a removed slot", lambda: b.remove([2]), INVALID_ARG),
        ("removing a slot that was never written", lambda: b.remove([n]), INVALID_ARG),
        ("removing one slot twice", lambda: b.remove([1, 1]), INVALID_ARG),
        ("removing a live and a removed slot", lambda: b.remove([1, 2]), INVALID_ARG),
    ]
    for name, call, want in cases:
        assert call() == want, name
        assert b.lib.r3n_last_error(b.ctx), name
        s1 = state()
        assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1] and np.array_equal(s0[2], s1[2]) and s0[3] == s1[3], name
    b.ok(b.update([2], [small]))  # the context still works: the removed slot is the lowest free one
    assert int(b.descs()[2][1]) == 2
    b.close()


# ------------------------------------------------------------------ 7: frames
def image(seed, w, h, alpha=None):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha is not None:
        img[..., 3] = np.where(rng.random((h, w)) < 0.45, 40, 230).astype(np.uint8)
    return img


TEXTURES = {  # name -> add_texture_2d arguments
    "base": dict(rgba8=image(1, 32, 32), srgb=True, mip_count="maximum", mip_source="generated"),
    "normal": dict(rgba8=image(2, 32, 32), srgb=False, mip_count="maximum", mip_source="generated"),
    "cutout": dict(rgba8=image(3, 16, 16, alpha=True), srgb=True, mip_count="maximum", mip_source="generated"),
    "other": dict(rgba8=image(4, 24, 12), srgb=True, mip_count=1),
    "late": dict(rgba8=image(5, 8, 8), srgb=False, mip_count="maximum", mip_source="generated"),
}
W = H = 64
AMBIENT, CLEAR = (0.2, 0.2, 0.2, 1.0), (0.02, 0.03, 0.05, 1.0)


class Scene:
    """A few quads, textures handed over across three frames (TextureManager::add while frames are drawn), then one texture
    removed and its slot taken by another.  `upfront`: the final table -- slot 0 = "late" -- exists from the start instead (the
    fresh renderer of the last comparison); the opaque base quad then shows another texture in the first frames, which changes
    no depth and so no culling history."""

    def __init__(self, r, mk, upfront):
        self.r, self.mk, self.upfront = r, mk, upfront
        self.t = {}
        if upfront:
            for name in ("late", "normal", "cutout", "other"):
                self.t[name] = r.add_texture_2d(**TEXTURES[name])
            self.t["base"] = self.t["other"]
        pq = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=f32)
        iq = np.array([0, 2, 1, 0, 3, 2], dtype=np.uint32)
        nq = np.tile(np.array([[0, 1, 0]], dtype=f32), (4, 1))
        uv = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], dtype=f32)
        self.quad = r.add_mesh(pq, iq, normals=nq, uv0=uv, tangents=scenes._tangents(nq))
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -2.0, 0.4), distance=30.0, resolution=128)
        # a second light from below: the quads face it, so its shadow view rasterises them -- the cutout ones through the alpha of
        # their texture, on the shadow lanes
        r.add_directional_light(color=(1, 1, 1), intensity=2.0, direction=(0.3, 2.0, 0.4), distance=30.0, resolution=128)
        r.set_camera_data(oh.look_at_lh((0.0, 3.0, -5.0), (0.0, 0.0, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        self.mats = {}

    def tex(self, name):
        if name not in self.t:
            self.t[name] = self.r.add_texture_2d(**TEXTURES[name])
        return self.t[name]

    def base_material(self, albedo):
        return self.mk(albedo_mode="texture", albedo_texture=albedo, normal_texture=self.tex("normal"), roughness=0.6, metallic=0.2)

    def place(self, material, x, y, z):
        self.r.add_object(self.quad, material, oh.mat4_mul(oh.translation((x, y, z)), oh.scale((1.4, 1.0, 1.4))))

    def step(self, k, samples=1):
        r, mk = self.r, self.mk
        if k == 0:
            self.mats["base"] = r.add_material(self.base_material(self.tex("base")))
            self.place(self.mats["base"], -1.6, 0.0, 0.0)
        elif k == 1:
            m = r.add_material(mk(albedo_mode="texture", albedo_texture=self.tex("cutout"), roughness=0.5, cutout=0.5), CUTOUT)
            self.place(m, 0.4, 1.0, 0.5)   # above the others
            self.place(m, 1.6, 0.0, 2.5)
        elif k == 2:
            m = r.add_material(mk(albedo_mode="texture_value", albedo_texture=self.tex("other"), albedo=(0.9, 0.8, 0.7, 1.0), roughness=0.8))
            self.place(m, 1.2, -0.2, -0.6)
        elif k == 3:
            # "base" goes: its material is re-pointed to "other" first, then the slot is taken by "late"
            r.update_material(self.mats["base"], self.base_material(self.tex("other")))
            if not self.upfront:
                r.remove_texture(self.t.pop("base"))
                assert self.tex("late") == 0, "the lowest free slot"
            m = r.add_material(mk(albedo_mode="texture", albedo_texture=self.tex("late"), roughness=0.4))
            self.place(m, -0.6, 0.3, 2.2)
        return r.render(W, H, samples=samples, ambient=AMBIENT, clear_color=CLEAR)


def identical(a, b, tag):
    """Two product frames: every array of the frame dict, bit for bit."""
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].shape == b[key].shape and np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), f"{tag}: {key}"
        elif key == "shadows":
            assert len(a[key]) == len(b[key])
            for k, (sa, sb) in enumerate(zip(a[key], b[key])):
                identical(sa, sb, f"{tag} shadow view {k}")
        elif key == "draw_calls":
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), f"{tag}: draw calls"


def test_frames_stream_equals_whole_equals_oracle(r3):
    from test_gpu_parity import compare_frames
    aspect = f32(W) / f32(H)
    mkp = r3.material_record
    stream = Scene(r3.Renderer(oh.LEFT, aspect, texture_upload="stream"), mkp, upfront=False)
    grown = Scene(r3.Renderer(oh.LEFT, aspect), mkp, upfront=False)
    oracle = Scene(OracleRenderer(oh.LEFT, aspect), omk, upfront=False)
    fresh = Scene(r3.Renderer(oh.LEFT, aspect), mkp, upfront=True)
    fresh_oracle = Scene(OracleRenderer(oh.LEFT, aspect), omk, upfront=True)
    for k in range(3):  # textures arrive while frames are drawn
        fs, fw, fo = stream.step(k), grown.step(k), oracle.step(k)
        fresh.step(k), fresh_oracle.step(k)
        identical(fw, fs, f"frame {k}")
        compare_frames(fo, fs, f"stream frame {k}")
    assert (fo["vis"] != 0).mean() > 0.25  # the quads cover a good part of the target (the oracle's frame: 0.29)
    assert (fo["atlas"] != 0).mean() > 0.005  # and are drawn into the shadow atlas (the oracle's frame: 0.012)
    st = stream.r.texture_stats()
    print("stream renderer after three frames:", st)
    assert st["update_calls"] == 3  # one call per frame that had new textures, whatever their number
    assert stream.r.readback_texture_descs()[:, 1].tolist() == [32, 32, 16, 24]
    # one texture removed and its slot reused: the fresh whole-mode renderer holds the same slot numbering
    fs, fw, fo = stream.step(3), fresh.step(3), fresh_oracle.step(3)
    identical(fw, fs, "frame 3")
    compare_frames(fo, fs, "stream frame 3")
    assert stream.r.readback_texture_descs()[:, 1].tolist() == [8, 32, 16, 24]
    texels = stream.r.readback_texels(per_texture=True)
    want = fresh.r.readback_texels(per_texture=True)
    assert len(texels) == len(want) and all(np.array_equal(a, b) for a, b in zip(texels, want))
    # removed and unreferenced: None in the stream renderer's read-back
    stream.r.remove_texture(stream.t["late"] + 3)
    assert stream.r.readback_texels(per_texture=True)[3] is None
    with pytest.raises(ValueError):
        stream.r.remove_texture(3)
    # one multisampled frame (the removed slot 3 is still named by a material: put it back first)
    assert stream.r.add_texture_2d(**TEXTURES["other"]) == 3
    fs, fw, fo = stream.step(4, samples=4), fresh.step(4, samples=4), fresh_oracle.step(4, samples=4)
    identical(fw, fs, "multisampled frame")
    compare_frames(fo, fs, "stream multisampled frame")
