"""GPU: the bloom kernels behind r3n_bloom_set (rend3_amd/csrc/bloom.hip, the composite in exposure.hip) against
tests/bloom_reference.py -- every level of the down and of the up chain word for word under every launch plan, output bytes byte
for byte, the float view within the tolerances of tests/test_tonemap_ops_gpu.py.  HDR targets are injected with r3n_hdr_write; the
last test renders real frames.  The reference itself is tied down in tests/test_bloom.py."""
import ctypes
import functools

import numpy as np
import pytest

import bloom_reference as B
import scenes
import tonemap_reference as T
from oracle import host as oh
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
ONE = 0x3C00
TAIL_ALL = 1 << 24  # every level that fits the tail kernel's LDS goes into it


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def set_tonemap(r, o):
    from rend3_amd import _ffi
    c = _ffi.TonemapOpts()
    for k, v in (o or {}).items():
        setattr(c, k, v)
    return r.lib.r3n_tonemap_set(r.ctx, ctypes.byref(c) if o is not None else None)


def set_bloom(r, o):
    from rend3_amd import _ffi
    c = _ffi.BloomOpts()
    for k, v in (o or {}).items():
        setattr(c, k, v)
    return r.lib.r3n_bloom_set(r.ctx, ctypes.byref(c) if o is not None else None)


def tune(r, kv):
    fn = r.lib.r3n_internal_set_tuning
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    assert fn(r.ctx, kv.encode()) == 0, r.lib.r3n_last_error(r.ctx)


def frame(r3, r, hdr, w, h, tonemaps=1, expect=0):
    """one frame whose HDR target is `hdr` ((h, w, 4) half bits): begin, r3n_hdr_write, r3n_tonemap x tonemaps, end"""
    from rend3_amd import _ffi
    lib = r.lib
    hdr = np.ascontiguousarray(hdr, dtype=np.uint16).reshape(w * h, 4)
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (w, h))
    clear = np.zeros(4, dtype=f32)
    assert lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), w, h, 1, _ffi.ptr(clear), 32, 32) == 0
    assert lib.r3n_hdr_write(r.ctx, _ffi.ptr(hdr), 0, w * h) == 0
    for _ in range(tonemaps):
        assert lib.r3n_tonemap(r.ctx, None, 0) == expect
    assert lib.r3n_frame_end(r.ctx) == 0


def output(r, w, h, floats=True):
    from rend3_amd import _ffi
    got8 = np.zeros((w * h, 4), dtype=np.uint8)
    gotf = np.zeros((w * h, 4), dtype=f32) if floats else None
    assert r.lib.r3n_readback_output(r.ctx, _ffi.ptr(got8), _ffi.ptr(gotf)) == 0
    return got8, gotf


def readback_hdr(r, w, h):
    from rend3_amd import _ffi
    hdr = np.zeros((h, w, 4), dtype=np.uint16)
    assert r.lib.r3n_readback_hdr(r.ctx, _ffi.ptr(hdr)) == 0
    return hdr


def check_output(got8, gotf, want8, wantf, output_format, what):
    bad = np.nonzero((got8 != want8).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got8[bad[:5]], want8[bad[:5]])
    if gotf is not None:
        assert np.allclose(gotf, wantf, rtol=0, atol=2e-7 if output_format < 2 else 1e-6, equal_nan=True), what


def check_pyramid(r, d, a, what, kept=True):
    n = r.bloom_levels()
    assert n == len(a), what
    for k in range(n):
        got = r.readback_bloom(k)
        assert got.shape == a[k].shape, (what, k)
        bad = np.argwhere(got != a[k])
        assert len(bad) == 0, (what, "a", k, len(bad), bad[:4], got[tuple(bad[0])], a[k][tuple(bad[0])])
        if kept:
            got = r.readback_bloom(n + k)
            bad = np.argwhere(got != d[k])
            assert len(bad) == 0, (what, "d", k, len(bad), bad[:4], got[tuple(bad[0])], d[k][tuple(bad[0])])


# ------------------------------------------------------------------ the targets
SPECIAL = np.array([[0x7E00, ONE, ONE, ONE], [0xFC00, 0x4000, 0, ONE], [0x7C00, 0, 0, ONE], [0xBC00, 0xC000, 0x8000, ONE], [0x7BFF, 0x7BFF, 0x7BFF, ONE],
                    [0x7C00, 0x7C00, 0x7C00, ONE], [0xFE00, 0xFE00, 0xFE00, ONE], [1, 1, 1, ONE],
                    [28172, 29170, 29170, ONE]], dtype=np.uint16)  # NaN, -inf, inf, negatives, max, ...; the last: at 1.37 EV the bright pass's
# product is 16004.0003, f32 16004, a tie of the half grid (16000): a product folded into its conversion would give 16008


def random_target(w, h, seed):
    """random halves over +-14 octaves, 5 % zeros, and a block of NaN / inf / negative pixels where the size allows"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 4), dtype=np.uint16)
    img[..., :3] = (np.exp2(rng.uniform(-14, 14, (h, w, 1))) * rng.uniform(0.1, 1.0, (h, w, 3))).astype(np.float16).view(np.uint16)
    img[..., 3] = ONE
    img[rng.random((h, w)) < 0.05, :3] = 0
    flat = img.reshape(-1, 4)
    if w * h >= 4 * len(SPECIAL):
        bw = min(w, 4)
        for i in range(2 * len(SPECIAL)):  # a block bw wide somewhere inside
            x, y = w // 3 + i % bw, h // 3 + i // bw
            if x < w and y < h:
                img[y, x] = SPECIAL[i % len(SPECIAL)]
    else:
        flat[::3] = SPECIAL[np.arange(len(flat[::3])) % len(SPECIAL)]
    return img


def impulse_target(w, h):
    """the impulse set of tests/test_bloom.py: every corner and the middle of every edge, on black"""
    img = np.zeros((h, w, 4), dtype=np.uint16)
    img[..., 3] = ONE
    for k, (x, y) in enumerate([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)]):
        img[y, x, :3] = np.array([64.0 * (k + 1), 3.0, 1000.0], dtype=np.float64).astype(np.float16).view(np.uint16)
    return img


# (65, 33): one texel past the 32 x 16 destination tile of the tiled down kernel in each direction; (257, 131): several workgroups
# both ways with odd extents at every level; (1024, 600): levels on both sides of every plan's tail
SIZES = [(1, 1), (2, 1), (2, 2), (3, 3), (5, 3), (17, 9), (64, 64), (65, 33), (257, 131), (1024, 600)]
TONEMAP = T.default_opts(op=2, exposure_ev=1.37)
BLOOM = B.default_opts(intensity=0.3, threshold=1.0, knee=0.5, scatter=0.7)


@functools.lru_cache(maxsize=None)
def reference(w, h, kind, max_levels):
    img = random_target(w, h, 1000 + w * 7 + h) if kind == "random" else impulse_target(w, h)
    d, a = B.pyramid(img, T.exp2_lin(TONEMAP["exposure_ev"]), dict(BLOOM, max_levels=max_levels))
    for lvl in d + a:
        lvl.setflags(write=False)
    img.setflags(write=False)
    return img, d, a


# ------------------------------------------------------------------ 1. the pyramid, word for word, under every plan
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_bits_under_every_plan(r3, size):
    w, h = size
    r = r3.Renderer(oh.LEFT)
    assert set_tonemap(r, TONEMAP) == 0
    launches = {}
    for tail in (None, 0, TAIL_ALL):  # (the default first: the context is fresh)
        tune(r, "bloom_keep_down=1" + (f" bloom_tail={tail}" if tail is not None else ""))
        for max_levels in (1, 2, 16):
            assert set_bloom(r, dict(BLOOM, max_levels=max_levels)) == 0
            for kind in ("random", "impulses"):
                img, d, a = reference(w, h, kind, max_levels)
                r.stage_times(reset=True)
                frame(r3, r, img, w, h)
                launches[(tail, max_levels)] = r.stage_times(reset=True)["tonemap"][1]
                check_pyramid(r, d, a, (size, tail, max_levels, kind))
    n16 = len(B.levels(w, h, 16))
    assert launches[(0, 16)] == 2 * n16, "bloom_tail=0: one launch per level down, one per level up, the operator"
    assert launches[(0, 1)] == 2
    if sum(lw * lh for lw, lh in B.levels(w, h, 16)) * 8 <= 160 * 1024:
        assert launches[(TAIL_ALL, 16)] == 2, "every level in the tail: one launch, and the operator"
    if size == (1024, 600):  # 10 levels; the tail starts at level 2 (128 x 75 and below fit the LDS) / at level 3 (64 x 38 <= 4096 texels)
        assert launches[(TAIL_ALL, 16)] == 2 + 1 + 2 + 1 and launches[(None, 16)] == 3 + 1 + 3 + 1
    # in place (the default): the same up chain, and the down chain is not there to be read
    tune(r, "bloom_keep_down=0")
    assert set_bloom(r, dict(BLOOM, max_levels=16)) == 0
    img, d, a = reference(w, h, "random", 16)
    frame(r3, r, img, w, h)
    check_pyramid(r, d, a, (size, "in place"), kept=False)
    from rend3_amd import _ffi
    assert r.lib.r3n_readback_bloom(r.ctx, len(a), None, 0, None, None, None) == ERR_INVALID_ARG
    small = np.zeros(3, dtype=np.uint16)
    if a[0].size > 3:
        assert r.lib.r3n_readback_bloom(r.ctx, 0, _ffi.ptr(small), 1, None, None, None) == ERR_INVALID_ARG
    r.close()


# ------------------------------------------------------------------ 2. output bytes and float view
@pytest.mark.parametrize("output_format", [0, 1, 2, 3])
def test_output_bytes_and_float_view(r3, output_format):
    """3 operators x MANUAL and AUTO on a target that spans several workgroups with odd extents; the float tap twice"""
    w, h = 257, 131
    img = random_target(w, h, 77)
    hist, _ = T.histogram(img.reshape(-1, 4))
    r = r3.Renderer(oh.LEFT)
    r.set_output_format(output_format)
    o = dict(BLOOM, max_levels=6)
    assert set_bloom(r, o) == 0
    for op, white in ((0, 4.0), (1, 0.75), (2, 4.0)):
        for ev in (0.0, 1.37, "auto"):
            if ev == "auto":
                t = T.default_opts(op=op, white=white, exposure_mode=1, exposure_ev=-0.5)
                scale = T.step(T.INVALID, hist, t)["scale"]
            else:
                t = T.default_opts(op=op, white=white, exposure_ev=ev)
                scale = T.exp2_lin(ev)
            # (BLIT, MANUAL, 0 EV) is "no options": bloom alone then runs the operator path as BLIT at scale 1
            assert set_tonemap(r, t) == 0
            frame(r3, r, img, w, h)
            want8, wantf, (d, a) = B.render(img, scale, op, output_format, o, white)
            assert (want8 != T.tonemap(img.reshape(-1, 4), scale, op, output_format, white)[0]).any(), "the case must show bloom"
            got8, gotf = output(r, w, h)
            check_output(got8, gotf, want8, wantf, output_format, (op, white, ev))
            check_pyramid(r, d, a, (op, ev), kept=False)
            again8, againf = output(r, w, h)  # the float tap re-runs the operator over the stored pyramid, never the chain
            assert np.array_equal(again8, got8) and np.array_equal(againf.view(np.uint32), gotf.view(np.uint32))
            check_pyramid(r, d, a, (op, ev, "after the float tap"), kept=False)
            assert r.readback_exposure()["scale"] == scale
    r.close()


def test_odd_width_pairs_that_straddle_rows(r3):
    """an odd width: every other row starts at an odd pixel index, so pairs straddle row ends and start at odd x"""
    for (w, h) in ((5, 3), (17, 9), (1, 7), (7, 1)):
        img = random_target(w, h, 5 + w)
        r = r3.Renderer(oh.LEFT)
        o = dict(BLOOM, max_levels=16, intensity=1.0)
        assert set_bloom(r, o) == 0  # no tonemap options: BLIT at scale 1
        frame(r3, r, img, w, h)
        want8, wantf, _ = B.render(img, f32(1.0), 0, 0, o)
        check_output(*output(r, w, h), want8, wantf, 0, (w, h))
        r.close()


# ------------------------------------------------------------------ 3. off means off
def test_off_means_off(r3):
    w, h = 130, 67
    img = random_target(w, h, 91)
    dim = img.copy()  # wholly below threshold - knee after the exposure
    with np.errstate(all="ignore"):
        dim[..., :3] = np.minimum(B.halves(img[..., :3]), f32(0.2)).clip(0).astype(np.float16).view(np.uint16)
    for t in (None, T.default_opts(op=2, exposure_ev=1.0), T.default_opts(op=1, exposure_mode=1)):
        r = r3.Renderer(oh.LEFT)
        assert set_tonemap(r, t) == 0

        def shot(image):
            assert set_tonemap(r, t) == 0  # restarts the adaptation: every shot meters from scratch
            r.stage_times(reset=True)
            frame(r3, r, image, w, h)
            n = r.stage_times(reset=True)["tonemap"][1]
            return output(r, w, h, floats=False)[0], n

        base8, base_n = shot(img)
        assert base_n == (1 if t is None or t["exposure_mode"] == 0 else 3)
        assert set_bloom(r, dict(BLOOM)) == 0
        on8, on_n = shot(img)
        assert on_n > base_n and (on8 != base8).any()
        r.set_bloom(None)
        got8, n = shot(img)
        assert np.array_equal(got8, base8) and n == base_n, "set_bloom(None)"
        assert r.lib.r3n_readback_bloom(r.ctx, 0, None, 0, None, None, None) == ERR_STATE
        assert set_bloom(r, dict(BLOOM)) == 0
        assert set_bloom(r, dict(BLOOM, intensity=0.0)) == 0
        got8, n = shot(img)
        assert np.array_equal(got8, base8) and n == base_n, "intensity = 0"
        # an image wholly below the knee: the chain runs, the pyramid is zero, no byte changes
        dim8, dim_n = shot(dim)
        assert set_bloom(r, dict(BLOOM, threshold=8.0, knee=2.0) if t is None or t["exposure_mode"] == 0 else dict(BLOOM, threshold=60000.0, knee=0.0)) == 0
        got8, n = shot(dim)
        assert n > dim_n and np.array_equal(got8, dim8)
        for k in range(r.bloom_levels()):
            assert not r.readback_bloom(k).any()
        r.close()


# ------------------------------------------------------------------ 4. state and refusals
def test_state_and_refusals(r3):
    from rend3_amd import _ffi
    w, h = 64, 40
    img = random_target(w, h, 13)
    r = r3.Renderer(oh.LEFT)
    assert r.lib.r3n_readback_bloom(r.ctx, 0, None, 0, None, None, None) == ERR_STATE, "before any bloom frame"
    good = dict(BLOOM, max_levels=3)
    assert set_bloom(r, good) == 0
    assert r.lib.r3n_readback_bloom(r.ctx, 0, None, 0, None, None, None) == ERR_STATE, "set, but no frame yet"
    nan, inf = float("nan"), float("inf")
    bad = [dict(intensity=nan), dict(threshold=nan), dict(knee=nan), dict(scatter=nan), dict(intensity=-0.5), dict(intensity=1025.0), dict(intensity=inf),
           dict(threshold=-1.0), dict(threshold=65536.0), dict(threshold=inf), dict(knee=-0.1), dict(knee=1.5), dict(scatter=-0.1), dict(scatter=1.5),
           dict(max_levels=0), dict(max_levels=17), dict(intensity=0.0, scatter=nan), dict(intensity=0.0, max_levels=0)]
    for over in bad:
        assert set_bloom(r, dict(good, **over)) == ERR_INVALID_ARG, over
    assert b"bloom_set" in r.lib.r3n_last_error(r.ctx)
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (w, h))
    clear = np.zeros(4, dtype=f32)
    assert r.lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), w, h, 1, _ffi.ptr(clear), 32, 32) == 0
    assert set_bloom(r, dict(BLOOM)) == ERR_STATE and set_bloom(r, None) == ERR_STATE, "inside a frame"
    assert r.lib.r3n_frame_end(r.ctx) == 0
    with pytest.raises(ValueError):
        r.set_bloom(0.1, knee=2.0)
    # nothing changed: the options are still `good`
    frame(r3, r, img, w, h)
    want8, wantf, (d, a) = B.render(img, f32(1.0), 0, 0, good)
    assert r.bloom_levels() == 3
    check_output(*output(r, w, h), want8, wantf, 0, "after the refusals")
    assert np.array_equal(readback_hdr(r, w, h), img), "the HDR target is never written"
    # a partial row range: refused, nothing launched, nothing written
    before8, _ = output(r, w, h, floats=False)
    assert r.lib.r3n_set_row_range(r.ctx, 1, 3) == 0
    r.stage_times(reset=True)
    frame(r3, r, img[::-1].copy(), w, h, expect=ERR_UNSUPPORTED)
    assert r.stage_times(reset=True)["tonemap"][1] == 0
    assert np.array_equal(output(r, w, h, floats=False)[0], before8)
    assert r.lib.r3n_set_row_range(r.ctx, 0, 0xFFFFFFFF) == 0
    # the target grows, then shrinks: the pyramid follows, the bits are right
    for (w2, h2) in ((257, 131), (33, 17), (64, 40)):
        img2 = random_target(w2, h2, w2)
        assert set_bloom(r, dict(BLOOM, max_levels=16)) == 0
        frame(r3, r, img2, w2, h2)
        want8, wantf, (d, a) = B.render(img2, f32(1.0), 0, 0, dict(BLOOM, max_levels=16))
        check_output(*output(r, w2, h2), want8, wantf, 0, (w2, h2))
        check_pyramid(r, d, a, (w2, h2), kept=False)
        assert np.array_equal(readback_hdr(r, w2, h2), img2)
    r.close()


# ------------------------------------------------------------------ 5. frames in flight
@pytest.mark.parametrize("multi_stream", [0, 1])
def test_four_frames_in_flight(r3, multi_stream):
    """four frames with different targets, AUTO exposure with adapt < 1: every frame's output and exposure state is the
    reference's, stepped in frame order -- the one pyramid is never shared between frames"""
    w, h = 200, 90
    t = T.default_opts(op=2, exposure_mode=1, adapt=0.5, exposure_ev=0.25)
    o = dict(BLOOM, max_levels=5)
    imgs = []
    for k in range(4):
        img = random_target(w, h, 300 + k)
        with np.errstate(all="ignore"):
            img[..., :3] = (B.halves(img[..., :3]) * f32(2.0 ** (2 * k - 3))).astype(np.float16).view(np.uint16)
        imgs.append(img)
    r = r3.Renderer(oh.LEFT)
    assert r.lib.r3n_set_multi_stream(r.ctx, multi_stream) == 0
    assert set_tonemap(r, t) == 0 and set_bloom(r, o) == 0
    st, want = dict(T.INVALID), []
    for img in imgs:
        st = T.step(st, T.histogram(img.reshape(-1, 4))[0], t)
        want.append((dict(st), B.render(img, st["scale"], 2, 0, o)))
    assert len({T.state_words(s)[3] for s, _ in want}) == 4, "the exposure moves in every frame"
    # every frame checked as it is enqueued behind the one before (the read-back waits for it alone)
    for k, img in enumerate(imgs):
        frame(r3, r, img, w, h)
        state, (want8, wantf, (d, a)) = want[k]
        assert T.state_words(r.readback_exposure()) == T.state_words(state), k
        check_output(*output(r, w, h), want8, wantf, 0, ("frame", k))
        check_pyramid(r, d, a, ("frame", k), kept=False)
    # the same four again without a wait in between: the last one's results, stepped through all eight
    for img in imgs:
        st = T.step(st, T.histogram(img.reshape(-1, 4))[0], t)
        frame(r3, r, img, w, h)
    want8, wantf, (d, a) = B.render(imgs[3], st["scale"], 2, 0, o)
    assert T.state_words(r.readback_exposure()) == T.state_words(st)
    check_output(*output(r, w, h), want8, wantf, 0, "eighth frame")
    check_pyramid(r, d, a, "eighth frame", kept=False)
    r.close()


# ------------------------------------------------------------------ 6. one rendered frame
@pytest.mark.parametrize("samples", [1, 4])
def test_rendered_frame_with_an_hdr_sky(r3, samples):
    """a lit scene in front of an HDR cube: the output is the reference applied to that frame's HDR target, which bloom leaves as
    it is without bloom; frames rendered in flight agree; back at the default nothing runs after the resolve"""
    w, h, n = 320, 192, 8
    rng = np.random.default_rng(53)
    faces = [[(rng.random((n * n, 4)) * np.array([30.0, 20.0, 40.0, 1.0])).astype(np.float16).tobytes()] for _ in range(6)]
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    scenes.build_random_scene(p, oh, r3.material_record, 60, 0xE0E0, lights=1)
    p.set_background_texture(p.add_texture_cube_encoded(C.RGBA16F, n, faces))
    p.set_camera_data(oh.look_at_lh((3.0, 2.0, -6.0), (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))
    kw = dict(ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0), samples=samples)
    first = p.render(w, h, **kw)
    p.set_tonemapping("aces", exposure_ev=-1.0)
    plain = p.render(w, h, **kw)
    assert np.array_equal(plain["hdr16"], first["hdr16"])
    o = dict(BLOOM, max_levels=6)
    p.set_bloom(o["intensity"], o["threshold"], o["knee"], o["scatter"], o["max_levels"])
    got = p.render(w, h, **kw)
    assert np.array_equal(got["hdr16"], first["hdr16"]), "r3n_readback_hdr shows the same bits with bloom on or off"
    hdr = got["hdr16"].reshape(h, w, 4)
    assert (B.halves(hdr[..., :3]) * f32(0.5) > 1.0).mean() > 0.01, "the sky must be brighter than display white"
    want8, wantf, (d, a) = B.render(hdr, T.exp2_lin(-1.0), 2, 0, o)
    assert np.array_equal(got["rgba8"].reshape(-1, 4), want8)
    assert (got["rgba8"] != plain["rgba8"]).any()
    check_pyramid(p, d, a, "rendered", kept=False)
    for _ in range(3):  # in flight
        p.render(w, h, readback=False, **kw)
    check_output(*output(p, w, h), want8, wantf, 0, "in flight")
    p.set_bloom(None)
    p.set_tonemapping()
    p.stage_times(reset=True)
    p.render(w, h, readback=False, **kw)
    assert p.stage_times(reset=True)["tonemap"][1] == 0, "nothing is launched after a resolve"
    again = p.render(w, h, **kw)
    assert np.array_equal(again["rgba8"], first["rgba8"]) and np.array_equal(again["hdr16"], first["hdr16"])
    p.close()
