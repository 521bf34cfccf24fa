"""GPU: the luminance histogram, the metering step and the operator kernels behind r3n_tonemap_set (rend3_amd/csrc/exposure.hip)
against tests/tonemap_reference.py -- counts and state words bit for bit, output bytes byte for byte, the float view within the
tolerances of test_gpu_parity.py::test_tonemap_every_half_value (the same transfer function).  HDR targets are injected with
r3n_hdr_write; the last test renders real frames.  The reference itself is tied to the oracle in tests/test_tonemap_ops.py."""
import ctypes

import numpy as np
import pytest

import scenes
import tonemap_reference as T
from oracle import host as oh
from rend3_amd import containers as C

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
ALL_HALVES = np.arange(65536, dtype=np.uint16)
ONE = 0x3C00


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def c_opts(o):
    from rend3_amd import _ffi
    c = _ffi.TonemapOpts()
    for k, v in o.items():
        setattr(c, k, v)
    return c


def set_opts(r, o):
    return r.lib.r3n_tonemap_set(r.ctx, ctypes.byref(c_opts(o)) if o is not None else None)


def frame(r3, r, hdr, w, h, tonemaps=1, expect=0):
    """one frame whose HDR target is `hdr` ((w * h, 4) half bits): begin, r3n_hdr_write, r3n_tonemap x tonemaps, end"""
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


def words(st):
    return T.state_words(st)


def grey(levels):
    """(n, 4) half bits: r = g = b = the half nearest to each level, alpha 1"""
    x = np.asarray(levels, dtype=np.float64).astype(np.float16).view(np.uint16)
    return np.stack([x, x, x, np.full_like(x, ONE)], axis=1)


def every_half_image():
    return np.stack([ALL_HALVES, ALL_HALVES[::-1], np.roll(ALL_HALVES, 12345), ALL_HALVES], axis=1).copy()


def edge_pool():
    """grey pixels whose f32 luminance is exactly a bin edge, or one ulp below one"""
    h = np.arange(1, 0x7C00, dtype=np.uint16)
    px = np.stack([h, h, h, np.full_like(h, ONE)], axis=1)
    low = T.luminance(px).view(np.uint32) & 0xFFFFF
    on, below = px[low == 0], px[low == 0xFFFFF]
    assert len(on) > 100 and len(below) > 20
    return np.concatenate([on, below])


# ------------------------------------------------------------------ 1. the histogram
def histogram_targets():
    rng = np.random.default_rng(41)

    def rand(n, spread=14.0):
        px = np.zeros((n, 4), dtype=np.uint16)
        px[:, :3] = (np.exp2(rng.uniform(-spread, spread, (n, 1))) * rng.uniform(0.1, 1.0, (n, 3))).astype(np.float16).view(np.uint16)
        px[:, 3] = ONE
        px[rng.random(n) < 0.05, :3] = 0
        return px

    def tiled(px, n):
        return px[np.arange(n) % len(px)]

    excluded = np.array([[0, 0, 0, ONE], [0x8000, 0x8000, 0x8000, ONE], [0xBC00, 0xBC00, 0xBC00, ONE], [0x7E00, 0, 0, ONE],
                         [0xFC00, 0, 0, ONE], [0x7C00, 0xFC00, 0, ONE]], dtype=np.uint16)  # 0, -0, -1, NaN, -inf, inf - inf
    limits = np.concatenate([grey([2.0 ** -17, 2.0 ** -20, 6e-8, 2.0 ** -16, 65504.0, 40000.0]),
                             np.array([[0x7C00, 0x7C00, 0x7C00, ONE], [0x7BFF, 0x7BFF, 0x7BFF, ONE], [1, 1, 1, ONE], [0, 1, 0, ONE]], dtype=np.uint16)])
    return {
        "1x1": (1, 1, rand(1)), "2x1": (2, 1, rand(2)), "3x1": (3, 1, rand(3)), "255x3": (255, 3, rand(765)), "513x3": (513, 3, rand(1539)),
        "every half": (256, 256, every_half_image()[rng.permutation(65536)]),
        "one bin": (512, 512, tiled(grey([0.4]), 512 * 512)),
        "1024x600": (1024, 600, rand(1024 * 600)),
        "only excluded": (64, 5, tiled(excluded, 320)),
        "bin edges": (97, 7, tiled(edge_pool(), 679)),
        "limits": (33, 3, tiled(limits, 99)),
    }


TARGETS = histogram_targets()


@pytest.mark.parametrize("name", list(TARGETS))
def test_histogram_and_excluded_count(r3, name):
    """every pixel lands in the reference's bin: waves whose lanes share a bin (one add of the lane count), mixed waves, pair tails"""
    w, h, hdr = TARGETS[name]
    want, want_excluded = T.histogram(hdr)
    assert int(want.sum()) + want_excluded == w * h
    if name == "one bin":
        assert (want > 0).sum() == 1 and want_excluded == 0
    if name == "only excluded":
        assert want.sum() == 0
    if name == "limits":
        assert want[0] >= 4 and want[255] >= 3
    r = r3.Renderer(oh.LEFT)
    o = T.default_opts(exposure_mode=1, op=2)
    assert set_opts(r, o) == 0
    for _ in range(2):  # twice: the counters are left zero for the next frame
        frame(r3, r, hdr, w, h)
        st = r.readback_exposure()
        assert np.array_equal(st["histogram"], want), np.nonzero(st["histogram"] != want)[0][:8]
        assert st["excluded"] == want_excluded
    assert words(st) == words(T.step(T.INVALID, want, o))
    r.close()


# ------------------------------------------------------------------ 2. the state over a sequence
SEQ_W, SEQ_H = 100, 30


def sequence_frames():
    """six frames of 3000 pixels.  0: mid greys; 1: very bright (the target falls below min_ev); 2: three bins holding 1500 / 1350 /
    150 pixels, so that ranks [500, 950) permille begin and end exactly on a cumulative count; 3: nothing to meter; 4: very dark
    (the target rises above max_ev); 5: a wide mix"""
    rng = np.random.default_rng(43)
    n = SEQ_W * SEQ_H
    f0 = grey(np.exp2(rng.uniform(-3, 1, n)))
    f1 = grey(np.exp2(rng.uniform(9, 12, n)))
    f2 = grey(np.repeat([0.03, 0.3, 5.0], [1500, 1350, 150]))[rng.permutation(n)]
    f3 = np.zeros((n, 4), dtype=np.uint16)
    f4 = grey(np.exp2(rng.uniform(-15, -12, n)))
    f5 = grey(np.exp2(rng.uniform(-10, 4, n)))
    f5[::7, :3] = 0
    return [f0, f1, f2, f3, f4, f5]


@pytest.mark.parametrize("adapt", [1.0, 0.5, 0.05])
def test_state_words_over_a_sequence(r3, adapt):
    frames = sequence_frames()
    o = T.default_opts(exposure_mode=1, op=1, adapt=adapt, min_ev=-6.0, max_ev=7.5, exposure_ev=0.25)
    c2 = np.cumsum(T.histogram(frames[2])[0])
    assert 1500 in c2 and 2850 in c2, "frame 2: the rank window must begin and end on a cumulative count"
    r = r3.Renderer(oh.LEFT)
    assert set_opts(r, o) == 0
    st = dict(T.INVALID)
    hit_min = hit_max = 0
    for k, hdr in enumerate(frames):
        hist, excluded = T.histogram(hdr)
        prev = st
        st = T.step(prev, hist, o)
        frame(r3, r, hdr, SEQ_W, SEQ_H)
        got = r.readback_exposure()
        assert np.array_equal(got["histogram"], hist) and got["excluded"] == excluded, k
        assert words(got) == words(st), (k, got, st)
        if k == 0:
            assert st["current_ev"] == st["target_ev"], "the first frame adapts instantly"
        if k == 3:
            assert hist.sum() == 0 and words(st) == words(prev), "nothing to meter: the state is held"
        elif k > 0 and adapt < 1.0:
            assert st["current_ev"] != st["target_ev"]
        hit_min += st["target_ev"] == f32(o["min_ev"]) and k != 3
        hit_max += st["target_ev"] == f32(o["max_ev"]) and k != 3
    assert (hit_min, hit_max) == (1, 1)
    r.close()


# ------------------------------------------------------------------ 3. output bytes and float view
def check_output(got8, gotf, want8, wantf, output_format, what, rows=None):
    if rows is not None:
        got8, gotf, want8, wantf = got8[rows], gotf[rows], want8[rows], wantf[rows]
    bad = np.nonzero((got8 != want8).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), got8[bad[:5]], want8[bad[:5]])
    assert np.allclose(gotf, wantf, rtol=0, atol=2e-7 if output_format < 2 else 1e-6, equal_nan=True), what


@pytest.mark.parametrize("output_format", [0, 1, 2, 3])
def test_output_bytes_and_float_view(r3, output_format):
    """3 operators x MANUAL stops {0, -2.5, 1.37} and AUTO, on the image that holds every half in every channel"""
    w = h = 256
    hdr = every_half_image()
    hist, _ = T.histogram(hdr)
    r = r3.Renderer(oh.LEFT)
    r.set_output_format(output_format)
    for op, white in ((0, 4.0), (1, 4.0), (1, 0.75), (2, 4.0)):
        for ev in (0.0, -2.5, 1.37, "auto"):
            if ev == "auto":
                o = T.default_opts(op=op, white=white, exposure_mode=1, exposure_ev=-0.5)
                scale = T.step(T.INVALID, hist, o)["scale"]
            else:
                o = T.default_opts(op=op, white=white, exposure_ev=ev)
                scale = T.exp2_lin(ev)
            assert set_opts(r, o) == 0
            r.stage_times(reset=True)
            frame(r3, r, hdr, w, h)
            launches = r.stage_times(reset=True)["tonemap"][1]
            assert launches == (3 if ev == "auto" else 1), "histogram + step + operator, or the operator (or the plain blit) alone"
            got8, gotf = output(r, w, h)
            want8, wantf = T.tonemap(hdr, scale, op, output_format, white)
            check_output(got8, gotf, want8, wantf, output_format, (op, white, ev))
            assert r.readback_exposure()["scale"] == scale
    r.close()


def test_manual_on_a_partial_row_range(r3):
    """width 255, rows [1, 3): the first pixel is odd, so every pair takes the scalar loads; rows outside keep what they held"""
    w, h = 255, 4
    rng = np.random.default_rng(47)
    hdr = every_half_image()[rng.permutation(65536)[:w * h]]
    r = r3.Renderer(oh.LEFT)
    frame(r3, r, hdr, w, h)
    before8, _ = output(r, w, h, floats=False)
    assert np.array_equal(before8, T.transfer(hdr, 0)[0])
    o = T.default_opts(op=2, exposure_ev=1.37)
    assert set_opts(r, o) == 0
    assert r.lib.r3n_set_row_range(r.ctx, 1, 3) == 0
    frame(r3, r, hdr, w, h)
    got8, gotf = output(r, w, h)
    want8, wantf = T.tonemap(hdr, T.exp2_lin(1.37), 2, 0)
    inside = np.zeros(w * h, dtype=bool)
    inside[w:3 * w] = True
    check_output(got8, gotf, want8, wantf, 0, "rows [1, 3)", rows=inside)
    assert np.array_equal(got8[~inside], before8[~inside])
    assert (got8[inside] != before8[inside]).any()
    # AUTO meters the whole target: refused under a split, nothing launched, nothing written
    assert set_opts(r, T.default_opts(op=2, exposure_mode=1)) == 0
    r.stage_times(reset=True)
    frame(r3, r, hdr, w, h, expect=ERR_UNSUPPORTED)
    assert r.stage_times(reset=True)["tonemap"][1] == 0
    assert np.array_equal(output(r, w, h, floats=False)[0], got8)
    assert r.lib.r3n_set_row_range(r.ctx, 0, 0xFFFFFFFF) == 0
    frame(r3, r, hdr, w, h)
    assert r.readback_exposure()["valid"] == 1
    r.close()


# ------------------------------------------------------------------ 4. idempotence
def test_second_tonemap_and_second_readback_change_nothing(r3):
    w, h = SEQ_W, SEQ_H
    frames = sequence_frames()
    o = T.default_opts(exposure_mode=1, op=2, adapt=0.5)
    r = r3.Renderer(oh.LEFT)
    assert set_opts(r, o) == 0
    st = T.step(T.INVALID, T.histogram(frames[0])[0], o)
    frame(r3, r, frames[0], w, h)
    assert words(r.readback_exposure()) == words(st)
    st = T.step(st, T.histogram(frames[5])[0], o)
    assert st["current_ev"] != st["target_ev"]
    frame(r3, r, frames[5], w, h, tonemaps=2)  # the second node of the frame repeats the step, it does not take another
    got = r.readback_exposure()
    assert words(got) == words(st) and np.array_equal(got["histogram"], T.histogram(frames[5])[0])
    want8, wantf = T.tonemap(frames[5], st["scale"], 2, 0)
    for _ in range(2):  # the float tap re-runs the operator with the stored exposure and never meters again
        got8, gotf = output(r, w, h)
        check_output(got8, gotf, want8, wantf, 0, "read-back")
        assert words(r.readback_exposure()) == words(st)
    st = T.step(st, T.histogram(frames[0])[0], o)
    frame(r3, r, frames[0], w, h)
    assert words(r.readback_exposure()) == words(st), "the next frame steps from the state that frame committed"
    r.close()


# ------------------------------------------------------------------ 5. real frames
@pytest.mark.parametrize("multi_stream", [True, False], ids=["lanes", "one stream"])
def test_lit_frames_in_flight(r3, multi_stream):
    """a lit scene in front of an HDR cube, four frames with a moving camera enqueued without a wait in between: the state after
    the fourth is the reference's over the four HDR targets (taken from a first, waited run of the same frames), its output the
    reference's of its HDR target; back at the default the blit is the oracle's again and nothing runs after the resolve"""
    w, h, n = 320, 192, 8
    rng = np.random.default_rng(53)
    faces = [[(rng.random((n * n, 4)) * np.array([30.0, 20.0, 40.0, 1.0])).astype(np.float16).tobytes()] for _ in range(6)]
    p = r3.Renderer(oh.LEFT, f32(w) / f32(h))
    p.set_multi_stream(multi_stream)
    scenes.build_random_scene(p, oh, r3.material_record, 60, 0xE0E0, lights=1)
    p.set_background_texture(p.add_texture_cube_encoded(C.RGBA16F, n, faces))
    eyes = [(3.0, 2.0, -6.0), (2.0, 2.5, -7.0), (0.0, 6.0, -5.0), (-2.0, 1.0, -6.5)]
    kw = dict(ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))

    def look(eye):
        p.set_camera_data(oh.look_at_lh(eye, (0, 0, 4), (0, 1, 0)), ("perspective", 60.0, 0.1))

    look(eyes[0])
    first = p.render(w, h, **kw)
    assert np.array_equal(first["rgba8"].reshape(-1, 4), T.transfer(first["hdr16"], 0)[0])
    o = T.default_opts(exposure_mode=1, op=2, adapt=0.5, exposure_ev=0.5)
    assert set_opts(p, o) == 0
    hdrs = []
    for eye in eyes:  # waited run: each frame's HDR target
        look(eye)
        hdrs.append(p.render(w, h, **kw)["hdr16"].reshape(-1, 4).copy())
    assert (T.halves_f32(hdrs[0][:, :3]) > 1.0).mean() > 0.01, "the sky must be brighter than the blit can show"
    st, states = dict(T.INVALID), []
    for hdr in hdrs:
        st = T.step(st, T.histogram(hdr)[0], o)
        states.append(st)
    assert len({words(s)[3] for s in states}) == 4, "the exposure moves in every frame"
    assert words(p.readback_exposure()) == words(st)
    assert set_opts(p, o) == 0  # restarts the adaptation
    p.stage_times(reset=True)
    for eye in eyes:  # the same four frames, in flight
        look(eye)
        p.render(w, h, readback=False, **kw)
    got = p.readback_exposure()
    assert p.stage_times(reset=True)["tonemap"][1] == 12
    assert words(got) == words(st) and np.array_equal(got["histogram"], T.histogram(hdrs[3])[0])
    hdr_now = np.zeros((w * h, 4), dtype=np.uint16)
    from rend3_amd import _ffi
    assert p.lib.r3n_readback_hdr(p.ctx, _ffi.ptr(hdr_now)) == 0
    assert np.array_equal(hdr_now, hdrs[3])
    got8, gotf = output(p, w, h)
    want8, wantf = T.tonemap(hdr_now, st["scale"], 2, 0)
    check_output(got8, gotf, want8, wantf, 0, "fourth frame")
    p.set_tonemapping()  # the default: the reference's behaviour
    look(eyes[0])
    p.stage_times(reset=True)
    p.render(w, h, readback=False, **kw)
    assert p.stage_times(reset=True)["tonemap"][1] == 0, "nothing is launched after a resolve"
    again = p.render(w, h, **kw)
    assert np.array_equal(again["rgba8"], first["rgba8"]) and np.array_equal(again["hdr16"], first["hdr16"])
    p.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing(r3):
    w, h = SEQ_W, SEQ_H
    frames = sequence_frames()
    good = T.default_opts(exposure_mode=1, op=1, adapt=0.5)
    nan = float("nan")
    bad = [dict(op=3), dict(exposure_mode=2), dict(exposure_ev=nan), dict(white=nan), dict(key_log2=nan), dict(min_ev=nan), dict(max_ev=nan),
           dict(adapt=nan), dict(white=0.0), dict(white=-1.0), dict(white=65536.0), dict(low_permille=950, high_permille=950),
           dict(low_permille=960, high_permille=950), dict(high_permille=1001), dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5),
           dict(min_ev=2.0, max_ev=1.0), dict(exposure_ev=33.0), dict(min_ev=-33.0), dict(max_ev=40.0), dict(key_log2=float("inf"))]
    r = r3.Renderer(oh.LEFT)
    from rend3_amd import _ffi
    assert set_opts(r, good) == 0
    st = T.step(T.INVALID, T.histogram(frames[0])[0], good)
    frame(r3, r, frames[0], w, h)
    for over in bad:
        # a MANUAL option set is validated field by field too
        assert set_opts(r, T.default_opts(**dict(good, **over))) == ERR_INVALID_ARG, over
        assert set_opts(r, T.default_opts(**dict(dict(good, exposure_mode=0), **over))) == ERR_INVALID_ARG, over
    assert b"tonemap_set" in r.lib.r3n_last_error(r.ctx)
    # inside a frame
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (w, h))
    clear = np.zeros(4, dtype=f32)
    assert r.lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), w, h, 1, _ffi.ptr(clear), 32, 32) == 0
    assert set_opts(r, T.default_opts(op=2)) == ERR_STATE and set_opts(r, None) == ERR_STATE
    assert r.lib.r3n_frame_end(r.ctx) == 0
    # nothing changed: the options are still `good` and the adaptation was not restarted -- the next frame takes half a step
    st = T.step(st, T.histogram(frames[5])[0], good)
    assert st["current_ev"] != st["target_ev"]
    frame(r3, r, frames[5], w, h)
    assert words(r.readback_exposure()) == words(st)
    got8, _ = output(r, w, h, floats=False)
    assert np.array_equal(got8, T.tonemap(frames[5], st["scale"], 1, 0)[0])
    with pytest.raises(r3.R3nError):
        r.set_tonemapping("reinhard", white=0.0)
    with pytest.raises(ValueError):
        r.set_tonemapping("filmic")
    # a valid set restarts the adaptation: the next frame adapts instantly
    assert set_opts(r, good) == 0
    frame(r3, r, frames[0], w, h)
    assert words(r.readback_exposure()) == words(T.step(T.INVALID, T.histogram(frames[0])[0], good))
    r.close()
