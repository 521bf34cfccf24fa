"""The bloom contract (DESIGN.md section 2 "Bloom", include/r3n.h r3n_bloom_set) restated in numpy, independent of the product:
level by level, f32 in the pinned order, one rounding per operation, every stored texel rounded to half (nearest even).  Exposure,
operators and the transfer are tests/tonemap_reference.py's: with a zero pyramid `render` is `tonemap_reference.tonemap`."""
import numpy as np

import tonemap_reference as T

f32 = np.float32
MAX_HALF = T.MAX_HALF
MAX_LEVELS = 16


def default_opts(**kw):
    """r3n_bloom_opts as a dict, Renderer.set_bloom's defaults"""
    o = dict(intensity=0.04, threshold=1.0, knee=0.5, scatter=0.7, max_levels=8)
    o.update(kw)
    return o


def constants(o):
    """(lo, k2, inv): computed once, in f32"""
    threshold, knee = f32(o["threshold"]), f32(o["knee"])
    return f32(threshold - knee), f32(f32(2.0) * knee), (f32(f32(0.25) / knee) if knee > 0 else f32(0.0))


def levels(W, H, max_levels):
    """[(w, h)] of the levels: ((W + 1) / 2, (H + 1) / 2), halved again (rounding up) until the larger side is 1 or max_levels"""
    out, w, h = [], W, H
    while len(out) < min(max_levels, MAX_LEVELS):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if max(w, h) == 1:
            break
    return out


def halves(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(f32)


def to_half_bits(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=f32).astype(np.float16).view(np.uint16)


def exposed(hdr, scale):
    """(H, W, 4) half bits -> (H, W, 3) f32: h * scale; NaN, zero and negatives become 0; capped at 65504"""
    with np.errstate(all="ignore"):
        v = halves(np.asarray(hdr, dtype=np.uint16)[..., :3]) * f32(scale)
        return np.where(v > 0, np.where(v >= MAX_HALF, MAX_HALF, v), f32(0)).astype(f32)


def bright_pass(hdr, scale, o):
    """(H, W, 4) half bits -> (H, W, 3) half bits of the virtual bright-pass image"""
    lo, k2, inv = constants(o)
    v = exposed(hdr, scale)
    m = np.maximum(v[..., 0], np.maximum(v[..., 1], v[..., 2]))
    s = np.minimum(np.maximum(m - lo, f32(0)), k2)
    q = (s * s) * inv
    e = np.maximum(q, m - f32(o["threshold"]))
    w = e / np.maximum(m, f32(2.0 ** -14))
    assert w.dtype == f32
    return to_half_bits(v * w[..., None])


def down(src_bits):
    """one down step: (h, w, 3) half bits -> ((h + 1) / 2, (w + 1) / 2, 3) half bits; 4x4 tent, rows first"""
    s = halves(src_bits)
    h, w = s.shape[:2]
    dw, dh = (w + 1) // 2, (h + 1) // 2
    cx = [np.clip(2 * np.arange(dw) - 1 + i, 0, w - 1) for i in range(4)]
    cy = [np.clip(2 * np.arange(dh) - 1 + i, 0, h - 1) for i in range(4)]
    three = f32(3.0)
    r = (s[:, cx[0]] + three * s[:, cx[1]]) + (three * s[:, cx[2]] + s[:, cx[3]])
    d = ((r[cy[0]] + three * r[cy[1]]) + (three * r[cy[2]] + r[cy[3]])) * f32(1.0 / 64.0)
    assert d.dtype == f32
    return to_half_bits(d)


def upsample(coarse_bits, w, h):
    """the 2x tent up-sample of (ch, cw, 3) half bits to w x h, f32 (not rounded to half)"""
    a = halves(coarse_bits)
    ch, cw = a.shape[:2]
    assert (cw, ch) == ((w + 1) // 2, (h + 1) // 2)
    x, y = np.arange(w), np.arange(h)
    xn, xf = x >> 1, np.clip((x >> 1) + np.where(x & 1, 1, -1), 0, cw - 1)
    yn, yf = y >> 1, np.clip((y >> 1) + np.where(y & 1, 1, -1), 0, ch - 1)
    with np.errstate(all="ignore"):
        hrow = f32(3.0) * a[:, xn] + a[:, xf]
        u = (f32(3.0) * hrow[yn] + hrow[yf]) * f32(1.0 / 16.0)
    assert u.dtype == f32
    return u


def up(d_bits, coarse_bits, scatter):
    """a_k = half(d_k + scatter * up(a_{k+1}))"""
    h, w = d_bits.shape[:2]
    with np.errstate(all="ignore"):
        return to_half_bits(halves(d_bits) + f32(scatter) * upsample(coarse_bits, w, h))


def pyramid(hdr, scale, o):
    """hdr: (H, W, 4) half bits.  -> (d, a): lists of (h_k, w_k, 3) half bits, the down chain and the up chain"""
    hdr = np.asarray(hdr, dtype=np.uint16)
    H, W = hdr.shape[:2]
    n = len(levels(W, H, o["max_levels"]))
    d = [down(bright_pass(hdr, scale, o))]
    for _ in range(1, n):
        d.append(down(d[-1]))
    assert [(x.shape[1], x.shape[0]) for x in d] == levels(W, H, o["max_levels"])
    a = [None] * n
    a[n - 1] = d[n - 1].copy()
    for k in range(n - 2, -1, -1):
        a[k] = up(d[k], a[k + 1], o["scatter"])
    return d, a


def composited_halves(hdr, scale, op, o, a0, white=4.0):
    """(H, W, 4) half bits -> (H * W, 4) half bits: exposed, bloom added, capped, operated, rounded to half; alpha unchanged"""
    hdr = np.asarray(hdr, dtype=np.uint16)
    H, W = hdr.shape[:2]
    v = exposed(hdr, scale)
    with np.errstate(all="ignore"):
        v = np.minimum(v + f32(o["intensity"]) * upsample(a0, W, H), MAX_HALF).astype(f32)
    out = hdr.reshape(-1, 4).copy()
    with np.errstate(all="ignore"):
        out[:, :3] = T.operate(v.reshape(-1, 3), f32(1.0), op, white).astype(np.float16).view(np.uint16)  # (v is exposed already: x 1, clamp: no-ops)
    return out


def render(hdr, scale, op, output_format, o, white=4.0, a0=None):
    """what r3n_tonemap shows with bloom `o` (None, or intensity 0: off): (bytes (n, 4) uint8, float view (n, 4) f32, (d, a))"""
    hdr = np.asarray(hdr, dtype=np.uint16)
    if o is None or f32(o["intensity"]) == 0:
        return T.tonemap(hdr.reshape(-1, 4), scale, op, output_format, white) + (None,)
    pyr = pyramid(hdr, scale, o) if a0 is None else None
    a0 = pyr[1][0] if a0 is None else a0
    return T.transfer(composited_halves(hdr, scale, op, o, a0, white), output_format) + (pyr,)
