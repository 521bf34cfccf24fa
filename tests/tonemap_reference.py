"""The exposure / tonemapping-operator contract (DESIGN.md section 2 "Exposure and tonemapping operators", include/r3n.h
r3n_tonemap_set) restated in numpy, independent of the product: f32 in the order written, one rounding per operation, the metering
in Python integers, the 256-bin loops plain Python.  The only borrowed piece is the oracle's r3o_tonemap_format for the transfer
(blit.wgsl + the 8-bit store), so only the rule and the two rational operators are restated here."""
import math

import numpy as np

f32 = np.float32
BINS = 256
OPS = {"blit": 0, "reinhard": 1, "aces": 2}
MAX_HALF = f32(65504.0)

# Lq[j]: nearest integer to log2 of the bin's middle, in 1/65536 steps; E[k] = (float)2^(k/256)
LQ = [int(round(((j >> 3) - 16 + math.log2(1.0 + ((j & 7) + 0.5) / 8.0)) * 65536.0)) for j in range(BINS)]
E = np.exp2(np.arange(257, dtype=np.float64) / 256.0).astype(f32)


def default_opts(**kw):
    """r3n_tonemap_opts as a dict, every field valid."""
    o = dict(op=0, exposure_mode=0, exposure_ev=0.0, white=4.0, key_log2=math.log2(0.18), min_ev=-16.0, max_ev=16.0, adapt=1.0,
             low_permille=500, high_permille=950)
    o.update(kw)
    return o


def halves_f32(u16):
    return np.asarray(u16, dtype=np.uint16).view(np.float16).astype(f32)


def luminance(hdr):
    """hdr: (n, 4) uint16 half bits -> f32 luminance, (0.2126 r + 0.7152 g) + 0.0722 b"""
    c = halves_f32(np.asarray(hdr, dtype=np.uint16).reshape(-1, 4))
    with np.errstate(all="ignore"):
        return (f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]) + f32(0.0722) * c[:, 2]


def bins_of(lum):
    """bin per luminance; -1: excluded (NaN, zero, negative)"""
    lum = np.asarray(lum, dtype=f32)
    with np.errstate(invalid="ignore"):
        counted = lum > 0
    b = np.clip((lum.view(np.uint32) >> 20).astype(np.int64) - 888, 0, BINS - 1)
    return np.where(counted, b, -1)


def histogram(hdr):
    """(256 counts, excluded) of an HDR image"""
    b = bins_of(luminance(hdr))
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32), int((b < 0).sum())


def meter(hist, o):
    """(S, N): the clipped integer sum over ranks [lo, hi) and its count"""
    total = sum(int(n) for n in hist)
    lo, hi = total * o["low_permille"] // 1000, total * o["high_permille"] // 1000
    s, c = 0, 0
    for j in range(BINS):
        c1 = c + int(hist[j])
        s += max(0, min(c1, hi) - max(c, lo)) * LQ[j]
        c = c1
    return s, hi - lo


def exp2_lin(e):
    e = f32(e)
    i = f32(math.floor(e))
    f = f32(e - i)
    t = f32(f * f32(256.0))
    k = int(t)
    w = f32(t - f32(k))
    m = f32(E[k] + f32(f32(E[min(k + 1, 256)] - E[k]) * w))
    return f32(np.ldexp(m, int(i)))


def clamp(v, lo, hi):
    v, lo, hi = f32(v), f32(lo), f32(hi)
    return lo if v < lo else (hi if v > hi else v)


INVALID = dict(valid=0, mean_log2=f32(0), target_ev=f32(0), current_ev=f32(0), scale=f32(1))


def step(prev, hist, o):
    """the state after one metered frame, from the state the previous frame committed"""
    s, n = meter(hist, o)
    if n == 0:
        if prev["valid"]:
            return dict(prev)
        ev = clamp(o["exposure_ev"], o["min_ev"], o["max_ev"])
        return dict(valid=0, mean_log2=f32(0), target_ev=ev, current_ev=ev, scale=exp2_lin(ev))
    mean = f32(float(s) / (float(n) * 65536.0))
    target = clamp(f32(f32(f32(o["key_log2"]) - mean) + f32(o["exposure_ev"])), o["min_ev"], o["max_ev"])
    if not prev["valid"] or f32(o["adapt"]) == f32(1):
        cur = target
    else:
        cur = f32(prev["current_ev"] + f32(f32(target - prev["current_ev"]) * f32(o["adapt"])))
    return dict(valid=1, mean_log2=mean, target_ev=target, current_ev=cur, scale=exp2_lin(cur))


def state_words(st):
    """the five words of r3n_exposure_state behind `excluded`, as uint32"""
    return [int(st["valid"])] + [int(np.asarray(st[k], dtype=f32).view(np.uint32)) for k in ("mean_log2", "target_ev", "current_ev", "scale")]


def operate(values, scale, op, white=4.0):
    """f32 channel values -> exposed, clamped, operated f32 (before the rounding to half)"""
    x = np.asarray(values, dtype=f32)
    with np.errstate(all="ignore"):
        v = x * f32(scale)
        v = np.where(v > 0, np.where(v >= MAX_HALF, MAX_HALF, v), f32(0)).astype(f32)
        if op == OPS["reinhard"]:
            white_sq = f32(f32(white) * f32(white))
            return ((v * (f32(1) + v / white_sq)) / (f32(1) + v)).astype(f32)
        if op == OPS["aces"]:
            return ((v * (f32(2.51) * v + f32(0.03))) / (v * (f32(2.43) * v + f32(0.59)) + f32(0.14))).astype(f32)
        return v


def operated_halves(hdr, scale, op, white=4.0):
    """(n, 4) half bits in -> (n, 4) half bits out: colour exposed / operated / rounded to half (RNE), alpha unchanged"""
    hdr = np.asarray(hdr, dtype=np.uint16).reshape(-1, 4)
    out = hdr.copy()
    with np.errstate(all="ignore"):
        out[:, :3] = operate(halves_f32(hdr[:, :3]), scale, op, white).astype(np.float16).view(np.uint16)
    return out


def transfer(halves, output_format):
    """the oracle's blit + 8-bit store of (n, 4) half bits: (bytes (n, 4) uint8, float view (n, 4) f32)"""
    from oracle import lib as olib
    o = olib.get()
    halves = np.ascontiguousarray(halves, dtype=np.uint16).reshape(-1, 4)
    n = len(halves)
    out8, outf = np.zeros((n, 4), dtype=np.uint8), np.zeros((n, 4), dtype=f32)
    o.r3o_tonemap_format(o.ptr(halves), n, o.ptr(outf), o.ptr(out8), output_format)
    return out8, outf


def tonemap(hdr, scale, op, output_format, white=4.0):
    return transfer(operated_halves(hdr, scale, op, white), output_format)
