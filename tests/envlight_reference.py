"""Environment lights (DESIGN.md section 2 "Environment lights", include/r3n.h r3n_environment_lights) restated in numpy: float32
in the order rend3_amd/csrc/envlight_rule.h writes, Python integers for everything that is summed, Python floats (IEEE double) for
the few f64 steps.  tests/test_envlight.py holds it to the header, word for word, and to independent float64 evaluations;
tests/test_envlight_gpu.py holds the kernels to it."""
import math

import numpy as np

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
MAX_LIGHTS, MAX_EXTENT, W_SCALE_EXP, SHIFT_STEPS = 16, 1024, 44, 2
WEIGHTS = (13933, 46871, 4732)
FOUR_PI = 12.566370614359172
F32_MAX = float(np.finfo(np.float32).max)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(u32)


def word(x):
    """the bits of one float32, as a Python int"""
    return int(bits(x).reshape(-1)[0])


def isum(a):
    """exact sum of an array of non-negative integers below 2^64, as a Python int"""
    a = np.asarray(a, dtype=u64).reshape(-1)
    return (int(np.sum(a >> u64(32), dtype=u64)) << 32) + int(np.sum(a & u64(0xFFFFFFFF), dtype=u64))


# ---------------------------------------------------------------- 1. texel quantities, arrays of shape (6, n, n) indexed [f, j, i]
def geometry(n):
    """u (6, n, n, 3) and w (6, n, n), float32"""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    fn = f32(n)
    sc = (2 * i + 1 - n).astype(f32) / fn
    tc = (2 * j + 1 - n).astype(f32) / fn
    one = np.ones_like(sc)
    d = np.stack([np.stack(v, -1) for v in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one))], 0)
    r2 = (f32(1) + sc * sc) + tc * tc
    r = np.sqrt(r2)
    u = (d / r[None, :, :, None]).astype(f32)
    w = f32(4) / ((fn * fn) * (r2 * r))
    assert u.dtype == f32 and w.dtype == f32
    return u, np.broadcast_to(w, (6, n, n)).copy()


def sanitise(c):
    c = np.asarray(c, dtype=f32)
    with np.errstate(invalid="ignore"):
        return np.where((c > 0) & (c <= f32(F32_MAX)), c, f32(0)).astype(f32)


def luminance(rgb):
    with np.errstate(over="ignore"):
        return (f32(0.2126) * rgb[..., 0] + f32(0.7152) * rgb[..., 1]) + f32(0.0722) * rgb[..., 2]


# ---------------------------------------------------------------- 2. order-free sums
def exp_field(b):
    x = (np.asarray(b, dtype=u32) >> u32(23)) & u32(255)
    return np.maximum(x, u32(1)).astype(np.int64)


def shifted_mantissa(b, places):
    b = np.asarray(b, dtype=u32)
    x = (b >> u32(23)) & u32(255)
    m = ((b & u32(0x7FFFFF)) | np.where(x != 0, u32(0x800000), u32(0))).astype(u64)
    places = np.asarray(places, dtype=np.int64)
    left = m << np.clip(places, 0, 40).astype(u64)
    right = np.where(places > -64, m >> np.clip(-places, 0, 63).astype(u64), u64(0))
    return np.where(places >= 0, left, right).astype(u64)


def scale_exp_of(emax_bits):
    return 166 - int(exp_field(emax_bits)) if emax_bits else 0


def quantise(e_bits, emax_bits):
    return shifted_mantissa(e_bits, 16 + exp_field(e_bits) - int(exp_field(emax_bits)))


def quantise_w(w):
    b = bits(w)
    return shifted_mantissa(b, exp_field(b) - 150 + W_SCALE_EXP)


def energy(q):
    return (u64(WEIGHTS[0]) * q[..., 0] + u64(WEIGHTS[1]) * q[..., 1] + u64(WEIGHTS[2]) * q[..., 2]) >> u64(16)


def dir_q(u):
    x = np.asarray(u, dtype=f32) * f32(32767.0)
    return np.where(x < 0, -np.trunc(f32(0.5) - x).astype(np.int64), np.trunc(x + f32(0.5)).astype(np.int64))


# ---------------------------------------------------------------- 3. peaks
def dot3(u, c):
    c = np.asarray(c, dtype=f32)
    return (u[..., 0] * c[0] + u[..., 1] * c[1]) + u[..., 2] * c[2]


def shifted(old, s):
    v = [float(s[c]) * 1048576.0 + float(s[3 + c]) for c in range(3)]
    len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    if not len2 > 0.0:
        return np.asarray(old, dtype=f32)
    ln = math.sqrt(len2)
    return np.array([f32(v[0] / ln), f32(v[1] / ln), f32(v[2] / ln)], dtype=f32)


def share_floor(min_share):
    return int(float(f32(min_share)) * 4294967296.0)


def emits(cone_qy, total_qy, share):
    return cone_qy != 0 and not ((cone_qy << 32) < share * total_qy)


# ---------------------------------------------------------------- 4. outputs
def scaled(total, scale_exp):
    v = float(total) * 2.0 ** -scale_exp
    return f32(F32_MAX) if v > F32_MAX else f32(v)


def ambient_of(total, scale_exp):
    v = (float(total) * 2.0 ** -scale_exp) / FOUR_PI
    return f32(F32_MAX) if v > F32_MAX else f32(v)


def sums_of(q, qy, qw, mask):
    return {"q": [isum(q[..., c][mask]) for c in range(3)], "qy": isum(qy[mask]), "qw": isum(qw[mask]), "texels": int(np.count_nonzero(mask))}


ZERO_SUMS = {"q": [0, 0, 0], "qy": 0, "qw": 0, "texels": 0}


def extract(rgb, max_lights, cone_cos, min_share):
    """rgb: (6, n, n, 3) decoded float32 radiance, not sanitised.  Returns the state and the outputs as one dict; `masks` (the texels
    of every emitted light) rides along for the tests."""
    rgb = np.asarray(rgb, dtype=f32)
    n = rgb.shape[1]
    assert rgb.shape == (6, n, n, 3) and 1 <= n <= MAX_EXTENT and 0 <= max_lights <= MAX_LIGHTS
    cone_cos = f32(cone_cos)
    share = share_floor(min_share)
    u, w = geometry(n)
    c = sanitise(rgb)
    e_bits = bits(c * w[..., None])
    emax_bits = int(e_bits.max())
    st = {"n": n, "emax_bits": emax_bits, "total": dict(ZERO_SUMS), "seed": [0] * (MAX_LIGHTS + 1), "shift": [[[0] * 6 for _ in range(SHIFT_STEPS)] for _ in range(MAX_LIGHTS)],
          "light": [dict(ZERO_SUMS) for _ in range(MAX_LIGHTS)], "masks": []}
    dirs = []
    if emax_bits:
        q = quantise(e_bits, emax_bits)
        qy = energy(q)
        qw = quantise_w(w)
        lum = luminance(c)
        index = np.arange(6 * n * n, dtype=u64).reshape(6, n, n)
        keys = (bits(lum).astype(u64) << u64(32)) | (~index & u64(0xFFFFFFFF))
        dq = dir_q(u)
        hi, lo = (qy >> u64(20)).astype(np.int64), (qy & u64(0xFFFFF)).astype(np.int64)
        everything = np.ones((6, n, n), dtype=bool)
        st["total"] = sums_of(q, qy, qw, everything)
        st["seed"][0] = int(keys.max())
        live = everything.copy()
        for k in range(max_lights):
            if st["seed"][k] >> 32 == 0:
                break
            seed = ~st["seed"][k] & 0xFFFFFFFF
            centre = u.reshape(-1, 3)[seed]
            for step in range(SHIFT_STEPS):
                m = live & (dot3(u, centre) >= cone_cos)
                st["shift"][k][step] = [int(np.sum(hi[m] * dq[..., a][m])) for a in range(3)] + [int(np.sum(lo[m] * dq[..., a][m])) for a in range(3)]
                centre = shifted(centre, st["shift"][k][step])
            m = live & (dot3(u, centre) >= cone_cos)
            st["light"][k] = sums_of(q, qy, qw, m)
            rest = live & ~m
            st["seed"][k + 1] = int(keys[rest].max()) if rest.any() else 0
            if not emits(st["light"][k]["qy"], st["total"]["qy"], share):
                break
            dirs.append(centre)
            st["masks"].append(m)
            live = rest
    # outputs
    n_lights = len(dirs)
    st["n_lights"] = n_lights
    st["ran"] = n_lights + (1 if emax_bits and n_lights < max_lights and st["seed"][n_lights] >> 32 else 0)
    st["scale_exp"] = scale_exp_of(emax_bits)
    rem = {k: (list(v) if isinstance(v, list) else v) for k, v in st["total"].items()}
    st["lights"] = []
    for k in range(n_lights):
        l = st["light"][k]
        st["lights"].append({"direction": dirs[k], "solid_angle": scaled(l["qw"], W_SCALE_EXP), "irradiance": [scaled(l["q"][a], st["scale_exp"]) for a in range(3)],
                             "texels": l["texels"], "seed": ~st["seed"][k] & 0xFFFFFFFF})
        rem = {"q": [rem["q"][a] - l["q"][a] for a in range(3)], "qy": rem["qy"] - l["qy"], "qw": rem["qw"] - l["qw"], "texels": rem["texels"] - l["texels"]}
    st["remainder"] = rem
    st["ambient"] = [ambient_of(rem["q"][a], st["scale_exp"]) if emax_bits else f32(0) for a in range(3)] + [f32(1)]
    return st


def _flat_sums(s):
    return list(s["q"]) + [s["qy"], s["qw"], s["texels"]]


def flat(st):
    """the integers tests/envlight_rule_check.cpp prints for `extract`, in its order"""
    out = [st["emax_bits"]] + _flat_sums(st["total"]) + list(st["seed"])
    for k in range(MAX_LIGHTS):
        out += [v for step in st["shift"][k] for v in step] + _flat_sums(st["light"][k])
    out += [st["n_lights"], st["ran"], st["scale_exp"]] + [word(a) for a in st["ambient"]] + _flat_sums(st["remainder"])
    for k in range(MAX_LIGHTS):
        if k < st["n_lights"]:
            l = st["lights"][k]
            out += [int(b) for b in bits(l["direction"])] + [word(l["solid_angle"])] + [word(a) for a in l["irradiance"]] + [l["texels"]]
        else:
            out += [0] * 8
    return out


def result_struct(st):
    """the r3n_env_lights_result the library returns for this extraction (rend3_amd._ffi.EnvLightsResult)"""
    from rend3_amd import _ffi
    r = _ffi.EnvLightsResult()

    def put(dst, s):
        for a in range(3):
            dst.q[a] = s["q"][a]
        dst.qy, dst.qw, dst.texels = s["qy"], s["qw"], s["texels"]

    r.n_lights, r.scale_exp, r.extent, r.emax_bits = st["n_lights"], st["scale_exp"], st["n"], st["emax_bits"]
    for a in range(4):
        r.ambient[a] = float(st["ambient"][a])
    put(r.total, st["total"])
    put(r.remainder, st["remainder"])
    for k in range(MAX_LIGHTS + 1):
        r.seeds[k] = st["seed"][k]
    for k in range(st["ran"]):
        l = r.lights[k]
        l.seed = ~st["seed"][k] & 0xFFFFFFFF
        for step in range(SHIFT_STEPS):
            for a in range(6):
                l.shift[step][a] = st["shift"][k][step][a]
        put(l.sums, st["light"][k])
        if k < st["n_lights"]:
            o = st["lights"][k]
            for a in range(3):
                l.direction[a] = float(o["direction"][a])
                l.irradiance[a] = float(o["irradiance"][a])
            l.solid_angle, l.texels = float(o["solid_angle"]), o["texels"]
    return r


# ---------------------------------------------------------------- worlds shared by the CPU and the GPU tests
def directions64(n):
    """unit directions of the texel centres in float64, independent of geometry(): (6, n, n, 3)"""
    j, i = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    sc, tc = (2 * i + 1 - n) / n, (2 * j + 1 - n) / n
    one = np.ones_like(sc)
    d = np.stack([np.stack(v, -1) for v in ((one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one))], 0)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def solid_angles64(n):
    """float64 solid angle of every texel by the centre rule 4 / (n^2 r^3), (6, n, n)"""
    j, i = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    sc, tc = (2 * i + 1 - n) / n, (2 * j + 1 - n) / n
    return np.broadcast_to(4.0 / (n * n * (1 + sc * sc + tc * tc) ** 1.5), (6, n, n)).copy()


SUNS = (((0.3, 0.8, 0.5), 3.0, 5000.0), ((-1.0, 0.2, -0.4), 4.0, 300.0))


def sky(n, suns=SUNS):
    """radiance 1 + 0.5 u.y on every channel, and discs (axis, radius in degrees, radiance) on top: (6, n, n, 3) float32"""
    d = directions64(n)
    lum = 1.0 + 0.5 * d[..., 1]
    for axis, radius, value in suns:
        a = np.asarray(axis, dtype=np.float64)
        a /= np.linalg.norm(a)
        lum = np.where(d @ a > math.cos(math.radians(radius)), value, lum)
    return np.repeat(lum[..., None], 3, axis=-1).astype(f32)
