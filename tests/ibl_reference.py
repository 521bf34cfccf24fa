"""The environment prefilter (DESIGN.md section 2 "Environment prefilter", include/r3n.h r3n_environment_prefilter) restated in
numpy: float32 in the order rend3_amd/csrc/ibl_rule.h writes, every sum through the header's tree (per source row in ascending i,
the rows of a face in ascending j, the six faces in order), and the two lookups of rend3_amd/csrc/ibl_lookup.h.  The same functions
take dtype=float64 and then evaluate the same formulas FROM THE SAME float32 INPUTS in double: the yardstick of the header's error
bound.  tests/test_ibl.py holds this file to the header, word for word; tests/test_ibl_gpu.py holds the kernels to it."""
import numpy as np

import envlight_reference as E
import skybox_lod_reference as lodref

f32 = np.float32
MAX_EXTENT, MAX_LEVELS, SH_EXTENT = 256, 16, 32
F32_CLASS = 33  # a format id of the float class, for skybox_lod_reference.sample
Y00, Y1, Y2A, Y20, Y22 = f32(0.282095), f32(0.488603), f32(1.092548), f32(0.315392), f32(0.546274)
BAND = [f32(1.0)] + [f32(0.6666667)] * 3 + [f32(0.25)] * 5


def level_extent(S, k):
    return max(1, S >> k)


def max_levels(S, stored):
    return min(S.bit_length(), stored, MAX_LEVELS)


def sh_level(S, L):
    return next((k for k in range(L) if level_extent(S, k) <= SH_EXTENT), L - 1)


def roughness(k, L):
    r = f32(k) / f32(L - 1)
    a = r * r
    a2 = a * a
    return a2, f32(1) - a2


def tree_sum(terms):
    """(..., 6, n, n) indexed [f, j, i] -> (...): the header's tree, in the dtype of `terms`"""
    n = terms.shape[-1]
    row = np.zeros(terms.shape[:-1], dtype=terms.dtype)
    for i in range(n):
        row = row + terms[..., i]
    face = np.zeros(row.shape[:-1], dtype=terms.dtype)
    for j in range(n):
        face = face + row[..., j]
    total = np.zeros(face.shape[:-1], dtype=terms.dtype)
    for f in range(6):
        total = total + face[..., f]
    return total


def prefilter_level(rgb, k, L, dtype=f32, chunk=256, pick=None):
    """result level k >= 1 from ONE source level rgb (6, n, n, 3) float32, decoded, not sanitised -> (6, n, n, 4) of `dtype`.
    pick: linear indices of the output texels wanted -> (len(pick), 4): every one still integrates the whole source level"""
    rgb = np.asarray(rgb, dtype=f32)
    n = rgb.shape[1]
    u32_, w32 = E.geometry(n)
    a2, oma = roughness(k, L)
    u, w, c = u32_.astype(dtype), w32.astype(dtype), E.sanitise(rgb).astype(dtype)
    a2, oma = dtype(a2), dtype(oma)
    N = u.reshape(-1, 3) if pick is None else u.reshape(-1, 3)[np.asarray(pick)]
    out = np.ones((len(N), 4), dtype=dtype)
    two, half, quarter, one = dtype(2), dtype(0.5), dtype(0.25), dtype(1)
    with np.errstate(over="ignore", invalid="ignore"):
        for at in range(0, len(N), chunk):
            Nc = N[at:at + chunk]
            dx = Nc[:, 0, None, None, None] - u[None, ..., 0]
            dy = Nc[:, 1, None, None, None] - u[None, ..., 1]
            dz = Nc[:, 2, None, None, None] - u[None, ..., 2]
            q = (dx * dx + dy * dy) + dz * dz
            cs = one - q * half
            d = a2 + (q * quarter) * oma
            wt = np.where(q < two, (cs * w[None]) / (d * d), dtype(0)).astype(dtype)
            den = tree_sum(wt)
            for ch in range(3):
                out[at:at + chunk, ch] = tree_sum(wt * c[None, ..., ch]) / den
    assert out.dtype == dtype
    return out.reshape(6, n, n, 4) if pick is None else out


def prefilter(levels_rgb, dtype=f32):
    """levels_rgb[k]: source level k, (6, n_k, n_k, 3) float32 -> the result's levels, (6, n_k, n_k, 4)"""
    L = len(levels_rgb)
    first = np.ones(levels_rgb[0].shape[:3] + (4,), dtype=dtype)
    first[..., :3] = levels_rgb[0]
    return [first] + [prefilter_level(levels_rgb[k], k, L, dtype) for k in range(1, L)]


def basis(u):
    """(..., 3) -> (..., 9), in the dtype of u"""
    t = u.dtype.type
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    return np.stack([np.full(x.shape, t(Y00), dtype=u.dtype), t(Y1) * y, t(Y1) * z, t(Y1) * x, (t(Y2A) * x) * y, (t(Y2A) * y) * z,
                     t(Y20) * (((t(3) * z) * z) - t(1)), (t(Y2A) * x) * z, t(Y22) * (x * x - y * y)], axis=-1)


def sh9(rgb, dtype=f32, absolute=False):
    """the nine coefficients of one level (6, n, n, 3): (9, 3) of `dtype`; absolute: the sums of |term| instead"""
    rgb = np.asarray(rgb, dtype=f32)
    n = rgb.shape[1]
    u, w = E.geometry(n)
    u, w, c = u.astype(dtype), w.astype(dtype), E.sanitise(rgb).astype(dtype)
    wy = w[..., None] * basis(u)  # (6, n, n, 9)
    out = np.zeros((9, 3), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(9):
            for ch in range(3):
                terms = c[..., ch] * wy[..., m]
                out[m, ch] = tree_sum(np.abs(terms) if absolute else terms)
    return out


def irradiance(sh, n, dtype=f32):
    """E(n) / pi: sh (9, 3+), n (count, 3) -> (count, 3)"""
    sh, n = np.asarray(sh, dtype=f32).astype(dtype), np.asarray(n, dtype=f32).astype(dtype)
    Y = basis(n)
    out = np.zeros((len(n), 3), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(9):
            out = out + (dtype(BAND[m]) * sh[m, :3])[None, :] * Y[:, m, None]
    return out


def lod_of(roughness_, mips):
    """level, fraction of ibl_specular: float32"""
    top = f32(mips - 1)
    with np.errstate(invalid="ignore"):
        lod = np.asarray(roughness_, dtype=f32) * top
        lod = np.where(lod > 0, lod, f32(0)).astype(f32)
        lod = np.where(lod > top, top, lod).astype(f32)
    level = lod.astype(np.int64)
    return level, (lod - level.astype(f32)).astype(f32)


def specular(levels, d, roughness_):
    """ibl_specular on the levels of a float-class cube ((6, n_k, n_k, 4) each): (count, 3) float32, level, fraction"""
    level, frac = lod_of(roughness_, len(levels))
    return lodref.sample(levels, F32_CLASS, np.asarray(d, dtype=f32), level, frac)[:, :3], level, frac


# ---------------------------------------------------------------- inputs
def nasty(levels):
    """plants every kind of texel the rule must survive into source levels (a list of (6, n, n, 3) arrays), in place"""
    for lv in levels:
        flat = lv.reshape(-1, 3)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 1e-45, 1e-39, 1e30, 0.0, -0.0)):
            flat[(k * 7 + 3) % len(flat), k % 3] = v
    return levels


def random_levels(S, L, seed, octaves=6.0):
    """unrelated random radiance on every level: the rule reads each stored level as it is"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(L):
        n = level_extent(S, k)
        out.append((np.exp2(rng.uniform(-octaves, octaves, (6, n, n, 1))) * rng.uniform(0.05, 1.0, (6, n, n, 3))).astype(f32))
    return out
