"""numpy restatement of the skybox contract for cubes with mip chains and float texels ("Skybox: levels"),
the judge of tests/test_skybox_lod_gpu.py.  Built on tests/skybox_reference.py: steps 1-4, the face table, resolve_texel, the
footprint and the texel fetch with its corner rule are imported from there; the level rule is tests/sampler_queries.py's lod()
(tex_footprint's, with W = H = N).  What is stated here is what is new:

 gradients   dx, dy = the directions of the pixel centres (x + 1, y) and (x, y + 1) by steps 1-3 (also outside the target).  A
             neighbour direction e is projected onto d's face with d's row of the cube table -- the same axis and sign, not
             re-selected from e: m_e = the signed component of e along that axis; !(m_e > 0) -> the footprint is unbounded: level =
             mips - 1, frac = 0; else s_e = 0.5 * (sc_e / m_e) + 0.5, t_e likewise.  ddx = (s_dx - s, t_dx - t), ddy likewise.
 level       lod(N, N, mips, ddx, ddy); a one-level cube is level 0, frac 0 whatever the gradients are.
 filter      the seamless bilinear of skybox_reference on level `level` with n = max(1, N >> level); frac > 0: the same on level + 1
             and a * (1 - frac) + b * frac per channel.  RGBA8 classes decode through the table before filtering, the f32 class
             reads r, g, b as stored.  Alpha 1.  Rounded to half.

Texels per (face, level) come from the ORACLE's decoders (oracle/bcn.c), not from the product."""
import numpy as np

import skybox_reference as sky
from sampler_queries import lod

f32 = np.float32
SRGB_FORMATS = (1, 5, 7, 9, 11, 15)  # R3N_TEXTURE_*_SRGB: RGBA8, BGRA8, BC1, BC2, BC3, BC7


def is_float(fmt):
    return 16 <= fmt < 34  # R3N_TEXTURE_R8_SNORM .. : decoded to four f32 per texel


def level_extent(width, k):
    return max(1, width >> k)


def decode_cube(fmt, width, faces):
    """faces[f][k] = encoded bytes -> levels[k] = (6, n_k, n_k, 4) uint8 (RGBA8 classes) or float32 (f32 class)"""
    from oracle import lib as olib
    c = olib.get().c
    levels = []
    for k in range(len(faces[0])):
        n = level_extent(width, k)
        out = np.zeros((6, n, n, 4), dtype=f32 if is_float(fmt) else np.uint8)
        for f in range(6):
            src = np.ascontiguousarray(np.frombuffer(bytes(faces[f][k]), dtype=np.uint8))
            assert c.r3o_texture_level_bytes(fmt, n, n) == len(src), "level byte count"
            dec = c.r3o_texture_decode_level_f32 if is_float(fmt) else c.r3o_texture_decode_level
            assert dec(fmt, n, n, src.ctypes.data, out[f].ctypes.data) == 0
        levels.append(out)
    return levels


def bordered_face(level, f):
    """(n + 2, n + 2, 4) of face f of one decoded level: the interior, and across every edge the texel resolve_texel names; the
    second result marks the four corner positions, which hold no texel"""
    n = level.shape[1]
    by, bx = np.mgrid[0:n + 2, 0:n + 2]
    i, j = (bx - 1).reshape(-1), (by - 1).reshape(-1)
    out_i, out_j = (i < 0) | (i >= n), (j < 0) | (j >= n)
    corner = out_i & out_j
    ci, cj = np.where(corner, np.clip(i, 0, n - 1), i), np.where(corner, np.clip(j, 0, n - 1), j)
    nf, ni, nj = sky.resolve_texel(np.full(len(i), f), ci, cj, n)
    return level[nf, nj, ni].reshape(n + 2, n + 2, level.shape[-1]), corner.reshape(n + 2, n + 2)


class _AsStored:
    """the f32 class's "decode table": a texel's channels are used as they are"""

    def __getitem__(self, v):
        return v


def project(face, e):
    """a neighbour direction e (n, 3) on the GIVEN face: (sc, tc, m) by that face's row of the cube table"""
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    neg = (face & 1) == 1
    is_z, is_y = face >= 4, (face >= 2) & (face < 4)
    sc = np.where(is_z, np.where(neg, -x, x), np.where(is_y, x, np.where(neg, z, -z)))
    tc = np.where(is_z, -y, np.where(is_y, np.where(neg, -z, z), -y))
    m = np.where(is_z, np.where(neg, -z, z), np.where(is_y, np.where(neg, -y, y), np.where(neg, -x, x)))
    return sc.astype(f32), tc.astype(f32), m.astype(f32)


def select_level(inv_origin_view_proj, width, height, xs, ys, n, mips):
    """per pixel: d, level, frac, unbounded, rho"""
    xs, ys = np.asarray(xs), np.asarray(ys)
    d = sky.pixel_directions(inv_origin_view_proj, width, height, xs, ys)
    count = len(d)
    if mips == 1:
        return d, np.zeros(count, dtype=np.int64), np.zeros(count, dtype=f32), np.zeros(count, dtype=bool), np.zeros(count, dtype=f32)
    face, sc, tc, ma = sky.select_face(d)
    half = f32(0.5)
    with np.errstate(all="ignore"):
        s, t = half * (sc / ma) + half, half * (tc / ma) + half
        grads, unbounded = [], np.zeros(count, dtype=bool)
        for ox, oy in ((1, 0), (0, 1)):
            e = sky.pixel_directions(inv_origin_view_proj, width, height, xs + ox, ys + oy)
            sce, tce, me = project(face, e)
            unbounded |= ~(me > 0)
            grads.append(np.stack([(half * (sce / me) + half) - s, (half * (tce / me) + half) - t], axis=-1).astype(f32))
    level, frac, rho = lod(n, n, mips, grads[0], grads[1])
    level = np.where(unbounded, mips - 1, level)
    frac = np.where(unbounded, f32(0.0), frac).astype(f32)
    return d, level, frac, unbounded, rho


def bilinear(level_texels, table, d):
    """the seamless bilinear of the contract's step 5 on one decoded level for directions d: (n, 3) f32"""
    n = level_texels.shape[1]
    face, i0, j0, fx, fy = sky.footprint(d, n)
    with np.errstate(all="ignore"):
        c00, c10 = sky._fetch(level_texels, table, face, i0, j0), sky._fetch(level_texels, table, face, i0 + 1, j0)
        c01, c11 = sky._fetch(level_texels, table, face, i0, j0 + 1), sky._fetch(level_texels, table, face, i0 + 1, j0 + 1)
        fx, fy = fx[:, None], fy[:, None]
        omx, omy = f32(1.0) - fx, f32(1.0) - fy
        top, bot = c00 * omx + c10 * fx, c01 * omx + c11 * fx
        return (top * omy + bot * fy).astype(f32)


def sample(levels, fmt, d, level, frac):
    """(n, 4) f32 BEFORE the rounding to half"""
    table = _AsStored() if is_float(fmt) else sky.decode_table(fmt in SRGB_FORMATS)
    rgb = np.zeros((len(d), 3), dtype=f32)
    for k in range(len(levels)):
        m = level == k
        if m.any():
            rgb[m] = bilinear(levels[k], table, d[m])
        m = m & (frac > 0)
        if m.any():
            hi = bilinear(levels[k + 1], table, d[m])
            fr = frac[m][:, None]
            with np.errstate(all="ignore"):
                rgb[m] = (rgb[m] * (f32(1.0) - fr) + hi * fr).astype(f32)
    return np.concatenate([rgb, np.ones((len(rgb), 1), dtype=f32)], axis=1)


def sky_frame(levels, fmt, inv_origin_view_proj, width, height):
    """the sky of every pixel: (height, width, 4) uint16 half bits"""
    ys, xs = np.mgrid[0:height, 0:width]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    d, level, frac, _, _ = select_level(inv_origin_view_proj, width, height, xs, ys, levels[0].shape[1], len(levels))
    with np.errstate(all="ignore"):
        return sample(levels, fmt, d, level, frac).astype(np.float16).view(np.uint16).reshape(height, width, 4)


def may_be_nan(levels, fmt, inv_origin_view_proj, width, height):
    """(height, width) bool: pixels whose value the contract leaves NaN -- a footprint texel of a used level is not finite (the
    blend's weights can then meet inf * 0), or the direction itself is NaN.  Stated from the cube and the camera alone."""
    ys, xs = np.mgrid[0:height, 0:width]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    d, level, frac, _, _ = select_level(inv_origin_view_proj, width, height, xs, ys, levels[0].shape[1], len(levels))
    out = np.isnan(d).any(axis=1)
    if not is_float(fmt) or all(np.isfinite(lv[..., :3]).all() for lv in levels):
        return out.reshape(height, width)
    for k in range(len(levels)):
        for lv, m in ((k, level == k), (k + 1, (level == k) & (frac > 0))):
            for p in np.nonzero(m)[0]:
                n = levels[lv].shape[1]
                if any(not np.isfinite(levels[lv][f, j, i, :3]).all() for f, i, j in sky.footprint_texels(d[p], n)):
                    out[p] = True
    return out.reshape(height, width)


PATHS = ("level 0", "two levels", "clamped", "unbounded", "edge above 0", "corner above 0", "extent 1")


def classify(inv_origin_view_proj, width, height, n, mips):
    """names the paths each pixel takes: {path: (height, width) bool}
      level 0         rho <= 1 (or NaN): level 0 alone
      two levels      frac > 0: levels k and k + 1
      clamped         the footprint asks for the last level or beyond (bounded gradients)
      unbounded       a neighbour at or behind the face's horizon (m_e <= 0)
      edge above 0    a footprint that crosses one edge of the face on a level > 0
      corner above 0  a footprint on a cube corner on a level > 0
      extent 1        a used level with n_k = 1"""
    ys, xs = np.mgrid[0:height, 0:width]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    d, level, frac, unbounded, rho = select_level(inv_origin_view_proj, width, height, xs, ys, n, mips)
    out = {p: np.zeros(len(d), dtype=bool) for p in PATHS}
    with np.errstate(all="ignore"):
        out["level 0"] = ~unbounded & ~(rho > f32(1.0))
    out["two levels"] = frac > 0
    out["clamped"] = ~unbounded & (level == mips - 1) & (mips > 1) & (rho > f32(1.0))
    out["unbounded"] = unbounded.copy()
    for k in range(1, mips):
        nk = level_extent(n, k)
        used = (level == k) | ((level == k - 1) & (frac > 0))
        _, i0, j0, _, _ = sky.footprint(d, nk)
        over_i, over_j = (i0 < 0) | (i0 + 1 >= nk), (j0 < 0) | (j0 + 1 >= nk)
        out["edge above 0"] |= used & (over_i ^ over_j)
        out["corner above 0"] |= used & over_i & over_j
        if nk == 1:
            out["extent 1"] |= used
    return {p: m.reshape(height, width) for p, m in out.items()}
