"""The pieces of the shadow views' two-phase depth draw (kernels_raster.h: occ_depth_bound, occ_level_offset, occ_tile_min,
k_shadow_tile_min) restated in numpy f32, nothing of the product imported, plus the small worlds the GPU test draws.

  depth plane   z(x, y) = (z0 * (x + 0.5) + z1 * (y + 0.5)) + z2, every operation rounded to f32 once (raster_reference.py has
                the contract: depth is affine in window space); the scans keep 0 <= z <= 1
  bound         the same expression at the corner of the scan box picked by the signs of z0 and z1, then min(., 1)
  pyramid       level L (2..6) holds the minimum of the view's texels over 2^L x 2^L tiles, row-major, levels back to back
  box test      at level max(2, ceil_log2(longest side)) a box of at most 64 texels per side touches at most 2 x 2 tiles
"""
import os
import re

import numpy as np

f32 = np.float32
MAX_BOX = 64
LEVELS = (2, 3, 4, 5, 6)


def kernel_defines():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rend3_amd", "csrc", "kernels_raster.h")).read()
    return {name: int(re.search(r"^#define\s+" + name + r"\s+(\d+)", text, flags=re.M).group(1)) for name in ("R3N_OCC_MAX_BOX", "R3N_SMALL_MAX", "R3N_TILE")}


def plane(z, x, y):
    """frag_depth at the centres of pixels (x, y) (integer arrays) in f32"""
    z0, z1, z2 = (f32(v) for v in z)
    with np.errstate(all="ignore"):
        px, py = x.astype(f32) + f32(0.5), y.astype(f32) + f32(0.5)
        return ((z0 * px).astype(f32) + (z1 * py).astype(f32)).astype(f32) + z2


def positive(v):
    """device_math.h f32_positive: the bits as a signed integer are > 0"""
    return np.asarray(v, dtype=f32).view(np.int32) > 0


def depth_bound(z, x0, y0, x1, y1):
    cx = np.array([x1 if positive(z[0]) else x0]), np.array([y1 if positive(z[1]) else y0])
    v = plane(z, cx[0], cx[1])[0]
    return f32(1.0) if not v <= f32(1.0) else v  # fminf(v, 1): NaN -> 1


def written(z, x0, y0, x1, y1):
    """every value a scan of the whole box could write: the per-pixel depths that pass the depth clip"""
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    v = plane(z, xs, ys)
    with np.errstate(invalid="ignore"):
        return v[(v >= 0) & (v <= 1)]


def level_offset(log2_size, level):
    return sum(1 << (2 * (log2_size - l)) for l in range(2, level))


def pyramid(view):
    """the levels of a square power-of-two view (float array) as one flat array, as the kernel lays them out"""
    n = view.shape[0]
    assert view.shape == (n, n) and n >= 64 and n & (n - 1) == 0
    out = []
    for level in LEVELS:
        t = 1 << level
        out.append(view.reshape(n // t, t, n // t, t).min(axis=(1, 3)).reshape(-1))
    return np.concatenate(out).astype(f32)


def box_level(x0, y0, x1, y1):
    m = max(x1 - x0, y1 - y0)
    return max(2, int(m).bit_length())  # ceil_log2(m + 1)


def tile_min(pyr, log2_size, x0, y0, x1, y1):
    level = box_level(x0, y0, x1, y1)
    lv = pyr[level_offset(log2_size, level):]
    n = log2_size - level
    rows, cols = (y0 >> level, y1 >> level), (x0 >> level, x1 >> level)
    return min(lv[(r << n) + c] for r in rows for c in cols)


def scan_box(tri_px, size):
    """device_math.h tri_bounds for a triangle in front of the eye plane, from its window-space vertices (f32 array [3, 2]):
    (x0, y0, x1, y1) inclusive, or None"""
    mn, mx = tri_px.min(axis=0), tri_px.max(axis=0)
    lo, hi = np.floor(mn) - 1, np.ceil(mx) + 1
    c = lambda v, edge_lo, edge_hi: edge_lo if v < 0 else (edge_hi if v > size - 1 else int(v))
    x0, y0, x1, y1 = c(lo[0], 0, size), c(lo[1], 0, size), c(hi[0], -1, size - 1), c(hi[1], -1, size - 1)
    return (x0, y0, x1, y1) if x1 >= x0 and y1 >= y0 else None


# ------------------------------------------------------------------ worlds: triangles in the window space of a shadow view
# A light with direction (0, 0, 1) and distance 2 seen from a camera at the origin (raster_reference.py): clip x, y = world x, y,
# depth = 1/2 - z/2.  A triangle is given as three (px, py, depth) in the pixels of a view of `size` texels.
def to_world(tris_px, size):
    t = np.asarray(tris_px, dtype=np.float64).reshape(-1, 3, 3)
    out = np.empty_like(t)
    out[..., 0] = t[..., 0] / (size / 2) - 1
    out[..., 1] = 1 - t[..., 1] / (size / 2)
    out[..., 2] = 1 - 2 * t[..., 2]
    return out.astype(f32)


def both_windings(tris):
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([t, t[:, [0, 2, 1]]])


def quad(x0, y0, x1, y1, depth):
    return both_windings([[(x0, y0, depth), (x1, y0, depth), (x1, y1, depth)], [(x0, y0, depth), (x1, y1, depth), (x0, y1, depth)]])


def field(x0, y0, x1, y1, step, leg, depth, slope=0.0):
    """right triangles with legs of `leg` px every `step` px; depth rises by `slope` per px in x"""
    tris = []
    y = y0
    while y + leg <= y1:
        x = x0
        while x + leg <= x1:
            d = depth + slope * (x - x0)
            tris.append([(x, y, d), (x + leg, y, d + slope * leg), (x, y + leg, d)])
            x += step
        y += step
    return both_windings(tris)


def sided(side, x, y, depth):
    """a right triangle whose scan box is `side` px wide and high (side >= 4) with its corner in pixel (x, y)"""
    a, e = 0.25, side - 4 + 0.5
    return both_windings([[(x + 1 + a, y + 1 + a, depth), (x + 1 + a + e, y + 1 + a, depth), (x + 1 + a, y + 1 + a + e, depth)]])


def slivers(x0, y0, n, depth_a, depth_c, width=24.0, height=0.07):
    """edge-on slivers: `width` px long, `height` px high, the apex `depth_c - depth_a` away in depth -- a gradient of several
    units per pixel across the sliver, so the plane leaves [depth_a, depth_c] within the scan box (which is 2-3 px higher)"""
    tris = []
    for k in range(n):
        y = y0 + 3.0 * k + 0.5 - 0.03 + 0.011 * k  # the rows of pixel centres run through some of them
        tris.append([(x0, y, depth_a), (x0 + width, y, depth_a), (x0 + width / 2, y + height, depth_c)])
    return both_windings(tris)
