"""CPU: the two facts the shadow views' two-phase depth draw rests on (kernels_raster.h), on the numpy restatement in
tests/shadow_occlusion_reference.py.

  1. the depth plane evaluated at the corner of the scan box picked by the signs of its gradients is >= every value a scan of
     that box writes -- for every box up to 9 x 9 at several origins and a sample of boxes up to 64 x 64, over planes with
     ordinary, tiny, huge, zero and negative-zero coefficients (and how far above the vertex depths it lies on a sliver);
  2. the four loads at level max(2, ceil_log2(longest side)) of the tile-min pyramid cover the box: their minimum is <= the
     minimum of the box's texels; and the pyramid's levels are the tile minima, laid out level after level.
Also: the worlds of the GPU test reach the box sizes they claim to."""
import numpy as np

import shadow_occlusion_reference as so

f32 = np.float32


def planes(rng, n):
    out = []
    mags = (1.0, 1e-3, 1e-6, 40.0, 1e4, 1e-30, 1e30)
    for _ in range(n):
        z = [rng.choice(mags) * rng.uniform(-1, 1) for _ in range(2)] + [rng.uniform(-0.5, 1.5)]
        out.append(z)
    specials = (0.0, -0.0, 1e-45, -1e-45, 3.0e38, -3.0e38)
    for a in specials:
        for b in specials:
            out.append([a, b, 0.5])
    # planes through depth 0 and depth 1 inside a box, and exactly representable gradients (ties between pixels)
    out += [[0.125, -0.25, 0.5], [-0.125, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [2.0 ** -20, 2.0 ** -21, 0.75]]
    return out


def check(z, x0, y0, x1, y1):
    bound = so.depth_bound(z, x0, y0, x1, y1)
    vals = so.written(z, x0, y0, x1, y1)
    assert bound <= f32(1.0)
    if vals.size:
        assert vals.max() <= bound, (z, (x0, y0, x1, y1), float(vals.max()), float(bound))
    return vals.size


def test_corner_value_bounds_every_written_depth():
    rng = np.random.default_rng(0x0CC1)
    ps = planes(rng, 60)
    written = 0
    for z in ps:
        for ox, oy in ((0, 0), (7, 120), (2041, 1)):
            for w in range(1, 10):
                for h in range(1, 10):
                    written += check(z, ox, oy, ox + w - 1, oy + h - 1)
    for z in ps:
        for _ in range(12):
            w, h = int(rng.integers(10, 65)), int(rng.integers(10, 65))
            ox, oy = int(rng.integers(0, 2048 - 64)), int(rng.integers(0, 2048 - 64))
            written += check(z, ox, oy, ox + w - 1, oy + h - 1)
        written += check(z, 0, 0, 63, 63)
    assert written > 100_000  # the planes do pass the depth clip


def test_corner_value_of_a_sliver_is_far_above_its_vertices():
    """An edge-on sliver of the GPU test's world: across the three or four rows of its scan box the plane leaves the range of the
    vertex depths by more than the gap to the occluder that test puts in front of it -- the bound answers "may be visible" where
    the largest vertex depth would answer "hidden"."""
    tri = so.slivers(20.0, 30.0, 1, 0.30, 0.35)[0]  # (px, py, depth) x 3
    (ax, ay, da), (bx, by, _), (cx, cy, dc) = tri
    gy = (dc - da) / (cy - ay)  # depth per pixel across the sliver; along it the depth is constant
    z = [0.0, gy, da - gy * ay]
    box = so.scan_box(np.asarray(tri, dtype=f32)[:, :2], 128)
    assert box[3] - box[1] + 1 in (3, 4)
    assert so.depth_bound(z, *box) > max(da, dc) + 0.25


def test_pyramid_levels_and_layout():
    rng = np.random.default_rng(0x0CC2)
    for n, ls in ((64, 6), (128, 7), (256, 8)):
        view = rng.random((n, n), dtype=f32)
        view[rng.random((n, n)) < 0.1] = 0.0  # texels nothing was drawn to
        pyr = so.pyramid(view)
        assert pyr.size == sum((n >> l) ** 2 for l in so.LEVELS) == so.level_offset(ls, 7)
        for level in so.LEVELS:
            t = n >> level
            lv = pyr[so.level_offset(ls, level):so.level_offset(ls, level + 1)].reshape(t, t)
            for ty, tx in ((0, 0), (t - 1, t - 1), (t // 2, 0), (0, t - 1)):
                assert lv[ty, tx] == view[ty << level:(ty + 1) << level, tx << level:(tx + 1) << level].min()
        assert pyr[-1] == view[-64:, -64:].min()


def test_four_loads_cover_the_box():
    rng = np.random.default_rng(0x0CC3)
    n, ls = 128, 7
    view = rng.random((n, n), dtype=f32)
    pyr = so.pyramid(view)
    sides = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
    for w in sides:
        for h in sides:
            level = so.box_level(0, 0, w - 1, h - 1)
            assert 2 <= level <= 6 and max(w, h) <= 1 << level and (level == 2 or max(w, h) > 1 << (level - 1))
            origins = {(0, 0), (n - w, n - h)} | {(int(rng.integers(0, n - w + 1)), int(rng.integers(0, n - h + 1))) for _ in range(6)}
            for x0, y0 in origins:
                x1, y1 = x0 + w - 1, y0 + h - 1
                assert (x1 >> level) - (x0 >> level) <= 1 and (y1 >> level) - (y0 >> level) <= 1
                assert so.tile_min(pyr, ls, x0, y0, x1, y1) <= view[y0:y1 + 1, x0:x1 + 1].min()


def test_constants_and_world_boxes():
    d = so.kernel_defines()
    assert d["R3N_OCC_MAX_BOX"] == so.MAX_BOX == 64 and d["R3N_SMALL_MAX"] == 8 and d["R3N_TILE"] == 32
    for side in (4, 5, 8, 9, 16, 17, 32, 33, 64, 65):
        tri = np.asarray(so.sided(side, 10, 20, 0.25)[0], dtype=f32)[:, :2]
        x0, y0, x1, y1 = so.scan_box(tri, 256)
        assert (x0, y0) == (10, 20) and x1 - x0 + 1 == side and y1 - y0 + 1 == side
    # at the view's left and top border the clamp leaves boxes of one and two texels
    for side, off in ((1, -1.5), (2, -0.5)):
        tri = np.asarray([(off - 0.25, 40.0), (off, 40.0), (off, 40.3)], dtype=f32)
        x0, _, x1, _ = so.scan_box(tri, 128)
        assert (x0, x1 - x0 + 1) == (0, side)
