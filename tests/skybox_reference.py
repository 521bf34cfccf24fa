"""numpy restatement of the skybox node's arithmetic contract ("Skybox"), the judge of tests/test_skybox.py
where the oracle cannot be (it has no cube sampler).  f32 throughout, one rounding per operation, IEEE division and square root:

 1. clip.x = ((x + 0.5) * 2) / W - 1, clip.y = 1 - ((y + 0.5) * 2) / H, clip = (clip.x, clip.y, 1, 1)
 2. world_undiv = inv_origin_view_proj * clip, as ((c0 * x + c1 * y) + c2 * z) + c3 * w
 3. world = xyz / w;  dir = world * (1 / sqrt(dot3(world)))
 4. face by the Vulkan / WebGPU cube table: major axis = largest magnitude, ties z over y over x, a major component that is not
    negative selects the positive face;  +X: (sc, tc) = (-z, -y)  -X: (z, -y)  +Y: (x, z)  -Y: (x, -z)  +Z: (x, -y)  -Z: (-x, -y);
    s = 0.5 * (sc / |ma|) + 0.5, t likewise
 5. bilinear on level 0: s * N - 0.5, floor, fractions, a * (1 - f) + b * f along rows then columns; texels decoded (c / 255, or
    the oracle's 256-entry sRGB table) BEFORE filtering.  A footprint texel one step outside the face is the adjacent face's texel
    across that edge; at a cube corner the missing diagonal texel is ((a + b) + c) / 3 per channel of the in-face texel a, the
    neighbour b across the s edge and the neighbour c across the t edge
 6. (r, g, b, 1) rounded to half

The texel across an edge is found GEOMETRICALLY, with no adjacency table: the texel centre is extended on the face's plane,
re-projected, and the face and nearest texel that direction selects are taken (the shift along the edge stays below half a texel,
so the choice is unambiguous).  That part runs in float64; it selects texels, it does not produce values.

A sample takes the sky iff the reference's depth test passes -- sky depth 0.0 GreaterEqual the stored depth (takes_sky): every
cleared sample, and a sample that holds a triangle at depth exactly 0.0 (the sky is drawn later and wins, as in the reference).
"""
import numpy as np

f32 = np.float32
FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")


def takes_sky(depth):
    return f32(0.0) >= np.asarray(depth, dtype=f32)


def decode_table(srgb):
    if not srgb:
        return np.arange(256, dtype=f32) / f32(255.0)
    from oracle.lib import get as get_lib
    lib = get_lib()
    out = np.zeros(256, dtype=f32)
    lib.r3o_srgb8_table(lib.ptr(out))
    return out


def pixel_directions(inv_origin_view_proj, width, height, xs, ys):
    """steps 1-3 for the pixel centres (xs, ys): (n, 3) f32"""
    m = np.asarray(inv_origin_view_proj, dtype=f32)
    x, y = np.asarray(xs).astype(f32), np.asarray(ys).astype(f32)
    cx = ((x + f32(0.5)) * f32(2.0)) / f32(width) - f32(1.0)
    cy = f32(1.0) - ((y + f32(0.5)) * f32(2.0)) / f32(height)
    one = f32(1.0)
    wu = [((m[r] * cx + m[4 + r] * cy) + m[8 + r] * one) + m[12 + r] * one for r in range(4)]
    with np.errstate(all="ignore"):
        w = [wu[k] / wu[3] for k in range(3)]
        r = one / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        return np.stack([w[0] * r, w[1] * r, w[2] * r], axis=-1).astype(f32)


def select_face(d):
    """step 4 without the final scale: (face, sc, tc, ma) for directions d (n, 3); dtype follows d"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_z = (az >= ax) & (az >= ay)
    is_y = ~is_z & (ay >= ax)
    nx, ny, nz = x < 0, y < 0, z < 0
    face = np.where(is_z, np.where(nz, 5, 4), np.where(is_y, np.where(ny, 3, 2), np.where(nx, 1, 0)))
    sc = np.where(is_z, np.where(nz, -x, x), np.where(is_y, x, np.where(nx, z, -z)))
    tc = np.where(is_z, -y, np.where(is_y, np.where(ny, -z, z), -y))
    ma = np.where(is_z, az, np.where(is_y, ay, ax))
    return face, sc, tc, ma


def _face_point(face, sc, tc):
    """the point (sc, tc) of a face's plane (|ma| = 1) as a direction: the table of step 4 read backwards (float64)"""
    one = np.ones_like(sc)
    px = np.choose(face, [one, -one, sc, sc, sc, -sc])
    py = np.choose(face, [-tc, -tc, one, -one, -tc, -tc])
    pz = np.choose(face, [-sc, sc, tc, -tc, one, -one])
    return np.stack([px, py, pz], axis=-1)


def resolve_texel(face, i, j, n):
    """(face, i, j) with i, j in [-1, n] and at most one of them outside [0, n) -> the texel that holds it: itself, or the
    adjacent face's texel across the edge, found by extending the texel centre on the face's plane and re-projecting"""
    sc = (2.0 * (i.astype(np.float64) + 0.5)) / n - 1.0
    tc = (2.0 * (j.astype(np.float64) + 0.5)) / n - 1.0
    nf, nsc, ntc, ma = select_face(_face_point(face, sc, tc))
    s, t = 0.5 * (nsc / ma) + 0.5, 0.5 * (ntc / ma) + 0.5
    ni = np.clip(np.floor(s * n), 0, n - 1).astype(np.int64)
    nj = np.clip(np.floor(t * n), 0, n - 1).astype(np.int64)
    return nf, ni, nj


def footprint(d, n):
    """step 5's footprint for directions d: face, first texel (i0, j0) in [-1, n - 1] and the fractions (fx, fy)"""
    d = np.asarray(d, dtype=f32)
    face, sc, tc, ma = select_face(d)
    with np.errstate(all="ignore"):
        s = f32(0.5) * (sc / ma) + f32(0.5)
        t = f32(0.5) * (tc / ma) + f32(0.5)
    tx, ty = s * f32(n) - f32(0.5), t * f32(n) - f32(0.5)
    fx0, fy0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - fx0).astype(f32), (ty - fy0).astype(f32)
    fx, fy = np.where(np.isnan(fx), f32(0), fx), np.where(np.isnan(fy), f32(0), fy)
    i0 = np.clip(np.nan_to_num(fx0, nan=-1.0), -1, n - 1).astype(np.int64)
    j0 = np.clip(np.nan_to_num(fy0, nan=-1.0), -1, n - 1).astype(np.int64)
    return face, i0, j0, fx, fy


def footprint_texels(d, n):
    """the set of (face, i, j) texels the footprint of ONE direction reads (corner positions contribute their three texels)"""
    face, i0, j0, _, _ = footprint(np.asarray(d, dtype=f32).reshape(1, 3), n)
    out = set()
    for di in (0, 1):
        for dj in (0, 1):
            i, j = i0 + di, j0 + dj
            ci, cj = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
            for a, b in ((i, cj), (ci, j)):
                nf, ni, nj = resolve_texel(face, a, b, n)
                out.add((int(nf[0]), int(ni[0]), int(nj[0])))
    return out


def _fetch(faces, table, face, i, j):
    """decoded rgb (n, 3) f32 of footprint position (i, j) of `face`"""
    n = faces.shape[1]
    out_i, out_j = (i < 0) | (i >= n), (j < 0) | (j >= n)
    ci, cj = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)

    def value(f, a, b):
        return table[faces[f, b, a, :3]]

    a = value(face, ci, cj)
    b = value(*resolve_texel(face, i, cj, n))   # across the s edge (itself when i is inside)
    c = value(*resolve_texel(face, ci, j, n))   # across the t edge
    corner = ((a + b) + c) / f32(3.0)
    oi, oj = out_i[:, None], out_j[:, None]
    return np.where(oi & oj, corner, np.where(oi, b, np.where(oj, c, a))).astype(f32)


def sample(faces, srgb, d):
    """steps 4-6 for directions d (n, 3): (n, 4) f32 BEFORE the rounding to half"""
    faces = np.asarray(faces, dtype=np.uint8)
    n = faces.shape[1]
    table = decode_table(srgb)
    face, i0, j0, fx, fy = footprint(d, n)
    c00, c10 = _fetch(faces, table, face, i0, j0), _fetch(faces, table, face, i0 + 1, j0)
    c01, c11 = _fetch(faces, table, face, i0, j0 + 1), _fetch(faces, table, face, i0 + 1, j0 + 1)
    fx, fy = fx[:, None], fy[:, None]
    omx, omy = f32(1.0) - fx, f32(1.0) - fy
    top, bot = c00 * omx + c10 * fx, c01 * omx + c11 * fx
    rgb = top * omy + bot * fy
    return np.concatenate([rgb.astype(f32), np.ones((len(rgb), 1), dtype=f32)], axis=1)


def sky_pixels(faces, srgb, inv_origin_view_proj, width, height, xs, ys):
    """the half bits (n, 4) uint16 of the sky at the pixel centres (xs, ys)"""
    d = pixel_directions(inv_origin_view_proj, width, height, xs, ys)
    return sample(faces, srgb, d).astype(np.float16).view(np.uint16)


def sky_frame(faces, srgb, inv_origin_view_proj, width, height):
    """the sky of every pixel: (height, width, 4) uint16 half bits"""
    ys, xs = np.mgrid[0:height, 0:width]
    return sky_pixels(faces, srgb, inv_origin_view_proj, width, height, xs.reshape(-1), ys.reshape(-1)).reshape(height, width, 4)
