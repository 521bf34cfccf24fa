"""An exact restatement of the rasteriser contract (DESIGN.md section 2 "Rasteriser", cull.wgsl:264-324) in Python ints,
fractions.Fraction and integer numpy arrays -- no float arithmetic, nothing of the product imported -- for worlds on which the
contract's f32 arithmetic is exact, and the launch plan of kernels_raster.h (which path scans a triangle, which work items it
queues) restated beside it.

Why it can be exact: the worlds' vertices are dyadic rationals k / 2^m in clip space with w = 1, the views map them to window
space through W/2 and H/2, and every product and sum the contract forms on the way to a sample's coverage and depth is then a
dyadic rational that a f32 holds -- so the rounded arithmetic of the oracle and of the kernels equals the arithmetic of the
rationals, in whatever order it is done.  guard() recomputes each of those intermediates and raises Inexact where a f32 would
round; only worlds that pass it ("the exact tier") are compared with this file.

  window mapping   X = (x + 1) W/2, Y = (1 - y) H/2; samples at the pixel centre or at the four standard positions
  coverage         oriented by the sign of the window-space area against the view's "positive area visible" flag (the depth-only
                   views draw the other winding); a sample is covered when every edge value is > 0, or == 0 on an edge with A > 0
                   or (A == 0 and B > 0)
  depth            affine in window space, anchored at vertex 0; kept for 0 <= z <= 1; -0 stored as +0
  winner           key target: max of f32 bits(z) << 32 | (tri_base + triangle + 1); depth target: max of the z bits
  triangle cull    back-face by sign; rint(smin) == rint(smax) in x or y (ties to even, y NOT flipped, off under the multisampled
                   flag); the viewport against an all-zero pyramid: largest vertex depth < 0
The views: the viewport with an identity view and a ("raw", identity) projection, and the shadow view of a directional light with
direction (0, 0, 1) and distance 2 seen from a camera at the origin (clip x, y = world x, y; clip z = 1/2 - z/2)."""
import bisect
import math
import os
import random
import re
from fractions import Fraction as Fr

import numpy as np

SMALL_MAX, TILE, ITEM_ALIGN = 8, 32, 16
DEFINES = {"R3N_SMALL_MAX": SMALL_MAX, "R3N_TILE": TILE, "R3N_ITEM_ALIGN": ITEM_ALIGN}
SAMPLES8 = {1: ((4, 4),), 4: ((3, 1), (7, 3), (1, 5), (5, 7))}  # sample positions in eighths of a pixel
OPAQUE, CUTOUT, BLEND = 0, 1, 2
EXTENTS = ((64, 64), (96, 40), (33, 17))
LATTICE = {(64, 64): 8, (96, 40): 6, (33, 17): 5}  # m of the clip-space lattice k / 2^m a world of that extent is drawn on
SHADOW_RESOLUTIONS = (64, 32)
LIGHT = dict(color=(1, 1, 1), intensity=1.0, direction=(0.0, 0.0, 1.0), distance=2.0)
i64 = np.int64


def kernel_defines():
    """the rasteriser's constants as kernels_raster.h has them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rend3_amd", "csrc", "kernels_raster.h")).read()
    return {name: [int(v) for v in re.findall(r"^#define\s+" + name + r"\s+(\d+)u?\b", text, flags=re.M)] for name in DEFINES}


# ------------------------------------------------------------------ what a f32 holds
class Inexact(AssertionError):
    pass


def f32(v, what=""):
    """v when a (normal) f32 holds it exactly"""
    v = Fr(v)
    n, d = abs(v.numerator), v.denominator
    if n == 0:
        return v
    if d & (d - 1):
        raise Inexact(f"{what}: {v} is not dyadic")
    n >>= (n & -n).bit_length() - 1
    if n >= 1 << 24 or not -100 < abs(v.numerator).bit_length() - d.bit_length() < 100:
        raise Inexact(f"{what}: {v} needs {n.bit_length()} significant bits")
    return v


def f32_all(a, what=""):
    """the same for an integer array of values in units of one power of two"""
    a = np.abs(np.asarray(a, dtype=i64))
    low = a & -a
    low[low == 0] = 1
    if a.size and int((a // low).max()) >= 1 << 24:
        raise Inexact(f"{what}: {int((a // low).max()).bit_length()} significant bits")


def f32_bits(n, q):
    """bits of the f32 that holds n / 2^q, 0 <= n / 2^q (exact by the guard)"""
    if n == 0:
        return 0
    top = n.bit_length() - 1
    e = top - q + 127
    assert 0 < e < 255 and (top <= 23 or n & ((1 << (top - 23)) - 1) == 0)
    mant = n << (23 - top) if top <= 23 else n >> (top - 23)
    return (e << 23) | (mant & 0x7FFFFF)


def log2_den(*values):
    out = 0
    for v in values:
        d = Fr(v).denominator
        assert d & (d - 1) == 0, v
        out = max(out, d.bit_length() - 1)
    return out


# ------------------------------------------------------------------ views
class View:
    """W x H samples of one camera.  shadow: the depth-only view of LIGHT (the other winding, no multisampling, no pyramid)."""

    def __init__(self, W, H, samples=1, shadow=False):
        assert not (shadow and (samples != 1 or W != H))
        self.W, self.H, self.samples, self.shadow = W, H, samples, shadow
        self.positive_visible = shadow  # left-handed world: (Cw, Back) -> negative areas, (Cw, Front) -> positive ones
        self.multisampled = samples != 1
        self.name = f"shadow {W}" if shadow else f"{W}x{H}x{samples}"

    def clip(self, v):
        """clip-space x, y, z of a world vertex (w = 1); mat4 * vec4 = ((c0 x + c1 y) + c2 z) + c3 with this view's matrix"""
        x, y, z = (f32(c, "vertex") for c in v)
        if not self.shadow:
            return x, y, z
        return x, y, f32(f32(Fr(-1, 2) * z, "clip z") + Fr(1, 2), "clip z")


# ------------------------------------------------------------------ one triangle in one view
def setup(view, tri):
    """Edge functions, orientation, the scan box of device_math.h tri_bounds (all vertices in front) and the depth plane of one
    triangle, every intermediate the kernel forms passed through f32().  Coordinates in window space, y down."""
    p = [view.clip(v) for v in tri]
    hw, hh = Fr(view.W, 2), Fr(view.H, 2)
    h = [(f32(f32(x + 1, "x + w") * hw, "h.x"), f32(f32(1 - y, "w - y") * hh, "h.y")) for x, y, _z in p]
    e = []
    for i in range(3):  # edge i joins vertices i + 1 and i + 2: e = a x b with third coordinates 1
        a, b = h[(i + 1) % 3], h[(i + 2) % 3]
        e.append([f32(a[1] - b[1], "A"), f32(b[0] - a[0], "B"), f32(f32(a[0] * b[1], "C") - f32(a[1] * b[0], "C"), "C")])
    det = f32(f32(f32(h[0][0] * e[0][0], "det") + f32(h[0][1] * e[0][1], "det"), "det") + e[0][2], "det")
    visible = det != 0 and (det < 0) == view.positive_visible
    if det < 0:
        e = [[-c for c in ei] for ei in e]
    out = dict(p=p, h=h, e=e, det=det, visible=visible, box=None)
    # scan box: one pixel of slack each side, clamped to the viewport
    xs, ys = [a[0] for a in h], [a[1] for a in h]
    fx0, fy0, fx1, fy1 = math.floor(min(xs)) - 1, math.floor(min(ys)) - 1, math.ceil(max(xs)) + 1, math.ceil(max(ys)) + 1
    W, H = view.W, view.H
    x0 = 0 if fx0 < 0 else (W if fx0 > W - 1 else fx0)
    y0 = 0 if fy0 < 0 else (H if fy0 > H - 1 else fy0)
    x1 = -1 if fx1 < 0 else (W - 1 if fx1 > W - 1 else fx1)
    y1 = -1 if fy1 < 0 else (H - 1 if fy1 > H - 1 else fy1)
    if x1 >= x0 and y1 >= y0:
        out["box"] = (x0, y0, x1, y1)
    if not visible:
        return out
    # depth plane through the window-space vertices, anchored at vertex 0
    (sx0, sy0), zn = h[0], [c[2] for c in p]
    ax, ay, bx, by = f32(h[1][0] - sx0), f32(h[1][1] - sy0), f32(h[2][0] - sx0), f32(h[2][1] - sy0)
    az, bz = f32(zn[1] - zn[0], "az"), f32(zn[2] - zn[0], "bz")
    area = f32(f32(ax * by, "area") - f32(bx * ay, "area"), "area")
    if az == 0 and bz == 0:  # 0 * (1 / area) = 0 whatever the reciprocal rounds to
        gx = gy = Fr(0)
        c = zn[0]
    else:
        ia = f32(1 / area, "1 / area")  # the doubled area is a power of two
        gx = f32(f32(f32(az * by, "gx") - f32(bz * ay, "gx"), "gx") * ia, "gx")
        gy = f32(f32(f32(bz * ax, "gy") - f32(az * bx, "gy"), "gy") * ia, "gy")
        c = f32(f32(zn[0] - f32(gx * sx0, "c"), "c") - f32(gy * sy0, "c"), "c")
    out.update(z=(gx, gy, c))
    return out


def cull(view, s):
    """cull.wgsl:264-324 on a frame whose pyramid is all zero: (passes, reason it did not)"""
    (ax, ay, _), (bx, by, _), (cx, cy, _) = s["p"]
    det = f32(f32(f32(ax * f32(by - cy), "ndc det") - f32(bx * f32(ay - cy), "ndc det"), "ndc det") + f32(cx * f32(ay - by), "ndc det"), "ndc det")
    if (view.positive_visible and det <= 0) or (not view.positive_visible and det >= 0):
        return False, "back"
    if not view.multisampled:
        for c, half in ((0, Fr(view.W, 2)), (1, Fr(view.H, 2))):
            lo, hi = min(v[c] for v in s["p"]), max(v[c] for v in s["p"])
            if round(f32(f32(lo + 1) * half, "smin")) == round(f32(f32(hi + 1) * half, "smax")):  # round(Fraction): ties to even
                return False, "rint"
    if not view.shadow and max(v[2] for v in s["p"]) < 0:
        return False, "hiz"
    return True, None


def grid(view, shift):
    """sample coordinates in units of 2^-shift px: x[W, S], y[H, S]"""
    assert shift >= 3
    pos = SAMPLES8[view.samples]
    gx = np.array([[(8 * x + ox) << (shift - 3) for ox, _ in pos] for x in range(view.W)], dtype=i64)
    gy = np.array([[(8 * y + oy) << (shift - 3) for _, oy in pos] for y in range(view.H)], dtype=i64)
    return gx, gy


def scan(view, s, guard=True):
    """Coverage and depth of a visible triangle at every sample of the view, as integers: dict of [H, W, S] arrays.  `guard`:
    every edge value inside the scan box and every depth of a covered sample is formed from terms a f32 holds."""
    assert s["visible"]
    W, H, S = view.W, view.H, view.samples
    sh = max(3, log2_den(*[c for a in s["h"] for c in a]))
    gx, gy = grid(view, sh)
    inside = np.ones((H, W, S), dtype=bool)
    nonneg = np.ones((H, W, S), dtype=bool)
    on_edge = np.zeros((H, W, S), dtype=bool)
    box = s["box"]
    for A, B, C in s["e"]:
        Ai, Bi, Ci = int(A * (1 << sh)), int(B * (1 << sh)), int(C * (1 << (2 * sh)))
        tx, ty = Ai * gx, Bi * gy
        E = (tx[None, :, :] + ty[:, None, :]) + Ci
        if guard and box is not None:
            x0, y0, x1, y1 = box
            f32_all(tx[x0:x1 + 1], "A px")
            f32_all(ty[y0:y1 + 1], "B py")
            f32_all(tx[None, x0:x1 + 1] + ty[y0:y1 + 1, None], "A px + B py")
            f32_all(E[y0:y1 + 1, x0:x1 + 1], "edge value")
        top_left = A > 0 or (A == 0 and B > 0)
        inside &= (E > 0) | ((E == 0) & top_left)
        nonneg &= E >= 0
        on_edge |= E == 0
    if box is None:
        assert not inside.any()
    else:
        x0, y0, x1, y1 = box
        outside = inside.copy()
        outside[y0:y1 + 1, x0:x1 + 1] = False
        assert not outside.any(), "the scan box holds every covered sample"
    gzx, gzy, c = s["z"]
    q = max(sh + log2_den(gzx, gzy), log2_den(c))
    Gx, Gy, Cq = int(gzx * (1 << (q - sh))), int(gzy * (1 << (q - sh))), int(c * (1 << q))
    zx, zy = Gx * gx, Gy * gy
    zi = (zx[None, :, :] + zy[:, None, :]) + Cq
    if guard and inside.any():
        f32_all(np.broadcast_to(zx[None], zi.shape)[inside], "gx px")
        f32_all(np.broadcast_to(zy[:, None], zi.shape)[inside], "gy py")
        f32_all((zx[None, :, :] + zy[:, None, :])[inside], "gx px + gy py")
        f32_all(zi[inside], "z")
    kept = inside & (zi >= 0) & (zi <= (1 << q))
    bits = np.zeros((H, W, S), dtype=np.uint64)
    if kept.any():
        values, inverse = np.unique(zi[kept], return_inverse=True)
        table = np.array([f32_bits(int(v), q) for v in values], dtype=np.uint64)
        bits[kept] = table[inverse.reshape(-1)]
    return dict(inside=inside, kept=kept, zbits=bits, below=inside & (zi < 0), above=inside & (zi > (1 << q)),
                edge_accepted=on_edge & inside, edge_rejected=on_edge & nonneg & ~inside)


# ------------------------------------------------------------------ worlds and frames
def triangles(world):
    """(object, triangle, canonical slot, vertices) of every triangle, objects in handle order"""
    slot = 0
    for o, ob in enumerate(world["objects"]):
        for t, tri in enumerate(ob["tris"]):
            yield o, t, slot, tri
            slot += 1


def check_objects_inside(world):
    """every object holds a vertex well inside both frusta (|x|, |y|, |z| <= 1/2): its bounding sphere passes the frustum test
    whatever its radius rounds to, so the triangle cull alone decides the pass set"""
    for ob in world["objects"]:
        assert any(all(abs(c) <= Fr(1, 2) for c in v) for tri in ob["tris"] for v in tri), world["name"]


def render(world, view, keys=(OPAQUE, CUTOUT), guard=True):
    """One frame of the view over an empty history: the pass set, the target (u64 keys [H, W] or [H, W, S]; the shadow view's u32
    depth bits [H, W]) and the per-triangle records behind them.  Objects whose material key is not in `keys` are culled but not
    drawn (the blend key)."""
    check_objects_inside(world)
    W, H, S = view.W, view.H, view.samples
    target = np.zeros((H, W, S), dtype=np.uint64)
    recs, passing = [], []
    count = dict(edge_accepted=0, edge_rejected=0, below=0, above=0, rint_covering=0, ties=0)
    for o, t, slot, tri in triangles(world):
        s = setup(view, tri)
        ok, why = cull(view, s)
        assert ok <= s["visible"], "a triangle that passes the cull has the visible winding"
        s.update(object=o, triangle=t, slot=slot, passes=ok, why=why, key=world["objects"][o].get("key", OPAQUE))
        passing.append(ok)
        recs.append(s)
        if not s["visible"] or why == "hiz":
            continue
        sc = scan(view, s, guard)
        s["scan"] = sc
        if why == "rint":
            count["rint_covering"] += int(sc["kept"].any())
            continue
        if s["key"] not in keys:
            continue
        for k in ("edge_accepted", "edge_rejected", "below", "above"):
            count[k] += int(sc[k].sum())
        s["drawn"] = True
        k64 = (sc["zbits"] << np.uint64(32)) | np.uint64(slot + 1)
        target = np.where(sc["kept"], np.maximum(target, k64), target)
    holders = np.zeros((H, W, S), dtype=np.int32)  # triangles that hold the sample's winning depth: more than one is a tie won by slot
    for s in recs:
        if s.get("drawn"):
            holders += s["scan"]["kept"] & (s["scan"]["zbits"] == target >> np.uint64(32))
    count["ties"] = int((holders > 1).sum())
    if view.shadow:
        out = (target[:, :, 0] >> np.uint64(32)).astype(np.uint32)
    else:
        out = target[:, :, 0] if S == 1 else target
    return dict(target=np.ascontiguousarray(out), recs=recs, count=count, **{"pass": np.array(passing, dtype=np.uint8)})


# ------------------------------------------------------------------ the launch plan of kernels_raster.h
def plan(view, s, blend=False):
    """Which path scans a drawn triangle: ("in_place", []) for boxes up to SMALL_MAX px in both axes (k_raster_small's own
    loop; k_blend_setup has no such path), else ("items", [...]) -- the work items k_raster_small / k_blend_setup queue, in
    queue order, each with its rectangle, the origin of its block grid and whether k_raster_big scans it in fine blocks (8 x 2 px,
    four per step) or coarse ones (8 x 8)."""
    if not s["visible"] or s["box"] is None:
        return "none", []
    x0, y0, x1, y1 = s["box"]
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    if not blend and bw <= SMALL_MAX and bh <= SMALL_MAX:
        return "in_place", []
    ax0 = x0 if blend else x0 & ~(ITEM_ALIGN - 1)
    tx = (bw + TILE - 1) // TILE if blend else (x1 - ax0 + TILE) // TILE
    ty = (bh + TILE - 1) // TILE
    items = []
    for t in range(tx * ty):
        ix, iy = t % tx, t // tx
        rx0, ry0 = max(ax0 + ix * TILE, x0), y0 + iy * TILE
        rx1, ry1 = min(ax0 + ix * TILE + TILE - 1, x1), min(ry0 + TILE - 1, y1)
        gx0 = rx0 & ~(ITEM_ALIGN - 1)
        items.append(dict(ix=ix, iy=iy, tx=tx, ty=ty, rect=(rx0, ry0, rx1, ry1), gx0=gx0, fine=rx1 - gx0 < 32 and ry1 - ry0 < 32,
                          empty=rx0 > rx1))
    return "items", items


def locate(view, s, x, y, blend=False):
    """the path, work item and block plan() assigns to pixel (x, y) of a triangle"""
    path, items = plan(view, s, blend)
    if path != "items":
        return path
    for n, it in enumerate(items):
        rx0, ry0, rx1, ry1 = it["rect"]
        if rx0 <= x <= rx1 and ry0 <= y <= ry1:
            bw, bh = (8, 2) if it["fine"] else (8, 8)
            return (f"work item {n} of {len(items)} (column {it['ix']} of {it['tx']}, row {it['iy']} of {it['ty']}, rect {it['rect']}, "
                    f"{'fine' if it['fine'] else 'coarse'}), block column {(x - it['gx0']) // bw}, block row {(y - ry0) // bh} of its grid from x = {it['gx0']}")
    return "outside the triangle's scan box"


def item_count(view, recs, blend=False):
    """work items one forward call queues over a frame's passing triangles (k_blend_setup's unaligned split when `blend`)"""
    return sum(len(plan(view, s, blend)[1]) for s in recs if s["passes"])


def describe_first_difference(world, view, ref, got, blend=False):
    """None when `got` equals the reference frame's target, else a message about the first differing sample"""
    want = ref["target"]
    if np.array_equal(want, got):
        return None
    d = np.argwhere(want != got)
    y, x = int(d[0][0]), int(d[0][1])
    sm = int(d[0][2]) if want.ndim == 3 else 0
    w, g = int(want[tuple(d[0])]), int(got[tuple(d[0])])
    msg = f"{world['name']} {view.name}: {len(d)} samples differ, first pixel ({x}, {y}) sample {sm}: expected {w:#x}, got {g:#x}"
    if view.shadow:
        on = [s for s in ref["recs"] if s.get("scan") is not None and s["passes"] and s["scan"]["inside"][y, x, sm]]
        return msg + "".join(f"; triangle {s['slot']} covers it: {locate(view, s, x, y)}" for s in on[:4])
    for name, key in (("expected", w), ("got", g)):
        slot = (key & 0xFFFFFFFF) - 1
        if 0 <= slot < len(ref["recs"]):
            s = ref["recs"][slot]
            msg += f"; {name} triangle {slot} (object {s['object']}, triangle {s['triangle']}, box {s['box']}): {locate(view, s, x, y, blend)}"
        else:
            msg += f"; {name} no triangle"
    return msg


# ------------------------------------------------------------------ worlds
def positions_f32(ob):
    """the object's vertices as the f32 array both renderers are given (conversion only: every coordinate is held exactly); the
    triangles listed in ob["neg_zero"] carry z = -0"""
    out = np.zeros((len(ob["tris"]) * 3, 3), dtype=np.float32)
    for t, tri in enumerate(ob["tris"]):
        for k, v in enumerate(tri):
            for c in range(3):
                out[3 * t + k, c] = v[c].numerator / v[c].denominator
                assert Fr(float(out[3 * t + k, c])) == v[c]
            if t in ob.get("neg_zero", ()):
                assert v[2] == 0
                out[3 * t + k, 2] = -0.0
    return out


ANCHOR = ((Fr(0), Fr(0), Fr(1, 2)),) * 3  # triangle 0 of every object: zero area, well inside both frusta


def _object(tris, **kw):
    return dict(tris=[ANCHOR] + [tuple(tuple(Fr(c) for c in v) for v in t) for t in tris], **kw)


def both_windings(tris):
    return [w for t in tris for w in (t, (t[0], t[2], t[1]))]


def flat(a, b, c, z):
    return ((a[0], a[1], z), (b[0], b[1], z), (c[0], c[1], z))


class Lattice:
    """clip-space points k / 2^m and where they fall in a W x H target"""

    def __init__(self, W, H):
        self.W, self.H, self.m = W, H, LATTICE[(W, H)]
        self.one = 1 << self.m
        g = math.gcd(W, H)
        px = Fr(W * H, g * 2 * self.one)  # pixels (in x and in y) of the step (H / g, W / g): a diagonal of the pixel grid
        t = max(1, round(4 / px))
        self.ux, self.uy = t * H // g, t * W // g

    def c(self, k):
        return Fr(k, self.one)

    def X(self, k):
        return (self.c(k) + 1) * Fr(self.W, 2)

    def Y(self, k):
        return (1 - self.c(k)) * Fr(self.H, 2)

    def at(self, fx8, fy8, near):
        """the lattice point whose window position is at (fx8, fy8) eighths inside its pixel, nearest to clip point `near`"""
        r = range(-self.one, self.one + 1)
        xs = [k for k in r if (self.X(k) * 8) % 8 == fx8 and 1 <= self.X(k) < self.W - 1]
        ys = [k for k in r if (self.Y(k) * 8) % 8 == fy8 and 1 <= self.Y(k) < self.H - 1]
        if not xs or not ys:
            return None
        return (min(xs, key=lambda k: abs(self.c(k) - near[0])), min(ys, key=lambda k: abs(self.c(k) - near[1])))


def edges_world(W, H):
    """Fans whose shared edges run through sample points (horizontal, vertical, diagonal in pixels, shallow), a strip along a row of
    pixel centres, vertices on pixel centres and on the 4x sample positions, slivers under a top edge through a row of pixel
    centres (they cover the centres on that edge and fall to the rint rule; under multisampling the rule is off), zero-area
    triangles; every triangle in both windings."""
    L = Lattice(W, H)
    ux, uy = L.ux, L.uy
    ring = [(2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (-2, 2), (-2, 0), (-2, -1), (-2, -2), (0, -2), (2, -2)]

    def fan(centre, z):
        cx, cy = centre
        pts = [(L.c(cx + dx * ux), L.c(cy + dy * uy)) for dx, dy in ring]
        return [flat((L.c(cx), L.c(cy)), pts[k], pts[(k + 1) % len(pts)], z) for k in range(len(pts))]

    fans = []
    for (fx8, fy8), near, z in (((4, 4), (Fr(-1, 3), Fr(1, 3)), Fr(1, 2)), ((3, 1), (Fr(1, 3), Fr(1, 2)), Fr(5, 8)), ((5, 7), (Fr(1, 2), Fr(-1, 3)), Fr(3, 8))):
        at = L.at(fx8, fy8, near)
        if at is not None:
            fans += fan(at, z)
    fans += fan((0, 0), Fr(1, 4))
    strip = []
    row = L.at(4, 4, (Fr(-3, 4), Fr(-3, 5)))
    for k in range(6):
        x0, x1, y0, y1 = L.c(row[0] + k * ux), L.c(row[0] + (k + 1) * ux), L.c(row[1]), L.c(row[1] - uy)
        strip += [flat((x0, y0), (x1, y0), (x1, y1), Fr(7, 16)), flat((x0, y0), (x1, y1), (x0, y1), Fr(7, 16))]
    # slivers: top edge through the pixel centres of a row j with H - j - 1 even, less than a pixel high
    rows = [k for k in range(-L.one, L.one + 1) if (L.Y(k) * 2) % 2 == 1 and (H - int(L.Y(k) - Fr(1, 2)) - 1) % 2 == 0 and 1 < L.Y(k) < H - 1]
    hy = max(1, math.floor(Fr(3, 4) / (Fr(H, 2 * L.one))))
    slivers = []
    for near in (Fr(3, 4), Fr(-1, 8), Fr(-7, 8)):
        k = min(rows, key=lambda r: abs(L.c(r) - near))
        slivers.append(flat((L.c(-3 * ux), L.c(k)), (L.c(3 * ux), L.c(k)), (L.c(ux), L.c(k - hy)), Fr(3, 4)))
    line = [flat((Fr(-1, 2), Fr(-1, 2)), (Fr(0), Fr(0)), (Fr(1, 2), Fr(1, 2)), Fr(1, 2)), flat((Fr(1, 4), Fr(0)), (Fr(1, 4), Fr(0)), (Fr(1, 2), Fr(1, 4)), Fr(1, 2))]
    return dict(name=f"edges {W}x{H}", objects=[_object(both_windings(fans)), _object(both_windings(strip)), _object(both_windings(slivers) + line)])


def boxes_world(W, H):
    """One right triangle per case (both windings): scan boxes 1, 8, 9, 16, 17, 32, 33, 64, 65 px and the full extent wide and high
    where the target has room, left edges at x0 mod 32 in {0, 1, 15, 16, 17, 31}, boxes that touch and cross the right and bottom
    borders with vertices outside the viewport, boxes one pixel wide outside it.  Constant depths, nearer from case to case."""
    L = Lattice(W, H)
    ks = range(-3 * L.one // 2, 3 * L.one // 2 + 1)

    def axis(n, pos):
        """the lattice points in window order with the box bounds they give as the smallest and as the largest coordinate"""
        pts = sorted((pos(k), k) for k in ks)
        return n, [(p, k, math.floor(p) - 1, math.ceil(p) + 1) for p, k in pts], [min(math.ceil(p) + 1, n - 1) for p, _k in pts]

    def span(ax, want, mod=None, kind="inside"):
        """lattice (ka, kb), a < b in window order, the longest whose scan box along that axis is `want` px: both vertices inside the
        target with the box unclamped, b on the border (touch), b a pixel or more outside (cross), a outside as well (beyond)"""
        n, info, his = ax
        best = None
        for i, (a, ka, f0, _) in enumerate(info):
            lo = max(f0, 0)
            if f0 > n - 1 or (kind == "inside" and f0 < 0) or (kind == "beyond" and a < n) or (mod is not None and lo % 32 != mod):
                continue
            first, last = bisect.bisect_left(his, lo + want - 1, i + 1), bisect.bisect_right(his, lo + want - 1, i + 1)
            for b, kb, _, f1 in reversed(info[first:last]):
                if f1 < 0 or (kind == "inside" and f1 > n - 1) or (kind == "touch" and b != n) or (kind == "cross" and b < n + 1):
                    continue
                if best is None or b - a > best[0]:
                    best = (b - a, ka, kb)
                break
        return None if best is None else best[1:]

    AX, AY = axis(W, L.X), axis(H, L.Y)
    widths = [8, 9, 16, 17, 32, 33, 64, 65]
    cases = []  # (x span, y span)
    mods = [0, 1, 15, 16, 17, 31]
    for i, bw in enumerate(widths):
        for bh in (widths[(i + 3) % len(widths)], widths[(i + 5) % len(widths)]):
            cases.append((span(AX, bw, mods[i % 6]) or span(AX, bw), span(AY, bh)))
    for mod in mods:
        cases.append((span(AX, 17, mod), span(AY, 9)))
        cases.append((span(AX, 33, mod), span(AY, 16)))
    cases.append((span(AX, W, None, "cross") or span(AX, W, None, "touch"), span(AY, H, None, "cross")))  # the full extent
    for kind in ("touch", "cross"):
        cases.append((span(AX, 17, None, kind), span(AY, 9)))
        cases.append((span(AX, 9, None, "inside"), span(AY, 16, None, kind)))
        cases.append((span(AX, 16, None, kind), span(AY, 9, None, kind)))
    cases.append((span(AX, 18, 15), span(AY, 9)))  # 18 px from x0 mod 16 = 15: a coarse item of k_blend_setup even in a 33 px target
    cases.append((span(AX, 1, None, "beyond"), span(AY, 9)))
    cases.append((span(AX, 9), span(AY, 1, None, "beyond")))
    tris = []
    for n, (sx, sy) in enumerate(c for c in cases if c[0] is not None and c[1] is not None):
        (xa, xb), (ya, yb) = (L.c(sx[0]), L.c(sx[1])), (L.c(sy[0]), L.c(sy[1]))
        corner = [(xa, ya), (xb, ya), (xb, yb), (xa, yb)]
        r = n % 4  # the right angle in each corner of the box in turn
        tris.append(flat(corner[r], corner[(r + 1) % 4], corner[(r + 3) % 4], Fr(n + 1, 128)))
    assert len(tris) >= 12, (W, H, len(tris))
    third = (len(tris) + 2) // 3
    obs = [_object(both_windings(tris[k:k + third])) for k in range(0, len(tris), third)]
    # the anchor lies in front of everything else at the origin only as a zero-area triangle: it draws nothing
    return dict(name=f"boxes {W}x{H}", objects=obs, cases=tris)


def depth_world(W, H):
    """Stacked constant-depth layers with exact ties (the same z in two slots: the higher slot wins), triangles at depth 0, -0, 1 and
    at the nearest dyadics outside [0, 1] of either view, and -- on power-of-two extents, where the doubled window-space area can be
    a power of two -- right triangles whose dyadic depth slopes cross z = 0 and z = 1 inside the triangle."""
    big = lambda dx, dy, z: flat((Fr(-3, 4) + dx, Fr(-1, 2) + dy), (Fr(3, 4) + dx, Fr(-1, 2) + dy), (dx, Fr(3, 4) + dy), z)
    e = Fr(1, 8)
    layers0 = [big(0, 0, Fr(1, 4)), big(e, 0, Fr(1, 2)), big(-e, e, Fr(3, 4))]
    layers1 = [big(-e, 0, Fr(1, 2)), big(0, e, Fr(3, 4)), big(e, e, Fr(1, 4)), big(0, -e, Fr(1, 2))]
    eps = Fr(1, 1 << 20)
    special, neg_zero = [], set()
    for k, z in enumerate((Fr(0), "-0", Fr(1), -eps, 1 + eps, -1 - 2 * eps, Fr(-1))):
        x = Fr(-15, 16) + k * Fr(1, 4)
        if z == "-0":
            z = Fr(0)
            neg_zero |= {1 + 2 * k, 2 + 2 * k}  # (triangle 0 is the anchor; both windings follow each other)
        special.append(flat((x, Fr(-15, 16)), (x + Fr(3, 16), Fr(-15, 16)), (x, Fr(-5, 8)), z))
    obs = [_object(both_windings(layers0)), _object(both_windings(special), neg_zero=neg_zero), _object(both_windings(layers1))]
    if W & (W - 1) == 0 and H & (H - 1) == 0:
        lx, ly = Fr(32, W), Fr(32, H)  # legs of 16 px
        sloped = []
        for k, (z0, az, bz) in enumerate(((Fr(-1, 4), Fr(3, 2), Fr(0)), (Fr(5, 4), Fr(0), Fr(-3, 2)), (Fr(-1, 4), Fr(1), Fr(1, 2)), (Fr(1, 2), Fr(3, 4), Fr(-3, 4)))):
            x, y = Fr(-7, 8) + k * Fr(7, 16), Fr(7, 8)
            sloped.append(((x, y, z0), (x + lx, y, z0 + az), (x, y - ly, z0 + bz)))
        obs.append(_object(both_windings(sloped)))
    return dict(name=f"depth {W}x{H}", objects=obs)


def random_world(W, H, seed=0x5EED, n=72):
    """seeded lattice triangles of mixed size at constant dyadic depths, either winding: the net under the planted worlds"""
    L = Lattice(W, H)
    rng = random.Random(seed * 1000 + W)
    one = L.one
    tris = []
    for k in range(n):
        reach = (one // 16, one // 4, one)[k % 3]
        cx, cy = rng.randint(-one, one), rng.randint(-one, one)
        v = [(L.c(max(-5 * one // 4, min(5 * one // 4, cx + rng.randint(-reach, reach)))),
              L.c(max(-5 * one // 4, min(5 * one // 4, cy + rng.randint(-reach, reach))))) for _ in range(3)]
        tris.append(flat(v[0], v[1], v[2], Fr(rng.randint(-1, 17), 16)))
    return dict(name=f"random {W}x{H}", objects=[_object(tris[k::3]) for k in range(3)])


_WORLDS = {}


def worlds(W, H):
    """the four worlds of an extent (built once, never modified)"""
    if (W, H) not in _WORLDS:
        _WORLDS[(W, H)] = {w["name"].split()[0]: w for w in (edges_world(W, H), boxes_world(W, H), depth_world(W, H), random_world(W, H))}
    return _WORLDS[(W, H)]


_FRAMES = {}


def frame(kind, W, H, samples=1, shadow=None):
    """render() of a world of extent (W, H) in its viewport (shadow = None) or in the shadow view of that resolution, computed once"""
    key = (kind, W, H, samples, shadow)
    if key not in _FRAMES:
        view = View(W, H, samples) if shadow is None else View(shadow, shadow, 1, shadow=True)
        _FRAMES[key] = (view, render(worlds(W, H)[kind], view))
    return _FRAMES[key]


def atlas_layout(resolutions):
    """(atlas width, height, [(x, y, size) per light]) for one or two lights of SHADOW_RESOLUTIONS, as shadow_alloc.rs lays them out:
    the largest map is a root of its own, a smaller one takes the first quarter of the next root"""
    if len(resolutions) == 1:
        return max(resolutions[0], 32), max(resolutions[0], 32), [(0, 0, resolutions[0])]
    assert list(resolutions) == [64, 32]
    return 128, 64, [(0, 0, 64), (64, 0, 32)]


def load(r, mk, world, identity, key=OPAQUE, **material):
    """The world in a renderer -- the oracle's or the product's, whichever `r` and its material_record `mk` are: per object one mesh
    (unindexed, constant normals), one unlit material under `key` and one object with the identity transform.  Returns the handles."""
    handles = []
    for n, ob in enumerate(world["objects"]):
        pos = positions_f32(ob)
        normals = np.zeros_like(pos)
        normals[:, 2] = -1.0
        kw = dict(albedo=(0.25 + 0.25 * (n % 3), 0.5, 0.75 - 0.25 * (n % 2), 1.0), albedo_mode="value", unlit=True)
        kw.update(material)
        handles.append(r.add_object(r.add_mesh(pos, normals=normals), r.add_material(mk(**kw), ob.get("key", key)), identity))
    return handles


# ------------------------------------------------------------------ the transparent pass's coverage
BLEND_LAYER_Z = Fr(9, 128)


def blend_setup(W, H, samples):
    """(view, world of the opaque layer -- z = 9/128 over the lower left half of the target --, its frame, its depth bits per sample,
    [(triangle, setup record)] of the boxes world's cases in the winding the viewport draws)"""
    view = View(W, H, samples)
    layer = flat((Fr(-1), Fr(-1)), (Fr(-1), Fr(1)), (Fr(1), Fr(-1)), BLEND_LAYER_Z)
    world = dict(name="opaque layer", objects=[_object([layer])])
    opaque = render(world, view)
    assert opaque["pass"].sum() == 1 and 0.3 < (opaque["target"] != 0).mean() < 0.7
    cases = []
    for tri in worlds(W, H)["boxes"]["cases"]:
        for t in (tri, (tri[0], tri[2], tri[1])):
            s = setup(view, t)
            if s["visible"]:
                s["passes"] = cull(view, s)[0]
                cases.append((t, s))
    assert len(cases) == len(worlds(W, H)["boxes"]["cases"])
    return view, world, opaque, (opaque["target"] >> np.uint64(32)).reshape(H, W, samples), cases


def blend_object(tri):
    """a one-triangle object without the anchor: moved away, it leaves the frustum whole"""
    return dict(objects=[dict(tris=[tuple(tuple(Fr(c) for c in v) for v in tri)])])


def blend_expected(view, s, depth_bits):
    """(pixels with a sample the transparent pass blends: covered, inside the depth clip, not behind the opaque depth; samples it
    drops behind the opaque layer)"""
    if not s["passes"]:
        return np.zeros((view.H, view.W), dtype=bool), 0
    sc = scan(view, s)
    kept = sc["kept"] & (sc["zbits"] >= depth_bits)
    return kept.any(axis=2), int((sc["kept"] & ~kept).sum())
