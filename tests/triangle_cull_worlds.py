"""The worlds tests/test_triangle_cull.py and tests/test_triangle_cull_gpu.py run through the triangle cull, and what
tests/triangle_cull_reference.py expects of each frame.

A world is arrays, written with one r3n_objects_write like the object pass's worlds (tests/object_pass_reference.py): every object
has the identity transform and a bounding sphere chosen freely (it is host-computed input of the ABI), and draws `ntri` consecutive
triangles of ONE shared index run from a start of its own.  The run draws from a table of triangles -- the catalogue of specials,
each a few triangles on either side of one rule of the decision, and a palette of robustly passing and robustly rejected ones --
in an order that gives a wave slot any ballot: all ones, all zeros, only lane 0, only lane 63, alternating, and a seeded mix.

Views: an identity view with a ("raw", M) projection -- M_AFFINE (w = 1; the 64 x 64 target's catalogue sits on the clip-space
lattice k / 2^8 where every intermediate is exact), M_ALT (the same with x and y halved: another camera for the frames with
history), M_W (w = mesh z: negative, zero and tiny w) -- and the shadow view of raster_reference.LIGHT; both handednesses; one and
four samples.  The viewport culls against the pyramid of an injected depth plane (cone_plane)."""
import numpy as np

import hiz_reference as hz
import object_pass_reference as op
import raster_reference as rr
import triangle_cull_reference as tc

f32, u32, i64 = np.float32, np.uint32, np.int64
EXTENTS = rr.EXTENTS
LIGHT = dict(rr.LIGHT, resolution=64)
DRAWN_SPHERE = np.array([0.0, 0.0, 0.0, 0.5], dtype=f32)
OUTSIDE_SPHERE = np.array([900.0, 0.0, 0.0, 0.5], dtype=f32)
MATERIAL_KEYS = np.array([tc.OPAQUE, tc.CUTOUT, tc.BLEND], dtype=np.uint8)
BEYOND_TABLE = 7  # a material index past the three-entry table: key 0


def raw(**entries):
    m = np.eye(4, dtype=f32).reshape(-1).copy()
    for k, v in entries.items():
        m[int(k[1:])] = v
    return m


M_AFFINE = raw()
M_ALT = raw(m0=0.5, m5=0.5)
# column-major: clip = (x, y, z / 8 + 1 / 4, z) -- last row (0, 0, 1, 0)
M_W = raw(m10=0.125, m14=0.25, m11=1.0, m15=0.0)
MATRICES = {"affine": M_AFFINE, "alt": M_ALT, "w": M_W}


# ------------------------------------------------------------------ the injected plane
OCC = f32(0.25)       # the occluder of the depth specials' windows
DEEP = f32(0.125)     # the smaller value in one texel of a MIN window
HOLE = (10, 10)       # (row, column) of the one texel at 0.0: only the last level sees it from the far corner


def cone_plane(w, h):
    """P[row, col] = 1/2 - max(col, h - 1 - row) / 128, exact: the level-k texel at the window's lower left corner (texel row
    mh - 1, column 0) is v_k = 1/2 - (2^k - 1) / 128, strictly decreasing in k, so the level a triangle reads decides.  On it: a
    texel at 0.0 (HOLE), and flat 2 x 2 windows at OCC with one texel at DEEP (the MIN windows) or none (the depth window)."""
    col, row = np.meshgrid(np.arange(w), np.arange(h))
    p = (f32(0.5) - np.maximum(col, h - 1 - row).astype(f32) / f32(128.0)).astype(f32)
    if w == 64 and h == 64:
        p[HOLE] = 0.0
        for j, c in enumerate(MIN_WINDOW_COLUMNS):
            p[40:42, c:c + 2] = OCC
            p[40 + j // 2, c + j % 2] = DEEP
        p[44:46, 44:46] = OCC
    return p


MIN_WINDOW_COLUMNS = (40, 44, 48, 52)  # window j has its DEEP texel at (row 40 + j // 2, column c + j % 2)


def cone_level(k):
    return f32(0.5) - f32(2 ** k - 1) / f32(128.0)


# ------------------------------------------------------------------ triangles of the 64 x 64 lattice
def clip64(s):
    """window coordinate (y up, as smin / smax count it) -> clip coordinate of the 64 x 64 target: exact on the lattice"""
    return f32(s) / f32(32.0) - f32(1.0)


def box(x0, y0, x1, y1, z=1.0, positive=False):
    """the right triangle whose window-space bounding box is [x0, x1] x [y0, y1] (64 x 64 target), det < 0 unless `positive`"""
    a, b, c = (clip64(x0), clip64(y0)), (clip64(x0), clip64(y1)), (clip64(x1), clip64(y0))
    if positive:
        b, c = c, b
    return np.array([(*a, z), (*b, z), (*c, z)], dtype=f32)


def clip_tri(pts, z=1.0):
    return np.array([(x, y, z) for x, y in pts], dtype=f32)


def catalogue():
    """[(name, positions[3, 3], expectation)] for the 64 x 64 target under M_AFFINE, a LEFT-handed viewport (visible: det < 0) and
    cone_plane.  expectation: what trace() must report for the entry -- values compared as bits.  A RIGHT-handed viewport sees
    the same triangles with the other sign rule, so every det entry is on its edge under both flag values."""
    s = f32(1.0) / f32(256.0)  # one lattice step
    out = []

    def add(name, pos, **expect):
        out.append((name, np.asarray(pos, dtype=f32), expect))
    # det: exactly 0 (collinear; a repeated vertex), one lattice step to either side
    add("det0_collinear", clip_tri([(0, 0), (8 * s, 8 * s), (16 * s, 16 * s)]), det=0.0, rule="backface")
    add("det0_repeated", clip_tri([(4 * s, 0), (4 * s, 0), (16 * s, 64 * s)]), det=0.0, rule="backface")
    add("det_step_negative", clip_tri([(0, 0), (64 * s, 64 * s + s), (128 * s, 128 * s)]), det_sign=-1, not_rule="backface")
    add("det_step_positive", clip_tri([(0, 0), (64 * s, 64 * s - s), (128 * s, 128 * s)]), det_sign=1, rule="backface")
    # rint, in x and in y: smin / smax at k + 0.5 and k + 1.5
    add("rint_x_k_even", box(2.5, 10, 3.5, 20), smin_x=2.5, smax_x=3.5, not_rule="rint_x")    # 2, 4
    add("rint_x_k_odd", box(3.5, 10, 4.5, 20), smin_x=3.5, smax_x=4.5, rule="rint_x")         # 4, 4
    add("rint_y_k_even", box(10, 6.5, 20, 7.5), smin_y=6.5, smax_y=7.5, not_rule="rint_y")    # 6, 8
    add("rint_y_k_odd", box(10, 7.5, 20, 8.5), smin_y=7.5, smax_y=8.5, rule="rint_y")         # 8, 8
    # ... and with the other winding, for the views that draw it (the shadow view, a RIGHT-handed viewport)
    add("rint_x_k_even_positive", box(2.5, 10, 3.5, 20, positive=True), smin_x=2.5, smax_x=3.5, det_sign=1)
    add("rint_x_k_odd_positive", box(3.5, 10, 4.5, 20, positive=True), smin_x=3.5, smax_x=4.5, det_sign=1)
    add("rint_y_k_even_positive", box(10, 6.5, 20, 7.5, positive=True), smin_y=6.5, smax_y=7.5, det_sign=1)
    add("rint_y_k_odd_positive", box(10, 7.5, 20, 8.5, positive=True), smin_y=7.5, smax_y=8.5, det_sign=1)
    # longest: below 1; exactly 2^k (level k: occluded) and the next value above (level k + 1: depth == occ passes)
    add("longest_below_1", box(2.25, 2.25, 2.75, 2.75), longest=0.5, mip=0)
    for k in range(0, 6):
        z = cone_level(k + 1) if k < 5 else f32(0.0)  # level 6 is one texel: the HOLE's 0.0
        exact = box(0, 0, 2 ** k, 2 ** k, z)
        above = exact.copy()
        # The smallest longest above 2^k that (mx + 1) * 32 can give, smin being 0.  2^4 and 2^5: the next f32 above, from
        # mx = -1/2 + 2^-24 (two ulps above -1/2: one alone is absorbed by mx + 1) and mx = 2^-23 -- then mx + 1 is the next f32
        # above 1/2 and above 1.  Up to 2^3 mx lies in [-1, -1/2), where a f32 steps by 2^-24 and mx + 1 is exact: the next mx
        # above gives 2^k + 2^-19, and nothing between that and 2^k is reachable (nextafter(2^k) would need a step of 2^-28 .. 2^-25
        # in mx).
        if k < 4:
            above[2, 0] = np.nextafter(exact[2, 0], f32(1.0))
            longest = f32(2 ** k) + f32(2.0) ** -19
        else:
            above[2, 0] = exact[2, 0] + (f32(2.0) ** -24 if k == 4 else f32(2.0) ** -23)
            longest = np.nextafter(f32(2 ** k), f32(np.inf))
        add(f"longest_2^{k}", exact, longest=float(2 ** k), mip=k, occ=float(cone_level(k)), rule="occluded", px_integer=True, py_integer=True)
        add(f"longest_above_2^{k}", above, longest=float(longest), next_above=(k >= 4), mip=k + 1, occ=float(z), depth=float(z), rule="visible",
            px_negative=True, py_above=True)
    # the clamp to the last level (6: one texel, the HOLE's 0.0); level 5's texel there is the cone's 1 / 128
    add("longest_64", box(0, 0, 64, 64, 0.0), longest=64.0, mip=6, occ=0.0, rule="visible", side_1=True)
    add("longest_128_clamped", box(0, 0, 128, 128, 0.0), longest=128.0, mip=6, occ=0.0, rule="visible", px_above=True, py_negative=True, side_1=True)
    add("larger_than_target", box(-64, -64, 192, 192, 0.0), longest=256.0, mip=6, occ=0.0, rule="visible")
    # the window: the far corner (px == mw - 1 and py == 0 exactly), one step wider (px > mw - 1, py < 0), centres outside [0, 1]
    add("far_corner_2^2", box(60, 60, 64, 64), mip=2, px_integer=True, py_integer=True)
    add("far_corner_wider", box(60 - 0.125, 60 - 0.125, 64, 64), mip=3, px_above=True, py_negative=True)
    add("centre_right_of_target", box(70, 30, 72, 32), mip=1, px_above=True, lx_clamped_high=True)
    add("centre_left_of_target", box(-6, 30, -4, 32), mip=1, px_negative=True, hx_clamped_low=True)
    add("centre_above_target", box(30, 70, 32, 72), mip=1, py_negative=True, hy_clamped_low=True)
    add("centre_below_target", box(30, -6, 32, -4), mip=1, py_above=True, ly_clamped_high=True)
    # depth against a flat window (texels 44 .. 45): equal passes, one ulp below is rejected, one ulp above passes
    for name, z, rule in (("depth_equal", OCC, "visible"), ("depth_ulp_below", np.nextafter(OCC, f32(0)), "occluded"),
                          ("depth_ulp_above", np.nextafter(OCC, f32(1)), "visible")):
        add(name, box(44.5, 18.5, 45.5, 19.5, z), mip=0, occ=float(OCC), depth=float(z), rule=rule, lx=44, hx=45, ly=44, hy=45)
    # MIN: the window's texels are OCC but one at DEEP, a depth between the two passes only because of that one
    for j, c in enumerate(MIN_WINDOW_COLUMNS):
        add(f"min_in_texel_{j}", box(c + 0.5, 22.5, c + 1.5, 23.5, 0.1875), mip=0, occ=float(DEEP), rule="visible", lx=c, hx=c + 1, ly=40, hy=41,
            deep_texel=j)
    return out


def w_catalogue():
    """triangles for M_W (clip w = mesh z): their rows of trace() are asserted by name in tests/test_triangle_cull.py"""
    t = f32(2.0) ** -20
    return [("w_one_negative", np.array([(0.25, 0.0, 1.0), (0.0, 0.5, -1.0), (0.5, 0.5, 1.0)], dtype=f32)),
            ("w_one_negative_flipped", np.array([(0.25, 0.0, 1.0), (0.5, 0.5, 1.0), (0.0, 0.5, -1.0)], dtype=f32)),
            ("w_all_negative", np.array([(0.25, 0.0, -1.0), (0.0, 0.5, -2.0), (0.5, 0.5, -1.0)], dtype=f32)),
            ("w_all_negative_flipped", np.array([(0.25, 0.0, -1.0), (0.5, 0.5, -1.0), (0.0, 0.5, -2.0)], dtype=f32)),
            ("w_one_zero", np.array([(0.25, 0.0, 1.0), (0.0, 0.5, 0.0), (0.5, 0.5, 1.0)], dtype=f32)),
            ("w_one_zero_flipped", np.array([(0.25, 0.0, 1.0), (0.5, 0.5, 1.0), (0.0, 0.5, 0.0)], dtype=f32)),
            ("w_two_zero", np.array([(0.5, 0.25, 0.0), (-0.5, 0.5, 0.0), (0.25, 0.0, 1.0)], dtype=f32)),      # x / w = +inf and -inf: a NaN centre
            ("w_two_zero_flipped", np.array([(0.5, 0.25, 0.0), (0.25, 0.0, 1.0), (-0.5, 0.5, 0.0)], dtype=f32)),
            ("w_tiny", np.array([(0.25 * t, 0.0, t), (0.0, 0.5 * t, t), (0.5 * t, 0.5 * t, t)], dtype=f32)),
            ("w_tiny_flipped", np.array([(0.25 * t, 0.0, t), (0.5 * t, 0.5 * t, t), (0.0, 0.5 * t, t)], dtype=f32)),
            ("w_two", np.array([(0.5, 0.0, 2.0), (0.0, 1.0, 2.0), (1.0, 1.0, 2.0)], dtype=f32)),
            ("w_two_flipped", np.array([(0.5, 0.0, 2.0), (1.0, 1.0, 2.0), (0.0, 1.0, 2.0)], dtype=f32))]


PALETTE_KINDS = ("pass", "back", "rint", "occluded")
PALETTE_WEIGHTS = (0.5, 0.3, 0.1, 0.1)
PALETTE_PER_KIND = 16


def palette(seed=7):
    """[(kind, positions)]: "pass" faces the LEFT viewport at depth 1 (nothing occludes it), "back" is its mirror (the shadow view
    and a RIGHT-handed viewport draw it instead), "rint" is a third of a pixel long, "occluded" faces the viewport at depth -1/2,
    below every texel of every plane.  Boxes of 2 .. 6 px on the quarter-pixel lattice, all over the target."""
    rng = np.random.default_rng(seed)
    out = []
    for kind in PALETTE_KINDS:
        for _ in range(PALETTE_PER_KIND):
            x0, y0 = rng.integers(8, 200, size=2) / 4.0
            dx, dy = rng.integers(9, 24, size=2) / 4.0
            if kind == "rint":
                x0, dx = np.floor(x0) + 0.625, 0.25
            out.append((kind, box(x0, y0, x0 + dx, y0 + dy, -0.5 if kind == "occluded" else 1.0, positive=kind == "back")))
    return out


class Table:
    """the triangles the index run draws from: the catalogue, the M_W triangles, the palette"""

    def __init__(self):
        self.cat, self.wcat, self.pal = catalogue(), w_catalogue(), palette()
        self.names = [n for n, *_ in self.cat] + [n for n, _ in self.wcat] + [f"{k}_{i}" for i, (k, _) in enumerate(self.pal)]
        self.positions = np.stack([p for _n, p, _e in self.cat] + [p for _n, p in self.wcat] + [p for _k, p in self.pal]).astype(f32)
        self.n_special = len(self.cat) + len(self.wcat)
        self.pal_kind = np.array([PALETTE_KINDS.index(k) for k, _ in self.pal])

    def __len__(self):
        return len(self.positions)

    def pal_ids(self, kind):
        return self.n_special + np.flatnonzero(self.pal_kind == PALETTE_KINDS.index(kind))


TABLE = Table()
FORMS = ("all_ones", "all_zeros", "lane_0", "lane_63", "alternating")  # the ballots of the run's first five wave slots
RUN_RANDOM = 4096


def index_run(seed=11):
    """triangle ids: five 64-entry stretches with the FORMS' ballots (for an object that starts at 0, under the LEFT affine
    viewport), every table entry once, then RUN_RANDOM palette draws by PALETTE_WEIGHTS"""
    rng = np.random.default_rng(seed)
    t = TABLE
    ok, no = t.pal_ids("pass"), np.concatenate([t.pal_ids("back"), t.pal_ids("rint"), t.pal_ids("occluded")])
    lane = np.arange(64)
    good, bad = ok[lane % len(ok)], no[lane % len(no)]
    parts = [good, bad, np.where(lane == 0, good, bad), np.where(lane == 63, good, bad), np.where(lane % 2 == 0, good, bad), np.arange(len(t))]
    kinds = rng.choice(len(PALETTE_KINDS), size=RUN_RANDOM, p=PALETTE_WEIGHTS)
    pick = rng.integers(0, PALETTE_PER_KIND, size=RUN_RANDOM)
    parts.append(np.array([t.pal_ids(PALETTE_KINDS[k])[j] for k, j in zip(kinds, pick)]))
    return np.concatenate(parts).astype(i64)


RUN = index_run()
MESH_INDICES = (3 * RUN[:, None] + np.arange(3)[None, :]).reshape(-1).astype(u32)
MESH_POSITIONS = TABLE.positions.reshape(-1, 3)
RANDOM_FROM = 5 * 64 + len(TABLE)


# ------------------------------------------------------------------ worlds
NTRI_VALUES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049)
# the order puts every slot kind into the launch (tests/test_triangle_cull.py asserts it from slot_plan)
STRUCTURE_ORDER = (2049, 65, 1, 129, 63, 1025, 64, 257, 127, 1024, 128, 255, 256, 1023, 1, 65, 1, 1, 127, 1)


def make_world(ntri, seed, materials=None, from_start=True):
    """objects with the given triangle counts: those of 320 triangles and more start at the run's first entry (their first five
    wave slots carry the FORMS), the others somewhere in the seeded part; keys in turn unless `materials` is given"""
    rng = np.random.default_rng([seed, len(ntri)])
    ntri = np.asarray(ntri, dtype=i64)
    n = len(ntri)
    # (no object ends in the run's last 64 entries: the wave slot a triangle count leaves partly filled still lies inside the run)
    start = np.array([0 if (t >= 320 and from_start) else int(rng.integers(RANDOM_FROM, len(RUN) - 64 - t + 1)) for t in ntri], dtype=i64)
    if materials is None:
        materials = np.array([(0, 1, 0, BEYOND_TABLE, 0, 1)[i % 6] for i in range(n)], dtype=u32)
    return dict(capacity=n, ntri=ntri.copy(), start=start, enabled=np.ones(n, dtype=bool), material=np.asarray(materials, dtype=u32).copy(),
                spheres=np.tile(DRAWN_SPHERE, (n, 1)))


def structure_world(blend=True):
    w = make_world(STRUCTURE_ORDER, seed=1)
    if blend:  # two blend objects: their passing triangles go to key 2's regions (the residual list alone is drawn from there)
        w["material"][[1, 3]] = tc.BLEND
    return w


def wrap_world():
    """more than 32 chunks (512 wave slots): chunk 32 appends to sub-list 0 again, behind chunk 0's entries"""
    return make_world([2049, 1025, 1024, 257] * 8 + [65, 1, 129, 64], seed=2)


def second_trip_world():
    """65 700 one-triangle objects: 4 107 chunks on a grid capped at 4 096 blocks, so blocks 0 .. 10 take a second trip"""
    n = 65_700
    return make_world(np.ones(n, dtype=i64), seed=3, materials=(np.arange(n) % 2).astype(u32))


def records(world, mesh, first=0, slots=None):
    """r3n_object128 rows of the world's slots [first, capacity) or of `slots`"""
    sl = np.arange(first, world["capacity"]) if slots is None else np.asarray(slots)
    rec = np.zeros((len(sl), 32), dtype=u32)
    rf = rec.view(f32)
    rf[:, 0] = rf[:, 5] = rf[:, 10] = rf[:, 15] = 1.0
    rf[:, 16:20] = world["spheres"][sl]
    rec[:, 20] = mesh.first_index + 3 * world["start"][sl]
    rec[:, 21] = 3 * world["ntri"][sl]
    rec[:, 22] = world["material"][sl]
    rec[:, 23:29] = np.asarray(mesh.attr_off, dtype=u32)
    rec[:, 29] = world["enabled"][sl]
    return rec


def setup_renderer(r, mk, oracle_side=False):
    """the shared mesh and the three materials (index == key) on an oracle or product renderer.  The oracle indexes its material
    table unchecked, so it gets what the product defines for an index beyond the table spelled out: entries up to BEYOND_TABLE
    that repeat material 0 with key 0."""
    m = r.add_mesh(MESH_POSITIONS, MESH_INDICES, mesh_handedness=0)
    r.add_material(mk(albedo=(0.2, 0.6, 0.9, 1.0), albedo_mode="value", unlit=True), tc.OPAQUE)
    r.add_material(mk(albedo=(0.9, 0.5, 0.1, 0.9), albedo_mode="value", unlit=True, cutout=0.5), tc.CUTOUT)
    r.add_material(mk(albedo=(0.3, 0.9, 0.3, 0.5), albedo_mode="value", unlit=True), tc.BLEND)
    if oracle_side:
        for _ in range(3, BEYOND_TABLE + 1):
            r.add_material(mk(albedo=(0.2, 0.6, 0.9, 1.0), albedo_mode="value", unlit=True), tc.OPAQUE)
    return r.meshes[m]


class _BlendMesh:
    def __init__(self, ntri):
        self.index_count = 3 * int(ntri)


def load_oracle(o, world, mesh):
    """the world's records as the oracle's object buffer; blend objects get the bookkeeping its transparent pass reads"""
    recs = records(world, mesh)
    o.objects = recs
    o.capacity = world["capacity"]
    o.object_meta = {}
    for h in np.flatnonzero((world["material"] == tc.BLEND) & world["enabled"]):
        o.meshes.append(_BlendMesh(world["ntri"][h]))
        o.object_meta[int(h)] = dict(mesh=len(o.meshes) - 1, material=tc.BLEND, enabled=True, location=recs[h].view(f32)[16:19].copy())
    return recs


# ------------------------------------------------------------------ what a frame must leave
def view_headers(matrix, handedness, extent, samples, capacity, light):
    """[(name, header, shadow view's atlas record or None)]: the shadow view first (when `light`), then the viewport"""
    from oracle import host as oh
    from oracle.lib import get as get_lib
    W, H = extent
    cam = oh.CameraState(oh.identity(), ("raw", matrix), handedness, f32(W) / f32(H))
    out = []
    if light:
        _size, shadows, _buf = oh.evaluate_directional_lights([LIGHT], cam)
        sh = shadows[0]
        out.append(("shadow", oh.camera_header(sh["camera"], 0, (sh["size"], sh["size"]), 1, capacity, get_lib()), sh))
    out.append(("viewport", oh.camera_header(cam, None, (W, H), samples, capacity, get_lib()), None))
    return out


def frame_expectation(world, hdr, pyramid, prev=None):
    """the reference's answer for one camera of one frame: expected_lists over the world, the verdicts from the table.  `hdr`: the
    camera's header (flags, resolution, shadow index); the matrices are the oracle's baked ones (the object pass's pin ties
    them to the product), one for all objects since every transform is the identity."""
    recs = records(world, op.NoMesh)
    hu = hdr.view(u32)
    shadow = int(hu[32]) != tc.INVALID
    flags = int(hu[58])
    res = (hdr[56], hdr[57])
    drawn = op.oracle_inside(hdr, recs)
    baked = op.oracle_baked(hdr, recs)
    live = np.flatnonzero(world["enabled"] & (world["ntri"] > 0))
    mvp = baked[live[0], 16:32] if len(live) else np.eye(4, dtype=f32).reshape(-1)
    assert (baked[live, 16:32].view(u32) == mvp.view(u32)).all(), "one matrix for every object"
    desc = None if shadow else tc.hiz_desc(int(res[0]), int(res[1]))
    tr = tc.trace(flags, shadow, res, mvp, TABLE.positions, pyramid, desc)
    ntri = np.where(world["enabled"], world["ntri"], 0)
    obj = np.repeat(np.arange(world["capacity"]), ntri)
    base = np.zeros(world["capacity"], dtype=i64)
    base[1:] = np.cumsum(ntri[:-1])
    ids = RUN[world["start"][obj] + (np.arange(len(obj)) - base[obj])]
    e = tc.expected_lists(ntri, tc.material_key(world["material"], MATERIAL_KEYS), drawn, tr["visible"][ids], shadow=shadow, prev=prev)
    e.update(trace=tr, ids=ids, baked=baked, shadow=shadow, flags=flags, start=world["start"], plan=tc.slot_plan(ntri[e["drawn"]]))
    return e


def pyramid_of(plane):
    return hz.pyramid(plane)


# ------------------------------------------------------------------ sequences with history
def sequence_steps():
    """[(matrix name, edit)] of the six frames: the camera alternates (last frame's bits differ per lane from this frame's); slots
    are disabled and re-enabled (the slot bases move); the world grows past its capacity (no last-frame slot base for the new
    slots); a slot is rewritten with another triangle count; a slot leaves the frustum for a frame (no history on return)."""
    def f1(w):
        w["enabled"][[0, 4, 5]] = False

    def f2(w):
        w["enabled"][[0, 4, 5]] = True
        grown = make_world(list(w["ntri"]) + [257, 64, 1, 1025, 65, 64], seed=5)
        n = w["capacity"]
        for k in ("ntri", "start", "enabled", "material", "spheres"):
            w[k] = np.concatenate([w[k], grown[k][n:]])
        w["capacity"] = grown["capacity"]

    def f3(w):
        w["ntri"][2], w["start"][2] = 129, 0      # was 1
        w["ntri"][5], w["start"][5] = 640, 0      # was 1025
        w["spheres"][[3, 6]] = OUTSIDE_SPHERE

    def f4(w):
        w["spheres"][[3, 6]] = DRAWN_SPHERE

    return [("affine", None), ("alt", f1), ("affine", f2), ("alt", f3), ("affine", f4), ("alt", None)]


# ------------------------------------------------------------------ the runs of both test files
# world, target, handedness, samples, the projection of every frame (frame 1 has history), whether LIGHT is in the world
RUNS = {
    "structure-64x64-left": dict(world="structure", extent=(64, 64), hand="left", samples=1, frames=("affine", "alt"), light=True),
    "structure-64x64-right": dict(world="structure", extent=(64, 64), hand="right", samples=1, frames=("affine", "alt"), light=True),
    "structure-64x64-left-4-samples": dict(world="structure", extent=(64, 64), hand="left", samples=4, frames=("affine", "alt"), light=False),
    "structure-96x40-left": dict(world="structure", extent=(96, 40), hand="left", samples=1, frames=("affine", "alt"), light=False),
    "structure-33x17-right": dict(world="structure", extent=(33, 17), hand="right", samples=1, frames=("affine", "alt"), light=False),
    "structure-64x64-left-w": dict(world="structure", extent=(64, 64), hand="left", samples=1, frames=("w", "affine"), light=False),
    "structure-64x64-right-w": dict(world="structure", extent=(64, 64), hand="right", samples=1, frames=("w", "w"), light=True),
    "wrap-64x64-left": dict(world="wrap", extent=(64, 64), hand="left", samples=1, frames=("affine", "alt"), light=True),
    "second-trip-64x64-left": dict(world="second_trip", extent=(64, 64), hand="left", samples=1, frames=("affine",), light=True),
}
WORLDS = {"structure": structure_world, "wrap": wrap_world, "second_trip": second_trip_world}
ORACLE_FRAME_MAX = 4096  # worlds up to here are also compared against whole oracle frames on the GPU


def handedness(name):
    from oracle import host as oh
    return oh.LEFT if name == "left" else oh.RIGHT


def copy_world(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def rewritten_slots(before, after):
    """slots whose triangle count changed in place between two frames' worlds (both counts non-zero)"""
    n = min(before["capacity"], after["capacity"])
    a = np.where(before["enabled"][:n], before["ntri"][:n], 0)
    b = np.where(after["enabled"][:n], after["ntri"][:n], 0)
    return np.flatnonzero((a != 0) & (b != 0) & (a != b))


def run_frames(run):
    """[(world, matrix name)] of a run's frames: RUNS' static worlds, or the six frames of sequence_steps"""
    if run == "sequence":
        w, out = structure_world(), []
        for name, edit in sequence_steps():
            w = copy_world(w)
            if edit is not None:
                edit(w)
            out.append((w, name))
        return dict(extent=(64, 64), hand="left", samples=1, light=True), out
    cfg = RUNS[run]
    w = WORLDS[cfg["world"]]()
    return cfg, [(w, name) for name in cfg["frames"]]


class Expect:
    """the reference's expectations frame after frame, history kept per view"""

    def __init__(self, cfg):
        self.cfg, self.prev = cfg, {}

    def frame(self, world, matrix_name, pyramid):
        cfg = self.cfg
        out = {}
        for name, hdr, sh in view_headers(MATRICES[matrix_name], handedness(cfg["hand"]), cfg["extent"], cfg["samples"], world["capacity"], cfg["light"]):
            e = frame_expectation(world, hdr, None if name == "shadow" else pyramid, self.prev.get(name))
            e["header"] = hdr
            out[name] = self.prev[name] = e
        return out


class OracleRun:
    """whole oracle frames of a run's worlds, the plane injected at the oracle's pass-1 depth hook (one sample; with four the
    oracle exchanges keys there and the pyramid is the frame's own)"""

    def __init__(self, cfg):
        from oracle import host as oh
        from oracle.world import OracleRenderer, material_record
        self.oh, self.cfg = oh, cfg
        self.o = OracleRenderer(handedness(cfg["hand"]), f32(cfg["extent"][0]) / f32(cfg["extent"][1]))
        self.mesh = setup_renderer(self.o, material_record, oracle_side=True)
        if cfg["light"]:
            self.o.add_directional_light(**LIGHT)
        self.world = None

    def frame(self, world, matrix_name, plane):
        o, cfg = self.o, self.cfg
        if self.world is not None and "viewport" in o.cam_state:
            # the product's rule for a slot rewritten in place with another triangle count (it is "not batched last frame"); rend3's
            # own API cannot do that -- a handle rests a frame before it is reused -- so the oracle is told
            st = o.cam_state["viewport"]["tri_base_or_invalid"]
            for s in rewritten_slots(self.world, world):
                if s < len(st):
                    st[s] = tc.INVALID
        self.world = world
        load_oracle(o, world, self.mesh)
        o.set_camera_data(self.oh.identity(), ("raw", MATRICES[matrix_name]))
        from test_hiz_gpu import oracle_hook  # (the module needs no GPU to import)
        return o.render(*cfg["extent"], samples=cfg["samples"], exchange=oracle_hook(plane))


def plane_of(cfg):
    """the plane a frame injects; None with four samples"""
    return cone_plane(*cfg["extent"]) if cfg["samples"] == 1 else None


def ballots(e):
    """u64 per wave slot of e["plan"] (padding: 0): bit l = triangle 64 wrel + l of the slot's object passes"""
    plan = e["plan"]
    out = np.zeros(len(plan["entry"]), dtype=np.uint64)
    slots = np.flatnonzero(e["drawn"])
    entry_of = np.full(len(e["drawn"]), -1, dtype=i64)
    entry_of[slots] = np.arange(len(slots))
    sel = np.flatnonzero(e["pass"] != 0)
    obj, tri = e["object"][sel], e["triangle"][sel]
    np.bitwise_or.at(out, plan["wave_start"][entry_of[obj]] + tri // 64, np.uint64(1) << (tri % 64).astype(np.uint64))
    return out


def previous_ballots(e, prev):
    """last frame's bits of each of this frame's wave slots (0 where the object has no history)"""
    out = np.zeros(len(e["plan"]["entry"]), dtype=np.uint64)
    if prev is None:
        return out
    pb, slots, pslots = ballots(prev), np.flatnonzero(e["drawn"]), np.flatnonzero(prev["drawn"])
    pentry = np.full(max(len(prev["drawn"]), len(e["drawn"])), -1, dtype=i64)
    pentry[pslots] = np.arange(len(pslots))
    for s in np.flatnonzero(e["plan"]["entry"] >= 0):
        o = slots[e["plan"]["entry"][s]]
        if pentry[o] >= 0 and o < len(prev["ntri"]) and prev["ntri"][o] == e["ntri"][o]:
            out[s] = pb[prev["plan"]["wave_start"][pentry[o]] + e["plan"]["wrel"][s]]
    return out


# ------------------------------------------------------------------ a list as the device holds it, against the expectation
def where(e, obj, tri):
    """an (object, triangle) in the terms of the launch that culled it"""
    obj, tri = int(obj), int(tri)
    if obj >= len(e["drawn"]) or not e["drawn"][obj]:
        return f"object {obj} triangle {tri}: the object is not drawn in this view"
    entry = int(np.searchsorted(np.flatnonzero(e["drawn"]), obj))
    slot = int(e["plan"]["wave_start"][entry]) + tri // 64
    name = TABLE.names[int(RUN[int(e["start"][obj]) + tri])] if tri < int(e["ntri"][obj]) else "beyond the object"
    return (f"object {obj} (key {int(e['key'][obj])}, {int(e['ntri'][obj])} triangles) triangle {tri} = lane {tri % 64} of wave slot {tri // 64} of the "
            f"object, table entry {name}: {tc.describe_slot(e['plan'], slot)}")


def key64(rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 2)
    return (rows[:, 0] << np.uint64(32)) | rows[:, 1]


def expected_subcap(e, capacity):
    """r3n_cull's reservation per (key, sub-list): every chunk of the launch's upper bound of wave slots (triangles / 64 +
    capacity + 1), all of its slots passing under one key"""
    max_waves = e["total"] // 64 + capacity + 1
    chunks = (max_waves + tc.CHUNK_WAVES - 1) // tc.CHUNK_WAVES
    return (chunks + tc.SUBQ - 1) // tc.SUBQ * tc.CHUNK_WAVES * 64


LIST_NAMES = ("predicted", "residual")


def check_list(e, which, refs, counts, subcap, capacity, vertex_counts, pass_set, tag):
    """One list of one camera as r3n_readback_triangle_lists returned it (refs: the regions' entries in (key, sub-list) order,
    counts[3][SUBQ]) against expectation `e`: no count above the reservation; 3 x the counts are the draw calls' vertex counts;
    every entry names a triangle of an object; none occurs twice; none sits under another key or in another sub-list than its
    chunk's; per key exactly the expected entries; the predicted list names exactly the triangles of the result-bit set."""
    u64 = np.uint64
    want = e["predicted"] if which == 0 else e["residual_list"]
    t = f"{tag} {LIST_NAMES[which]} list"
    assert subcap == expected_subcap(e, capacity), f"{t}: {subcap} entries reserved per region, {expected_subcap(e, capacity)} expected"
    over = np.argwhere(counts > subcap)
    assert len(over) == 0, f"{t}: count {int(counts[tuple(over[0])])} of key {over[0][0]} sub-list {over[0][1]} exceeds the {subcap} reserved"
    assert np.array_equal(3 * counts.sum(axis=1, dtype=i64), np.asarray(vertex_counts, dtype=i64)), f"{t}: 3 x counts {3 * counts.sum(axis=1)} != vertex counts {vertex_counts}"
    flat = counts.reshape(-1).astype(i64)
    assert len(refs) == flat.sum()
    ek = np.repeat(np.repeat(np.arange(3), tc.SUBQ), flat)  # the region every entry sits in
    eq = np.repeat(np.tile(np.arange(tc.SUBQ), 3), flat)
    obj, tri = refs[:, 0].astype(i64), refs[:, 1].astype(i64)
    bad = np.flatnonzero((obj >= capacity) | (tri >= e["ntri"][np.minimum(obj, capacity - 1)]))
    assert len(bad) == 0, f"{t}: entry ({obj[bad[0]]}, {tri[bad[0]]}) in key {ek[bad[0]]} sub-list {eq[bad[0]]} names no triangle (stale or never written)"
    all_keys = key64(refs)
    _u, first, n = np.unique(all_keys, return_index=True, return_counts=True)
    dup = np.flatnonzero(n > 1)
    assert len(dup) == 0, f"{t}: {len(dup)} entries occur more than once, first {where(e, obj[first[dup[0]]], tri[first[dup[0]]])}"
    foreign = np.flatnonzero(e["key"][obj] != ek)
    assert len(foreign) == 0, f"{t}: {len(foreign)} entries sit in another key's region, first in key {ek[foreign[0]]}: {where(e, obj[foreign[0]], tri[foreign[0]])}"
    for k in range(3):
        have, need = np.sort(all_keys[ek == k]), np.sort(key64(want[k]))
        missing, extra = np.setdiff1d(need, have), np.setdiff1d(have, need)
        assert len(missing) == 0, f"{t}: key {k} lacks {len(missing)} entries, first {where(e, missing[0] >> u64(32), missing[0] & u64(0xFFFFFFFF))}"
        assert len(extra) == 0, f"{t}: key {k} holds {len(extra)} entries too many, first {where(e, extra[0] >> u64(32), extra[0] & u64(0xFFFFFFFF))}"
    entry = np.searchsorted(np.flatnonzero(e["drawn"]), obj)
    chunk = (e["plan"]["wave_start"][entry] + tri // 64) // tc.CHUNK_WAVES
    stray = np.flatnonzero(chunk % tc.SUBQ != eq)
    assert len(stray) == 0, f"{t}: {len(stray)} entries sit in another sub-list than their chunk's, first in sub-list {eq[stray[0]]}: {where(e, obj[stray[0]], tri[stray[0]])}"
    if which == 0:
        rebuilt = np.zeros(max(e["total"], 1), dtype=np.uint8)
        rebuilt[e["tri_base"][obj] + tri] = 1
        assert np.array_equal(rebuilt[: e["total"]], np.asarray(pass_set)[: e["total"]]), f"{t}: not the set the result bits give"


def simulate_list(e, which):
    """(refs, counts) of a list as a launch that handles the chunks in order leaves it: a chunk's entries of a key in wave-slot
    and lane order, behind those of the earlier chunks of its sub-list"""
    rows = np.concatenate(e["predicted"] if which == 0 else e["residual_list"]).astype(i64).reshape(-1, 2)
    obj, tri = rows[:, 0], rows[:, 1]
    entry = np.searchsorted(np.flatnonzero(e["drawn"]), obj)
    slot = e["plan"]["wave_start"][entry] + tri // 64
    chunk = slot // tc.CHUNK_WAVES
    key, q = e["key"][obj], chunk % tc.SUBQ
    order = np.lexsort((tri, slot, chunk, q, key))
    counts = np.zeros((3, tc.SUBQ), dtype=u32)
    np.add.at(counts, (key, q), 1)
    return rows[order].astype(u32), counts
