"""Textures, query sets and the path classifier of the texture-sampler tests (test_sampler.py on the CPU, test_sampler_gpu.py on the
GPU).  Nothing of the product is imported here: the table is added to any renderer that has the two texture calls tests/scenes.py
uses (add_texture_2d_encoded for the stored chains, so that every level holds texels of its own and a mixed-up level shows), the
query sets are plain structured arrays in the layout of r3n_sample_query40 / r3o_sample_queries, and `paths` restates -- in f32
arithmetic carried out by numpy, operation by operation -- the conditions rend3_amd/csrc/texture.h branches on: UPDATE IT WITH THEM.

Wave structure: the probe runs one thread per query and 64 consecutive queries as one wavefront.  Every set is laid out by
`arrange`: first whole waves of one kind each (a kind's queries, padded to a multiple of 64 with its own), then the same queries
again interleaved lane by lane, so that neighbouring lanes are of different kinds."""
import numpy as np

f32 = np.float32
QUERY = np.dtype([("id", np.uint32, 3), ("nearest", np.uint32), ("u", f32), ("v", f32), ("ddx", f32, 2), ("ddy", f32, 2)])
RESULT = np.dtype([("rgba", f32, (3, 4)), ("flags", np.uint32)])
assert QUERY.itemsize == 40 and RESULT.itemsize == 52
WAVE = 64

# index = R3N_PROBE_* (include/r3n.h)
FORMS = ("grad", "grad_rgb", "short", "short_rgb", "share", "alpha", "alpha_short", "batched")
SHORT_ONLY_FORMS = ("short", "short_rgb", "share", "alpha_short", "batched")
THREE_MAP_FORMS = ("share", "batched")

RGBA8, RGBA8_SRGB, RGBA16F, RGBA32F = 0, 1, 21, 24  # R3N_TEXTURE_* ids of the formats the table uses
POOL_FLOAT = 2                                        # device-side descriptor format of the float-decoded textures


# ------------------------------------------------------------------------------------------------------------------ the table
def full_mips(w, h):
    return int(max(w, h)).bit_length()


#        name         w    h   mips (None = full chain)  source format  contents
SPECS = [
    ("s64",          64,  64, None, RGBA8_SRGB, "random"),
    ("l64",          64,  64, None, RGBA8,      "random"),
    ("l32",          32,  32, None, RGBA8,      "random"),
    ("s16",          16,  16, None, RGBA8_SRGB, "random"),
    ("r128x32",     128,  32, None, RGBA8,      "random"),
    ("r32x128",      32, 128, None, RGBA8_SRGB, "random"),
    ("w64x1",        64,   1, None, RGBA8,      "random"),
    ("h1x64",         1,  64, None, RGBA8,      "random"),
    ("t2",            2,   2, None, RGBA8,      "random"),
    ("t1",            1,   1, None, RGBA8_SRGB, "random"),
    ("c64m3",        64,  64, 3,    RGBA8,      "random"),
    ("big256",      256, 256, 1,    RGBA8,      "random"),
    ("odd37x19",     37,  19, None, RGBA8_SRGB, "random"),
    ("odd3x5",        3,   5, None, RGBA8,      "random"),
    ("f32_8",         8,   8, None, RGBA32F,    "float"),
    ("f16_16x4",     16,   4, None, RGBA16F,    "float"),
    ("a255",         32,  32, None, RGBA8,      ("alpha", 255, 255)),
    ("a0",           32,  32, None, RGBA8,      ("alpha", 0, 0)),
    ("a0_255",       32,  32, None, RGBA8,      ("alpha", 0, 255)),
    ("a254_255",     32,  32, None, RGBA8,      ("alpha", 254, 255)),
    ("a0_1",         32,  32, None, RGBA8,      ("alpha", 0, 1)),
    ("a128",         32,  32, None, RGBA8,      ("alpha", 128, 128)),
    ("last16",       16,  16, None, RGBA8,      "random"),
]
ALPHA_NAMES = ("a255", "a0", "a0_255", "a254_255", "a0_1", "a128")
ORDERS = ("a", "b")  # "a": as listed, last16's 1x1 level is the pool's final word; "b": w64x1 moved behind it instead


def _levels(spec, seed):
    """The stored levels' bytes of one texture, largest first: contents depend on the texture's name alone, not on its slot."""
    name, w, h, mips, fmt, kind = spec
    mips = full_mips(w, h) if mips is None else mips
    rng = np.random.default_rng([seed, sum(ord(c) * (k + 1) for k, c in enumerate(name))])
    out = []
    for k in range(mips):
        lw, lh = max(1, w >> k), max(1, h >> k)
        if kind == "float":
            # finite, some above 1, some negative; halves are exact in both float formats' decoders
            vals = rng.integers(-64, 192, (lh, lw, 4)).astype(np.float32) / np.float32(64.0)
            out.append(vals.astype(np.float16).tobytes() if fmt == RGBA16F else vals.astype(np.float32).tobytes())
            continue
        texels = rng.integers(0, 256, (lh, lw, 4), dtype=np.uint8)
        if kind != "random":
            _, lo, hi = kind
            block = max(1, 8 >> k)  # 8x8 blocks at level 0, halved with the level
            yy, xx = np.mgrid[0:lh, 0:lw]
            texels[..., 3] = np.where(((xx // block) + (yy // block)) % 2 == 0, lo, hi).astype(np.uint8)
        out.append(texels.tobytes())
    return out


class Table:
    """The texture table in one of its two orders.  Descriptors as both libraries hold them (offset, width, height, mips, pool
    format) follow from the specs alone; `pool` is set by `build` from a renderer that keeps its decoded words (the oracle)."""

    def __init__(self, order="a", seed=0x5A4D):
        assert order in ORDERS
        specs = list(SPECS)
        if order == "b":
            specs.append(specs.pop([s[0] for s in specs].index("w64x1")))
        self.order, self.seed, self.specs = order, seed, specs
        self.names = [s[0] for s in specs]
        self.descs = np.zeros((len(specs), 8), dtype=np.uint32)
        at = 0
        for row, (name, w, h, mips, fmt, kind) in zip(self.descs, specs):
            is_float = fmt in (RGBA16F, RGBA32F)
            at = (at + 3) & ~3  # every texture starts on a 4-word boundary of the pool
            mips = full_mips(w, h) if mips is None else mips
            row[:5] = (at, w, h, mips, POOL_FLOAT if is_float else fmt)
            at += sum(max(1, w >> k) * max(1, h >> k) for k in range(mips)) * (4 if is_float else 1)
        self.pool_words = at
        self.pool = None

    def id(self, name):
        """material texture id (slot + 1)"""
        return self.names.index(name) + 1

    def desc(self, name):
        return self.descs[self.names.index(name)]

    def is_short(self, idx):
        """r3n.hip texture_is_short: power-of-two extents, RGBA8 pool texels"""
        _, w, h, _, fmt = (int(x) for x in self.descs[idx][:5])
        return w > 0 and h > 0 and (w & (w - 1)) == 0 and (h & (h - 1)) == 0 and fmt < POOL_FLOAT

    def short_names(self):
        return [n for i, n in enumerate(self.names) if self.is_short(i)]

    def build(self, r):
        """Adds the table to a renderer, in order; returns the handles (== slot indices)."""
        handles = []
        for spec in self.specs:
            name, w, h, mips, fmt, kind = spec
            handles.append(r.add_texture_2d_encoded(fmt, w, h, _levels(spec, self.seed)))
        assert handles == list(range(len(self.specs)))
        pool = getattr(r, "tex_pool", None)
        if pool is not None and pool.dtype == np.uint32:
            # a renderer that keeps its decoded pool words (the oracle): the classifier and the known answers read texels there, at
            # ITS offsets (it packs RGBA8 textures without the 4-word alignment of the product's pool; nothing else differs)
            assert np.array_equal(r.tex_descs[:, 1:5], self.descs[:, 1:5]), "the table's descriptors are not what the renderer derived"
            self.descs, self.pool = r.tex_descs.copy(), pool
        return handles

    def levels_of(self, name):
        return _levels(self.specs[self.names.index(name)], self.seed)

    def level_start(self, idx, level):
        """pool word of the first texel of a level (the walk over the chain)"""
        off, w, h, mips, fmt = (int(x) for x in self.descs[idx][:5])
        words = 4 if fmt == POOL_FLOAT else 1
        return off + words * sum(max(1, w >> k) * max(1, h >> k) for k in range(level))


# ------------------------------------------------------------------------------------------------------------------ f32 helpers
def up(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return x


def down(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return x


def lod(w, h, mips, ddx, ddy):
    """(level, frac, rho) of the contract for arrays of gradients -- every operation in f32, as r3o.c and texture.h write it; level
    and frac AFTER the clamp to the last level, BEFORE the nearest sampler's rounding."""
    ddx = np.asarray(ddx, dtype=f32).reshape(-1, 2)
    ddy = np.asarray(ddy, dtype=f32).reshape(-1, 2)
    W, H = np.asarray(w).astype(f32), np.asarray(h).astype(f32)
    mips = np.broadcast_to(np.asarray(mips, dtype=np.int64), (len(ddx),))
    with np.errstate(all="ignore"):
        ax, ay, bx, by = ddx[:, 0] * W, ddx[:, 1] * H, ddy[:, 0] * W, ddy[:, 1] * H
        rho = np.fmax(np.sqrt(ax * ax + ay * ay), np.sqrt(bx * bx + by * by)).astype(f32)  # fmaxf: a NaN operand loses
        bits = rho.view(np.uint32).astype(np.int64)
        fin = (rho > f32(1.0)) & (rho < f32(np.inf))
    level = np.where(fin, (bits >> 23) - 127, 0)
    frac = np.where(fin, (bits & 0x7FFFFF).astype(f32) / f32(8388608.0), f32(0.0)).astype(f32)
    level = np.where(rho == f32(np.inf), mips, level)
    clamp = level >= mips - 1
    level = np.where(clamp, mips - 1, level)
    frac = np.where(clamp, f32(0.0), frac).astype(f32)
    return level, frac, rho


def grad_for_rho(extent, rho):
    """g with fl(g * extent) == rho exactly (rho a power of two or any f32 when the extent is one): an exact quotient for power-of-two
    extents, found among the neighbours of the rounded quotient otherwise (37 m hits every power of two's rounding window)."""
    rho, e = f32(rho), f32(extent)
    if not np.isfinite(rho) or rho == 0:
        return f32(rho)
    g = f32(rho / e)
    cands = [g]
    lo = hi = g
    for _ in range(64):
        lo, hi = down(lo), up(hi)
        cands += [lo, hi]
    for c in cands:
        if f32(c * e) == rho:
            return c
    raise AssertionError(f"no gradient gives rho {rho} on extent {extent}")


def wrap_index(f, n):
    """tex_wrap / wrap_texel_i: f = floor(coordinate) in f32; Repeat; NaN and |f| >= 1e9 -> texel 0"""
    f = np.asarray(f, dtype=f32)
    with np.errstate(all="ignore"):
        ok = (f == f) & (np.abs(f) < f32(1e9))
        i = np.where(ok, f, 0).astype(np.int64)
    return np.mod(i, np.asarray(n, dtype=np.int64))


def footprint(w, h, u, v):
    """The bilinear footprint of one level: x0, x1, y0, y1 (wrapped texel coordinates), fx, fy, tame (both floors below 2^24 in
    magnitude and not NaN: what tex_level_fast calls tame).  w, h, u, v: arrays."""
    w, h = np.asarray(w, dtype=np.int64), np.asarray(h, dtype=np.int64)
    u, v = np.asarray(u, dtype=f32), np.asarray(v, dtype=f32)
    with np.errstate(all="ignore"):
        tx, ty = u * w.astype(f32) - f32(0.5), v * h.astype(f32) - f32(0.5)
        fx0, fy0 = np.floor(tx), np.floor(ty)
        fx, fy = tx - fx0, ty - fy0
        fx, fy = np.where(fx == fx, fx, f32(0)), np.where(fy == fy, fy, f32(0))
        tame = (np.abs(fx0) < f32(16777216.0)) & (np.abs(fy0) < f32(16777216.0))
        x0, x1 = wrap_index(fx0, w), wrap_index(fx0 + f32(1.0), w)
        y0, y1 = wrap_index(fy0, h), wrap_index(fy0 + f32(1.0), h)
    return dict(x0=x0, x1=x1, y0=y0, y1=y1, fx=fx.astype(f32), fy=fy.astype(f32), tame=tame)


# ------------------------------------------------------------------------------------------------------------------ layout of a set
def make(ids, u, v, ddx, ddy, nearest=0):
    """One query record (ids: an id or a triple)."""
    q = np.zeros(1, dtype=QUERY)
    q["id"][0] = (ids, 0, 0) if np.isscalar(ids) else ids
    q["nearest"], q["u"], q["v"], q["ddx"][0], q["ddy"][0] = nearest, u, v, ddx, ddy
    return q


def arrange(kinds):
    """kinds: list of query arrays, one per kind.  Whole waves of one kind first (each kind padded to a multiple of 64 with its own
    queries, cyclically), then every query once more with the kinds interleaved lane by lane (padded to whole waves likewise).
    Returns (queries, first_mixed): queries[first_mixed:] is the interleaved part."""
    kinds = [k for k in kinds if len(k)]
    whole = []
    for k in kinds:
        n = -(-len(k) // WAVE) * WAVE
        whole.append(np.resize(k, n))
    # round robin over the kinds while they last: lane j of the mixed part takes the next query of the next kind
    rank = np.concatenate([np.arange(len(k)) for k in kinds])
    kind_of = np.concatenate([np.full(len(k), i) for i, k in enumerate(kinds)])
    mixed = np.concatenate(kinds)[np.lexsort((kind_of, rank))]
    mixed = np.resize(mixed, -(-len(mixed) // WAVE) * WAVE)
    first_mixed = sum(len(w) for w in whole)
    return np.concatenate(whole + [mixed]), first_mixed


def _records(ids, u, v, ddx, ddy, nearest=0):
    """Arrays -> query records: u, v broadcast against each other; ids / ddx / ddy one value for all."""
    u, v = np.broadcast_arrays(np.asarray(u, dtype=f32), np.asarray(v, dtype=f32))
    q = np.zeros(u.size, dtype=QUERY)
    q["id"] = (ids, 0, 0) if np.isscalar(ids) else ids
    q["nearest"] = nearest
    q["u"], q["v"] = u.reshape(-1), v.reshape(-1)
    q["ddx"], q["ddy"] = np.asarray(ddx, dtype=f32), np.asarray(ddy, dtype=f32)
    return q


def level_gradient(w, level):
    """ddx = (g, 0) with rho == 2^level exactly (level 0: no gradient at all)"""
    return (f32(0.0) if level == 0 else grad_for_rho(w, f32(2.0) ** level), f32(0.0))


# ------------------------------------------------------------------------------------------------------------------ the query sets
def _lattice_coords(n):
    """(k + 0.5) / n and k / n for k in -2 .. n + 2 (a stride above 16: both ends whole, the middle thinned), and the f32 on either
    side of each."""
    ks = list(range(-2, n + 3))
    if n > 16:
        ks = sorted(set(list(range(-2, 3)) + list(range(n - 2, n + 3)) + list(range(3, n - 2, max(1, n // 4)))))
    out = []
    for k in ks:
        for c in (f32(f32(k + 0.5) / f32(n)), f32(f32(k) / f32(n))):
            out += [down(c), c, up(c)]
    return np.array(out, dtype=f32)


def texel_lattice(table):
    """Every texture, every level, as the only level of the sample: the texel lattice of that level and its f32 neighbours.  The
    three slots name the same texture.  Levels no wider or higher than 16 texels are also asked through the nearest sampler."""
    kinds = []
    for idx, name in enumerate(table.names):
        _, w, h, mips, _ = (int(x) for x in table.descs[idx][:5])
        tid = idx + 1
        for level in range(mips):
            lw, lh = max(1, w >> level), max(1, h >> level)
            U, V = _lattice_coords(lw), _lattice_coords(lh)
            n = max(len(U), len(V))
            u = np.concatenate([np.resize(U, n), np.resize(U, n)])
            v = np.concatenate([np.resize(V, n), np.resize(np.roll(V, 7), n)])
            g = level_gradient(w, level)
            kind = _records((tid, tid, tid), u, v, g, (0.0, 0.0))
            if lw <= 16 and lh <= 16:
                kind = np.concatenate([kind, _records((tid, tid, tid), u[:n], v[:n], g, (0.0, 0.0), nearest=1)])
            kinds.append(kind)
    return arrange(kinds)


def wild_values():
    """(coordinates whose floor leaves the short path's range on every texture wider than one texel, coordinates that stay tame)"""
    wild = np.array([2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 25, down(1e9), 1e9, 3e9, 1e30, np.inf, -np.inf, np.nan, -3e9], dtype=f32)
    tame = np.array([1000.25, -1000.25, -0.0, 1.4e-45, 0.75], dtype=f32)
    return wild, tame


def wild_coordinates(table):
    """u and / or v far outside the texture: beyond 2^24 (floor + 1 and the integer increment part ways), at 1e9 (the wrap gives
    up: texel 0), infinite, NaN; and -0, the smallest subnormal and +-1000.25, which stay on the short path; per texture the
    coordinates whose floors are 2^24 - 1 (the last tame one) and +-2^24.  At level 0 and between two levels in the middle of the
    chain; both samplers.  Kinds: (texture, gradient, sampler, wild or tame)."""
    wild, tame = wild_values()
    kinds = []
    for idx, name in enumerate(table.names):
        _, w, h, mips, _ = (int(x) for x in table.descs[idx][:5])
        tid = idx + 1
        groups = [np.concatenate([wild, [f32(f32(2.0 ** 24 + 0.5) / f32(w)), f32(f32(-(2.0 ** 24) + 0.5) / f32(w))]]).astype(f32),
                  np.concatenate([tame, [f32(f32(2.0 ** 24 - 0.5) / f32(w))]]).astype(f32)]
        mid = max(0, (mips - 1) // 2)
        grads = [(f32(0.0), f32(0.0)), (grad_for_rho(w, f32(1.5) * f32(2.0) ** mid) if (w & (w - 1)) == 0 else f32(1.5 * 2.0 ** mid / w), f32(0.0))]
        for vals in groups:
            u = np.concatenate([vals, np.full(len(vals), 0.3, dtype=f32), vals, vals])
            v = np.concatenate([np.full(len(vals), 0.3, dtype=f32), vals, vals, np.roll(vals, 5)])
            for g in grads:
                for nearest in (0, 1):
                    kinds.append(_records((tid, 0, 0), u, v, g, (0.0, 0.0), nearest=nearest))
    # ids past the table (one past, further, the largest): the general forms answer zeros without reading anything
    n = len(table.names)
    wild_all = np.concatenate([wild, tame])
    for nearest in (0, 1):
        kinds.append(np.concatenate([_records((tid, 0, 0), wild_all, np.roll(wild_all, 3), (f32(0.01), f32(0.0)), (0.0, f32(0.02)), nearest=nearest)
                                     for tid in (n + 1, n + 7, 0xFFFFFFFF)]))
    return arrange(kinds)


def lod_rhos(mips):
    """The values of rho the level of detail has edges at, for a chain of `mips` levels."""
    out = [f32(0.0), f32(1.0), up(1.0)]
    for k in range(0, mips + 2):
        p = f32(2.0) ** k
        out += [p, down(f32(1.5) * p), f32(1.5) * p, up(f32(1.5) * p)]
    out += [down(2.0), f32(1e18), f32(1e20), f32(np.nan)]  # 1e20^2 overflows: rho = +inf
    return out


def lod_edges(table):
    """Per texture every edge of the level of detail -- through ddx alone (exact on power-of-two extents), through ddy alone and
    through a skewed pair of gradients -- under both samplers, at two points."""
    kinds = []
    for idx, name in enumerate(table.names):
        _, w, h, mips, _ = (int(x) for x in table.descs[idx][:5])
        tid = idx + 1
        pts_u, pts_v = np.array([0.3, 0.97], dtype=f32), np.array([0.7, 0.02], dtype=f32)
        for nearest in (0, 1):
            kind = []
            for rho in lod_rhos(mips):
                with np.errstate(all="ignore"):
                    gx, gy = f32(rho / f32(w)), f32(rho / f32(h))
                    pairs = [((gx, 0.0), (0.0, 0.0)), ((0.0, 0.0), (0.0, gy)),
                             ((f32(gx * f32(0.6)), f32(gy * f32(0.8))), (f32(gx * f32(-0.25)), f32(gy * f32(0.5))))]
                for ddx, ddy in pairs:
                    kind.append(_records((tid, 0, 0), pts_u, pts_v, ddx, ddy, nearest=nearest))
            kinds.append(np.concatenate(kind))
    return arrange(kinds)


def share_relations(table):
    """(name, id triple): every relation between the maps of one material that TexShare and the batched form distinguish."""
    t = table.id
    return [
        ("same x3", (t("l32"), t("a0_255"), t("a254_255"))),
        ("same x3 square 64", (t("s64"), t("l64"), t("s64"))),
        ("one texture x3", (t("l64"), t("l64"), t("l64"))),
        ("half in slot 1", (t("s64"), t("l32"), t("l64"))),
        ("half in slot 2", (t("s64"), t("l64"), t("l32"))),
        ("half first", (t("l32"), t("s64"), t("l64"))),
        ("two halves behind", (t("l64"), t("l32"), t("a128"))),
        ("two halves around", (t("l32"), t("s64"), t("a0_1"))),
        ("two halves in front", (t("l32"), t("a255"), t("s64"))),
        ("half of half", (t("l32"), t("s16"), t("last16"))),
        ("unbound slot 0", (0, t("s64"), t("l32"))),
        ("unbound slot 1", (t("s64"), 0, t("l32"))),
        ("unbound slot 2", (t("l32"), t("s64"), 0)),
        ("only slot 2", (0, 0, t("l32"))),
        ("quarter", (t("s64"), t("s16"), t("l64"))),
        ("quarter then half", (t("s64"), t("s16"), t("l32"))),
        ("rectangle against square", (t("r128x32"), t("s64"), t("r32x128"))),
        ("square against rectangle", (t("l32"), t("r32x128"), t("l32"))),
        ("short chain first", (t("c64m3"), t("l64"), t("l32"))),
        ("short chain behind", (t("l64"), t("c64m3"), t("l32"))),
        ("2x2 over 1x1", (t("t2"), t("t1"), t("t2"))),
        ("1x1 before 2x2", (t("t1"), t("t2"), t("t1"))),
        ("1-wide maps", (t("h1x64"), t("h1x64"), t("w64x1"))),
        ("nothing bound", (0, 0, 0)),
    ]


def share_gradients(w, mips):
    """Groups of gradients, relative to a map of width w with `mips` levels: the level of detail at 0 (rho 0, a fraction below 1,
    exactly 1); on a level from 1 up (1, the middle of the chain, the last but one, the last, past it); between two levels (below 1.0
    of detail, and further up); then one component of order 1 beside one of 2^-70 and less, whose squares are subnormal or zero for
    this map and for one of half the size."""
    mid = max(1, (mips - 1) // 2)

    def both(rhos):
        out = []
        for rho in rhos:
            g = f32(f32(rho) / f32(w))
            out += [((g, 0.0), (0.0, 0.0)), ((0.0, 0.0), (f32(g * f32(0.5)), g))]
        return out
    groups = {
        "level 0": both((0.0, 0.75, 1.0)),
        "on a level": both((2.0, 2.0 ** mid, 2.0 ** max(0, mips - 2), 2.0 ** (mips - 1), 2.0 ** mips)),
        "between 0 and 1": both((1.5, 1.0000001, 1.9999999)),
        "between two": both((3.0, 1.25 * 2.0 ** mid, 1.75 * 2.0 ** max(0, mips - 2))),
        "subnormal squares": [],
    }
    for big in (f32(3.3) / f32(w), f32(1.0) / f32(w), f32(2.9) / f32(w)):
        for tiny in (2.0 ** -70, 1.7 * 2.0 ** -72, 1.3 * 2.0 ** -74, 2.0 ** -75, 1.9 * 2.0 ** -78, 2.0 ** -80):
            groups["subnormal squares"] += [((big, f32(tiny)), (0.0, 0.0)), ((f32(tiny), big), (f32(tiny), f32(tiny))),
                                            ((0.0, f32(tiny)), (big, f32(-tiny)))]
    return groups


SHARE_POINTS = ((0.3, 0.7), (0.999, 0.4), (0.0, 0.0), (0.508, 0.992), (-0.26, 1.24))


def _fits_batched(table, ids):
    """whether tex_sample3_batched takes the triple: every bound map has the widest one's extents and mips, or half with one less"""
    rows = [tuple(int(x) for x in table.descs[i - 1][1:4]) for i in ids if i]
    if not rows:
        return True
    W, H, M = max(rows, key=lambda r: r[0])
    return all(r == (W, H, M) or (r[0] * 2 == W and r[1] * 2 == H and r[2] + 1 == M) for r in rows)


def share_triples(table):
    """Three maps per query; one kind per (relation, group of gradients).  The relations the batched form takes are laid out
    first (whole waves, then interleaved among themselves: waves the batched form accepts with lanes of different relations), then
    the ones it declines likewise, then everything interleaved: waves that decline because SOME lane's maps do not fit."""
    u = np.array([p[0] for p in SHARE_POINTS], dtype=f32)
    v = np.array([p[1] for p in SHARE_POINTS], dtype=f32)
    fit, misfit = [], []
    for name, ids in share_relations(table):
        widest = max((i for i in ids if i), key=lambda i: int(table.descs[i - 1][1]), default=1)
        _, w, h, mips, _ = (int(x) for x in table.descs[widest - 1][:5])
        for group, grads in share_gradients(w, mips).items():
            kind = np.concatenate([_records(ids, u, v, ddx, ddy) for ddx, ddy in grads])
            (fit if _fits_batched(table, ids) else misfit).append(kind)
    a, first_mixed = arrange(fit)
    b, _ = arrange(misfit)
    c, at = arrange(fit + misfit)
    return np.concatenate([a, b, c[at:]]), first_mixed


def alpha_footprints(table):
    """The alpha textures (32 x 32, alpha in 8 x 8 blocks at level 0, blocks halved per level) at block interiors, borders and
    corners: one level (0, 1 and the last) and between two."""
    j = np.arange(0, 33)
    # (texel borders, texel centres, and weights that are no dyadic fractions: a * (1 - f) + a * f misses a there)
    c = np.concatenate([(j / 32.0).astype(f32), ((j + 0.5) / 32.0).astype(f32), ((j + (j * 0.6180339) % 1.0) / 32.0).astype(f32),
                        ((j + (j * 0.4142135 + 0.3) % 1.0) / 32.0).astype(f32),
                        # (weights next to 0 and 1, where they keep bits below 2^-24: found by search, these are the coordinates at
                        # which 128 / 255 * (1 - f) + 128 / 255 * f is NOT 128 / 255 -- about one weight in 10^5)
                        np.array([0x3c7e8380, 0x3c7ee31f, 0x3c80ec12, 0x3c809f5f, 0x3c7ec73d, 0x3c80a35b, 0x3c7e738f, 0x3c80f00e, 0x3c80b14d,
                                  0x3c80ee10, 0x3c809c62, 0x3c7e6f95], dtype=np.uint32).view(f32)])
    u = np.concatenate([c, c, c])
    v = np.concatenate([c, np.full(len(c), 0.4, dtype=f32), np.roll(c, 8)])
    kinds = []
    for name in ALPHA_NAMES:
        tid = table.id(name)
        for rho in (0.0, 2.0, 1.5, 1.3, 2.7, 32.0):
            kinds.append(_records((tid, 0, 0), u, v, (f32(rho / 32.0), 0.0), (0.0, 0.0)))
    return arrange(kinds)


def row_wrap(table):
    """Footprint rows that wrap at the right edge (from inside: x0 = w - 1; from outside: floor = -1), beside rows that do not, on
    every level of every texture -- the 1-texel-wide levels, where a row never is a pair, and the pool's last word (the last
    texture's 1 x 1 level) included -- as the only level and as the first of two.  One kind per (wrapping or not) so that `arrange`
    gives waves of each alone and waves that mix them."""
    wrapping, plain = [], []
    for idx, name in enumerate(table.names):
        _, w, h, mips, _ = (int(x) for x in table.descs[idx][:5])
        tid = idx + 1
        for level in range(mips):
            lw, lh = max(1, w >> level), max(1, h >> level)
            grads = [level_gradient(w, level)]
            if level + 1 < mips:
                grads.append((f32(level_gradient(w, level)[0] * f32(1.5)) if level else f32(f32(1.5) / f32(w)), f32(0.0)))
            vs = np.array([0.5 / lh, (lh - 0.25) / lh], dtype=f32)
            for g in grads:
                wrapping.append(_records((tid, tid, tid), np.array([(lw - 0.25) / lw, 0.1 / lw, 0.1 / lw - 3.0], dtype=f32)[:, None], vs[None, :], g, (0.0, 0.0)))
                plain.append(_records((tid, tid, tid), np.array([0.5 + 0.25 / lw, 1.0 / lw], dtype=f32)[:, None], vs[None, :], g, (0.0, 0.0)))
    return arrange([np.concatenate(wrapping), np.concatenate(plain)])


SETS = {"texel_lattice": texel_lattice, "wild_coordinates": wild_coordinates, "lod_edges": lod_edges, "share_triples": share_triples,
        "alpha_footprints": alpha_footprints, "row_wrap": row_wrap}


# ------------------------------------------------------------------------------------------------------------------ the classifier
# every path name, and the forms (texture.h instantiations) it can be taken by
VOCABULARY = {
    "unbound": FORMS,                                  # id 0 (every form) or past the table (general forms; wild_coordinates): zeros
    "general": ("grad", "grad_rgb", "alpha"),          # tex_footprint / tex_apply
    "general_remainder_wrap": ("grad", "grad_rgb", "alpha"),   # an extent that is no power of two
    "general_float_texels": ("grad", "grad_rgb", "alpha"),     # R3N_POOL_FLOAT texels
    "general_nearest": ("grad", "grad_rgb", "alpha"),          # the nearest sampler
    "nearest_rounds_up": ("grad", "grad_rgb", "alpha"),        # frac >= 0.5: the next level
    "short": FORMS,                                    # mask wrap, 32-bit byte offsets
    "short_fallback": ("grad", "grad_rgb", "alpha"),   # tex_level_fast<false> reports a wild floor: the general code takes over
    "total_block": SHORT_ONLY_FORMS,                   # tex_level_fast<true> rewrites the footprint by the general formulas
    "one_level": FORMS,
    "two_levels": FORMS,
    "closed_form_tail": SHORT_ONLY_FORMS,              # tex_level_start_pow2: L > min(log2 W, log2 H) + 1, one extent stuck at 1
    "share_recomputed": ("share",),
    "share_same": ("share",),
    "share_half": ("share",),
    "batched_accepts": ("batched",),
    "batched_declines": ("batched",),
    "batched_lane_misfit": ("batched",),               # this lane binds a map that fits neither rule (its wave declines)
    "batched_first_is_f1": ("batched",),               # a half-size map while the reference map is at level 0
    "batched_half_shifted": ("batched",),              # a half-size map at the reference's level - 1
    "batched_unbound_slot": ("batched",),              # a slot without a map beside bound ones: its loads go to the pool's start
    "row_pair": ("batched",),                          # every 8-byte row load of the lane is its two texels
    "row_wrap": ("batched",),                          # some row of the lane wraps (or is 1 texel wide): patched
    "alpha_one": ("alpha", "alpha_short"),             # every alpha byte of the footprint(s) 255: 1.0f without the filter
    "alpha_zero": ("alpha", "alpha_short"),            # every byte 0: +0
    "alpha_arithmetic": ("alpha", "alpha_short"),
}


def _desc_cols(table, ids):
    """per query: bound, width, height, mips, fmt, offset of texture id (arrays); an unbound / out-of-table id reads as zeros"""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(table.descs)
    bound = (ids >= 1) & (ids <= n)
    d = table.descs[np.where(bound, ids - 1, 0)].astype(np.int64)
    return bound, d[:, 1], d[:, 2], d[:, 3], d[:, 4], d[:, 0]


def _pow2(x):
    return (x > 0) & ((x & (x - 1)) == 0)


def _ilog2(x):
    return np.floor(np.log2(np.maximum(x, 1))).astype(np.int64)


def _mip(d, k):
    return np.maximum(d >> k, 1)


def _level_start_rel(w, h, level):
    """sum over k < level of mip(w, k) * mip(h, k): what the table, the walk and the closed form must all give"""
    out = np.zeros(len(w), dtype=np.int64)
    for k in range(int(level.max()) if len(level) else 0):
        out += np.where(k < level, _mip(w, k) * _mip(h, k), 0)
    return out


def _alpha_bytes(table, off, w, h, level, fp):
    """the alpha bytes of a footprint's four texels (RGBA8 textures only)"""
    base = off + _level_start_rel(w, h, level)
    lw = _mip(w, level)
    out = []
    for y, x in (("y0", "x0"), ("y0", "x1"), ("y1", "x0"), ("y1", "x1")):
        out.append((table.pool[base + fp[y] * lw + fp[x]] >> 24).astype(np.int64))
    return out


def paths(queries, form, table):
    """{path name: bool array over the queries}: which of VOCABULARY's paths each query takes under `form` (a name of FORMS), with
    `table` as the bound textures (its .pool is needed by the alpha forms only).  "valid": whether the query is inside the form's
    preconditions (include/r3n.h r3n_sample_probe) -- callers drop the others before a short-path-only or batched call.
    For the batched form the wave-wide facts (declines, the flag) assume that queries[64 i : 64 i + 64] is wave i."""
    P = _paths(np.atleast_1d(queries), form, table)
    for name in VOCABULARY:  # a query outside the form's preconditions takes no path: it is never sent
        P[name] = P[name] & P["valid"] if form in VOCABULARY[name] else np.zeros_like(P["valid"])
    return P


def _paths(q, form, table):
    n = len(q)
    P = {name: np.zeros(n, dtype=bool) for name in VOCABULARY}
    nslots = 3 if form in THREE_MAP_FORMS else 1
    short_only = form in SHORT_ONLY_FORMS
    nearest = q["nearest"] != 0
    cols = [_desc_cols(table, q["id"][:, k]) for k in range(3)]
    is_short = [c[0] & _pow2(c[1]) & _pow2(c[2]) & (c[4] < POOL_FLOAT) for c in cols]
    valid = np.ones(n, dtype=bool)
    if short_only:
        valid &= ~nearest
        for k in range(nslots):
            valid &= (q["id"][:, k] == 0) | is_short[k]
    P["valid"] = valid

    def one_map(w, h, level, frac):
        """footprint facts of a map sampled at (level, frac) on the short path"""
        f0 = footprint(_mip(w, level), _mip(h, level), q["u"], q["v"])
        two = frac > 0
        f1 = footprint(_mip(w, level + 1), _mip(h, level + 1), q["u"], q["v"])
        tame = f0["tame"] & (f1["tame"] | ~two)
        return f0, f1, two, tame

    if form in ("grad", "grad_rgb", "short", "short_rgb", "alpha", "alpha_short"):
        bound, w, h, mips, fmt, off = cols[0]
        level, frac, rho = lod(np.maximum(w, 0), np.maximum(h, 0), np.maximum(mips, 1), q["ddx"], q["ddy"])
        P["unbound"] = ~bound
        try_short = bound & (is_short[0] if short_only else (is_short[0] & ~nearest))
        f0, f1, two, tame = one_map(w, h, level, frac)
        P["short"] = try_short & (tame | short_only)
        P["short_fallback"] = try_short & ~tame & (not short_only)
        P["total_block"] = try_short & ~tame & short_only
        P["general"] = bound & ~P["short"]
        P["general_remainder_wrap"] = P["general"] & ~(_pow2(w) & _pow2(h))
        P["general_float_texels"] = P["general"] & (fmt == POOL_FLOAT)
        P["general_nearest"] = P["general"] & nearest
        P["nearest_rounds_up"] = P["general"] & nearest & (frac >= f32(0.5))
        P["two_levels"] = bound & two & ~(P["general"] & nearest)
        P["one_level"] = bound & ~P["two_levels"]
        if short_only:
            P["closed_form_tail"] = P["short"] & (level > np.minimum(_ilog2(w), _ilog2(h)) + 1)
        if form in ("alpha", "alpha_short"):
            sh = P["short"]
            if sh.any():
                assert table.pool is not None, "the alpha forms' shortcut is classified from the texels: build the table first"
                idx = np.nonzero(sh)[0]
                sub = lambda a: a[idx]  # noqa: E731
                g0 = {k: v[idx] for k, v in f0.items()}
                g1 = {k: v[idx] for k, v in f1.items()}
                a = _alpha_bytes(table, sub(off), sub(w), sub(h), sub(level), g0)
                b = _alpha_bytes(table, sub(off), sub(w), sub(h), np.where(sub(two), sub(level) + 1, sub(level)), {k: np.where(sub(two), g1[k], g0[k]) for k in g0})
                all_and, all_or = a[0], a[0]
                for x in a[1:] + b:
                    all_and, all_or = all_and & x, all_or | x
                P["alpha_one"][idx] = all_and == 255
                P["alpha_zero"][idx] = (all_or == 0) & (all_and != 255)
            P["alpha_arithmetic"] = sh & ~P["alpha_one"] & ~P["alpha_zero"]
        return P

    if form == "share":
        # the cache as tex_sample_grad<.., SHORT_ONLY, SHARE> keeps it: extents and mips of the map it was computed for, its level
        sw = np.zeros(n, dtype=np.int64); sh_ = np.zeros(n, dtype=np.int64); sm = np.zeros(n, dtype=np.int64)
        slevel = np.zeros(n, dtype=np.int64); sfrac = np.zeros(n, dtype=f32)
        any_bound = np.zeros(n, dtype=bool)
        for k in range(3):
            bound, w, h, mips, fmt, off = cols[k]
            bound = bound & valid
            any_bound |= bound
            same = bound & (sw == w) & (sh_ == h) & (sm == mips)
            half = bound & (sw == w << 1) & (sh_ == h << 1) & (sm == mips + 1) & (slevel >= 1) & (w != 0)
            rec = bound & ~(same | half)
            level, frac, rho = lod(np.maximum(w, 0), np.maximum(h, 0), np.maximum(mips, 1), q["ddx"], q["ddy"])
            sw, sh_, sm = np.where(rec, w, sw), np.where(rec, h, sh_), np.where(rec, mips, sm)
            slevel, sfrac = np.where(rec, level, slevel), np.where(rec, frac, sfrac).astype(f32)
            P["share_recomputed"] |= rec
            P["share_same"] |= same
            P["share_half"] |= half & ~same
            mylevel = slevel - np.where(half & ~same, 1, 0)
            f0, f1, two, tame = one_map(sw, sh_, slevel, sfrac)
            P["total_block"] |= bound & ~tame
            P["two_levels"] |= bound & (sfrac > 0)
            P["closed_form_tail"] |= bound & (mylevel > np.minimum(_ilog2(w), _ilog2(h)) + 1)
        P["short"] = any_bound
        P["unbound"] = (q["id"] == 0).any(axis=1)
        P["one_level"] = any_bound & ~P["two_levels"]
        return P

    assert form == "batched"
    present = [(q["id"][:, k] != 0) for k in range(3)]
    W = np.zeros(n, dtype=np.int64); H = np.zeros(n, dtype=np.int64); MI = np.zeros(n, dtype=np.int64)
    for k in range(3):
        _, w, h, mips, _, _ = cols[k]
        take = present[k] & cols[k][0] & (w > W)
        W, H, MI = np.where(take, w, W), np.where(take, h, H), np.where(take, mips, MI)
    ok = np.ones(n, dtype=bool)
    half = []
    for k in range(3):
        _, w, h, mips, _, _ = cols[k]
        same = (w == W) & (h == H) & (mips == MI)
        hk = present[k] & ~same & ((w << 1) == W) & ((h << 1) == H) & (mips + 1 == MI)
        half.append(hk)
        ok &= ~present[k] | same | hk
    # the vote: a wave declines when any of its lanes (valid ones: the others are dropped before the call) binds a map that fits neither
    pad = -n % WAVE
    wave_ok = np.concatenate([ok | ~valid, np.ones(pad, dtype=bool)]).reshape(-1, WAVE).all(axis=1)
    accepts = np.repeat(wave_ok, WAVE)[:n]
    P["batched_declines"] = ~accepts
    P["batched_lane_misfit"] = ~ok
    P["batched_accepts"] = accepts
    any_present = present[0] | present[1] | present[2]
    level, frac, rho = lod(W, H, np.maximum(MI, 1), q["ddx"], q["ddy"])
    level = np.where(MI == 0, 0, level)
    f0 = footprint(_mip(W, level), _mip(H, level), q["u"], q["v"])
    f1 = footprint(_mip(W, level + 1), _mip(H, level + 1), q["u"], q["v"])
    any_half = half[0] | half[1] | half[2]
    need1 = (frac > 0) | (any_half & (level == 0))
    pair0 = f0["x1"] == f0["x0"] + 1
    pair1 = np.where(need1, f1["x1"] == f1["x0"] + 1, pair0)
    tame = f0["tame"] & (f1["tame"] | ~need1)
    wraps = np.zeros(n, dtype=bool)
    for k in range(3):
        _, w, h, mips, _, _ = cols[k]
        first_is_f1 = half[k] & (level == 0)
        two = (frac > 0) & ~first_is_f1
        P["batched_first_is_f1"] |= accepts & first_is_f1
        P["batched_half_shifted"] |= accepts & half[k] & (level >= 1)
        P["batched_unbound_slot"] |= accepts & ~present[k] & any_present
        la = np.where(half[k], np.where(level == 0, 0, level - 1), level)
        P["closed_form_tail"] |= accepts & present[k] & (la > np.minimum(_ilog2(w), _ilog2(h)) + 1)
        # (every slot's loads are issued, bound or not)
        wraps |= ~np.where(first_is_f1, pair1, pair0)
        wraps |= (frac > 0) & ~np.where(two | first_is_f1, pair1, pair0)
        P["two_levels"] |= accepts & present[k] & two
    P["row_wrap"] = accepts & wraps
    P["row_pair"] = accepts & ~wraps
    P["short"] = accepts & any_present
    P["total_block"] = accepts & ~tame
    P["unbound"] = ~any_present
    P["one_level"] = accepts & any_present & ~P["two_levels"]
    return P


def first_levels(queries, table):
    """(texture index, level) pairs that are the first level of slot 0's sample of some query, as a set"""
    q = np.atleast_1d(queries)
    bound, w, h, mips, fmt, off = _desc_cols(table, q["id"][:, 0])
    level, frac, rho = lod(np.maximum(w, 0), np.maximum(h, 0), np.maximum(mips, 1), q["ddx"], q["ddy"])
    level = level + ((q["nearest"] != 0) & (frac >= f32(0.5)))
    return set(zip((q["id"][bound, 0] - 1).tolist(), level[bound].tolist()))
