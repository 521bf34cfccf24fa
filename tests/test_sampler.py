"""The texture sampler's test conditions, on the CPU (oracle only): that the query sets of tests/sampler_queries.py reach every path
the classifier names -- as whole wavefronts and inside mixed ones --, that they start a sample on every level of every texture of
the table, that every reference value is finite (so that the GPU comparison can be bit for bit, the sign of zero included), and
the answers that are known without any sampler: texel centres, the 1 x 1 texture, uniform alpha, and the half-size rule of
texture.h's TexShare -- on the numpy restatement of the level-of-detail arithmetic (sq.lod), and on the oracle's own results, which
also tie that restatement to r3o.c.

Floors asserted below are what the sets give on the oracle (order "a"), rounded down; a set that is thinned below them no longer
pins what test_sampler_gpu.py's docstring says it pins."""
import numpy as np
import pytest

import sampler_queries as sq
from oracle import host as oh
from oracle.world import OracleRenderer

f32 = np.float32
# what a vote over the wavefront decides has no mixed wave by construction: the per-lane cause (batched_lane_misfit) has
WAVE_UNIFORM = ("batched_accepts", "batched_declines")


class Reference:
    """The table on the oracle, every query set and its oracle results: computed once per table order, shared, never changed."""

    def __init__(self, order):
        self.table = sq.Table(order)
        self.oracle = OracleRenderer(oh.LEFT, f32(1.0))
        self.table.build(self.oracle)
        self.sets = {}
        for name, fn in sq.SETS.items():
            q, first_mixed = fn(self.table)
            self.sets[name] = (q, first_mixed, self.sample(q))

    def sample(self, q, oracle=None):
        o = oracle or self.oracle
        q = np.ascontiguousarray(q)
        out = np.zeros(len(q), dtype=sq.RESULT)
        d, n, p = o._tex_args()
        o.lib.r3o_sample_queries(d, n, p, o.lib.ptr(q), len(q), o.lib.ptr(out))
        return out


_REFS = {}


def reference(order="a"):
    if order not in _REFS:
        _REFS[order] = Reference(order)
    return _REFS[order]


def wave_counts(mask, valid):
    """(waves whose every valid lane has the path, waves where some valid lanes have it and some do not)"""
    pad = -len(mask) % sq.WAVE
    m = np.concatenate([mask & valid, np.zeros(pad, dtype=bool)]).reshape(-1, sq.WAVE)
    v = np.concatenate([valid, np.zeros(pad, dtype=bool)]).reshape(-1, sq.WAVE)
    return int(((m | ~v).all(axis=1) & v.any(axis=1)).sum()), int((m.any(axis=1) & (v & ~m).any(axis=1)).sum())


def decode(table, idx, words):
    """pool words of texture idx -> (n, 4) f32 as the contract decodes them"""
    fmt = int(table.descs[idx][4])
    if fmt == sq.POOL_FLOAT:
        return words.reshape(-1, 4).view(f32)
    c = np.stack([(words >> s) & 0xFF for s in (0, 8, 16, 24)], axis=1)
    out = c.astype(f32) / f32(255.0)
    if fmt == 1:
        lut = np.zeros(256, dtype=f32)
        lib = reference().oracle.lib
        lib.r3o_srgb8_table(lib.ptr(lut))
        out[:, :3] = lut[c[:, :3]]
    return out


@pytest.mark.parametrize("order", sq.ORDERS)
def test_every_reference_value_is_finite(order):
    ref = reference(order)
    for name, (q, _, out) in ref.sets.items():
        assert np.isfinite(out["rgba"]).all(), name
        assert len(q) % sq.WAVE == 0 and 1000 < len(q) < 60000, (name, len(q))


@pytest.mark.parametrize("form", sq.FORMS)
def test_every_path_is_reached_by_whole_and_mixed_waves(form):
    ref = reference("a")
    whole = {name: 0 for name, forms in sq.VOCABULARY.items() if form in forms}
    mixed = dict(whole)
    lanes = dict(whole)
    where = {name: [] for name in whole}
    for set_name, (q, _, _) in ref.sets.items():
        q = q[sq.paths(q, form, ref.table)["valid"]]  # what the form's preconditions exclude is never sent: the waves are of the rest
        P = sq.paths(q, form, ref.table)
        assert P["valid"].all()
        for name in sq.VOCABULARY:
            if name not in whole:
                assert not P[name].any(), f"{name} is not a path of {form}"
                continue
            w, m = wave_counts(P[name], P["valid"])
            whole[name] += w
            mixed[name] += m
            lanes[name] += int(P[name].sum())
            if w or m:
                where[name].append(set_name)
    print(form, {k: (lanes[k], whole[k], mixed[k], where[k]) for k in whole})
    for name in whole:
        assert whole[name] >= 1, f"{form}: no whole wave takes {name}"
        assert name in WAVE_UNIFORM or mixed[name] >= 1, f"{form}: no mixed wave has {name}"
    # floors (what the sets give, rounded down)
    floors = {"short_fallback": 4000, "total_block": 4000, "closed_form_tail": 4000, "nearest_rounds_up": 6000, "share_half": 5000,
              "share_same": 15000, "batched_first_is_f1": 4000, "batched_half_shifted": 7000, "batched_lane_misfit": 9000, "row_wrap": 30000,
              "alpha_one": 6000, "alpha_zero": 9000, "general_remainder_wrap": 6000, "general_float_texels": 6000}
    for name, floor in floors.items():
        if name in lanes:
            assert lanes[name] >= floor, (form, name, lanes[name])


@pytest.mark.parametrize("order", sq.ORDERS)
def test_every_level_of_every_texture_starts_a_sample(order):
    ref = reference(order)
    seen = set()
    for name, (q, _, _) in ref.sets.items():
        seen |= sq.first_levels(q, ref.table)
    want = {(i, k) for i in range(len(ref.table.names)) for k in range(int(ref.table.descs[i][3]))}
    assert want <= seen, sorted(want - seen)
    # and the lattice alone does, with that level as its ONLY level, under the linear sampler
    q = ref.sets["texel_lattice"][0]
    q = q[q["nearest"] == 0]
    assert want <= sq.first_levels(q, ref.table)
    P = sq.paths(q, "grad", ref.table)
    assert P["one_level"].all()


@pytest.mark.parametrize("order", sq.ORDERS)
def test_texel_centres_return_the_texel(order):
    """A query at a texel centre of level k, with gradients that select level k alone, is that texel's decoded value: weights 1, 0,
    0, 0 leave c00 * 1 + c10 * 0 = c00 in every blend."""
    ref = reference(order)
    t = ref.table
    q, _, out = ref.sets["texel_lattice"]
    keep = q["nearest"] == 0
    q, out = q[keep], out[keep]
    idx = q["id"][:, 0].astype(np.int64) - 1
    d = t.descs[idx].astype(np.int64)
    level, frac, _ = sq.lod(d[:, 1], d[:, 2], d[:, 3], q["ddx"], q["ddy"])
    assert (frac == 0).all()
    fp = sq.footprint(sq._mip(d[:, 1], level), sq._mip(d[:, 2], level), q["u"], q["v"])
    centre = (fp["fx"] == 0) & (fp["fy"] == 0)
    assert centre.sum() >= 3000
    checked = 0
    for i in range(len(t.names)):
        sel = centre & (idx == i)
        assert sel.any(), t.names[i]
        words = 4 if int(t.descs[i][4]) == sq.POOL_FLOAT else 1
        start = np.array([t.level_start(i, int(k)) for k in level[sel]], dtype=np.int64)
        at = start + words * (fp["y0"][sel] * sq._mip(d[sel, 1], level[sel]) + fp["x0"][sel])
        pool_words = np.stack([t.pool[at + c] for c in range(words)], axis=1).reshape(-1)
        want = decode(t, i, np.ascontiguousarray(pool_words))
        got = out["rgba"][sel][:, 0, :]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), t.names[i]
        assert set(level[sel].tolist()) == set(range(int(t.descs[i][3]))), t.names[i]  # on every level
        checked += int(sel.sum())
    assert checked == centre.sum()


def test_the_1x1_texture_returns_its_texel_wherever_it_is_asked():
    ref = reference("a")
    t = ref.table
    q, _, out = ref.sets["wild_coordinates"]
    i = t.names.index("t1")
    sel = q["id"][:, 0] == i + 1
    assert sel.sum() >= 300
    want = decode(t, i, t.pool[int(t.descs[i][0]): int(t.descs[i][0]) + 1])[0]
    got = out["rgba"][sel][:, 0, :]
    assert (got.view(np.uint32) == want.view(np.uint32)[None, :]).all()


def test_uniform_alpha_is_exact():
    """255 everywhere: every blend is fl(fl(1 - f) + f) = 1.0f; 0 everywhere: +0.  (Nothing of the kind holds for uniform 128: there
    the oracle's arithmetic is simply the reference.)"""
    ref = reference("a")
    t = ref.table
    n = 0
    for name, (q, _, out) in ref.sets.items():
        for tex, bits in (("a255", f32(1.0).view(np.uint32)), ("a0", np.uint32(0))):
            sel = q["id"][:, 0] == t.id(tex)
            n += int(sel.sum())
            assert (out["rgba"][sel][:, 0, 3].view(np.uint32) == bits).all(), (name, tex)
    assert n >= 8000
    q, _, out = ref.sets["alpha_footprints"]
    a128 = out["rgba"][q["id"][:, 0] == t.id("a128")][:, 0, 3]
    assert len(np.unique(a128.view(np.uint32))) > 1, "uniform 128 filtered to one value everywhere: the inexact case is not in the set"


def test_a_half_size_map_is_one_level_down_with_the_same_fraction():
    """texture.h TexShare / tex_sample3_batched: with W' = W / 2, H' = H / 2 and one level less, rho' = rho / 2 bit for bit, so
    level' = level - 1 and frac' = frac wherever level >= 1 (the clamp included), and level' = 0, frac' = 0 where level == 0.  Over
    every gradient pair of share_triples -- the ones whose squares are subnormal or vanish included -- and every pair of table
    textures that stand in that relation."""
    ref = reference("a")
    t = ref.table
    q = ref.sets["share_triples"][0]
    grads = np.unique(np.concatenate([q["ddx"], q["ddy"]], axis=1).view(np.uint32), axis=0).view(f32)
    ddx, ddy = grads[:, :2], grads[:, 2:]
    assert len(grads) >= 250
    pairs = 0
    subnormal_seen = False
    for a in range(len(t.names)):
        for b in range(len(t.names)):
            _, wa, ha, ma, fa = (int(x) for x in t.descs[a][:5])
            _, wb, hb, mb, fb = (int(x) for x in t.descs[b][:5])
            if not (wa == 2 * wb and ha == 2 * hb and ma == mb + 1):
                continue
            pairs += 1
            la, fra, rho_a = sq.lod(wa, ha, ma, ddx, ddy)
            lb, frb, rho_b = sq.lod(wb, hb, mb, ddx, ddy)
            fin = np.isfinite(rho_a)
            assert np.array_equal((rho_a[fin] * f32(0.5)).view(np.uint32), rho_b[fin].view(np.uint32)), (t.names[a], t.names[b])
            up = la >= 1
            assert up.any() and (~up).any()
            assert (lb[up] == la[up] - 1).all() and np.array_equal(frb[up].view(np.uint32), fra[up].view(np.uint32))
            assert (lb[~up] == 0).all() and (frb[~up] == 0).all()
            with np.errstate(all="ignore"):
                sq_small = (ddx[:, 1] * f32(ha)) * (ddx[:, 1] * f32(ha))
            subnormal_seen |= bool(((sq_small > 0) & (sq_small < f32(1.1754944e-38))).any() and (sq_small == 0).any())
    assert pairs >= 10 and subnormal_seen


def test_the_oracle_agrees_with_the_restated_level_of_detail_and_with_the_half_size_rule():
    """The test above runs on sq.lod, the numpy restatement of the level-of-detail arithmetic.  Here r3o.c speaks: textures whose
    level k is one byte value b[k] everywhere, sampled at (0, 0) -- both weights 0.5 on every level, so a level's bilinear value is
    exactly b[k] / 255 -- return fl(fl(lo * (1 - frac)) + fl(hi * frac)), which names level and frac.  (a) The oracle's value is the
    one sq.lod's (level, frac) predict, bit for bit, for every gradient pair of share_triples on every size: the restatement is the
    oracle's arithmetic.  (b) A half-size map whose level k carries the full-size map's byte of level k + 1 returns the SAME WORDS
    as the full-size map wherever that one is at level >= 1, and its own level 0 where it is at level 0: the TexShare claim in the
    oracle's own results."""
    ref = reference("a")
    q0 = ref.sets["share_triples"][0]
    grads = np.unique(np.concatenate([q0["ddx"], q0["ddy"]], axis=1).view(np.uint32), axis=0).view(f32)
    b = np.array([10 + 30 * k for k in range(8)], dtype=np.uint8)
    o = OracleRenderer(oh.LEFT, f32(1.0))
    sizes = [(64, 0), (32, 1), (16, 2), (2, 5), (1, 6)]  # (extent, the level of the 64 x 64 map its level 0 stands for)
    for size, first in sizes:
        mips = size.bit_length()
        levels = [np.full((max(1, size >> k) ** 2, 4), b[first + k], dtype=np.uint8).tobytes() for k in range(mips)]
        o.add_texture_2d_encoded(sq.RGBA8, size, size, levels)
    q = np.zeros(len(grads), dtype=sq.QUERY)
    q["ddx"], q["ddy"] = grads[:, :2], grads[:, 2:]
    results, lods = [], []
    for i, (size, first) in enumerate(sizes):
        q["id"] = (i + 1, 0, 0)
        got = ref.sample(q, o)["rgba"][:, 0, :]
        assert (got == got[:, :1]).all()
        mips = size.bit_length()
        level, frac, _ = sq.lod(size, size, mips, q["ddx"], q["ddy"])
        lo = b[first + level].astype(f32) / f32(255.0)
        hi = b[np.minimum(first + level + 1, len(b) - 1)].astype(f32) / f32(255.0)
        want = np.where(frac > 0, lo * (f32(1.0) - frac) + hi * frac, lo).astype(f32)
        assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)), f"(a) {size} x {size}"
        assert (mips == 1 or (frac > 0).any()) and (level == mips - 1).any()
        results.append(got[:, 0].view(np.uint32))
        lods.append(level)
    for full, half in ((0, 1), (1, 2), (3, 4)):
        up = lods[full] >= 1
        assert up.any() and (~up).any()
        assert np.array_equal(results[half][up], results[full][up]), f"(b) {sizes[half][0]} under {sizes[full][0]}"
        own = (b[sizes[half][1]].astype(f32) / f32(255.0)).view(np.uint32)
        assert (results[half][~up] == own).all()


def test_wild_coordinates_ask_ids_past_the_table():
    ref = reference("a")
    q, _, out = ref.sets["wild_coordinates"]
    past = q["id"][:, 0] > len(ref.table.names)
    assert past.sum() >= 128 and (out["rgba"][past].view(np.uint32) == 0).all()
    assert sq.paths(q[past], "grad", ref.table)["unbound"].all() and not sq.paths(q[past], "short", ref.table)["valid"].any()


def test_the_classifier_takes_single_queries_and_names_only_its_vocabulary():
    ref = reference("a")
    q = ref.sets["lod_edges"][0]
    for form in sq.FORMS:
        one = sq.paths(q[5], form, ref.table)
        assert set(one) == set(sq.VOCABULARY) | {"valid"}
        assert all(v.shape == (1,) for v in one.values())
    # the second table order really ends in the 64 x 1 texture, the first in last16's 1 x 1 level
    assert reference("a").table.names[-1] == "last16" and reference("b").table.names[-1] == "w64x1"
    for order in sq.ORDERS:
        t = sq.Table(order)
        last = t.descs[-1]
        assert int(last[0]) + sum(max(1, int(last[1]) >> k) * max(1, int(last[2]) >> k) for k in range(int(last[3]))) == t.pool_words
