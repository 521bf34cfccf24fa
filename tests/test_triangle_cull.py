"""The conditions tests/test_triangle_cull_gpu.py rests on, on the CPU: tests/triangle_cull_reference.py equals the oracle on every
world and sequence of tests/triangle_cull_worlds.py as bits; every catalogue entry sits on the edge it is named after; every rule
decides, every slot kind, ballot form, the sub-list wrap and the second loop trip are reached; the structure worlds pass between a
quarter and three quarters of their triangles."""
import functools

import numpy as np
import pytest

import triangle_cull_reference as tc
import triangle_cull_worlds as tw

f32, u32, u64 = np.float32, np.uint32, np.uint64
ALL_RUNS = list(tw.RUNS) + ["sequence"]


def bits(v):
    return np.asarray(v, dtype=f32).view(u32)


def test_the_launch_constants_are_the_sources():
    got = tc.source_constants()
    assert got == {"CHUNK_ITERS": [tc.CHUNK_ITERS], "CHUNK_WAVES": [tc.CHUNK_WAVES], "SUBQ": [tc.SUBQ], "GRID_CAP": [tc.GRID_CAP]}, got


@functools.lru_cache(maxsize=None)
def frames_of(run):
    """[(oracle frame, {view: expectation})] of a run; the expectations take the oracle's pyramid, which for one sample is
    asserted to be the injected plane's"""
    cfg, frames = tw.run_frames(run)
    ex, orc, out = tw.Expect(cfg), tw.OracleRun(cfg), []
    for world, matrix in frames:
        plane = tw.plane_of(cfg)
        fo = orc.frame(world, matrix, plane)
        if plane is not None:
            assert np.array_equal(bits(tw.pyramid_of(plane)), bits(fo["hiz"]))
        out.append((fo, ex.frame(world, matrix, fo["hiz"])))
    return cfg, out


@pytest.mark.parametrize("run", ALL_RUNS)
def test_reference_equals_oracle(run):
    """verdict() and expected_lists() against r3o_cull_triangles inside whole OracleRenderer.render frames: headers, pass and
    residual sets of every view of every frame, as bits"""
    cfg, frames = frames_of(run)
    for f, (fo, es) in enumerate(frames):
        assert set(es) == ({"viewport", "shadow"} if cfg["light"] else {"viewport"})
        for name, e in es.items():
            got = fo if name == "viewport" else fo["shadows"][0]
            tag = f"{run} frame {f} {name}"
            assert np.array_equal(got["header"].view(u32), e["header"].view(u32)), tag
            assert np.array_equal(got["visible"].astype(bool), e["drawn"]), tag
            n = e["total"]
            d = np.flatnonzero(got["pass"][:n] != e["pass"])
            assert len(d) == 0, f"{tag}: pass differs at {[(int(e['object'][i]), int(e['triangle'][i]), tw.TABLE.names[e['ids'][i]]) for i in d[:4]]}"
            if name == "viewport":
                d = np.flatnonzero(got["residual"][:n] != e["residual"])
                assert len(d) == 0, f"{tag}: residual differs at {[(int(e['object'][i]), int(e['triangle'][i])) for i in d[:4]]}"
                if f == 0:
                    assert np.array_equal(e["residual"], e["pass"])
            else:
                assert not e["residual"].any()
            assert e["calls"][:3].sum() == 3 * int(e["pass"].sum()) and e["calls"][3:].sum() == 3 * int(e["residual"].sum())


def test_sequence_has_every_kind_of_history():
    """between its frames: residual triangles although the object was drawn last frame (the camera changed), slot bases that moved,
    slots beyond last frame's capacity, rewritten slots, a slot back from outside the frustum -- all newly visible where they pass"""
    _cfg, frames = frames_of("sequence")
    es = [e["viewport"] for _fo, e in frames]
    for f in range(1, len(es)):
        e, p = es[f], es[f - 1]
        assert 0 < e["residual"].sum() < e["pass"].sum(), f
    assert not np.array_equal(es[1]["tri_base"][:8], es[0]["tri_base"][:8]) and es[2]["total"] > es[1]["total"]
    assert len(es[2]["ntri"]) > len(es[1]["ntri"]) and es[2]["drawn"][len(es[1]["ntri"]):].all()
    steps = tw.run_frames("sequence")[1]
    assert list(tw.rewritten_slots(steps[2][0], steps[3][0])) == [2, 5]
    for slot in (2, 5):  # rewritten: every passing triangle is residual
        e = es[3]
        sel = e["object"] == slot
        assert e["pass"][sel].any() and np.array_equal(e["pass"][sel], e["residual"][sel])
    for slot in (3, 6):  # outside in frame 3, back in frame 4 without history
        assert not es[3]["drawn"][slot] and es[4]["drawn"][slot]
        sel = es[4]["object"] == slot
        assert es[4]["pass"][sel].any() and np.array_equal(es[4]["pass"][sel], es[4]["residual"][sel])


# ------------------------------------------------------------------ the catalogue
def catalogue_trace(flags=0):
    return tc.trace(flags, False, (64, 64), tw.M_AFFINE, tw.TABLE.positions, tw.pyramid_of(tw.cone_plane(64, 64)), tc.hiz_desc(64, 64))


def test_every_catalogue_entry_is_on_its_edge():
    tr = catalogue_trace()
    checked = set()
    for i, (name, _pos, want) in enumerate(tw.TABLE.cat):
        rule = tc.RULES[tr["rule"][i]]
        for k, v in want.items():
            checked.add(k)
            tag = f"{name}: {k}"
            if k == "rule":
                assert rule == v, f"{tag}: {rule}"
            elif k == "not_rule":
                assert rule != v and tc.RULES.index(rule) > tc.RULES.index(v), f"{tag}: {rule}"
            elif k == "det_sign":
                assert np.sign(tr["det"][i]) == v, tag
            elif k in ("det", "longest", "occ", "depth"):
                assert bits(tr[k][i]) == bits(v), f"{tag}: {tr[k][i]!r}"
            elif k == "next_above":
                edge = f32(2 ** (want["mip"] - 1))
                if v:  # the next f32 above the edge, as bits
                    assert bits(tr["longest"][i]) == bits(np.nextafter(edge, f32(np.inf))), f"{tag}: {tr['longest'][i]!r}"
                else:  # not reachable: the clip coordinate is the next f32 above the edge's own, which gives edge + 2^-19 exactly
                    assert bits(tr["clip"][i, 2, 0]) == bits(np.nextafter(tw.clip64(edge), f32(1.0))), tag
                    assert bits(tr["longest"][i] - edge) == bits(f32(2.0) ** -19), f"{tag}: {tr['longest'][i]!r}"
            elif k in ("smin_x", "smax_x", "smin_y", "smax_y"):
                assert bits(tr[k[:4]][i, "xy".index(k[-1])]) == bits(v), tag
            elif k in ("mip", "lx", "hx", "ly", "hy"):
                assert int(tr[k][i]) == v, f"{tag}: {tr[k][i]}"
            elif k in ("px_integer", "py_integer"):
                p = tr[k[:2]][i]
                assert p == np.floor(p) and int(tr["l" + k[1]][i]) == int(tr["h" + k[1]][i]) == int(p), tag
            elif k in ("px_negative", "py_negative"):
                assert tr[k[:2]][i] < 0 and int(tr["l" + k[1]][i]) == 0, tag
            elif k in ("px_above", "py_above"):
                side = int(tr["mw" if k[1] == "x" else "mh"][i])
                assert tr[k[:2]][i] > side - 1 and int(tr["h" + k[1]][i]) == side - 1, tag
            elif k == "side_1":
                assert int(tr["mw"][i]) == int(tr["mh"][i]) == 1, tag
            elif k in ("lx_clamped_high", "ly_clamped_high"):
                side = int(tr["mw" if k[1] == "x" else "mh"][i])
                assert np.floor(tr["p" + k[1]][i]) > side - 1 and int(tr[k[:2]][i]) == side - 1, tag
            elif k in ("hx_clamped_low", "hy_clamped_low"):
                assert np.ceil(tr["p" + k[1]][i]) < 0 and int(tr[k[:2]][i]) == 0, tag
            elif k == "deep_texel":
                assert [bits(t) == bits(tw.DEEP) for t in tr["texels"][i]] == [j == v for j in range(4)], tag
                assert sum(bits(t) == bits(tw.OCC) for t in tr["texels"][i]) == 3, tag
            else:
                raise AssertionError(f"no check for {k}")
    assert len(checked) >= 25
    # the det entries under the other flag value: zero is rejected by both, the steps swap
    other = catalogue_trace(tc.POSITIVE_AREA_VISIBLE)
    names = [n for n, *_ in tw.TABLE.cat]
    for name, want in (("det0_collinear", True), ("det0_repeated", True), ("det_step_negative", True), ("det_step_positive", False)):
        assert (tc.RULES[other["rule"][names.index(name)]] == "backface") == want, name
    # the multisampled flag: no entry is rejected by the rint rule, and the ties' triangles pass
    ms = catalogue_trace(tc.MULTISAMPLED)
    assert not np.isin(ms["rule"], [tc.RULES.index("rint_x"), tc.RULES.index("rint_y")]).any()
    for name in ("rint_x_k_odd", "rint_y_k_odd"):
        assert ms["visible"][names.index(name)] and not tr["visible"][names.index(name)]


def test_the_w_triangles_are_what_their_names_say():
    tr = tc.trace(0, False, (64, 64), tw.M_W, tw.TABLE.positions, tw.pyramid_of(tw.cone_plane(64, 64)), tc.hiz_desc(64, 64))
    first = len(tw.TABLE.cat)
    w = {n: tr["clip"][first + i, :, 3] for i, (n, _p) in enumerate(tw.TABLE.wcat)}
    at = {n: first + i for i, (n, _p) in enumerate(tw.TABLE.wcat)}
    assert sorted(w["w_one_negative"] < 0) == [False, False, True] and (w["w_all_negative"] < 0).all()
    assert sorted(w["w_one_zero"] == 0) == [False, False, True] and np.isinf(tr["ndc"][at["w_one_zero"]]).any()
    assert int(tr["mip"][at["w_one_zero"]]) == 6 and np.isinf(tr["uv"][at["w_one_zero"]]).any(), "infinite NDC: the last level, an infinite centre"
    assert (w["w_two_zero"] == 0).sum() == 2 and int(tr["mip"][at["w_two_zero"]]) == 6 and np.isnan(tr["uv"][at["w_two_zero"]]).any(), "a NaN centre"
    assert (int(tr["lx"][at["w_two_zero"]]), int(tr["hx"][at["w_two_zero"]])) == (0, 0), "NaN -> texel 0 on both sides (a one-texel level)"
    assert (w["w_tiny"] == f32(2.0) ** -20).all() and (w["w_two"] == 2).all()
    later = [n for n in w if tc.RULES[tr["rule"][at[n]]] != "backface"]
    assert {n.replace("_flipped", "") for n in later} >= {"w_all_negative", "w_tiny", "w_two"}, later


# ------------------------------------------------------------------ what the worlds reach
def view_kind(run, matrix, name):
    return "shadow" if name == "shadow" else "viewport-w" if matrix == "w" else "viewport"


def test_every_rule_decides_in_every_view_kind():
    """over the triangles the worlds draw: every rule rejects some and lets some through (a later rule decided them)"""
    seen = {}
    for run in ALL_RUNS:
        _cfg, frames = frames_of(run)
        matrices = [m for _w, m in tw.run_frames(run)[1]]
        for (fo, es), matrix in zip(frames, matrices):
            for name, e in es.items():
                drawn_ids = np.unique(e["ids"][e["drawn"][e["object"]]])
                seen.setdefault(view_kind(run, matrix, name), set()).update(tc.RULES[r] for r in e["trace"]["rule"][drawn_ids])
    assert seen["viewport"] == seen["viewport-w"] == {"backface", "rint_x", "rint_y", "occluded", "visible"}, seen
    assert seen["shadow"] == {"backface", "rint_x", "rint_y", "shadow"}, seen


def test_every_slot_kind_the_wrap_and_the_second_trip_are_reached():
    plan = frames_of("structure-64x64-left")[1][0][1]["viewport"]["plan"]
    kind, why, lanes, it, wf, cont = (plan[k] for k in ("kind", "why", "lanes", "iteration", "wavefront", "continues"))
    assert {k for k in kind if k is not None} == {tc.PAIR_FIRST, tc.PAIR_SECOND, tc.SINGLE}
    assert {w for w in why if w is not None} == {tc.WHY_LAST_ITERATION, tc.WHY_NEXT_OBJECT, tc.WHY_LAST_SLOT}
    second = kind == tc.PAIR_SECOND
    assert (second & (lanes == 1)).any(), "a pair whose second slot ends in lane 0"
    assert (second & (lanes > 1) & (lanes < 64)).any(), "a pair whose second slot is partly filled"
    assert (second & (lanes == 64)).any()
    last_it = (kind == tc.SINGLE) & (it == tc.CHUNK_ITERS - 1) & cont
    assert (last_it & (wf < 3)).any(), "a single at it == 3 whose object goes on in the next wavefront"
    assert (last_it & (wf == 3)).any(), "a single at it == 3 whose object goes on in the next chunk"
    assert ((kind == tc.SINGLE) & (lanes < 64)).any() and ((kind == tc.SINGLE) & (lanes == 64)).any()
    assert (plan["entry"][plan["total_waves"]:] == -1).all() and plan["total_waves"] % tc.CHUNK_WAVES != 0, "padding slots in the last chunk"
    assert plan["nchunks"] <= tc.SUBQ and plan["trip"].max() == 0
    wrap = frames_of("wrap-64x64-left")[1][0][1]["viewport"]["plan"]
    assert wrap["nchunks"] > tc.SUBQ and wrap["trip"].max() == 0
    assert (wrap["sublist"][wrap["chunk"] == tc.SUBQ] == 0).all()
    trip = frames_of("second-trip-64x64-left")[1][0][1]["viewport"]["plan"]
    assert trip["grid"] == tc.GRID_CAP and trip["trip"].max() == 1 and trip["total_waves"] > 65_536
    # an object above 2 048 triangles: beyond the wavefront-wide first-entry store's first round
    assert max(tw.STRUCTURE_ORDER) == 2049 and set(tw.NTRI_VALUES) <= set(tw.STRUCTURE_ORDER)


def test_every_ballot_form_and_both_history_masks_are_reached():
    _cfg, frames = frames_of("structure-64x64-left")
    e0, e1 = frames[0][1]["viewport"], frames[1][1]["viewport"]
    b = tw.ballots(e0)
    full = u64(0xFFFFFFFFFFFFFFFF)
    forms = {"all_ones": full, "all_zeros": u64(0), "lane_0": u64(1), "lane_63": u64(1) << u64(63), "alternating": u64(0x5555555555555555)}
    assert [int(b[i]) for i in range(5)] == [int(forms[f]) for f in tw.FORMS], "object 0 starts at the run's first entry"
    full_slots = e0["plan"]["lanes"] == 64
    for name, v in forms.items():
        assert (b[full_slots] == v).any(), name
    assert len(np.unique(b)) > 40, "and a seeded mix"
    now, before = tw.ballots(e1), tw.previous_ballots(e1, e0)
    both = ((now & before) != 0) & ((now & ~before) != 0)
    assert both.any(), "a slot with triangles that passed last frame and triangles that did not"
    assert ((before & ~now) != 0).any(), "and one that lost triangles"
    for run in ("sequence", "wrap-64x64-left"):
        fr = frames_of(run)[1]
        es = [e["viewport"] for _fo, e in fr]
        assert any((((tw.ballots(es[f]) & tw.previous_ballots(es[f], es[f - 1])) != 0) & ((tw.ballots(es[f]) & ~tw.previous_ballots(es[f], es[f - 1])) != 0)).any()
                   for f in range(1, len(es))), run


def test_every_key_holds_entries_in_both_lists():
    for run in ("structure-64x64-left", "sequence"):
        e = frames_of(run)[1][0][1]["viewport"]
        assert all(len(e["predicted"][k]) and len(e["residual_list"][k]) for k in range(3)), run
        beyond = tw.structure_world()["material"] == tw.BEYOND_TABLE
        assert beyond.any() and (e["key"][: len(beyond)][beyond] == 0).all()
        assert np.isin(e["predicted"][0][:, 0], np.flatnonzero(beyond)).any(), "a material index beyond the table lists under key 0"


# ------------------------------------------------------------------ the list checker itself
def corruptions(e, refs, counts, subcap):
    """(what check_list must say, refs, counts) for every way a list can be wrong that the sets, the sums and the image do not
    show: what a slip in the compaction (a wrong lane prefix, a wrong running offset, a wrong region) leaves behind"""
    flat = counts.reshape(-1).astype(np.int64)
    begin = np.concatenate([[0], np.cumsum(flat)])
    big = [int(r) for r in np.argsort(-flat)]                     # regions by size
    r0 = next(r for r in big if r < tc.SUBQ)                      # a key-0 region
    r1 = next(r for r in big if tc.SUBQ <= r < 2 * tc.SUBQ)       # a key-1 region
    rq = next(r for r in big if r < tc.SUBQ and r != r0 and flat[r])  # another sub-list of key 0
    out = []
    dup = refs.copy()
    dup[begin[r0] + 1] = dup[begin[r0]]                            # the count right, one store missing, one made twice
    out.append(("more than once", dup, counts))
    swap = refs.copy()
    swap[[begin[r0], begin[r1]]] = swap[[begin[r1], begin[r0]]]
    out.append(("another key's region", swap, counts))
    stale = refs.copy()
    stale[begin[r0] + 2] = 0xFFFFFFFF                              # never written
    out.append(("names no triangle", stale, counts))
    beyond = refs.copy()
    o = int(beyond[begin[r0], 0])
    beyond[begin[r0], 1] = e["ntri"][o]                            # the object's clamped lane
    out.append(("names no triangle", beyond, counts))
    old = refs.copy()
    not_passing = np.flatnonzero((e["pass"] == 0) & e["drawn"][e["object"]] & (e["key"][e["object"]] == 0))[0]
    old[begin[r0] + 3] = (e["object"][not_passing], e["triangle"][not_passing])  # a stale entry that names a real triangle
    out.append(("lacks 1 entries", old, counts))
    moved = refs.copy()
    moved[[begin[r0], begin[rq]]] = moved[[begin[rq], begin[r0]]]  # the region of another chunk's sub-list
    out.append(("another sub-list", moved, counts))
    over = counts.copy()
    over.reshape(-1)[r0] = subcap + 1
    out.append(("exceeds", refs, over))
    short = counts.copy()
    short.reshape(-1)[r0] -= 1
    out.append(("3 x counts", np.delete(refs, begin[r0], axis=0), short))
    return out


@pytest.mark.parametrize("run,which", [("wrap-64x64-left", 0), ("wrap-64x64-left", 1), ("structure-64x64-left", 1)])
def test_the_list_checker_rejects_every_corruption(run, which):
    """check_list (what the GPU file holds every list to) on lists made on the CPU: the one a correct launch leaves passes, and each
    failure the sets and sums cannot show -- a duplicate, another key's region, an unwritten entry, a clamped lane, a stale entry
    inside the count, another sub-list's region, a count above the reservation, a missing entry -- is named"""
    _cfg, frames = frames_of(run)
    e = frames[0][1]["viewport"]
    refs, counts = tw.simulate_list(e, which)
    cap, subcap = len(e["ntri"]), tw.expected_subcap(e, len(e["ntri"]))
    vertex = e["calls"][3 * which:3 * which + 3]
    tw.check_list(e, which, refs, counts, subcap, cap, vertex, e["pass"], run)
    for says, bad_refs, bad_counts in corruptions(e, refs, counts, subcap):
        with pytest.raises(AssertionError, match=says):
            tw.check_list(e, which, bad_refs, bad_counts, subcap, cap, vertex, e["pass"], run)
    with pytest.raises(AssertionError, match="reserved per region"):
        tw.check_list(e, which, refs, counts, subcap + 1024, cap, vertex, e["pass"], run)
    if which == 0:
        with pytest.raises(AssertionError, match="result bits"):
            tw.check_list(e, which, refs, counts, subcap, cap, vertex, 1 - e["pass"], run)


@pytest.mark.parametrize("run", [r for r in tw.RUNS if r.startswith("structure")])
def test_structure_worlds_pass_a_quarter_to_three_quarters(run):
    """a condition on the inputs, on the reference alone: frame 0, every view"""
    _cfg, frames = frames_of(run)
    for name, e in frames[0][1].items():
        share = e["pass"].sum() / e["ntri"][e["drawn"]].sum()
        assert 0.25 <= share <= 0.75, f"{run} {name}: {share:.3f}"
