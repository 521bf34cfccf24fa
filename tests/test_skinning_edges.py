"""Row S1 (GPU skinning) at its edges, CPU part: tests/skinning_reference.py (numpy, from skinning.wgsl:37-94) against the
oracle's r3o_skinning word for word on the worlds of tests/skinning_worlds.py, proof that those worlds reach every path they
were built for, the float64 error bounds the GPU tests reuse, and the joint-count rules of the skeleton manager
(rend3/src/managers/skeleton.rs:67-163, mesh.rs:135-139) on OracleRenderer.

NaN rule: an arithmetic NaN has no defined sign or payload across machines, so two words that are both NaN as f32 compare equal.
To keep that rule from hiding a difference, the set of NaN OUTPUT words must be exactly the set each world declares (derived by
hand in the world's docstring), and empty in the finite worlds.

Float64 bounds (u = 2^-24, finite worlds only; derivation for the contract's order, one rounding per operation):
  position component r:  p_r = sum_i w_i * (((m_r0 x + m_r1 y) + m_r2 z) + m_r3).  A term's path crosses 1 product, 3 row adds,
    1 multiply by the weight and at most 4 accumulator adds: 9 roundings, so |p32 - p64| <= ((1 + u)^9 - 1) S <= 16 u S with
    S = sum_i |w_i| sum_k |m_rk| |p_k| (p_3 = 1).  The issue's count; kept.
  normal / tangent: acc_r = sum_i w_i * sum_k m_rk (n_k / dot(c_k, c_k)).  Path: dot 3 (one product, two adds of positive
    terms), the division 1, inv * n 1, the product with m 1, 2 row adds, the weight 1, 4 accumulator adds: 13 roundings, so
    |d acc|_2 <= 13 u |S_n|_2 (first order) with S_n,r = sum_i |w_i| sum_k |m_rk| |n_k| / dot(c_k, c_k).  Normalising moves a
    component by at most 2 |d acc|_2 / |acc|_2 (crude; first order it is 1), and normalize itself rounds dot (3), sqrt, the
    reciprocal and the product: (3 / 2 + 3) u < 8 u on a component of magnitude <= 1.  So
    |n32 - n64| <= 26 u |S_n| / |acc| + 4.5 u, inside the issue's 32 u |S_n| / |acc| + 8 u, which is what is asserted -- on the
    vertices with |acc| >= |S_n| / 64 (no catastrophic cancellation), which must be at least 95 % of them.
  The matrix-core order (r3o_skinning_mfma_order) crosses no more: position 4 fused steps + 3 adds of the slot's weight sum + 1
    product + 3 slot adds = 11 <= 16; normals 4 (dot, division) + 1 (column scale) + 4 + 3 + 1 + 3 = 16, times the crude factor 2
    = 32.  The same bounds hold.
"""
import numpy as np
import pytest

import skinning_reference as sr
import skinning_worlds as sw
from oracle import host as oh
from oracle.lib import get as oracle_lib
from oracle.world import OracleRenderer

f32 = np.float32
U = 2.0 ** -24
WORLDS = sorted(sw.worlds())
FINITE = [n for n in WORLDS if sw.worlds()[n].finite]
MFMA = sorted(sw.mfma_worlds())


def same_words(a, b):
    """Word-wise equality under the NaN rule, as a bool array."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return (a == b) | (np.isnan(a.view(f32)) & np.isnan(b.view(f32)))


def assert_same_words(got, want, what):
    bad = np.nonzero(~same_words(got, want))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} words differ, first at word {bad[:6]}: {np.asarray(got)[bad[:6]]} != {np.asarray(want)[bad[:6]]}"


def assert_nan_cap(world, words, what):
    """The NaN output words are exactly the declared ones."""
    out = sw.output_words(world)
    got = out[np.isnan(np.asarray(words, dtype=np.uint32).view(f32)[out])]
    assert np.array_equal(got, world.nan_words), (f"{what}: NaN output words differ from the world's declaration: undeclared "
                                                  f"{sorted(set(got) - set(world.nan_words))[:8]}, missing {sorted(set(world.nan_words) - set(got))[:8]}")


_REFERENCE = {}


def reference(name):
    """skin() of a world, computed once and shared (read-only)."""
    if name not in _REFERENCE:
        w = sw.worlds()[name]
        out = sr.skin(w.words, w.records, w.matrices)
        out.setflags(write=False)
        _REFERENCE[name] = out
    return _REFERENCE[name]


_TRUTH = {}


def truth(name):
    if name not in _TRUTH:
        w = sw.worlds()[name]
        _TRUTH[name] = sr.skin_f64(w.words, w.records, w.matrices)
    return _TRUTH[name]


def oracle_skin(world, mfma_order=False):
    lib = oracle_lib()
    words = world.words.copy()
    records, mats = np.ascontiguousarray(world.records), np.ascontiguousarray(world.matrices)
    if mfma_order:
        nj = np.ascontiguousarray(world.joint_counts)
        lib.r3o_skinning_mfma_order(lib.ptr(words), lib.ptr(records), len(records), lib.ptr(mats), lib.ptr(nj))
    else:
        lib.r3o_skinning(lib.ptr(words), lib.ptr(records), len(records), lib.ptr(mats))
    return words


def check_f64_bounds(world, words, what, report=None):
    """The docstring's bounds on every output run of a finite world.  Returns (vertices with a normal or tangent output,
    those that qualify for the normalised bound)."""
    vals = np.asarray(words, dtype=np.uint32).view(f32).astype(np.float64)
    seen = qualified = 0
    worst_p = worst_n = 0.0
    for rec, t in zip(world.records, truth(world.name)):
        n = int(rec[9])

        def run(k):
            return vals[int(rec[k]) // 4:int(rec[k]) // 4 + 3 * n].reshape(n, 3)
        if int(rec[5]) != sr.INVALID:
            err, bound = np.abs(run(5) - t["pos"]), 16 * U * t["pos_S"]
            worst_p = max(worst_p, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), f"{what}: position off by up to {(err / np.maximum(bound, 1e-300)).max():.3f} of its bound"
        for k, key in ((6, "nrm"), (7, "tan")):
            if int(rec[k]) == sr.INVALID:
                continue
            acc, s = np.linalg.norm(t[key + "_acc"], axis=1), np.linalg.norm(t[key + "_S"], axis=1)
            ok = acc >= s / 64
            seen, qualified = seen + n, qualified + int(ok.sum())
            want = t[key + "_acc"][ok] / acc[ok, None]
            err, bound = np.abs(run(k)[ok] - want), (32 * U * s[ok] / acc[ok] + 8 * U)[:, None]
            worst_n = max(worst_n, float((err / bound).max()) if ok.any() else 0.0)
            assert (err <= bound).all(), f"{what}: {key} off by up to {(err / bound).max():.3f} of its bound"
    if report is not None:
        report.append((what, worst_p, worst_n))
    return seen, qualified


# ------------------------------------------------------------------ the worlds
def test_worlds_reach_every_class():
    total = sum((sw.classify(w) for w in sw.worlds().values()), sw.collections.Counter())
    missing = [c for c in sw.CLASSES if total[c] == 0]
    assert not missing, f"no world reaches {missing}"
    assert set(total) <= set(sw.CLASSES), sorted(set(total) - set(sw.CLASSES))


def test_worlds_are_what_the_tests_need():
    ws = sw.worlds()
    exact, mfma = ws["mixed_exact"], ws["mixed_mfma"]
    for w in (exact, mfma):
        assert sorted(int(n) for n in w.records[:, 9]) == list(sw.VERTEX_COUNTS)
        assert sw.wave_count(w) % 4 != 0  # the last block of four waves has idle waves
    assert {1, 2, 5, 300, 65536} <= set(int(c) for c in exact.joint_counts)
    assert sorted(set(int(c) for c in mfma.joint_counts)) == [1, 2, 3, 4]
    for w in ws.values():
        # matrix bases are the running sums of the joint counts; no joint index, in any slot, reaches its skeleton's count
        assert np.array_equal(w.records[:, 8], np.concatenate([[0], np.cumsum(w.joint_counts)[:-1]]))
        assert int(w.joint_counts.sum()) == len(w.matrices)
        for rec, joints in zip(w.records, w.joint_counts):
            _n, ji, _jw, _attrs = sr._inputs(w.words, rec, f32)
            assert int(ji.max()) < int(joints)
        # sentinels in front of, behind and between all runs; the outputs hold their fill pattern
        assert w.words[0] == sw.SENTINEL and w.words[-1] == sw.SENTINEL
        out = sw.output_words(w)
        assert (w.words[out] == sw.FILL).all() and (w.words[out[np.r_[True, np.diff(out) > 1]] - 1] == sw.SENTINEL).all()
        if w.finite:
            assert len(w.nan_words) == 0 and np.isfinite(w.words.view(f32)).all() and np.isfinite(w.matrices).all()
    assert set(MFMA) == {"mixed_mfma", "weights_special", "matrices_special", "hand_records"}


# ------------------------------------------------------------------ reference == oracle, NaNs capped
@pytest.mark.parametrize("name", WORLDS)
def test_reference_equals_oracle_word_for_word(name):
    w = sw.worlds()[name]
    want = oracle_skin(w)
    assert_same_words(reference(name), want, f"{name}: skin() against r3o_skinning")
    assert_nan_cap(w, reference(name), name)
    assert_nan_cap(w, want, name + " (oracle)")
    # nothing but the output runs changes, and they all do
    changed = np.nonzero(reference(name) != w.words)[0]
    assert np.array_equal(changed, sw.output_words(w))


@pytest.mark.parametrize("name", FINITE)
def test_reference_within_float64_bounds(name):
    w = sw.worlds()[name]
    assert np.isfinite(reference(name).view(f32)).all()
    seen, qualified = check_f64_bounds(w, reference(name), name)
    assert seen > 0 and qualified >= 0.95 * seen, f"{name}: only {qualified} of {seen} normals / tangents are well conditioned"


@pytest.mark.parametrize("name", [n for n in FINITE if n in MFMA])
def test_mfma_order_within_float64_bounds(name):
    w = sw.worlds()[name]
    fused = oracle_skin(w, mfma_order=True)
    assert np.isfinite(fused.view(f32)).all()
    check_f64_bounds(w, fused, name + " (matrix-core order)")
    assert (fused != reference(name)).any(), "the two operation orders never differ: is the fused path wired up?"
    assert np.array_equal(np.nonzero(fused != w.words)[0], sw.output_words(w))


@pytest.mark.parametrize("name", MFMA)
def test_mfma_order_has_the_shader_s_nan_words(name):
    """The matrix-core order weights joint SLOTS, not influences.  A slot no taken influence names must add nothing, whatever
    its matrix holds, or one degenerate joint (a zero-scale column, a NaN entry, an inf translation) would put NaN into every
    vertex of its skeleton: the NaN output words are exactly the ones the world declares for the shader's order."""
    w = sw.worlds()[name]
    fused = oracle_skin(w, mfma_order=True)
    assert_nan_cap(w, fused, name + " (matrix-core order)")
    assert np.array_equal(np.nonzero(fused != w.words)[0], sw.output_words(w))


def test_reference_is_order_sensitive():
    """The bit equality above is not vacuous: the permuted-slot vertices of the mixed worlds hold the same influences in
    reversed slot order over the same attributes, and left-to-right f32 sums tell the two apart somewhere."""
    differ = close = 0
    for name in FINITE:
        w, ref = sw.worlds()[name], reference(name).view(f32)
        for rec in w.records:
            _n, ji, jw, _attrs = sr._inputs(w.words, rec, f32)
            for v in range(1, int(rec[9])):
                if (jw[v] > 0).all() and np.array_equal(ji[v], ji[v - 1, ::-1]) and np.array_equal(jw[v], jw[v - 1, ::-1]) and (ji[v] != ji[v - 1]).any():
                    a, b = ref[int(rec[5]) // 4 + 3 * (v - 1):][:3], ref[int(rec[5]) // 4 + 3 * v:][:3]
                    differ += int((a != b).any())
                    close += int(np.allclose(a, b, rtol=1e-5, atol=1e-6))
    assert close >= 8 and differ >= 1 and close >= differ


# ------------------------------------------------------------------ joint-count rules (skeleton.rs:67-163, mesh.rs:135-139)
def _tri(r, joint_indices, **kw):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=f32)
    kw.setdefault("joint_weights", np.tile(np.array([1, 0, 0, 0], dtype=f32), (3, 1)))
    return r.add_mesh(pos, np.array([0, 1, 2], dtype=np.uint32), joint_indices=np.asarray(joint_indices, dtype=np.uint16), **kw)


def _ident(n):
    return np.tile(oh.identity(), (n, 1))


def test_required_joint_count_is_the_highest_index_of_any_slot_plus_one():
    o = OracleRenderer(oh.LEFT)
    # joint 7 sits in a slot of weight 0: it counts all the same (mesh.rs:135-139 looks at the indices only)
    m = _tri(o, [[0, 7, 0, 0], [1, 0, 0, 0], [0, 0, 2, 0]])
    assert o.meshes[m].required_joint_count == 8
    assert o.meshes[_tri(o, np.zeros((3, 4)))].required_joint_count == 1
    assert o.meshes[_tri(o, [[0, 0, 0, 65535]] * 3)].required_joint_count == 65536
    plain = o.add_mesh(np.zeros((3, 3), dtype=f32), np.array([0, 1, 2], dtype=np.uint32))
    assert o.meshes[plain].required_joint_count is None
    from rend3_amd.renderer import checked_joint_matrices, required_joint_count
    assert required_joint_count([[0, 7, 0, 0], [1, 0, 0, 0]]) == 8 and required_joint_count([[0, 0, 0, 65535]]) == 65536
    assert checked_joint_matrices(8, _ident(9)).shape == (9, 16)  # the surplus is kept: the stored count is the given one
    with pytest.raises(ValueError, match=r"NotEnoughJoints.* 8 joints.* 7 joint matrices"):
        checked_joint_matrices(8, _ident(7))
    with pytest.raises(ValueError, match="joint indices"):
        checked_joint_matrices(None, _ident(1))


def test_joint_indices_without_weights_are_refused():
    o = OracleRenderer(oh.LEFT)
    with pytest.raises(ValueError, match="MissingAttributesJointWeights"):
        _tri(o, np.zeros((3, 4)), joint_weights=None)
    assert len(o.meshes) == 0 and len(o.mesh_words) == 0


def test_not_enough_joints_is_refused_before_anything_is_allocated():
    o = OracleRenderer(oh.LEFT)
    m = _tri(o, [[0, 4, 0, 0]] * 3)
    words = len(o.mesh_words)
    with pytest.raises(ValueError, match=r"NotEnoughJoints.* 5 joints.* 4 joint matrices"):
        o.add_skeleton(m, _ident(4))
    assert len(o.mesh_words) == words and o.skeletons == []
    sk = o.add_skeleton(m, _ident(5))
    assert len(o.skeletons[sk]["matrices"]) == 5 and len(o.mesh_words) == words + 2 * 9  # position and normal copies


def test_stored_count_is_fixed_at_creation():
    o = OracleRenderer(oh.LEFT)
    m2, m1 = _tri(o, [[0, 1, 0, 0]] * 3), _tri(o, np.zeros((3, 4)))
    a, b, c = o.add_skeleton(m2, _ident(6)), o.add_skeleton(m1, _ident(1)), o.add_skeleton(m2, _ident(2))
    assert [len(o.skeletons[s]["matrices"]) for s in (a, b, c)] == [6, 1, 2]  # not truncated to the mesh's 2: the documented deviation
    assert o.skinning_buffers()[0][:, 8].tolist() == [0, 6, 7]
    more = np.arange(8 * 16, dtype=f32).reshape(8, 16)
    o.set_skeleton_joint_matrices(a, more)  # two extra: truncated to the stored six (skeleton.rs:160-162)
    assert np.array_equal(o.skeletons[a]["matrices"], more[:6])
    with pytest.raises(ValueError, match=r"stores 6 joint matrices.* 5 joint matrices"):
        o.set_skeleton_joint_matrices(a, _ident(5))  # the reference's assert (skeleton.rs:153-159)
    assert np.array_equal(o.skeletons[a]["matrices"], more[:6])
    records, mats = o.skinning_buffers()
    assert records[:, 8].tolist() == [0, 6, 7] and len(mats) == 9
