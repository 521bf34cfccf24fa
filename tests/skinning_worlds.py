"""Small skinning worlds for tests/test_skinning_edges.py and tests/test_skinning_edges_gpu.py, as the raw triples the C ABI
takes: mesh-buffer words, GpuSkinningInput records (ten u32 each) and joint matrices.  Every run of every world lies between
sentinel words, output runs are pre-filled with a pattern of their own, so comparing the WHOLE buffer after a pass shows a write
outside an output run, a write to an input and a write through an INVALID output.  classify() names, per world, the paths its
vertices and influences take; CLASSES is what all worlds together must reach.

Finite worlds (every input and every result finite): "mixed_exact", "mixed_mfma".  Degenerate worlds, each declaring the exact
set of output words that are NaN (World.nan_words): "weights_special", "matrices_special", "hand_records".  No vertex of any
world names a joint at or beyond its skeleton's matrix count, in any slot.
"""
import collections

import numpy as np

f32 = np.float32
INVALID = 0xFFFFFFFF
SENTINEL = 0x5E171E15  # between all runs; as f32 a finite number (a NaN pattern would hide behind the NaN rule)
FILL = 0xC0DEC0DE      # what output runs hold before the pass; finite as f32 too
VERTEX_COUNTS = (1, 15, 16, 17, 48, 49, 63, 64, 65, 130)
ATTRS = ("pos", "nrm", "tan")

World = collections.namedtuple("World", "name words records matrices finite nan_words joint_counts meta")


def random_matrices(rng, n):
    """n joint matrices rotation * translation * non-uniform scale (0.5 .. 2 per axis), every third one mirrored (x scale
    negative), (n, 16) f32 column-major."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                    2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                    2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)  # [column][row]
    scale = rng.uniform(0.5, 2.0, (n, 3))
    scale[2::3, 0] *= -1.0
    m = np.zeros((n, 16))
    for k in range(3):
        m[:, 4 * k:4 * k + 3] = rot[:, k, :] * scale[:, k:k + 1]
    m[:, 12:15] = rng.uniform(-1.0, 1.0, (n, 3))
    m[:, 15] = 1.0
    return m.astype(f32)


def identity():
    return np.eye(4, dtype=f32).reshape(16)


class _Builder:
    def __init__(self, name, finite):
        self.name, self.finite = name, finite
        self.chunks, self.at = [], 0
        self.records, self.matrices, self.nan, self.meta = [], [], [], []

    def _push(self, words):
        self.chunks.append(np.ascontiguousarray(words, dtype=np.uint32).reshape(-1))
        self.at += len(self.chunks[-1])

    def run(self, words, mod=None):
        """A run behind at least one sentinel word; mod = (m, r): its byte offset is r modulo m.  Returns the byte offset."""
        self._push([SENTINEL])
        while mod is not None and (4 * self.at) % mod[0] != mod[1]:
            self._push([SENTINEL])
        off = 4 * self.at
        self._push(words)
        return off

    def skeleton(self, pos, nrm, tan, ji, jw, matrices, out=(True, True, True), base=(True, True, True), mods=None):
        """One mesh and one skeleton of it.  nrm / tan None: the mesh lacks the attribute (base and output INVALID).  out / base
        False: that offset of the record is INVALID although the mesh has the run (hand-built records).  mods: run name ->
        (m, r) for "pos", "nrm", "tan", "idx", "wgt", "out_pos", "out_nrm", "out_tan"."""
        mods = mods or {}
        n = len(pos)
        rec = [INVALID] * 8 + [sum(len(m) for m in self.matrices), n]
        for a, data in enumerate((pos, nrm, tan)):
            if data is not None:
                off = self.run(np.ascontiguousarray(data, dtype=f32).reshape(-1).view(np.uint32), mods.get(ATTRS[a]))
                if base[a]:
                    rec[a] = off
        rec[3] = self.run(np.ascontiguousarray(ji, dtype=np.uint16).reshape(-1, 4).view(np.uint32).reshape(-1), mods.get("idx"))
        rec[4] = self.run(np.ascontiguousarray(jw, dtype=f32).reshape(-1, 4).view(np.uint32).reshape(-1), mods.get("wgt"))
        for a, data in enumerate((pos, nrm, tan)):
            if data is not None and out[a]:
                rec[5 + a] = self.run(np.full(3 * n, FILL, dtype=np.uint32), mods.get("out_" + ATTRS[a]))
        assert int(np.asarray(ji).max()) < len(matrices), "a vertex names a joint its skeleton has no matrix for"
        self.records.append(rec)
        self.matrices.append(np.ascontiguousarray(matrices, dtype=f32).reshape(-1, 16))
        self.meta.append(dict(has=(True, nrm is not None, tan is not None)))
        return len(self.records) - 1

    def declare_nan(self, rec, vertex, attr, comps=(0, 1, 2)):
        """Output component(s) of one vertex that the shader's arithmetic makes NaN."""
        off = self.records[rec][5 + ATTRS.index(attr)]
        assert off != INVALID
        self.nan += [off // 4 + 3 * vertex + c for c in comps]

    def build(self):
        self._push([SENTINEL])
        records = np.array(self.records, dtype=np.uint32).reshape(-1, 10)
        return World(self.name, np.concatenate(self.chunks), records, np.concatenate(self.matrices), self.finite,
                     np.array(sorted(self.nan), dtype=np.int64), np.array([len(m) for m in self.matrices], dtype=np.uint32), self.meta)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


# weight patterns of the first vertices of every mesh of the finite worlds, one vertex each: (weights, joints drawn as: None = four random joints,
# "same" = one joint four times, "reverse" = the previous vertex's joints in reversed order)
_FINITE_RECIPES = (
    ((1.0, 0.0, 0.0, 0.0), None),       # one influence, first slot
    ((0.0, 0.0, 0.0, 1.0), None),       # one influence, last slot
    ((0.25, 0.25, 0.25, 0.25), None),   # four equal weights
    ((0.3, 0.2, 0.1, 0.05), None),      # sum below 1
    ((0.6, 0.5, 0.4, 0.3), None),       # sum above 1
    ((0.1, 0.2, 0.3, 0.4), "same"),     # all four influences on one joint
    ((0.4, 0.3, 0.2, 0.1), None),       # vertex 6 ...
    ((0.1, 0.2, 0.3, 0.4), "reverse"),  # ... and vertex 7: the same influences in reversed slot order, same attributes
)


def _finite_mesh(rng, n, joints, named):
    """n vertices over `joints` joints: the first vertices take the recipes above in turn, all the others random joints and
    random normalised weights (four influences, all taken).  named: joint indices that the vertices right behind the recipe
    block name in their first slot, one each, as far as the mesh has vertices there."""
    pos = rng.uniform(-2.0, 2.0, (n, 3)).astype(f32)
    nrm, tan = _unit(rng, n), _unit(rng, n)
    ji = rng.integers(0, joints, (n, 4)).astype(np.uint16)
    jw = rng.uniform(0.05, 1.0, (n, 4))
    jw = (jw / jw.sum(axis=1, keepdims=True)).astype(f32)
    for v, (w, how) in enumerate(_FINITE_RECIPES[:n]):
        jw[v] = w
        if how == "same":
            ji[v] = ji[v, 0]
        elif how == "reverse":
            ji[v], pos[v], nrm[v], tan[v] = ji[v - 1, ::-1], pos[v - 1], nrm[v - 1], tan[v - 1]
    for v, j in zip(range(len(_FINITE_RECIPES), n), named):
        ji[v, 0] = j
    return pos, nrm, tan, ji, jw


# (normals, tangents) present, per skeleton of the mixed worlds, and the runs that are pushed off the wide boundaries
_PRESENCE = ((1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (1, 0), (1, 1), (0, 1), (1, 1), (1, 1))
_MODS = ({}, {"wgt": (16, 4)}, {"idx": (8, 4)}, {"out_pos": (16, 4)}, {"out_nrm": (16, 8)}, {"out_pos": (16, 8), "wgt": (16, 4)},
         {"out_tan": (16, 4), "idx": (8, 4)}, {"pos": (16, 4)}, {"out_nrm": (16, 4), "wgt": (16, 4), "idx": (8, 4)}, {"out_tan": (16, 8)})


def _mixed(name, seed, joint_counts, named):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = _Builder(name, finite=True)
    for k, (n, joints) in enumerate(zip(VERTEX_COUNTS, joint_counts)):
        pos, nrm, tan, ji, jw = _finite_mesh(rng, n, joints, [j for j in named if j < joints])
        mats = random_matrices(rng, joints)
        if k % 2 == 0:
            mats[0] = identity()
        b.skeleton(pos, nrm if _PRESENCE[k][0] else None, tan if _PRESENCE[k][1] else None, ji, jw, mats, mods=_MODS[k])
    return b.build()


def mixed_exact():
    """Ten meshes of ten sizes in one launch (13 waves: the last block has idle waves), joint counts 1, 2, 5, 300 and 65 536,
    joints 0, 255, 256 and 65 535 named, every combination of normals / tangents, runs on 4- and 8-byte boundaries."""
    return _mixed("mixed_exact", 0x51A1, (1, 2, 5, 2, 1, 5, 2, 5, 300, 65536), (0, 255, 256, 65535, 299, 1, 4))


def mixed_mfma():
    """The same ten sizes over rigs of 1, 2, 3 and 4 joints, matrix bases spaced by the joint count."""
    return _mixed("mixed_mfma", 0x51A2, (1, 2, 3, 4, 4, 3, 2, 1, 3, 4), (0, 1, 2, 3))


def weights_special():
    """One 2-joint skeleton whose vertices carry the weights a file can hold and a sane exporter never writes.  The shader takes
    an influence iff weight > 0, so 0, -0, negatives and NaN are skipped; a vertex with no influence left has zero accumulators
    and normalize(0) = 0 * (1 / sqrt(0)) = 0 * inf = NaN in normal and tangent, while its position is a plain 0.  +inf is
    taken: position +-inf (no component of the transformed position is 0 here), normal +-inf before normalize, then
    inf * (1 / sqrt(inf)) = inf * 0 = NaN.  1e-45 and 1e-40 are subnormal and taken; next to a normal weight everything stays
    finite; alone, 1e-40 leaves a subnormal normal whose squares underflow to 0: v * (1 / sqrt(0)) = +-inf, not NaN."""
    rng = np.random.Generator(np.random.PCG64(0x51A3))
    nan, inf = np.nan, np.inf
    rows = [((0.0, 0.0, 0.0, 0.0), ("nrm", "tan")),
            ((-0.5, 1.5, 0.0, 0.0), ()),
            ((-0.0, 1.0, 0.0, 0.0), ()),
            ((nan, 1.0, 0.0, 0.0), ()),
            ((inf, 0.0, 0.0, 0.0), ("nrm", "tan")),
            ((inf, 1.0, 0.0, 0.0), ("nrm", "tan")),
            ((-1.0, -0.0, nan, 0.0), ("nrm", "tan")),
            ((1e-45, 1.0, 0.0, 0.0), ()),
            ((1e-40, 0.5, 0.0, 0.0), ()),
            ((1e-40, 0.0, 0.0, 0.0), ()),
            ((0.0, 0.0, 0.0, 1.0), ()),
            ((0.5, 0.5, 0.0, 0.0), ())]
    n = len(rows)
    pos = (rng.uniform(0.5, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
    ji = np.tile(np.array([0, 1, 1, 0], dtype=np.uint16), (n, 1))
    jw = np.array([r[0] for r in rows], dtype=f32)
    mats = random_matrices(rng, 2)
    b = _Builder("weights_special", finite=False)
    rec = b.skeleton(pos, _unit(rng, n), _unit(rng, n), ji, jw, mats)
    for v, (_w, attrs) in enumerate(rows):
        for a in attrs:
            b.declare_nan(rec, v, a)
    return b.build()


def matrices_special():
    """Two skeletons (4 and 3 joints) whose matrices are an identity and one degenerate matrix each; every vertex has one
    influence of weight 1 (the last two vertices of each: a degenerate joint in a slot of weight 0, which must not be read
    into the result, and an even blend with the identity).  With inv_k = 1 / dot(c_k, c_k) (math/matrix.wgsl):
      zero column c_1:       inv_1 = 1 / 0 = inf, c_1 * (inf * n_y) = 0 * inf = NaN in every row: normal and tangent NaN; the
                             position only loses its y term and is finite;
      c_0 = (1e20, 0, 0):    dot = 1e40 rounds to inf, inv_0 = 0, the x term drops out: everything finite;
      c_2 = (0, 0, 1e-20):   dot = 1e-40 (subnormal), inv_2 = inf, c_2 * (inf * n_z) = (NaN, NaN, inf): normalize spreads the
                             NaN to all three components; position finite;
      NaN at row 1 of c_1:   position y NaN (the only row that entry enters), inv_1 = NaN: normal and tangent NaN;
      inf translation x:     position x = +inf, not NaN; normal and tangent do not see the translation."""
    rng = np.random.Generator(np.random.PCG64(0x51A4))
    b = _Builder("matrices_special", finite=False)

    def degenerate(edit):
        m = identity()
        edit(m)
        return m

    def col(m, k, v):
        m[4 * k:4 * k + 3] = v

    def put(m, at, v):
        m[at] = v

    sets = [([identity(), degenerate(lambda m: col(m, 1, (0, 0, 0))), degenerate(lambda m: col(m, 0, (1e20, 0, 0))),
              degenerate(lambda m: col(m, 2, (0, 0, 1e-20)))],
             {1: (("nrm", (0, 1, 2)), ("tan", (0, 1, 2))), 2: (), 3: (("nrm", (0, 1, 2)), ("tan", (0, 1, 2)))}),
            ([identity(), degenerate(lambda m: put(m, 5, np.nan)), degenerate(lambda m: put(m, 12, np.inf))],
             {1: (("pos", (1,)), ("nrm", (0, 1, 2)), ("tan", (0, 1, 2))), 2: ()})]
    for mats, nan_of in sets:
        joints = len(mats)
        n = joints + 2 * (joints - 1)
        pos = (rng.uniform(0.5, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
        nrm = (rng.uniform(0.5, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
        tan = (rng.uniform(0.5, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(f32)
        ji, jw = np.zeros((n, 4), dtype=np.uint16), np.zeros((n, 4), dtype=f32)
        blends = {}
        for j in range(joints):  # one influence of weight 1 on joint j
            ji[j, 0], jw[j, 0] = j, 1.0
        for j in range(1, joints):
            v = joints + 2 * (j - 1)
            ji[v], jw[v] = (0, j, j, j), (1.0, 0.0, -1.0, np.nan)   # the degenerate joint only in skipped slots
            ji[v + 1], jw[v + 1] = (0, j, 0, 0), (0.5, 0.5, 0.0, 0.0)  # an even blend with the identity
            blends[v + 1] = j
        rec = b.skeleton(pos, nrm, tan, ji, jw, np.array(mats, dtype=f32))
        for v, j in list(enumerate(range(joints))) + list(blends.items()):
            for attr, comps in nan_of.get(j, ()):
                b.declare_nan(rec, v, attr, comps)
    return b.build()


def hand_records():
    """Records no renderer builds: an attribute whose base offset is INVALID while its output is valid (the shader reads zeros:
    a zero normal or tangent normalises to NaN, a zero position becomes the blended translation) and one whose base is valid
    while its output is INVALID (computed, never stored: the words where the renderer would have put it stay as they are)."""
    rng = np.random.Generator(np.random.PCG64(0x51A5))
    b = _Builder("hand_records", finite=False)
    for n, base, out, nan_attrs in ((17, (True, False, True), (True, True, False), ("nrm",)),
                                    (5, (False, True, False), (True, True, True), ("tan",)),
                                    (64, (True, True, True), (False, True, False), ())):
        pos, nrm, tan, ji, jw = _finite_mesh(rng, n, 2, (0, 1))
        rec = b.skeleton(pos, nrm, tan, ji, jw, random_matrices(rng, 2), out=out, base=base)
        for a in nan_attrs:
            for v in range(n):
                b.declare_nan(rec, v, a)
    return b.build()


_BUILDERS = (mixed_exact, mixed_mfma, weights_special, matrices_special, hand_records)
_CACHE = {}


def worlds():
    """Every world, built once (read-only: the tests copy what they change)."""
    if not _CACHE:
        for fn in _BUILDERS:
            w = fn()
            for a in (w.words, w.records, w.matrices, w.nan_words, w.joint_counts):
                a.setflags(write=False)
            _CACHE[w.name] = w
    return dict(_CACHE)


def mfma_worlds():
    """The worlds R3N_SKIN_MFMA takes: every rig has at most four joints."""
    return {k: w for k, w in worlds().items() if int(w.joint_counts.max()) <= 4}


def wave_count(world):
    return int(sum((int(n) + 63) // 64 for n in world.records[:, 9]))


def output_words(world):
    """Word indices of every output run of the world, ascending."""
    idx = [np.arange(int(r[k]) // 4, int(r[k]) // 4 + 3 * int(r[9])) for r in world.records for k in (5, 6, 7) if int(r[k]) != INVALID]
    return np.sort(np.concatenate(idx))


# ------------------------------------------------------------------ classifier
CLASSES = tuple(
    ["influence:taken", "influence:taken_inf", "influence:taken_subnormal", "influence:skipped_zero", "influence:skipped_negative_zero",
     "influence:skipped_negative", "influence:skipped_nan"]
    + [f"joint:{j}" for j in (0, 255, 256, 65535)] + ["joint:high_byte"]
    + ["vertex:first_slot_only", "vertex:last_slot_only", "vertex:four_equal", "vertex:sum_below_1", "vertex:sum_above_1",
       "vertex:all_skipped", "vertex:one_joint_four_times", "vertex:permuted_slots"]
    + [f"skeleton:vertices_{n}" for n in VERTEX_COUNTS] + ["skeleton:ragged_16_block", "skeleton:ragged_wave", "skeleton:several_waves"]
    + [f"skeleton:joints_{n}" for n in (1, 2, 3, 4, 5, 300, 65536)]
    + [f"skeleton:normals_{a}_tangents_{b}" for a in ("yes", "no") for b in ("yes", "no")]
    + ["skeleton:base_invalid_output_valid", "skeleton:base_valid_output_invalid"]
    + ["matrix:identity", "matrix:mirrored", "matrix:zero_column", "matrix:huge_column", "matrix:tiny_column", "matrix:nan_entry",
       "matrix:inf_translation", "matrix:scaled_rotation"]
    + ["align:weights_4_mod_16", "align:indices_4_mod_8", "align:output_4_mod_16", "align:output_8_mod_16"]
    + ["launch:mixed_sizes", "launch:mixed_joint_counts", "launch:idle_waves_in_last_block", "launch:mfma_rigs_1_2_3_4"])


def _matrix_classes(m):
    m = m.astype(np.float64)
    out = []
    c = m[[0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(3, 3)
    if np.isnan(m).any():
        return ["matrix:nan_entry"]
    if np.isinf(m[12:15]).any():
        return ["matrix:inf_translation"]
    lens = np.linalg.norm(c, axis=1)
    if (lens == 0).any():
        out.append("matrix:zero_column")
    if (lens >= 1e19).any():
        out.append("matrix:huge_column")
    if ((lens > 0) & (lens <= 1e-19)).any():
        out.append("matrix:tiny_column")
    if out:
        return out
    if np.array_equal(m, np.eye(4).reshape(16)):
        return ["matrix:identity"]
    return ["matrix:mirrored" if np.linalg.det(c) < 0 else "matrix:scaled_rotation"]


def classify(world):
    """The classes of CLASSES this world reaches, as a Counter (influences and vertices counted one by one)."""
    from skinning_reference import _inputs
    got = collections.Counter()
    rec_list = world.records
    for s, rec in enumerate(rec_list):
        n, ji, jw, _attrs = _inputs(world.words, rec, f32)
        joints = int(world.joint_counts[s])
        with np.errstate(all="ignore"):
            take = jw > 0
        bits = jw.view(np.uint32)
        got["influence:taken"] += int(take.sum())
        got["influence:taken_inf"] += int((take & np.isinf(jw)).sum())
        got["influence:taken_subnormal"] += int((take & ((bits & 0x7F800000) == 0)).sum())
        got["influence:skipped_zero"] += int((bits == 0).sum())
        got["influence:skipped_negative_zero"] += int((bits == 0x80000000).sum())
        got["influence:skipped_negative"] += int((jw < 0).sum())
        got["influence:skipped_nan"] += int(np.isnan(jw).sum())
        for j in (0, 255, 256, 65535):
            got[f"joint:{j}"] += int((take & (ji == j)).sum())
        got["joint:high_byte"] += int((take & (ji > 255)).sum())
        for m in np.unique(ji[take]):
            for c in _matrix_classes(world.matrices[int(rec[8]) + int(m)]):
                got[c] += 1
        ntake = take.sum(axis=1)
        got["vertex:first_slot_only"] += int(((ntake == 1) & take[:, 0]).sum())
        got["vertex:last_slot_only"] += int(((ntake == 1) & take[:, 3]).sum())
        got["vertex:all_skipped"] += int((ntake == 0).sum())
        full = ntake == 4
        finite = np.isfinite(jw).all(axis=1)
        with np.errstate(all="ignore"):
            total = jw.astype(np.float64).sum(axis=1)
        got["vertex:four_equal"] += int((full & (jw == jw[:, :1]).all(axis=1)).sum())
        got["vertex:sum_below_1"] += int((full & finite & (total < 0.999)).sum())
        got["vertex:sum_above_1"] += int((full & finite & (total > 1.001)).sum())
        got["vertex:one_joint_four_times"] += int((full & (ji == ji[:, :1]).all(axis=1)).sum())
        if n > 1:
            same = full[1:] & (ji[1:] == ji[:-1, ::-1]).all(axis=1) & (jw[1:] == jw[:-1, ::-1]).all(axis=1) & (ji[1:] != ji[:-1]).any(axis=1)
            got["vertex:permuted_slots"] += int(same.sum())
        if n in VERTEX_COUNTS:
            got[f"skeleton:vertices_{n}"] += 1
        got["skeleton:ragged_16_block"] += int(n % 16 != 0)
        got["skeleton:ragged_wave"] += int(n % 64 != 0)
        got["skeleton:several_waves"] += int(n > 64)
        got[f"skeleton:joints_{joints}"] += 1
        has = world.meta[s]["has"]
        base_valid, out_valid = [int(rec[k]) != INVALID for k in (0, 1, 2)], [int(rec[k]) != INVALID for k in (5, 6, 7)]
        if all(b == h and o == h for b, o, h in zip(base_valid, out_valid, has)):
            got[f"skeleton:normals_{'yes' if has[1] else 'no'}_tangents_{'yes' if has[2] else 'no'}"] += 1
        got["skeleton:base_invalid_output_valid"] += sum(1 for b, o in zip(base_valid, out_valid) if o and not b)
        got["skeleton:base_valid_output_invalid"] += sum(1 for b, o in zip(base_valid, out_valid) if b and not o)
        got["align:weights_4_mod_16"] += int(int(rec[4]) % 16 == 4)
        got["align:indices_4_mod_8"] += int(int(rec[3]) % 8 == 4)
        for k in (5, 6, 7):
            if int(rec[k]) != INVALID:
                got["align:output_4_mod_16"] += int(int(rec[k]) % 16 == 4)
                got["align:output_8_mod_16"] += int(int(rec[k]) % 16 == 8)
    counts = [int(c) for c in world.joint_counts]
    got["launch:mixed_sizes"] += int(len(set(int(r[9]) for r in rec_list)) > 1)
    got["launch:mixed_joint_counts"] += int(len(set(counts)) > 1)
    got["launch:idle_waves_in_last_block"] += int(wave_count(world) % 4 != 0)
    got["launch:mfma_rigs_1_2_3_4"] += int(set(counts) == {1, 2, 3, 4})
    return +got
