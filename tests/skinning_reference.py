"""Row S1 (GPU skinning): a numpy restatement of rend3-routine/shaders/src/skinning.wgsl:37-94 and math/matrix.wgsl:1-7, written
from the shader and from DESIGN.md section 2 (one rounding per operation, no FMA contraction, left-to-right sums:
`mat4 * vec4 = ((c0 x + c1 y) + c2 z) + c3 w`, `mat3 * vec3 = (c0 x + c1 y) + c2 z`, `dot3 = (x x' + y y') + z z'`,
`normalize(v) = v * (1 / sqrt(dot3(v, v)))`), over the ABI's own data: the u32 words of the mesh buffer, the 40-byte
GpuSkinningInput records (ten u32: base position / normal / tangent, joint indices, joint weights, updated position / normal /
tangent byte offsets, joint matrix base, vertex count) and the column-major joint matrices.

skin()     float32, every numpy operation rounds once: the bit reference of k_skinning and of oracle/r3o.c::r3o_skinning.
skin_f64() the same sums in float64 over the same f32 inputs, with the magnitude sums the error bounds of
           tests/test_skinning_edges.py are stated in.

There is no numpy restatement of the matrix-core order (R3N_SKIN_MFMA): numpy has no fused multiply-add and emulating one
through float64 rounds twice.  r3o_skinning_mfma_order stays that kernel's bit reference; skin_f64() is its independent check.
"""
import numpy as np

f32 = np.float32
INVALID = 0xFFFFFFFF
RECORD_WORDS = 10
(BASE_POS, BASE_NRM, BASE_TAN, JOINT_IDX, JOINT_WGT, OUT_POS, OUT_NRM, OUT_TAN, MATRIX_BASE, VERTEX_COUNT) = range(10)


def _fetch(words, byte_off, n, per_vertex):
    """extract_attribute_*: `per_vertex` consecutive words of each of the n vertices of the run at byte_off, (n, per_vertex)."""
    at = int(byte_off) // 4 + per_vertex * np.arange(n, dtype=np.int64)[:, None] + np.arange(per_vertex, dtype=np.int64)
    return words[at]


def _inputs(words, rec, dtype):
    """skinning.wgsl:45-64: joint indices (n, 4), weights (n, 4) f32, position / normal / tangent (n, 3) in dtype; an attribute
    whose base offset is INVALID reads as zeros."""
    n = int(rec[VERTEX_COUNT])
    jj = _fetch(words, rec[JOINT_IDX], n, 2)  # extract_attribute_vec4_u16: two u16 per word, low half first
    ji = np.stack([jj[:, 0] & 0xFFFF, jj[:, 0] >> 16, jj[:, 1] & 0xFFFF, jj[:, 1] >> 16], axis=1).astype(np.int64)
    jw = _fetch(words, rec[JOINT_WGT], n, 4).view(f32)
    attrs = []
    for k in (BASE_POS, BASE_NRM, BASE_TAN):
        attrs.append(np.zeros((n, 3), dtype=dtype) if int(rec[k]) == INVALID else _fetch(words, rec[k], n, 3).view(f32).astype(dtype))
    return n, ji, jw, attrs


def _store(words, byte_off, values):
    if int(byte_off) != INVALID:  # store_attribute_vec3_f32, skinning.wgsl:85-93
        at = int(byte_off) // 4
        words[at:at + values.size] = np.ascontiguousarray(values, dtype=f32).reshape(-1).view(np.uint32)


def _mat3_vec3(m, v):
    return (m[:, 0:3] * v[:, 0:1] + m[:, 4:7] * v[:, 1:2]) + m[:, 8:11] * v[:, 2:3]


def _dot_columns(m):
    """dot(c_k, c_k) of the three mat3 columns (math/matrix.wgsl:1-7), (n, 3)."""
    return np.stack([(m[:, 4 * k] * m[:, 4 * k] + m[:, 4 * k + 1] * m[:, 4 * k + 1]) + m[:, 4 * k + 2] * m[:, 4 * k + 2] for k in range(3)], axis=1)


def _normalize(v, one):
    d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return v * (one / np.sqrt(d))[:, None]


def skin(mesh_words, records, matrices):
    """skinning.wgsl:37-94 for every record in order (the reference dispatches skeleton by skeleton, skinning.rs:181-198), in
    float32.  Returns the mesh words after the pass; the arguments are left alone."""
    words = np.array(mesh_words, dtype=np.uint32, copy=True).reshape(-1)
    records = np.asarray(records, dtype=np.uint32).reshape(-1, RECORD_WORDS)
    mats = np.ascontiguousarray(matrices, dtype=f32).reshape(-1, 16)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        for rec in records:
            n, ji, jw, (pos, nrm, tan) = _inputs(words, rec, f32)
            pa, na, ta = (np.zeros((n, 3), dtype=f32) for _ in range(3))
            for i in range(4):
                wt = jw[:, i]
                take = wt > 0  # skinning.wgsl:69: false for 0, -0, negatives and NaN
                # a skipped influence reads no matrix: give it one that exists
                m = mats[np.where(take, int(rec[MATRIX_BASE]) + ji[:, i], 0)]
                w1, t1 = wt[:, None], take[:, None]
                p4 = ((m[:, 0:3] * pos[:, 0:1] + m[:, 4:7] * pos[:, 1:2]) + m[:, 8:11] * pos[:, 2:3]) + m[:, 12:15] * one
                pa = np.where(t1, pa + p4 * w1, pa)
                inv = one / _dot_columns(m)
                na = np.where(t1, na + _mat3_vec3(m, inv * nrm) * w1, na)
                ta = np.where(t1, ta + _mat3_vec3(m, inv * tan) * w1, ta)
            assert pa.dtype == na.dtype == ta.dtype == f32
            _store(words, rec[OUT_POS], pa)
            _store(words, rec[OUT_NRM], _normalize(na, one))
            _store(words, rec[OUT_TAN], _normalize(ta, one))
    return words


def skin_f64(mesh_words, records, matrices):
    """The sums of skin() in float64 over the same f32 inputs, nothing stored.  Per record a dict of (n, 3) float64 arrays:
    pos, pos_S = sum_i |w_i| sum_k |m_rk| |p_k| (p_3 = 1); nrm_acc (not normalised), nrm_S = sum_i |w_i| sum_k |m_rk| |n_k| /
    dot(c_k, c_k); tan_acc, tan_S likewise.  The sums run over the influences the shader takes (weight > 0)."""
    words = np.asarray(mesh_words, dtype=np.uint32).reshape(-1)
    records = np.asarray(records, dtype=np.uint32).reshape(-1, RECORD_WORDS)
    mats = np.ascontiguousarray(matrices, dtype=f32).reshape(-1, 16).astype(np.float64)
    out = []
    with np.errstate(all="ignore"):
        for rec in records:
            n, ji, jw, (pos, nrm, tan) = _inputs(words, rec, np.float64)
            res = {k: np.zeros((n, 3)) for k in ("pos", "pos_S", "nrm_acc", "nrm_S", "tan_acc", "tan_S")}
            for i in range(4):
                take = jw[:, i] > 0
                m = mats[np.where(take, int(rec[MATRIX_BASE]) + ji[:, i], 0)]
                w1 = np.where(take, jw[:, i].astype(np.float64), 0.0)[:, None]
                am, aw = np.abs(m), np.abs(w1)
                inv = 1.0 / _dot_columns(m)
                terms = dict(pos=_mat3_vec3(m, pos) + m[:, 12:15], pos_S=_mat3_vec3(am, np.abs(pos)) + am[:, 12:15],
                             nrm_acc=_mat3_vec3(m, inv * nrm), nrm_S=_mat3_vec3(am, inv * np.abs(nrm)),
                             tan_acc=_mat3_vec3(m, inv * tan), tan_S=_mat3_vec3(am, inv * np.abs(tan)))
                for k, t in terms.items():
                    res[k] = np.where(take[:, None], res[k] + t * (aw if k.endswith("_S") else w1), res[k])
            out.append(res)
    return out
