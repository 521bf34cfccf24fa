"""The generated-tangents contract (DESIGN.md section 2 "Generated tangents", include/r3n.h r3n_vertex_tangents) restated in numpy,
independent of the product, twice: serial() transcribes Mesh::calculate_tangents_for_buffers (rend3-types/src/lib.rs:795-836,
zeroed = true, glam's scalar Vec3) line by line -- a scatter in index order -- and gather() walks normals_reference.adjacency the
way the kernel does.  Every f32 operation rounds once.

    T = floor(I / 3) triangles t = (i0, i1, i2); a remainder of the index run is ignored
    e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  a = uv[i1] - uv[i0];  b = uv[i2] - uv[i0]
    r = 1 / (a.x * b.y - a.y * b.x);  g_t = e1 * b.y - (e2 * a.y) * r                    (r multiplies the second product only)
    acc[v] = (+0, +0, +0);  for the triangles naming v, ascending, once per occurrence:  acc[v] = fl(acc[v] + g_t)
    d = (n.x * acc.x + n.y * acc.y) + n.z * acc.z;  q = acc - n * d
    rcp = 1 / sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);  out[v] = q * rcp if rcp is finite and > 0 else (+0, +0, +0)

The mesh set of the tangent tests lives here too, so that the CPU and the GPU tests look at the same shapes."""
import numpy as np

import normals_reference as NR

f32 = np.float32
_QUIET = dict(invalid="ignore", over="ignore", divide="ignore", under="ignore")


def _arrays(positions, normals, uvs, indices):
    p = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
    uv = np.ascontiguousarray(uvs, dtype=f32).reshape(-1, 2)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    assert len(n) == len(p) and len(uv) == len(p)
    return p, n, uv, idx


def _term(p, uv, i0, i1, i2):
    """lib.rs:809-825."""
    pos1, pos2, pos3 = p[i0], p[i1], p[i2]
    tex1, tex2, tex3 = uv[i0], uv[i1], uv[i2]
    edge1 = pos2 - pos1
    edge2 = pos3 - pos1
    uv1 = tex2 - tex1
    uv2 = tex3 - tex1
    r = f32(1.0) / f32(f32(uv1[0] * uv2[1]) - f32(uv1[1] * uv2[0]))
    # (edge1 * Vec3::splat(uv2.y)) - (edge2 * Vec3::splat(uv1.y)) * r
    return (edge1 * uv2[1]) - ((edge2 * uv1[1]) * r)


def _finish(tan, norm):
    """lib.rs:834-835: t = tan - norm * norm.dot(tan); normalize_or_zero."""
    d = f32(f32(f32(norm[0] * tan[0]) + f32(norm[1] * tan[1])) + f32(norm[2] * tan[2]))
    t = tan - (norm * d)
    l2 = f32(f32(f32(t[0] * t[0]) + f32(t[1] * t[1])) + f32(t[2] * t[2]))
    rcp = f32(1.0) / np.sqrt(l2)
    if np.isfinite(rcp) and rcp > 0:
        return t * rcp
    return np.zeros(3, dtype=f32)


def serial(positions, normals, uvs, indices):
    """f32[V, 3]: the reference's loop, in index order."""
    p, n, uv, idx = _arrays(positions, normals, uvs, indices)
    tangents = np.zeros((len(p), 3), dtype=f32)
    with np.errstate(**_QUIET):
        for c in range(len(idx) // 3):  # chunks_exact(3)
            i0, i1, i2 = (int(i) for i in idx[3 * c: 3 * c + 3])
            tangent = _term(p, uv, i0, i1, i2)
            tangents[i0] += tangent
            tangents[i1] += tangent
            tangents[i2] += tangent
        for v in range(len(p)):
            tangents[v] = _finish(tangents[v], n[v])
    assert tangents.dtype == f32
    return tangents


def gather(positions, normals, uvs, indices, adj=None, reverse_rows=False):
    """f32[V, 3], one vertex at a time over its adjacency row.  reverse_rows: walk every row backwards -- the same terms in another
    order, for the test that shows the order is observable."""
    p, n, uv, idx = _arrays(positions, normals, uvs, indices)
    v_count = len(p)
    adj = NR.adjacency(idx, v_count) if adj is None else np.asarray(adj, dtype=np.uint32)
    rows, lst = adj[: v_count + 1], adj[v_count + 1:]
    out = np.zeros((v_count, 3), dtype=f32)
    with np.errstate(**_QUIET):
        terms = np.zeros((len(idx) // 3, 3), dtype=f32)
        for t in range(len(terms)):
            terms[t] = _term(p, uv, *(int(i) for i in idx[3 * t: 3 * t + 3]))
        for v in range(v_count):
            row = lst[int(rows[v]): int(rows[v + 1])]
            acc = np.zeros(3, dtype=f32)  # +0
            for t in (row[::-1] if reverse_rows else row):
                acc = acc + terms[int(t)]
            out[v] = _finish(acc, n[v])
    return out


def unit_normals(rng, v):
    """Random unit vectors: the `normals given` case."""
    n = rng.normal(size=(v, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


# ------------------------------------------------------------------ the mesh set
SOUP_REPEAT = 32  # every 32nd triangle of a soup names a vertex twice


def soup(rng, v, n_tris):
    """Random triangles over the first three quarters of the vertices (the rest stay unreferenced), their three indices distinct,
    except that every SOUP_REPEAT-th one (t = 31, 63, ...) repeats an index, (i, i, j) and (i, j, i) alternately: such a triangle has
    no uv footprint and zeroes the tangent of every vertex it names.  Positions spread over several binades, so that the additions
    do not associate; one index word too many at the end (ignored, as chunks_exact(3) does)."""
    used = max(3, (3 * v) // 4)
    pos = (rng.uniform(-1.0, 1.0, (v, 3)) * np.exp2(rng.integers(-6, 7, (v, 1)))).astype(f32)
    idx = rng.permuted(np.tile(np.arange(used, dtype=np.uint32), (n_tris, 1)), axis=1)[:, :3].copy()
    for k, t in enumerate(range(SOUP_REPEAT - 1, n_tris, SOUP_REPEAT)):
        idx[t, 1 if k % 2 == 0 else 2] = idx[t, 0]
    return pos, np.concatenate([idx.reshape(-1), [0]]).astype(np.uint32)


def zero_share(pos, idx, uv):
    """The share of the referenced vertices whose serial() tangent is zero, with the normals the serial normals loop gives."""
    from oracle import host as oh
    whole = idx[: 3 * (len(idx) // 3)]
    got = serial(pos, oh.calculate_normals(pos, whole, True), uv, idx)
    ref = np.unique(whole)
    return float((~got[ref].any(axis=1)).sum()) / max(len(ref), 1)


def mesh_set(seed=0x54414E):
    """[(name, positions f32[V, 3], indices u32[I], uv0 f32[V, 2])]: the lone vertex, the triangle, the fans and the grids of
    normals_reference.mesh_set() (V in {1, 3, 63, 64, 65, 130, 257}) and this file's soups (V in {3, 63, 64, 65, 130, 257}); uv0 drawn per
    vertex from U(-2, 2)^2.  A condition of the set: no soup has more than a quarter of its referenced vertices at zero tangent."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = [m for m in NR.mesh_set() if not m[0].startswith("soup")]
    assert sorted({len(p) for _n, p, _i in out}) == [1, 3, 63, 64, 65, 130, 257] and len(out) == 8
    out += [(f"soup {v}",) + soup(rng, v, 2 * v) for v in (3, 63, 64, 65, 130, 257)]
    out = [(name, pos, idx, rng.uniform(-2.0, 2.0, (len(pos), 2)).astype(f32)) for name, pos, idx in out]
    for name, pos, idx, uv in out:
        if name.startswith("soup"):
            share = zero_share(pos, idx, uv)
            assert share <= 0.25, f"{name}: {share:.0%} of the referenced vertices have a zero tangent"
    return out
