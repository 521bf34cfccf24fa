"""The recomputed-normals contract (DESIGN.md section 2 "Recomputed normals", include/r3n.h r3n_vertex_normals) restated in numpy
in its GATHER form, independent of the product, and the adjacency layout it walks.  Every f32 operation rounds once.

    T = floor(I / 3) triangles t = (i0, i1, i2); a remainder of the index run is ignored
    e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  n_t = cross(e1, e2) left-handed, cross(e2, e1) otherwise   (origin always p[i0])
    acc[v] = (+0, +0, +0);  for the triangles naming v, ascending, once per occurrence:  acc[v] = fl(acc[v] + n_t)
    rcp = 1 / sqrt((x * x + y * y) + z * z);  out[v] = acc[v] * rcp if rcp is finite and > 0 else (+0, +0, +0)

Adjacency, u32[V + 1 + 3 T]: rows[0 .. V], then the triangle numbers; row v = list[rows[v] : rows[v + 1]].

The mesh set of the normals tests lives here too, so that the CPU and the GPU tests look at the same shapes."""
import numpy as np

f32 = np.float32


def adjacency(indices, vertex_count):
    idx = np.asarray(indices, dtype=np.uint32).reshape(-1)
    n_tris = len(idx) // 3
    rows = [[] for _ in range(vertex_count)]
    for t in range(n_tris):          # ascending t, corner by corner: every row comes out ascending, one entry per occurrence
        for k in range(3):
            rows[int(idx[3 * t + k])].append(t)
    out = np.zeros(vertex_count + 1 + 3 * n_tris, dtype=np.uint32)
    at = 0
    for v, row in enumerate(rows):
        out[v] = at
        out[vertex_count + 1 + at: vertex_count + 1 + at + len(row)] = row
        at += len(row)
    out[vertex_count] = at
    return out


def _cross(a, b):
    return np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])], dtype=f32)


def face_terms(positions, indices, left_handed):
    p = np.asarray(positions, dtype=f32).reshape(-1, 3)
    idx = np.asarray(indices, dtype=np.uint32).reshape(-1)
    terms = np.zeros((len(idx) // 3, 3), dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(terms)):
            i0, i1, i2 = (int(i) for i in idx[3 * t: 3 * t + 3])
            e1, e2 = p[i1] - p[i0], p[i2] - p[i0]
            terms[t] = _cross(e1, e2) if left_handed else _cross(e2, e1)
    return terms


def gather(positions, indices, left_handed=True, adj=None, reverse_rows=False):
    """f32[V, 3].  adj: the adjacency words to walk (default: adjacency()); reverse_rows: walk every row backwards -- the same
    terms in another order, for the test that shows the order is observable."""
    p = np.asarray(positions, dtype=f32).reshape(-1, 3)
    v_count = len(p)
    adj = adjacency(indices, v_count) if adj is None else np.asarray(adj, dtype=np.uint32)
    rows, lst = adj[: v_count + 1], adj[v_count + 1:]
    terms = face_terms(p, indices, left_handed)
    out = np.zeros((v_count, 3), dtype=f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v in range(v_count):
            row = lst[int(rows[v]): int(rows[v + 1])]
            acc = np.zeros(3, dtype=f32)  # +0
            for t in (row[::-1] if reverse_rows else row):
                acc = (acc + terms[int(t)]).astype(f32)
            l2 = f32(f32(f32(acc[0] * acc[0]) + f32(acc[1] * acc[1])) + f32(acc[2] * acc[2]))
            rcp = f32(1.0) / np.sqrt(l2)
            if np.isfinite(rcp) and rcp > 0:
                out[v] = acc * rcp
    return out


# ------------------------------------------------------------------ the mesh set
def lone_vertex():
    return np.array([[0.25, -1.5, 3.0]], dtype=f32), np.zeros(0, dtype=np.uint32)


def one_triangle(rng):
    return rng.uniform(-1.0, 1.0, (3, 3)).astype(f32), np.array([0, 1, 2], dtype=np.uint32)


def fan(rng, v):
    """Vertex 0 is the hub of v - 2 triangles (0, k, k + 1): one row of length v - 2."""
    ang = np.linspace(0.0, 5.0, v - 1)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.2 * np.sin(3.0 * ang)], axis=1)
    pos = (np.concatenate([[[0.0, 0.0, 0.5]], rim]) + rng.uniform(-0.05, 0.05, (v, 3))).astype(f32)
    idx = np.array([(0, k, k + 1) for k in range(1, v - 1)], dtype=np.uint32).reshape(-1)
    return pos, idx


def grid(rng, nx, ny, extra=0):
    """nx x ny vertices (valence up to 6) plus `extra` unreferenced ones, z from the seed."""
    u, w = np.meshgrid(np.linspace(-1.0, 1.0, nx), np.linspace(-1.0, 1.0, ny))
    pos = np.stack([u.reshape(-1), w.reshape(-1), rng.uniform(-0.2, 0.2, nx * ny)], axis=1)
    pos = np.concatenate([pos, rng.uniform(-1.0, 1.0, (extra, 3))]).astype(f32)
    idx = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            idx += [a, a + 1, a + nx, a + 1, a + nx + 1, a + nx]
    return pos, np.array(idx, dtype=np.uint32)


def soup(rng, v, n_tris):
    """Random triangles over the first three quarters of the vertices (the rest stay unreferenced), every fifth one with a repeated
    index, (i, i, j) or (i, j, i); positions spread over several binades, so that the additions do not associate; one index word
    too many at the end (ignored, as chunks_exact(3) does)."""
    used = max(2, (3 * v) // 4)
    pos = (rng.uniform(-1.0, 1.0, (v, 3)) * np.exp2(rng.integers(-6, 7, (v, 1)))).astype(f32)
    idx = rng.integers(0, used, (n_tris, 3)).astype(np.uint32)
    for t in range(0, n_tris, 5):
        idx[t, 1 if (t // 5) % 2 == 0 else 2] = idx[t, 0]
    return pos, np.concatenate([idx.reshape(-1), [0]]).astype(np.uint32)


def mesh_set(seed=0x4E52):
    """[(name, positions f32[V, 3], indices u32[I])]: V in {1, 3, 63, 64, 65, 130, 257} over a lone unreferenced vertex, one
    triangle, fans (hub valence V - 2), grids and random soups."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = [("lone vertex",) + lone_vertex(), ("one triangle",) + one_triangle(rng)]
    out += [(f"fan {v}",) + fan(rng, v) for v in (63, 65, 257)]
    out += [("grid 8x8",) + grid(rng, 8, 8), ("grid 13x10",) + grid(rng, 13, 10), ("grid 16x16+1",) + grid(rng, 16, 16, extra=1)]
    out += [(f"soup {v}",) + soup(rng, v, 2 * v) for v in (3, 63, 64, 65, 130, 257)]
    assert sorted({len(p) for _n, p, _i in out}) == [1, 3, 63, 64, 65, 130, 257]
    return out
