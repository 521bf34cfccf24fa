"""The morph-target contract (DESIGN.md section 2 "Morph targets", include/r3n.h r3n_morph) restated in numpy, independent of
the product: every f32 operation rounds once, zero weights are no terms, targets are summed in ascending order.

    acc = base[k]
    for t ascending:  if w[t] == 0.0f: continue  (+0 and -0; NaN is a term)
                      acc = fl(acc + fl(w[t] * delta[t][k]))
    out[k] = acc

Bounds: reach[t] = max_v sqrt((dx * dx + dy * dy) + dz * dz) over target t's position deltas;
radius' = (((r + |w0| * reach0) + |w1| * reach1) + ...) over the non-zero weights in target order.  All in f32."""
import numpy as np

f32 = np.float32


def blend(base, deltas, weights):
    """base: f32[...]; deltas: f32[T, ...]; weights: T floats.  Returns f32 of base's shape."""
    acc = np.array(base, dtype=f32, copy=True)
    deltas = np.asarray(deltas, dtype=f32)
    weights = np.asarray(weights, dtype=f32).reshape(-1)
    assert len(deltas) == len(weights) and deltas.shape[1:] == acc.shape
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(weights)):
            w = weights[t]
            if w == f32(0.0):
                continue
            product = (w * deltas[t]).astype(f32)   # one rounding
            acc = (acc + product).astype(f32)       # one rounding
    return acc


def reach(position_deltas):
    """f32[T]: how far target t moves any vertex at weight 1."""
    d = np.asarray(position_deltas, dtype=f32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    sq = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
    sq = (sq + (dz * dz).astype(f32)).astype(f32)
    return np.sqrt(sq).astype(f32).max(axis=1)


def radius(base_radius, weights, reaches):
    r = f32(base_radius)
    with np.errstate(invalid="ignore", over="ignore"):
        for w, rc in zip(np.asarray(weights, dtype=f32).reshape(-1), np.asarray(reaches, dtype=f32).reshape(-1)):
            if w == f32(0.0):
                continue
            r = f32(r + f32(f32(abs(w)) * f32(rc)))
    return r
