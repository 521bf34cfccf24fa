#!/usr/bin/env python3
"""GPU box: what the generated-tangents node (r3n_vertex_tangents, csrc/tangents.hip) costs, beside the `normals` stage of the same
flush, its algorithmic bytes and the host alternative it replaces.

Workload: the two shapes profiles/normals.md uses -- one instance of a 1024^2 grid (1 048 576 vertices) and 64 instances of a 256^2
grid (65 536 vertices each) -- interior valence 6, two triangles per vertex, uv0 the grid's own parametrisation with noise, one
POSITION-only morph target, `morph_normals="recompute"`, `build_tangents=True`, `morph_tangents="recompute"`.  Per figure: every
instance's weight is set, the renderer's flush makes its one r3n_morph, one r3n_vertex_normals and one r3n_vertex_tangents call, the
queue is drained and the stages (HIP events around each launch) are read and reset; medians over the timed repeats.  Next to it:
  * the algorithmic bytes per vertex: per adjacency entry 12 B of indices + 36 B of positions + 24 B of uv (every gather counted,
    although neighbouring rows gather the same words and the caches serve them), 4 B of adjacency per entry and per row, 12 B of
    normal read and 12 B written;
  * the host alternative for the same instances, timed in the same run: read the instance's positions and normals back,
    host.calculate_tangents (r3n_host_calculate_tangents), r3n_mesh_buffer_write of the run (wall clock, one instance timed, scaled
    by the instance count), and its ratio to the stage.
The tangent runs of the last repeat are compared with the host function's on the first and last instance.  No pass mark is set.

usage: python tools/tangents_cost.py [--repeats 20] [--warmup 3] [--out profiles/tangents.md]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

f32 = np.float32
SHAPES = ((1024, 1), (256, 64))  # (grid side, instances)
VALENCE = 6
BYTES_PER_ENTRY = 12 + 36 + 24
BYTES_PER_VERTEX = VALENCE * (BYTES_PER_ENTRY + 4) + 4 + 12 + 12


def grid(side, rng):
    u, w = np.meshgrid(np.linspace(-1.0, 1.0, side, dtype=f32), np.linspace(-1.0, 1.0, side, dtype=f32))
    pos = np.stack([u.reshape(-1), w.reshape(-1), rng.uniform(-0.01, 0.01, side * side).astype(f32)], axis=1).astype(f32)
    a = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None, :]).reshape(-1).astype(np.uint32)
    idx = np.stack([a, a + 1, a + side, a + 1, a + side + 1, a + side], axis=1).reshape(-1)
    uv = (np.stack([0.5 + 0.5 * pos[:, 0], 0.5 - 0.5 * pos[:, 1]], axis=1) + rng.uniform(-0.1, 0.1, (side * side, 2)) / side).astype(f32)
    return pos, idx, uv


def measure(r3, side, n_inst, repeats, warmup, rows):
    rng = np.random.default_rng(0x7A0F + side)
    pos, idx, uv = grid(side, rng)
    v = len(pos)
    delta = np.zeros((1, v, 3), dtype=f32)
    delta[0, :, 2] = 0.3 * (1.0 - pos[:, 0] * pos[:, 0]) * (1.0 - pos[:, 1] * pos[:, 1]) + rng.uniform(-0.01, 0.01, v).astype(f32)
    r = r3.Renderer(r3.host.LEFT)
    mesh = r.add_mesh(pos, idx, uv0=uv, morph_targets=dict(positions=delta, normals=None, tangents=None), morph_normals="recompute",
                      build_tangents=True, morph_tangents="recompute")
    insts = r.add_morph_instances_bulk(mesh, [None] * n_inst)
    r.timing_enable(True)
    times, normals_times = [], []
    for k in range(warmup + repeats):
        w = np.array([rng.uniform(0.2, 1.0)], dtype=f32)
        for h in insts:
            r.set_morph_weights(h, w)
        r.stage_times()
        r._flush_morphs()
        r.sync()
        t = r.stage_times()
        assert t["tangents"][1] == 1 and t["normals"][1] == 1 and t["morph"][1] == 1
        if k >= warmup:
            times.append(t["tangents"][0])
            normals_times.append(t["normals"][0])

    def host_words(out):
        morphed = r.readback_mesh_words(out[0], 3 * v).view(f32).reshape(-1, 3)
        normals = r.readback_mesh_words(out[1], 3 * v).view(f32).reshape(-1, 3)
        return np.ascontiguousarray(r3.host.calculate_tangents(morphed, normals, uv, idx)).reshape(-1).view(np.uint32)

    # the host alternative, one instance: read back, compute, write
    out = r.morphs[insts[0]]["out_off"]
    device_words = r.readback_mesh_words(out[2], 3 * v)
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        words = host_words(out)
        r._check(r.lib.r3n_mesh_buffer_write(r.ctx, out[2], r3._ffi.ptr(words), words.nbytes), "r3n_mesh_buffer_write")
        r.sync()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(device_words, words), (side, n_inst, "tangents differ from the host function's")
    last = r.morphs[insts[-1]]["out_off"]
    assert np.array_equal(r.readback_mesh_words(last[2], 3 * v), host_words(last)), (side, n_inst, "tangents differ from the host function's")
    nbytes = float(BYTES_PER_VERTEX) * v * n_inst
    med, med_n, host = float(np.median(times)), float(np.median(normals_times)), float(np.median(host_ms)) * n_inst
    rows.append(f"| {n_inst} x {side} x {side} = {n_inst} x {v:,} | {med * 1e3:.1f} µs ({min(times) * 1e3:.1f} – {max(times) * 1e3:.1f}) | "
                f"{med_n * 1e3:.1f} µs | {med / med_n:.2f} | {nbytes / 1e6:.1f} MB | {nbytes / med / 1e9:.2f} TB/s | "
                f"{1e3 * med / (v * n_inst) * 1e3:.3f} ns | {host:.1f} ms | {host / med:.0f} |")
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tangents_cost: needs the GPU (a timing taken anywhere else says nothing)")
    import rend3_amd as r3
    lines = ["# The generated-tangents node: cost, bytes, and the host alternative", "",
             f"`python tools/tangents_cost.py` on one MI355X: grid meshes (valence {VALENCE}) with uv0, one POSITION-only target, "
             "`morph_normals=\"recompute\"`, `build_tangents=True`, `morph_tangents=\"recompute\"`, "
             f"{args.repeats} timed repeats after {args.warmup} warm-up calls per figure, medians (range).  `tangents` stage = HIP events "
             "around the one launch of an `r3n_vertex_tangents` call, queue drained after every flush; the `normals` stage of the same "
             f"flush beside it.  Algorithmic bytes = {VALENCE} · ({BYTES_PER_ENTRY} + 4) + 4 + 12 + 12 = {BYTES_PER_VERTEX} B per vertex and "
             f"instance: per adjacency entry 12 B of indices, 36 B of positions, 24 B of uv and the entry's own 4 B, per vertex its row "
             "word, 12 B of normal and 12 B written -- every gather counted, although neighbouring rows gather the same words and the "
             "caches serve most of them, so the \"algorithmic rate\" is a gather rate, not HBM traffic.  Host alternative = read back "
             "the instance's positions and normals, `host.calculate_tangents`, `r3n_mesh_buffer_write` of the run, wall clock for one "
             "instance times the instance count, in the same run.  No pass mark is set on any of these figures.", "",
             "| instances x vertices | `tangents` stage | `normals` stage | tangents / normals | algorithmic bytes | algorithmic rate | per vertex | host alternative | host / stage |",
             "|---|---|---|---|---|---|---|---|---|"]
    for side, n_inst in SHAPES:
        measure(r3, side, n_inst, args.repeats, args.warmup, lines)
    lines.append("")
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
