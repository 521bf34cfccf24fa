#!/usr/bin/env python3
"""GPU box: what the recomputed-normals node (r3n_vertex_normals, csrc/normals.hip) costs, beside its algorithmic bytes, the
measured copy rate and the host alternative.

Workload: grid meshes (interior valence 6, two triangles per vertex) of 128^2, 256^2, 512^2 and 1024^2 vertices, one POSITION-only
morph target, `morph_normals="recompute"`, with 1, 8 and 64 instances of the mesh (fewer where the instances' runs would pass
256 MB).  Per figure: every instance's weight is set, the renderer's flush makes its one r3n_morph and one r3n_vertex_normals call,
the queue is drained and the `normals` stage (HIP events around the launch) is read and reset; medians over the timed repeats.
Next to each time:
  * the algorithmic bytes per vertex: 12 B position + 12 B normal written + 4 (1 + valence) B adjacency + 12 B per triangle of
    indices (two triangles per vertex on a grid), times the instances -- every instance counted in full, although the instances of
    one mesh share its indices and adjacency, which the caches serve after the first; positions gathered more than once (each is
    read by the ~6 triangles around it, from three vertices each) are counted once;
  * those bytes over the copy rate r3n_hbm_copy_rate measures in the same process;
  * the host alternative for the same instances: read the morphed positions back, host.calculate_normals, r3n_mesh_buffer_write
    (wall clock, one instance timed, scaled by the instance count).
The normal runs of the last repeat are compared with the host function's on the first and last instance.

--parent DIR: additionally `python bench.py` (the default workload: no recompute mesh, the node never launches) on this tree and
on a built checkout of the parent commit in DIR, alternated, `--bench-runs` times each; reported as the two ranges.

--only SIDE:INSTANCES: that one figure alone, no table -- the workload for a counter pass
(`rocprofv3 --pmc ... -- python tools/normals_cost.py --only 1024:1 --repeats 5`).

usage: python tools/normals_cost.py [--repeats 20] [--warmup 3] [--parent DIR] [--only SIDE:INSTANCES] [--out profiles/normals.md]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

f32 = np.float32
SIDES = (128, 256, 512, 1024)
INSTANCES = (1, 8, 64)
VALENCE = 6
BYTES_PER_VERTEX = 12 + 12 + 4 * (1 + VALENCE) + 12 * 2
MAX_RUN_BYTES = 256 << 20  # position + normal runs of all instances of one figure


def grid(side, rng):
    u, w = np.meshgrid(np.linspace(-1.0, 1.0, side, dtype=f32), np.linspace(-1.0, 1.0, side, dtype=f32))
    pos = np.stack([u.reshape(-1), w.reshape(-1), rng.uniform(-0.01, 0.01, side * side).astype(f32)], axis=1).astype(f32)
    a = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None, :]).reshape(-1).astype(np.uint32)
    idx = np.stack([a, a + 1, a + side, a + 1, a + side + 1, a + side], axis=1).reshape(-1)
    return pos, idx


def measure(r3, side, repeats, warmup, rows, instances=INSTANCES):
    rng = np.random.default_rng(0x4E0F + side)
    pos, idx = grid(side, rng)
    v = len(pos)
    delta = np.zeros((1, v, 3), dtype=f32)
    delta[0, :, 2] = 0.3 * (1.0 - pos[:, 0] * pos[:, 0]) * (1.0 - pos[:, 1] * pos[:, 1]) + rng.uniform(-0.01, 0.01, v).astype(f32)
    for n_inst in instances:
        if n_inst * v * 24 > MAX_RUN_BYTES:
            continue
        r = r3.Renderer(r3.host.LEFT)
        copy_gbs = r.hbm_copy_rate()
        mesh = r.add_mesh(pos, idx, morph_targets=dict(positions=delta, normals=None, tangents=None), morph_normals="recompute")
        insts = r.add_morph_instances_bulk(mesh, [None] * n_inst)
        r.timing_enable(True)
        times, morph_times = [], []
        for k in range(warmup + repeats):
            w = np.array([rng.uniform(0.2, 1.0)], dtype=f32)
            for h in insts:
                r.set_morph_weights(h, w)
            r.stage_times()
            r._flush_morphs()
            r.sync()
            t = r.stage_times()
            assert t["normals"][1] == 1 and t["morph"][1] == 1
            if k >= warmup:
                times.append(t["normals"][0])
                morph_times.append(t["morph"][0])
        # the host alternative, one instance: read back, compute, write
        out = r.morphs[insts[0]]["out_off"]
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            morphed = r.readback_mesh_words(out[0], 3 * v).view(f32).reshape(-1, 3)
            nrm = r3.host.calculate_normals(morphed, idx, True)
            words = np.ascontiguousarray(nrm).reshape(-1).view(np.uint32)
            r._check(r.lib.r3n_mesh_buffer_write(r.ctx, out[1], r3._ffi.ptr(words), words.nbytes), "r3n_mesh_buffer_write")
            r.sync()
            host_ms.append(1e3 * (time.perf_counter() - t0))
        # (the write above put the host function's normals into instance 0's run: the same words, or the check below fails)
        for h in (insts[0], insts[-1]):
            o = r.morphs[h]["out_off"]
            got = r.readback_mesh_words(o[1], 3 * v)
            if h != insts[0]:
                morphed = r.readback_mesh_words(o[0], 3 * v).view(f32).reshape(-1, 3)
                words = np.ascontiguousarray(r3.host.calculate_normals(morphed, idx, True)).reshape(-1).view(np.uint32)
            assert np.array_equal(got, words), (side, n_inst, "normals differ from the host function's")
        nbytes = float(BYTES_PER_VERTEX) * v * n_inst
        med = float(np.median(times))
        floor_ms = 1e3 * nbytes / (copy_gbs * 1e9)
        rows.append(f"| {side} x {side} = {v:,} | {n_inst} | {med * 1e3:.1f} µs ({min(times) * 1e3:.1f} – {max(times) * 1e3:.1f}) | "
                    f"{float(np.median(morph_times)) * 1e3:.1f} µs | {nbytes / 1e6:.1f} MB | {nbytes / med / 1e9:.2f} TB/s | {copy_gbs / 1e3:.2f} TB/s | "
                    f"{floor_ms / med:.2f} | {1e3 * med / (v * n_inst) * 1e3:.3f} ns | {float(np.median(host_ms)) * n_inst:.1f} ms |")
        r.close()


def bench_once(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    return 3840 * 2160 / (res["value"] * 1e6) * 1e3  # ms per frame from Mpixels/s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit: alternate bench.py with it")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=60)
    ap.add_argument("--only", default=None, metavar="SIDE:INSTANCES", help="one figure alone (the workload of a counter pass)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("normals_cost: needs the GPU (a timing taken anywhere else says nothing)")
    import rend3_amd as r3
    if args.only:
        side, n_inst = (int(x) for x in args.only.split(":"))
        rows = []
        measure(r3, side, args.repeats, args.warmup, rows, instances=(n_inst,))
        print("\n".join(rows))
        return
    lines = ["# The recomputed-normals node: cost, bytes, and the host alternative", "",
             f"`python tools/normals_cost.py` on one MI355X: grid meshes (valence {VALENCE}), one POSITION-only target, "
             f"`morph_normals=\"recompute\"`, {args.repeats} timed repeats after {args.warmup} warm-up calls per figure, medians (range).  "
             "`normals` stage = HIP events around the one launch of an `r3n_vertex_normals` call, queue drained after every call; `morph` "
             "stage of the same flush beside it.  Algorithmic bytes = "
             f"12 + 12 + 4 · (1 + {VALENCE}) + 12 · 2 = {BYTES_PER_VERTEX} B per vertex and instance (every instance counted in full: the "
             "indices and adjacency the instances of one mesh share come from the caches after the first, so with several instances the "
             "\"algorithmic\" rate counts bytes that never reach HBM; and up to 100 MB of runs fit the 256 MiB Infinity Cache from one "
             "repeat to the next).  Copy rate = `r3n_hbm_copy_rate` in the same process.  Host alternative = read back the morphed "
             "positions, `host.calculate_normals`, `r3n_mesh_buffer_write`, wall clock for one instance times the instance count.  "
             "No threshold is set on any of these figures.", "",
             "| vertices | instances | `normals` stage | `morph` stage | algorithmic bytes | algorithmic rate | copy rate | share of the copy rate | per vertex | host alternative |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for side in SIDES:
        measure(r3, side, args.repeats, args.warmup, lines)
    lines.append("")
    if args.parent:
        here, parent = [], []
        for _ in range(args.bench_runs):  # alternated: the two trees see the same drift
            parent.append(bench_once(args.parent, args.bench_steps, 8))
            here.append(bench_once(ROOT, args.bench_steps, 8))
        fmt = lambda v: f"{min(v):.4f} – {max(v):.4f} ms per frame ({', '.join(f'{x:.4f}' for x in v)})"  # noqa: E731
        lines += [f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup 8` (default workload, no recompute mesh, the node never "
                  f"launches), {args.bench_runs} runs each, alternated in this session:", "",
                  f"- parent commit: {fmt(parent)}", f"- this commit:   {fmt(here)}", ""]
    else:
        lines += ["`bench.py` against the parent commit: not measured in this run (`--parent DIR`).", ""]
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
