#!/usr/bin/env python3
"""GPU box: what the morph node (r3n_morph, csrc/morph.hip) costs, against its traffic floor.

Two workloads, both with POSITION + NORMAL deltas and T = 8 targets, each with 2 of 8 and with 8 of 8 weights non-zero:
  (a) 1 instance x 1 048 576 vertices
  (b) 10 000 instances x 1 000 vertices of ONE mesh (the deltas and the base runs are shared: after the first instance they come
      from the caches, only the output runs are unique bytes)
Per figure: every instance's weights are set, the renderer's one r3n_morph call is made, the queue is drained and the `morph`
stage (HIP events around the launch) is read and reset; medians over the timed repeats.  Next to each time: the algorithmic bytes
12 * A * (2 + T_active) per vertex for A = 2 morphed attributes, and those bytes over the copy rate r3n_hbm_copy_rate measures in
the same run.  The blended runs of the last repeat are compared with the numpy statement of the contract on a sample.

--parent DIR: additionally `python bench.py` (the default workload: no morph instance, the node never launches) on this tree and
on a built checkout of the parent commit in DIR, alternated, `--bench-runs` times each; reported as the two ranges.

usage: python tools/morph_cost.py [--repeats 20] [--warmup 3] [--parent DIR] [--out profiles/morph.md]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

f32 = np.float32
T, A = 8, 2
WORKLOADS = [("1 instance x 1 048 576 vertices", 1, 1_048_576), ("10 000 instances x 1 000 vertices", 10_000, 1_000)]


def reference(base, deltas, weights):
    acc = base.copy()
    for t, w in enumerate(weights):
        if w != 0.0:
            acc = (acc + (f32(w) * deltas[t]).astype(f32)).astype(f32)
    return acc


def measure(r3, name, n_instances, n_vertices, repeats, warmup, rows):
    rng = np.random.default_rng(0x4D0F)
    r = r3.Renderer(r3.host.LEFT)
    copy_gbs = r.hbm_copy_rate()
    base = {k: rng.uniform(-1.0, 1.0, (n_vertices, 3)).astype(f32) for k in ("positions", "normals")}
    deltas = {k: rng.uniform(-0.1, 0.1, (T, n_vertices, 3)).astype(f32) for k in ("positions", "normals")}
    mesh = r.add_mesh(base["positions"], np.zeros(3, dtype=np.uint32), normals=base["normals"],
                      morph_targets=dict(positions=deltas["positions"], normals=deltas["normals"], tangents=None))
    insts = r.add_morph_instances_bulk(mesh, [None] * n_instances)
    r.timing_enable(True)
    for active in (2, 8):
        times = []
        for k in range(warmup + repeats):
            w = np.zeros(T, dtype=f32)
            w[rng.choice(T, active, replace=False)] = rng.uniform(0.2, 1.0, active).astype(f32)
            for h in insts:
                r.set_morph_weights(h, w)
            r.stage_times()
            r._flush_morphs()
            r.sync()
            ms, launches = r.stage_times()["morph"]
            assert launches == 1
            if k >= warmup:
                times.append(ms)
        for h in (insts[0], insts[-1]):  # the last repeat's answer is the contract's
            for a, key in enumerate(("positions", "normals")):
                n = min(3 * n_vertices, 3 * 4096)
                got = r.readback_mesh_words(r.morphs[h]["out_off"][a], n)
                want = reference(base[key].reshape(-1)[:n], deltas[key].reshape(T, -1)[:, :n], w).view(np.uint32)
                assert np.array_equal(got, want), (name, active, key)
        nbytes = 12.0 * A * (2 + active) * n_vertices * n_instances
        med = float(np.median(times))
        floor_ms = 1e3 * nbytes / (copy_gbs * 1e9)
        rows.append(f"| {name} | {active} of {T} | {med * 1e3:.1f} µs ({min(times) * 1e3:.1f} – {max(times) * 1e3:.1f}) | {nbytes / 1e6:.1f} MB | "
                    f"{nbytes / med / 1e9:.2f} TB/s | {copy_gbs / 1e3:.2f} TB/s | {floor_ms / med:.2f} |")
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("morph_cost: needs the GPU (a timing taken anywhere else says nothing)")
    import rend3_amd as r3
    lines = ["# The morph node against its traffic floor", "",
             f"`python tools/morph_cost.py` on one MI355X: P + N deltas, T = {T}, {args.repeats} timed repeats after {args.warmup} warm-up calls "
             "per figure, medians (range).  `morph` stage = HIP events around the one launch of an `r3n_morph` call, queue drained after "
             f"every call.  Algorithmic bytes = 12 · A · (2 + T_active) per vertex, A = {A}.  Copy rate = `r3n_hbm_copy_rate` in the same "
             "process.  In the second workload the 10 000 instances share one mesh: its base runs and deltas (216 KB) are read from the "
             "caches after the first instance, so its \"algorithmic\" rate counts bytes that never reach HBM.", "",
             "| workload | non-zero weights | `morph` stage | algorithmic bytes | algorithmic rate | copy rate | share of the copy rate |",
             "|---|---|---|---|---|---|---|"]
    for name, n_inst, n_vert in WORKLOADS:
        measure(r3, name, n_inst, n_vert, args.repeats, args.warmup, lines)
    lines.append("")
    if args.parent:
        here, parent = [], []
        for _ in range(args.bench_runs):  # alternated: the two trees see the same drift
            parent.append(bench_once(args.parent, args.bench_steps, 8))
            here.append(bench_once(ROOT, args.bench_steps, 8))
        fmt = lambda v: f"{min(v):.4f} – {max(v):.4f} ms per frame ({', '.join(f'{x:.4f}' for x in v)})"  # noqa: E731
        lines += [f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup 8` (default workload, no morph instance, the node never "
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
