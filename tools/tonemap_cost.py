#!/usr/bin/env python3
"""GPU box: what the tonemapping operators and the auto-exposure (r3n_tonemap_set) cost at 3840 x 2160, one sample, on the
benchmark's workload (bench.py build_workload, its camera path) -- every figure from one session.

Each leg is a process of its own (one library per process):
  a  the parent commit's library, nothing set              (five runs: their spread is the yardstick for b)
  b  this library, nothing set                             (three runs; must lie within the spread of a)
  c  this library, MANUAL + ACES
  d  this library, AUTO + ACES
Per leg: the frame's wall time over `--frames` pipelined frames (as bench.py times them), then, with the stage taps on and the
streams serialised, the R3N_STAGE_TONEMAP time and launches per frame.  Legs c and d also tonemap an all-one-bin target (a
constant image injected with r3n_hdr_write) -- the histogram's worst case for LDS contention.

The histogram kernel has no stage of its own (R3N_STAGE_COUNT is pinned): "histogram + step" is the TONEMAP stage of d minus that of
c, in the same session, each span already net of the tap's overhead; the step kernel (one wave) is inside it.  It reads 8 B per
pixel, reported against r3n_hbm_copy_rate of the same process.

  python tools/tonemap_cost.py --build-parent HEAD~1    # the parent's csrc out of git into variants/parent/librend3_amd.so (needs no GPU)
  python tools/tonemap_cost.py [--frames 40] [--out profiles/tonemap.md]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT_SO = os.path.join(ROOT, "variants", "parent", "librend3_amd.so")
NEW_SYMBOLS = ("r3n_tonemap_set", "r3n_readback_exposure")
W, H = 3840, 2160


def build_parent(rev):
    import tarfile
    import io
    from rend3_amd import build
    src = os.path.join(ROOT, "variants", "src_parent")
    os.makedirs(src, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "rend3_amd/csrc", "include"], capture_output=True, check=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(src)
    units = set(build.UNITS)
    have = set(os.listdir(os.path.join(src, "rend3_amd", "csrc")))
    for u in units - have:  # units this commit adds do not exist there
        del build.UNITS[u]
    for u in build.UNITS:
        build.UNITS[u] = [h for h in build.UNITS[u] if os.path.exists(os.path.join(src, "rend3_amd", "csrc", h))]
    os.makedirs(os.path.dirname(PARENT_SO), exist_ok=True)
    print(build.build(force=True, out=PARENT_SO, obj_dir=os.path.join(ROOT, "variants", "obj_parent"), csrc=os.path.join(src, "rend3_amd", "csrc")))


def leg(mode, frames):
    import numpy as np
    import bench
    from rend3_amd import _ffi
    if os.environ.get("R3N_LIB"):  # the parent's library has no r3n_tonemap_set: this leg never calls it
        for name in NEW_SYMBOLS:
            _ffi.SIGNATURES.pop(name)
    import rend3_amd as r3
    args = argparse.Namespace(scene=None, config=3, objects=3000, tris=2_800_000, untextured=False, instanced=False, bistro_v2=False, samples=1)
    r = r3.Renderer(r3.host.RIGHT, np.float32(W) / np.float32(H))
    info = bench.build_workload(args, r, r3.host, r3.material_record)
    view0 = info["camera"][0]
    if mode == "manual":
        r.set_tonemapping("aces", exposure_ev=-1.0)
    elif mode == "auto":
        r.set_tonemapping("aces", auto_exposure=r3.AutoExposure(speed=3.0))
    step = [0]

    def frame():
        r.set_camera_data(bench.camera_path(r3.host, view0, step[0]), info["camera"][1])
        step[0] += 1
        r.render(W, H, samples=1, ambient=info["ambient"], clear_color=info["clear"], readback=False)

    for _ in range(8):
        frame()
    r.sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame()
    r.sync()
    out = dict(mode=mode, frame_ms=1e3 * (time.perf_counter() - t0) / frames)
    r.set_multi_stream(False)
    r.timing_enable(True)
    for _ in range(2):
        frame()
    r.sync()
    r.stage_times(reset=True)
    n = 10
    for _ in range(n):
        frame()
    r.sync()
    ms, launches = r.stage_times(reset=True)["tonemap"]
    out.update(tonemap_ms=ms / n, tonemap_launches=launches / n)
    if mode != "default":
        flat = np.empty((W * H, 4), dtype=np.uint16)
        flat[:] = np.array([0.4, 0.4, 0.4, 1.0], dtype=np.float16).view(np.uint16)
        fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (W, H))
        clear = np.zeros(4, dtype=np.float32)
        for k in range(n + 2):
            if k == 2:
                r.sync()
                r.stage_times(reset=True)
            r._check(r.lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), W, H, 1, _ffi.ptr(clear), 32, 32), "r3n_frame_begin")
            r._check(r.lib.r3n_hdr_write(r.ctx, _ffi.ptr(flat), 0, W * H), "r3n_hdr_write")
            r._check(r.lib.r3n_tonemap(r.ctx, None, 0), "r3n_tonemap")
            r._check(r.lib.r3n_frame_end(r.ctx), "r3n_frame_end")
        r.sync()
        out["one_bin_tonemap_ms"] = r.stage_times(reset=True)["tonemap"][0] / n
    r.timing_enable(False)
    out["hbm_gb_s"] = r.hbm_copy_rate(1 << 30, 5)
    r.close()
    print("LEG " + json.dumps(out))


def run_leg(mode, frames, lib=None):
    env = dict(os.environ)
    env.pop("R3N_LIB", None)
    if lib:
        env["R3N_LIB"] = lib
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", mode, "--frames", str(frames)], env=env, capture_output=True, text=True,
                         timeout=600)
    lines = [l for l in res.stdout.splitlines() if l.startswith("LEG ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"leg {mode} failed ({res.returncode}):\n" + res.stdout[-2000:] + res.stderr[-4000:])
    print(lines[-1], flush=True)
    return json.loads(lines[-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", default=None, metavar="REV")
    ap.add_argument("--leg", default=None, choices=("default", "manual", "auto"))
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tonemap.md"))
    args = ap.parse_args()
    if args.build_parent:
        return build_parent(args.build_parent)
    if args.leg:
        return leg(args.leg, args.frames)
    if not os.path.exists(PARENT_SO):
        raise SystemExit("no parent library: python tools/tonemap_cost.py --build-parent HEAD~1 first")
    a = [run_leg("default", args.frames, lib=PARENT_SO) for _ in range(5)]
    b = [run_leg("default", args.frames) for _ in range(3)]
    c = run_leg("manual", args.frames)
    d = run_leg("auto", args.frames)

    def spread(legs, key):
        v = sorted(l[key] for l in legs)
        return f"{v[len(v) // 2]:.4f} ({v[0]:.4f} - {v[-1]:.4f})"

    bytes_read = W * H * 8
    hbm = c["hbm_gb_s"]

    def hist(auto, key):
        ms = auto[key] - c[key]
        return ms, bytes_read / (ms * 1e-3) / 1e9

    a_lo, a_hi = min(l["frame_ms"] for l in a), max(l["frame_ms"] for l in a)
    b_mid = sorted(l["frame_ms"] for l in b)[1]
    rows = [("a  parent commit, nothing set (5 runs)", spread(a, "frame_ms"), spread(a, "tonemap_ms"), a[0]["tonemap_launches"]),
            ("b  this commit, nothing set (3 runs)", spread(b, "frame_ms"), spread(b, "tonemap_ms"), b[0]["tonemap_launches"]),
            ("c  MANUAL + ACES", f"{c['frame_ms']:.4f}", f"{c['tonemap_ms']:.4f}", c["tonemap_launches"]),
            ("d  AUTO + ACES", f"{d['frame_ms']:.4f}", f"{d['tonemap_ms']:.4f}", d["tonemap_launches"])]
    text = ["# Tonemapping operators and auto-exposure: cost at 3840 x 2160", "",
            "`python tools/tonemap_cost.py` on one MI355X, one session; the workload and camera path are bench.py's.  Frame: wall time per frame over "
            f"{args.frames} pipelined frames.  TONEMAP: the stage's time per frame with the taps on and the streams serialised (so the frame column and "
            "the stage column are different runs of the same process).  Median (min - max) where a leg ran more than once.", "",
            "| leg | frame ms | TONEMAP stage ms | TONEMAP launches per frame |", "|---|---|---|---|"]
    text += [f"| {n} | {f} | {t} | {l:g} |" for n, f, t, l in rows]
    text += ["", f"b within the spread of a: median of b {b_mid:.4f} ms against a's {a_lo:.4f} - {a_hi:.4f} ms: **{'yes' if a_lo <= b_mid <= a_hi else ('below it (faster)' if b_mid < a_lo else 'NO: slower')}**.", "",
             "## Histogram + step (stage of d minus stage of c; 8 B read per pixel, " + f"{bytes_read / 1e6:.1f} MB; r3n_hbm_copy_rate of the session: {hbm:.0f} GB/s)", "",
             "| input | ms | GB/s read | of the copy rate |", "|---|---|---|---|"]
    for label, key in (("bench frame", "tonemap_ms"), ("all one bin", "one_bin_tonemap_ms")):
        ms, gbs = hist(d, key)
        text.append(f"| {label} | {ms:.4f} | {gbs:.0f} | {100 * gbs / hbm:.0f} % |")
    text += ["", f"Operator kernel alone (stage of c): bench frame {c['tonemap_ms']:.4f} ms, all one bin {c['one_bin_tonemap_ms']:.4f} ms; it reads 8 B and writes 4 B per pixel.", "",
             "Launches: the histogram and the step are two launches.  A single launch with a last-block ticket was not built, so the two are not compared here; "
             "the step launch is inside the histogram + step figures above.", ""]
    open(args.out, "w").write("\n".join(text))
    print("\n".join(text))
    print(json.dumps(dict(a=a, b=b, c=c, d=d)))


if __name__ == "__main__":
    main()
