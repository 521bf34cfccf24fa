#!/usr/bin/env python3
"""GPU box: what bloom (r3n_bloom_set) costs at 3840 x 2160, one sample, on the benchmark's workload (bench.py build_workload,
its camera path) -- every figure from one session.  Modelled on tools/tonemap_cost.py, whose parent build it reuses.

Each leg is a process of its own (one library per process):
  a  the parent commit's library, nothing set              (three runs: their spread is the yardstick for b)
  b  this library, nothing set                             (three runs; must lie within the spread of a, and launch nothing new)
  c  this library, MANUAL + ACES
  d  this library, MANUAL + ACES + bloom (Renderer.set_bloom's defaults, all 12 levels), then the bloom_tail sweep in the same process
Per leg: the frame's wall time over `--frames` pipelined frames (as bench.py times them), then, with the stage taps on and the
streams serialised, the R3N_STAGE_TONEMAP time and launches per frame.  The cost of bloom is the stage of d minus the stage of c.

  python tools/tonemap_cost.py --build-parent HEAD~1     # the parent's csrc into variants/parent/librend3_amd.so (needs no GPU)
  python tools/bloom_cost.py [--frames 40] [--out profiles/bloom.md]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARENT_SO = os.path.join(ROOT, "variants", "parent", "librend3_amd.so")
NEW_SYMBOLS = ("r3n_bloom_set", "r3n_readback_bloom")
W, H = 3840, 2160
TAILS = (0, 256, 1024, 4096, 16384, 65536)
MAX_LEVELS = 16  # every level the target has: 12 at 3840 x 2160


def level_sizes(max_levels):
    out, w, h = [], W, H
    while len(out) < max_levels:
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
        if max(w, h) == 1:
            break
    return out


def chain_bytes(max_levels):
    """what the chain must move: the HDR target read once, every level written once and read once going down, every level read
    and written going up, a_0 read by the composite"""
    texels = [w * h for w, h in level_sizes(max_levels)]
    return W * H * 8 + 4 * sum(texels) * 8 + texels[0] * 8


def leg(mode, frames):
    import ctypes
    import numpy as np
    import bench
    from rend3_amd import _ffi
    if os.environ.get("R3N_LIB"):  # the parent's library has no bloom entries: this leg never calls them
        for name in NEW_SYMBOLS:
            _ffi.SIGNATURES.pop(name)
    import rend3_amd as r3
    args = argparse.Namespace(scene=None, config=3, objects=3000, tris=2_800_000, untextured=False, instanced=False, bistro_v2=False, samples=1)
    r = r3.Renderer(r3.host.RIGHT, np.float32(W) / np.float32(H))
    info = bench.build_workload(args, r, r3.host, r3.material_record)
    view0 = info["camera"][0]
    if mode in ("manual", "bloom"):
        r.set_tonemapping("aces", exposure_ev=-1.0)
    if mode == "bloom":
        r.set_bloom(max_levels=MAX_LEVELS)
    step = [0]

    def frame():
        r.set_camera_data(bench.camera_path(r3.host, view0, step[0]), info["camera"][1])
        step[0] += 1
        r.render(W, H, samples=1, ambient=info["ambient"], clear_color=info["clear"], readback=False)

    def stage(n=10):
        for _ in range(2):
            frame()
        r.sync()
        r.stage_times(reset=True)
        for _ in range(n):
            frame()
        r.sync()
        ms, launches = r.stage_times(reset=True)["tonemap"]
        return ms / n, launches / n

    for _ in range(8):
        frame()
    r.sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame()
    r.sync()
    out = dict(mode=mode, frame_ms=1e3 * (time.perf_counter() - t0) / frames)
    set_tuning = r.lib.r3n_internal_set_tuning
    set_tuning.argtypes, set_tuning.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    if mode == "bloom":  # the pipelined frame under each plan: what the launches cost where nothing subtracts their gaps
        default_tail = [t for t in TAILS if f'R3N_BLOOM_TAIL_DEFAULT {t}u' in open(os.path.join(ROOT, "rend3_amd", "csrc", "bloom.h")).read()][0]
        pipelined = []
        for rep in range(3):
            for tail in TAILS:
                assert set_tuning(r.ctx, f"bloom_tail={tail}".encode()) == 0
                for _ in range(8):
                    frame()
                r.sync()
                t0 = time.perf_counter()
                for _ in range(frames):
                    frame()
                r.sync()
                pipelined.append(dict(tail=tail, rep=rep, frame_ms=1e3 * (time.perf_counter() - t0) / frames))
        out["pipelined"] = pipelined
        assert set_tuning(r.ctx, f"bloom_tail={default_tail}".encode()) == 0
    r.set_multi_stream(False)
    r.timing_enable(True)
    out["tonemap_ms"], out["tonemap_launches"] = stage()
    if mode == "bloom":
        out["levels"] = r.bloom_levels()
        sweep = []
        for rep in range(2):  # twice through the values, so that a drift of the session shows
            for tail in TAILS:
                assert set_tuning(r.ctx, f"bloom_tail={tail}".encode()) == 0
                ms, launches = stage()
                sweep.append(dict(tail=tail, rep=rep, tonemap_ms=ms, launches=launches))
        out["sweep"] = sweep
    r.timing_enable(False)
    out["hbm_gb_s"] = r.hbm_copy_rate(1 << 30, 5)
    r.close()
    print("LEG " + json.dumps(out))


def inject_leg(frames):
    """bloom over an injected 3840 x 2160 target, nothing else in the frame: the leg to put under a kernel trace
    (rocprofv3 --kernel-trace --stats -- python tools/bloom_cost.py --leg inject), which names each kernel's share"""
    import numpy as np
    from rend3_amd import _ffi
    import rend3_amd as r3
    r = r3.Renderer(r3.host.RIGHT, np.float32(W) / np.float32(H))
    r.set_tonemapping("aces", exposure_ev=-1.0)
    r.set_bloom(max_levels=MAX_LEVELS)
    rng = np.random.default_rng(1)
    hdr = np.empty((W * H, 4), dtype=np.uint16)
    hdr[:, :3] = np.exp2(rng.uniform(-6, 6, (W * H, 3))).astype(np.float16).view(np.uint16)
    hdr[:, 3] = 0x3C00
    fu = r3.host.frame_uniforms(r.camera, (0, 0, 0, 0), (W, H))
    clear = np.zeros(4, dtype=np.float32)
    for _ in range(frames):
        r._check(r.lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), W, H, 1, _ffi.ptr(clear), 32, 32), "r3n_frame_begin")
        r._check(r.lib.r3n_hdr_write(r.ctx, _ffi.ptr(hdr), 0, W * H), "r3n_hdr_write")
        r._check(r.lib.r3n_tonemap(r.ctx, None, 0), "r3n_tonemap")
        r._check(r.lib.r3n_frame_end(r.ctx), "r3n_frame_end")
    r.sync()
    print("levels", r.bloom_levels())
    r.close()


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
    ap.add_argument("--leg", default=None, choices=("default", "manual", "bloom", "inject"))
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom.md"))
    args = ap.parse_args()
    if args.leg == "inject":
        return inject_leg(args.frames)
    if args.leg:
        return leg(args.leg, args.frames)
    if not os.path.exists(PARENT_SO):
        raise SystemExit("no parent library: python tools/tonemap_cost.py --build-parent HEAD~1 first")
    a = [run_leg("default", args.frames, lib=PARENT_SO) for _ in range(3)]
    b = [run_leg("default", args.frames) for _ in range(3)]
    c = run_leg("manual", args.frames)
    d = run_leg("bloom", args.frames)
    assert {l["tonemap_launches"] for l in b} == {l["tonemap_launches"] for l in a}, "bloom off must launch nothing new"

    def spread(legs, key):
        v = sorted(l[key] for l in legs)
        return f"{v[len(v) // 2]:.4f} ({v[0]:.4f} - {v[-1]:.4f})"

    a_lo, a_hi = min(l["frame_ms"] for l in a), max(l["frame_ms"] for l in a)
    b_mid = sorted(l["frame_ms"] for l in b)[1]
    cost = d["tonemap_ms"] - c["tonemap_ms"]
    moved = chain_bytes(d["levels"])
    hbm = d["hbm_gb_s"]
    ideal = moved / (hbm * 1e9) * 1e3
    rows = [("a  parent commit, nothing set (3 runs)", spread(a, "frame_ms"), spread(a, "tonemap_ms"), a[0]["tonemap_launches"]),
            ("b  this commit, nothing set (3 runs)", spread(b, "frame_ms"), spread(b, "tonemap_ms"), b[0]["tonemap_launches"]),
            ("c  MANUAL + ACES", f"{c['frame_ms']:.4f}", f"{c['tonemap_ms']:.4f}", c["tonemap_launches"]),
            ("d  MANUAL + ACES + bloom", f"{d['frame_ms']:.4f}", f"{d['tonemap_ms']:.4f}", d["tonemap_launches"])]
    text = ["# Bloom: cost at 3840 x 2160", "",
            "`python tools/bloom_cost.py` on one MI355X, one session; the workload and camera path are bench.py's.  Frame: wall time per frame over "
            f"{args.frames} pipelined frames.  TONEMAP: the stage's time per frame with the taps on and the streams serialised (so the frame column and "
            "the stage column are different runs of the same process).  Median (min - max) where a leg ran more than once.", "",
            "| leg | frame ms | TONEMAP stage ms | TONEMAP launches per frame |", "|---|---|---|---|"]
    text += [f"| {n} | {f} | {t} | {l:g} |" for n, f, t, l in rows]
    text += ["", f"Bloom off launches nothing new: {b[0]['tonemap_launches']:g} TONEMAP launches per frame in b, {a[0]['tonemap_launches']:g} in a (asserted).  "
             f"b within the spread of a: median of b {b_mid:.4f} ms against a's {a_lo:.4f} - {a_hi:.4f} ms: "
             f"**{'yes' if a_lo <= b_mid <= a_hi else ('below it (faster)' if b_mid < a_lo else 'NO: slower')}**.", "",
             f"## Cost of bloom (stage of d minus stage of c; {d['levels']} levels, bloom_tail at its default)", "",
             f"{cost:.4f} ms in {d['tonemap_launches'] - c['tonemap_launches']:g} launches more.  The chain must move {moved / 1e6:.1f} MB (the HDR target read once, "
             "every level written once and read once going down, every level read and written going up, a_0 read by the composite); at the session's "
             f"r3n_hbm_copy_rate of {hbm:.0f} GB/s that is {ideal:.4f} ms: the chain takes **{cost / ideal:.2f} x** the time of moving its bytes.", "",
             "## bloom_tail sweep (same process as d, several times through the values; TONEMAP stage with the operator included, and the whole pipelined frame)", "",
             "| bloom_tail (texels) | launches per frame | stage ms, first pass | stage ms, second pass | pipelined frame ms, three passes |", "|---|---|---|---|---|"]
    for tail in TAILS:
        p = [s for s in d["sweep"] if s["tail"] == tail]
        f = " / ".join(f"{s['frame_ms']:.4f}" for s in d["pipelined"] if s["tail"] == tail)
        text.append(f"| {tail} | {p[0]['launches']:g} | {p[0]['tonemap_ms']:.4f} | {p[1]['tonemap_ms']:.4f} | {f} |")
    text += ["", "Stage: spans of the serialised launches, each net of the tap's own overhead, so a launch's dispatch gap is not in it.  Pipelined frame: wall time "
             "per frame with frames in flight and no taps, where the gaps count."]
    text.append("")
    open(args.out, "w").write("\n".join(text))
    print("\n".join(text))
    print(json.dumps(dict(a=a, b=b, c=c, d=d)))


if __name__ == "__main__":
    main()
