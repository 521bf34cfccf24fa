#!/usr/bin/env python3
"""GPU box: what reading lights out of an environment costs (r3n_environment_lights) -- level 0 of an N = 1024 f32 cube built from a
4096 x 2048 RGBE8 panorama with a sun in it -- every figure from one session.

Legs (each a process of its own):
  device  one context; per plan (R3N_TUNE envlight_plane = 1, 0) and max_lights (1, 4, 16), 5 calls after one uncounted: the host
          time of the call, its launches and, between device events (r3n_timing_enable), the e_max pass, the quantise pass and all
          light passes together; min_share = 0 so that every light asked for is extracted
  host    the alternative: the level read back face by face (r3n_readback_cube_face) and the numpy reference
          (tests/envlight_reference.py) at max_lights = 4, once
  bench   `python bench.py` on this tree and on a checkout of the parent commit (variants/parent_tree, built beforehand with
          tools/equirect_cost.py --make-parent-tree), alternating

  python tools/envlight_cost.py [--out profiles/envlight.md] [--no-bench]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PARENT_TREE = os.path.join(ROOT, "variants", "parent_tree")
W, H, N = 4096, 2048, 1024
REPS = 5
LIGHTS = (1, 4, 16)
CONE_DEGREES = 6.0
BENCH = ["--gpus", "1", "--steps", "60", "--warmup", "8", "--no-cpu-baseline", "--no-op-tally"]


def panorama(w=W, h=H):
    """RGBE8 noise of a few exponents with a bright disc (a sun) and a dimmer one"""
    import numpy as np
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(124, 130, (h, w))
    y, x = np.mgrid[0:h, 0:w]
    for cx, cy, radius, e in ((0.3, 0.22, 0.012, 142), (0.7, 0.35, 0.016, 136)):
        img[(x / w - cx) ** 2 * 4 + (y / h - cy) ** 2 < radius ** 2] = (255, 240, 220, e)
    return img


def renderer_with_cube(w, h, n):
    import numpy as np
    import rend3_amd as r3
    r = r3.Renderer(r3.host.RIGHT, np.float32(1.0))
    cube = r.add_texture_cube_equirect(panorama(w, h), w, h, face_extent=n, mips=1)
    r._flush_cubes()
    return r, cube


def device_leg(w, h, n):
    import ctypes
    import numpy as np
    from rend3_amd import _ffi
    r, cube = renderer_with_cube(w, h, n)
    lib = r.lib
    lib.r3n_internal_set_tuning.argtypes, lib.r3n_internal_set_tuning.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    lib.r3n_internal_envlight_times.argtypes, lib.r3n_internal_envlight_times.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    lib.r3n_internal_envlight_launches.argtypes, lib.r3n_internal_envlight_launches.restype = [ctypes.c_void_p], ctypes.c_uint64
    r.timing_enable(True)
    cone_cos = float(np.float32(math.cos(math.radians(CONE_DEGREES))))
    runs, words = [], {}
    for plane in (1, 0):
        assert lib.r3n_internal_set_tuning(r.ctx, f"envlight_plane={plane}".encode()) == 0
        for lights in LIGHTS:
            params = _ffi.EnvLightsParams(cube, 0, lights, cone_cos, 0.0)
            for rep in range(-1, REPS):
                out = _ffi.EnvLightsResult()
                r.sync()
                t0 = time.perf_counter()
                code = lib.r3n_environment_lights(r.ctx, ctypes.addressof(params), ctypes.addressof(out))
                host_ms = 1e3 * (time.perf_counter() - t0)
                assert code == 0, lib.r3n_last_error(r.ctx)
                ms = np.zeros(3, dtype=np.float32)
                assert lib.r3n_internal_envlight_times(r.ctx, _ffi.ptr(ms)) == 0
                if rep >= 0:
                    runs.append(dict(plane=plane, lights=lights, found=int(out.n_lights), host_ms=host_ms, emax_ms=float(ms[0]), quantise_ms=float(ms[1]),
                                     lights_ms=float(ms[2]), launches=int(lib.r3n_internal_envlight_launches(r.ctx))))
            words.setdefault(lights, set()).add(bytes(out))
    assert all(len(v) == 1 for v in words.values()), "both plans give the same words"
    hbm = r.hbm_copy_rate(1 << 30, 5)
    r.close()
    print("LEG " + json.dumps(dict(leg="device", runs=runs, hbm_gb_s=hbm, w=w, h=h, n=n)))


def host_leg(w, h, n):
    import numpy as np
    import envlight_reference as E
    r, cube = renderer_with_cube(w, h, n)
    r.sync()
    t0 = time.perf_counter()
    rgb = np.stack([r.readback_cube_face(cube, 0, f)[1:-1, 1:-1, :3] for f in range(6)])
    readback_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    st = E.extract(rgb, 4, np.float32(math.cos(math.radians(CONE_DEGREES))), 0.0)
    extract_ms = 1e3 * (time.perf_counter() - t0)
    got = r.environment_lights(cube, max_lights=4, cone_degrees=CONE_DEGREES, min_share=0.0, level=0, raw=True)
    same = bytes(got) == bytes(E.result_struct(st))
    r.close()
    print("LEG " + json.dumps(dict(leg="host", readback_ms=readback_ms, extract_ms=extract_ms, found=st["n_lights"], same_words=same)))


def run_leg(name, w, h, n):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--size", f"{w}x{h}x{n}"], capture_output=True, text=True, timeout=900)
    lines = [l for l in res.stdout.splitlines() if l.startswith("LEG ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"leg {name} failed ({res.returncode}):\n" + res.stdout[-2000:] + res.stderr[-4000:])
    print(lines[-1][:400], flush=True)
    return json.loads(lines[-1][4:])


def run_bench(tree):
    res = subprocess.run([sys.executable, "bench.py"] + BENCH, cwd=tree, capture_output=True, text=True, timeout=900)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{") and '"ms_per_step"' in l]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py in {tree} failed ({res.returncode}):\n" + res.stdout[-2000:] + res.stderr[-4000:])
    out = json.loads(lines[-1])
    print(f"bench {os.path.relpath(tree, ROOT)}: {out['ms_per_step']} ms per step", flush=True)
    return out["ms_per_step"]


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("device", "host"))
    ap.add_argument("--size", default=f"{W}x{H}x{N}", help="WxHxN of the panorama and the cube")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envlight.md"))
    args = ap.parse_args()
    w, h, n = (int(v) for v in args.size.split("x"))
    if args.leg:
        return (device_leg if args.leg == "device" else host_leg)(w, h, n)
    dev = run_leg("device", w, h, n)
    host = run_leg("host", w, h, n)
    parent, this = [], []
    if not args.no_bench:
        if not os.path.exists(os.path.join(PARENT_TREE, "bench.py")):
            raise SystemExit("no parent tree: python tools/equirect_cost.py --make-parent-tree HEAD~1 first")
        for rep in range(3):
            parent.append(run_bench(PARENT_TREE))
            this.append(run_bench(ROOT))
    texels = 6 * n * n
    hbm = dev["hbm_gb_s"]
    bytes_of = dict(emax=16 * texels, quantise1=(16 + 20) * texels, quantise0=16 * texels, shift1=16 * texels, light1=20 * texels, shift0=16 * texels, light0=16 * texels)

    def ideal(b):
        return b / (hbm * 1e9) * 1e3

    def col(runs, key):
        v = [x[key] for x in runs]
        return f"{med(v):.3f} ({min(v):.3f} - {max(v):.3f})"

    text = [f"# Environment lights: cost on level 0 of an N = {n} f32 cube ({w} x {h} RGBE8 panorama)", "",
            f"`python tools/envlight_cost.py` on one MI355X, one session.  Every row is the median (min - max) of {REPS} calls in one context; one more "
            "call ran first, uncounted.  Host: wall time of r3n_environment_lights, which ends in a synchronise.  The other columns: between "
            f"device events on the call's stream (r3n_timing_enable).  Cone {CONE_DEGREES} degrees, min_share 0, so every light asked for is "
            "extracted.  Per light pass = the light column / (3 x lights): two mean-shift gathers and the final gather with the next seed search.", "",
            "| envlight_plane | max_lights | found | launches | host ms | e_max ms | quantise ms | all light passes ms | per light pass ms |", "|---|---|---|---|---|---|---|---|---|"]
    per_pass = {}
    for plane in (1, 0):
        for lights in LIGHTS:
            runs = [x for x in dev["runs"] if x["plane"] == plane and x["lights"] == lights]
            per_pass[(plane, lights)] = med([x["lights_ms"] for x in runs]) / (3 * lights)
            text.append(f"| {plane} | {lights} | {runs[0]['found']} | {runs[0]['launches']} | " + " | ".join(col(runs, k) for k in ("host_ms", "emax_ms", "quantise_ms", "lights_ms")) +
                        f" | {per_pass[(plane, lights)]:.3f} |")
    text += ["", f"Algorithmic bytes per pass over {texels} texels, and their time at the session's r3n_hbm_copy_rate of {hbm:.0f} GB/s (a copy moves "
             "each byte twice, so the rate counts read + written bytes):", "",
             "| pass | plan 1 bytes | ms | plan 0 bytes | ms |", "|---|---|---|---|---|",
             f"| e_max (reads the f32 texels) | {bytes_of['emax'] / 1e6:.1f} MB | {ideal(bytes_of['emax']):.3f} | {bytes_of['emax'] / 1e6:.1f} MB | {ideal(bytes_of['emax']):.3f} |",
             f"| quantise (reads the texels; plan 1 writes the 20-byte plane) | {bytes_of['quantise1'] / 1e6:.1f} MB | {ideal(bytes_of['quantise1']):.3f} | "
             f"{bytes_of['quantise0'] / 1e6:.1f} MB | {ideal(bytes_of['quantise0']):.3f} |",
             f"| mean-shift gather, at most (only texels inside the cone are read) | {bytes_of['shift1'] / 1e6:.1f} MB | {ideal(bytes_of['shift1']):.3f} | "
             f"{bytes_of['shift0'] / 1e6:.1f} MB | {ideal(bytes_of['shift0']):.3f} |",
             f"| final gather + next seed (every live texel) | {bytes_of['light1'] / 1e6:.1f} MB | {ideal(bytes_of['light1']):.3f} | {bytes_of['light0'] / 1e6:.1f} MB | "
             f"{ideal(bytes_of['light0']):.3f} |", "",
             f"Measured per light pass at 16 lights: {per_pass[(1, 16)]:.3f} ms (plane) and {per_pass[(0, 16)]:.3f} ms (texels decoded again).", "",
             "## The default plan", "",
             "Host time of the call, plane against no plane: " +
             ", ".join(f"{med([x['host_ms'] for x in dev['runs'] if x['plane'] == 1 and x['lights'] == k]):.3f} / "
                       f"{med([x['host_ms'] for x in dev['runs'] if x['plane'] == 0 and x['lights'] == k]):.3f} ms at {k}" for k in LIGHTS) +
             f" lights.  The plane costs {20 * texels / 1e6:.0f} MB of scratch; the default (R3N_ENVLIGHT_PLANE_DEFAULT in csrc/envlight.h) keeps none "
             "unless the plane is faster by more than the spread of these rows.", "",
             "## The host alternative", "",
             f"Reading the level back face by face: {host['readback_ms']:.0f} ms; the numpy reference at max_lights = 4 on it: {host['extract_ms']:.0f} ms "
             f"({host['found']} lights; the same words as the device: {host['same_words']}).  The device path at max_lights = 4: "
             f"{med([x['host_ms'] for x in dev['runs'] if x['plane'] == 1 and x['lights'] == 4]):.3f} ms."]
    if parent:
        text += ["", "## The default frame", "",
                 "No frame kernel, ShadeArgs field or default launch changes; `python bench.py " + " ".join(BENCH) + "` on this tree and on a checkout of the "
                 "parent commit, alternating, ms per step:", "",
                 f"parent: {', '.join(f'{v:.3f}' for v in parent)} (spread {max(parent) - min(parent):.3f}); this tree: {', '.join(f'{v:.3f}' for v in this)}.  "
                 f"Median difference {med(this) - med(parent):+.3f} ms: " +
                 ("inside" if min(parent) - (max(parent) - min(parent)) <= med(this) <= max(parent) + (max(parent) - min(parent)) else "OUTSIDE") +
                 " the parent's own run-to-run spread around its range."]
    out = "\n".join(text) + "\n"
    open(args.out, "w").write(out)
    print(out)
    print(json.dumps(dict(device=dev, host=host, bench_parent=parent, bench_this=this))[:200])


if __name__ == "__main__":
    main()
