#!/usr/bin/env python3
"""GPU box: what prefiltering an environment costs (r3n_environment_prefilter) -- a 4096 x 2048 RGBE8 panorama becomes a 1024^2 f32
cube with its full chain; the prefilter starts from the level of extent 256 and takes all nine levels from there -- every figure
from one session.

Legs (each a process of its own):
  device  one context; per launch plan (R3N_TUNE ibl_tile x ibl_block; tile 0 = the records through wave-uniform loads instead of
          LDS), REPS calls after one uncounted: the host time of the call, its launches and, between device events
          (r3n_timing_enable), records + mirror, the pair kernel, the SH passes and k_cube_assemble; the pair kernel against its
          pair count x FLOPS_PER_PAIR at the f32 vector rate; every plan must give the same words
  host    the alternative: the levels read back face by face (r3n_readback_cube_face) and tests/ibl_reference.py; the numpy
          restatement is run on the chain from extent HOST_EXTENT down and scaled to the whole call by the pair count
  sky     the `skybox` stage over an empty world at 1920 x 1080, one and four samples: the prefiltered cube at a fixed level
          against the same cube with the level selected per pixel
  bench   `python bench.py` on this tree and on a checkout of the parent commit (variants/parent_tree, built beforehand with
          tools/equirect_cost.py --make-parent-tree), alternating

  python tools/ibl_cost.py [--out profiles/ibl.md] [--no-bench]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARENT_TREE = os.path.join(ROOT, "variants", "parent_tree")
W, H, N, BASE_EXTENT = 4096, 2048, 1024, 256
REPS = 3
PLANS = ((256, 256), (256, 128), (256, 64), (64, 256), (512, 256), (0, 256), (0, 64))
HOST_EXTENT = 32
# per pair, as ibl_rule::weight and the four accumulations write it: q 8, the test 1, cs 2, d 3, cs w 1, d d 1, the division 1, the
# products and sums 7
FLOPS_PER_PAIR = 24
# MI355X: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz one-flop vector operations per second (the unit is built without contraction, so an
# operation is one flop; the 157.3 TFLOPS of the data sheet count a fused multiply-add as two)
VECTOR_OPS_PER_S = 256 * 4 * 32 * 2.4e9
BENCH = ["--gpus", "1", "--steps", "60", "--warmup", "8", "--no-cpu-baseline", "--no-op-tally"]
FRAME_W, FRAME_H = 1920, 1080


def renderer_with_cube():
    import numpy as np
    import rend3_amd as r3
    from envlight_cost import panorama
    r = r3.Renderer(r3.host.RIGHT, np.float32(FRAME_W / FRAME_H))
    cube = r.add_texture_cube_equirect(panorama(W, H), W, H, face_extent=N, mips="maximum")
    r._flush_cubes()
    return r, cube


def pairs_of(extent, levels):
    return sum((6 * max(1, extent >> k) ** 2) ** 2 for k in range(1, levels))


def device_leg():
    import ctypes
    import numpy as np
    from rend3_amd import _ffi
    r, cube = renderer_with_cube()
    lib = r.lib
    lib.r3n_internal_set_tuning.argtypes, lib.r3n_internal_set_tuning.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
    lib.r3n_internal_ibl_times.argtypes, lib.r3n_internal_ibl_times.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    lib.r3n_internal_ibl_launches.argtypes, lib.r3n_internal_ibl_launches.restype = [ctypes.c_void_p], ctypes.c_uint64
    r.timing_enable(True)
    level = next(k for k in range(N.bit_length()) if N >> k <= BASE_EXTENT)
    levels = BASE_EXTENT.bit_length()
    runs, words = [], set()
    for tile, block in PLANS:
        assert lib.r3n_internal_set_tuning(r.ctx, f"ibl_tile={tile} ibl_block={block}".encode()) == 0
        params = _ffi.EnvPrefilterParams(cube, level, levels)
        for rep in range(-1, REPS):
            out = _ffi.EnvPrefilterResult()
            r.sync()
            t0 = time.perf_counter()
            code = lib.r3n_environment_prefilter(r.ctx, ctypes.addressof(params), ctypes.addressof(out))
            host_ms = 1e3 * (time.perf_counter() - t0)
            assert code == 0, lib.r3n_last_error(r.ctx)
            ms = np.zeros(4, dtype=np.float32)
            assert lib.r3n_internal_ibl_times(r.ctx, _ffi.ptr(ms)) == 0
            if rep >= 0:
                runs.append(dict(tile=tile, block=block, host_ms=host_ms, records_ms=float(ms[0]), pairs_ms=float(ms[1]), sh_ms=float(ms[2]),
                                 assemble_ms=float(ms[3]), launches=int(lib.r3n_internal_ibl_launches(r.ctx))))
        handle = int(out.cube_id)
        faces = b"".join(r_face(r, handle, k, f) for k in (1, 4, levels - 1) for f in (0, 5))
        words.add(bytes(out)[4:] + faces)  # (without cube_id: every call appends a cube)
    assert len(words) == 1, "every plan gives the same words"
    r.close()
    print("LEG " + json.dumps(dict(leg="device", runs=runs, level=level, levels=levels, pairs=pairs_of(BASE_EXTENT, levels))))


def r_face(r, cube, level, face):
    import numpy as np
    from rend3_amd import _ffi
    p = max(1, BASE_EXTENT >> level) + 2
    words = np.zeros(p * p * 4, dtype=np.uint32)
    assert r.lib.r3n_readback_cube_face(r.ctx, cube, level, face, _ffi.ptr(words), words.size, None) == 0
    return words.tobytes()


def host_leg():
    import numpy as np
    import ibl_reference as I
    r, cube = renderer_with_cube()
    level = next(k for k in range(N.bit_length()) if N >> k <= BASE_EXTENT)
    levels = BASE_EXTENT.bit_length()
    r.sync()
    t0 = time.perf_counter()
    src = [np.stack([r.readback_cube_face(cube, level + k, f)[1:-1, 1:-1, :3] for f in range(6)]) for k in range(levels)]
    readback_ms = 1e3 * (time.perf_counter() - t0)
    first = next(k for k in range(levels) if BASE_EXTENT >> k <= HOST_EXTENT)
    t0 = time.perf_counter()
    want = [I.prefilter_level(src[k], k, levels) for k in range(first, levels)]
    part_ms = 1e3 * (time.perf_counter() - t0)
    part_pairs = sum((6 * max(1, BASE_EXTENT >> k) ** 2) ** 2 for k in range(first, levels))
    handle, sh = r.prefilter_environment(cube, level=level, levels=levels)
    same = all(np.array_equal(np.stack([r.readback_cube_face(handle, k, f)[1:-1, 1:-1] for f in range(6)]).view(np.uint32), want[k - first].view(np.uint32))
               for k in range(first, levels))
    same = same and np.array_equal(sh.view(np.uint32), I.sh9(src[I.sh_level(BASE_EXTENT, levels)]).view(np.uint32))
    r.close()
    print("LEG " + json.dumps(dict(leg="host", readback_ms=readback_ms, part_ms=part_ms, part_pairs=part_pairs, from_extent=BASE_EXTENT >> first,
                                   pairs=pairs_of(BASE_EXTENT, levels), same_words=bool(same))))


def sky_leg(frames=40, warmup=8):
    import numpy as np
    import rend3_amd as r3
    r, cube = renderer_with_cube()
    level = next(k for k in range(N.bit_length()) if N >> k <= BASE_EXTENT)
    handle, _ = r.prefilter_environment(cube, level=level)
    r.set_background_texture(handle)
    r.set_camera_data(r3.host.look_at_rh((0, 0, 0), (1.0, 0.4, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    r.set_multi_stream(False)
    r.timing_enable(True)
    out = {}
    for name, lod in (("automatic", None), ("level 0", 0.0), ("level 3", 3.0), ("level 3.5", 3.5)):
        r.set_skybox_level(lod)
        for samples in (1, 4):
            per_frame = []
            for k in range(warmup + frames):
                r.render(FRAME_W, FRAME_H, samples=samples, clear_color=(0, 0, 0, 1), readback=False)
                r.sync()
                st = r.stage_times(reset=True)
                if k >= warmup:
                    per_frame.append(st["skybox"][0])
            out[f"{name}|{samples}"] = [float(np.median(per_frame)) * 1e3, float(np.min(per_frame)) * 1e3, float(np.max(per_frame)) * 1e3]
    r.close()
    print("LEG " + json.dumps(dict(leg="sky", stages=out, frames=frames)))


def run_leg(name):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--leg", default=None, choices=("device", "host", "sky"))
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibl.md"))
    args = ap.parse_args()
    if args.leg:
        return dict(device=device_leg, host=host_leg, sky=sky_leg)[args.leg]()
    dev = run_leg("device")
    host = run_leg("host")
    sky = run_leg("sky")
    parent, this = [], []
    if not args.no_bench:
        if not os.path.exists(os.path.join(PARENT_TREE, "bench.py")):
            raise SystemExit("no parent tree: python tools/equirect_cost.py --make-parent-tree HEAD~1 first")
        for rep in range(3):
            parent.append(run_bench(PARENT_TREE))
            this.append(run_bench(ROOT))

    def col(runs, key):
        v = [x[key] for x in runs]
        return f"{med(v):.3f} ({min(v):.3f} - {max(v):.3f})"

    pairs = dev["pairs"]
    ideal_ms = pairs * FLOPS_PER_PAIR / VECTOR_OPS_PER_S * 1e3
    text = [f"# Environment prefilter: cost from the level of extent {BASE_EXTENT} of an N = {N} f32 cube ({W} x {H} RGBE8 panorama), {dev['levels']} levels", "",
            f"`python tools/ibl_cost.py` on one MI355X, one session.  Every row is the median (min - max) of {REPS} calls in one context; one more "
            "call per plan ran first, uncounted.  Host: wall time of r3n_environment_prefilter, which allocates and frees its scratch block and ends "
            "in a synchronise.  The other columns: between device events on the call's stream (r3n_timing_enable).  ibl_tile 0: the pair kernel "
            "reads the records through wave-uniform loads instead of an LDS tile.  Every plan gave the same words (checked on the result struct and "
            "six faces).", "",
            "| ibl_tile | ibl_block | launches | host ms | records + mirror ms | pair kernel ms | SH ms | k_cube_assemble ms |", "|---|---|---|---|---|---|---|---|"]
    by_plan = {}
    for tile, block in PLANS:
        runs = [x for x in dev["runs"] if x["tile"] == tile and x["block"] == block]
        by_plan[(tile, block)] = med([x["pairs_ms"] for x in runs])
        text.append(f"| {tile} | {block} | {runs[0]['launches']} | " + " | ".join(col(runs, k) for k in ("host_ms", "records_ms", "pairs_ms", "sh_ms", "assemble_ms")) + " |")
    best_lds = min(v for (tile, _), v in by_plan.items() if tile)
    best_uniform = min(v for (tile, _), v in by_plan.items() if not tile)
    text += ["", "## The pair kernel against its arithmetic", "",
             f"Pairs of the call (every output texel of levels 1 .. {dev['levels'] - 1} with every texel of its source level): {pairs:.4g}.  "
             f"{FLOPS_PER_PAIR} f32 operations per pair as the rule writes them (no contraction: an operation is one flop), one of them an IEEE division.  "
             f"At the vector rate of {VECTOR_OPS_PER_S / 1e12:.1f} T one-flop operations per second (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz) that is "
             f"{ideal_ms:.2f} ms; measured {by_plan[PLANS[0]]:.2f} ms under the default plan: {by_plan[PLANS[0]] / ideal_ms:.2f} x the count.  The correctly "
             "rounded division is a sequence of about ten instructions, which the count books as one.", "",
             "## LDS tile against wave-uniform loads", "",
             f"Best LDS plan {best_lds:.2f} ms, best plan without LDS {best_uniform:.2f} ms.  The default (R3N_IBL_TILE_DEFAULT / R3N_IBL_BLOCK_DEFAULT in "
             "csrc/ibl.h) is the faster of the two families unless they differ by less than the spread of the rows above.", "",
             "## The host alternative", "",
             f"Reading the {dev['levels']} levels back face by face: {host['readback_ms']:.0f} ms.  tests/ibl_reference.py (numpy float32, the same tree) on the levels "
             f"from extent {host['from_extent']} down: {host['part_ms']:.0f} ms for {host['part_pairs']:.3g} pairs (the same words as the device: {host['same_words']}); "
             f"scaled by the pair count to the whole call: {host['part_ms'] * host['pairs'] / host['part_pairs'] / 1e3:.0f} s.  The device call: "
             f"{med([x['host_ms'] for x in dev['runs'] if (x['tile'], x['block']) == PLANS[0]]):.2f} ms.", "",
             "## The skybox stage at a fixed level", "",
             f"`skybox` stage over an empty world at {FRAME_W} x {FRAME_H} (every pixel takes the sky), the prefiltered cube bound, median (min - max) of "
             f"{sky['frames']} frames in us:", "", "| level | 1 sample | 4 samples |", "|---|---|---|"]
    for name in ("automatic", "level 0", "level 3", "level 3.5"):
        a, b = sky["stages"][f"{name}|1"], sky["stages"][f"{name}|4"]
        text.append(f"| {name} | {a[0]:.1f} ({a[1]:.1f} - {a[2]:.1f}) | {b[0]:.1f} ({b[1]:.1f} - {b[2]:.1f}) |")
    inside = True
    if parent:
        inside = min(parent) - (max(parent) - min(parent)) <= med(this) <= max(parent) + (max(parent) - min(parent))
        text += ["", "## The default frame", "",
                 "No frame kernel changes its instructions and no default launch changes; `python bench.py " + " ".join(BENCH) + "` on this tree and on a checkout of "
                 "the parent commit (variants/parent_tree, which `python tools/equirect_cost.py --make-parent-tree HEAD~1` builds beforehand), alternating, "
                 "ms per step:", "",
                 f"parent: {', '.join(f'{v:.3f}' for v in parent)} (spread {max(parent) - min(parent):.3f}); this tree: {', '.join(f'{v:.3f}' for v in this)}.  "
                 f"Median difference {med(this) - med(parent):+.3f} ms: " + ("inside" if inside else "OUTSIDE") +
                 " the parent's own run-to-run spread around its range.  The default frame must lie inside it: the tool fails otherwise."]
    out = "\n".join(text) + "\n"
    open(args.out, "w").write(out)
    print(out)
    print(json.dumps(dict(device=dev, host=host, sky=sky, bench_parent=parent, bench_this=this))[:200])
    if not inside:
        raise SystemExit("the default frame lies OUTSIDE the parent's run-to-run spread")


if __name__ == "__main__":
    main()
