#!/usr/bin/env python3
"""GPU box: what building a cube from an equirectangular panorama on the device costs (r3n_texture_cubes_write_sources) -- a
4096 x 2048 RGBE8 panorama, N = 1024, a full chain -- every figure from one session.

Legs (each a process of its own):
  device  5 fresh contexts per tail threshold (the default and 0, alternating; one more context first, uncounted, loads the code):
          the host time of the call and, between device events (r3n_timing_enable), its copies, k_equirect_faces, the chain kernels
          and k_cube_assemble
  host    the alternative: the numpy reference conversion (tests/equirect_reference.py) once, then the result uploaded as Rgba32Float
          through r3n_texture_cubes_write_encoded in 5 fresh contexts
  bench   `python bench.py` on this tree and on a checkout of the parent commit (--parent-tree, built beforehand), alternating

  python tools/equirect_cost.py --make-parent-tree HEAD~1     # git archive + build into variants/parent_tree (needs no GPU)
  python tools/equirect_cost.py [--out profiles/equirect.md]"""
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
PARENT_TREE = os.path.join(ROOT, "variants", "parent_tree")
W, H, N = 4096, 2048, 1024
REPS = 5
BENCH = ["--gpus", "1", "--steps", "60", "--warmup", "8", "--no-cpu-baseline", "--no-op-tally"]


def panorama(w=W, h=H):
    import numpy as np
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(120, 136, (h, w))
    return img


def moved_bytes(w=W, h=H, n=N):
    """what the call must move: the source read once, every dense level written once and read once, the bordered pool written once"""
    mips = n.bit_length()
    dense = sum(6 * max(1, n >> k) ** 2 * 16 for k in range(mips))
    pool = sum(6 * (max(1, n >> k) + 2) ** 2 * 16 for k in range(mips))
    return dict(source=w * h * 4, dense=dense, pool=pool, total=w * h * 4 + 2 * dense + pool)


def make_parent_tree(rev):
    import io
    import shutil
    import tarfile
    if os.path.isdir(PARENT_TREE):
        shutil.rmtree(PARENT_TREE)
    os.makedirs(PARENT_TREE)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev], capture_output=True, check=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(PARENT_TREE)
    subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=PARENT_TREE, check=True)
    print(PARENT_TREE)


def device_leg(w, h, n):
    import ctypes
    import numpy as np
    import equirect_reference as Q
    import rend3_amd as r3
    from rend3_amd import _ffi
    img = panorama(w, h)
    mips = n.bit_length()
    src = (_ffi.CubeSource * 1)(_ffi.CubeSource(_ffi.CUBE_SOURCE_EQUIRECT, _ffi.CUBE_ENCODING_RGBE8, w, h, n, mips, 0))
    runs = []
    hbm = None
    for rep in range(-1, REPS):
        for tail in (Q.TAIL_DEFAULT, 0):
            r = r3.Renderer(r3.host.RIGHT, np.float32(1.0))
            set_tuning = r.lib.r3n_internal_set_tuning
            set_tuning.argtypes, set_tuning.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_int
            assert set_tuning(r.ctx, f"equirect_tail={tail}".encode()) == 0
            r.timing_enable(True)
            r.sync()
            t0 = time.perf_counter()
            code = r.lib.r3n_texture_cubes_write_sources(r.ctx, ctypes.addressof(src), 1, _ffi.ptr(img), img.size)
            host_ms = 1e3 * (time.perf_counter() - t0)
            assert code == 0, r.lib.r3n_last_error(r.ctx)
            ms = np.zeros(4, dtype=np.float32)
            fn = r.lib.r3n_internal_cube_source_times
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
            assert fn(r.ctx, _ffi.ptr(ms)) == 0
            launches = r.lib.r3n_internal_cube_source_launches
            launches.argtypes, launches.restype = [ctypes.c_void_p], ctypes.c_uint64
            if rep >= 0:
                runs.append(dict(tail=tail, rep=rep, host_ms=host_ms, copy_ms=float(ms[0]), faces_ms=float(ms[1]), chain_ms=float(ms[2]),
                                 assemble_ms=float(ms[3]), launches=int(launches(r.ctx))))
            if hbm is None:
                hbm = r.hbm_copy_rate(1 << 30, 5)
            r.close()
    print("LEG " + json.dumps(dict(leg="device", runs=runs, hbm_gb_s=hbm, w=w, h=h, n=n)))


def host_leg(w, h, n):
    import numpy as np
    import equirect_reference as Q
    import rend3_amd as r3
    from rend3_amd import _ffi, containers
    img = panorama(w, h)
    t0 = time.perf_counter()
    levels = Q.cube(Q.rgbe_decode(img), n)
    convert_ms = 1e3 * (time.perf_counter() - t0)
    payload = np.frombuffer(b"".join(np.ascontiguousarray(lvl[f]).tobytes() for f in range(6) for lvl in levels), dtype=np.uint8)
    desc = np.array([[0, n, n, len(levels), containers.RGBA32F, 0, 0, 0]], dtype=np.uint32)
    uploads = []
    for rep in range(-1, REPS):
        r = r3.Renderer(r3.host.RIGHT, np.float32(1.0))
        r.sync()
        t0 = time.perf_counter()
        code = r.lib.r3n_texture_cubes_write_encoded(r.ctx, _ffi.ptr(desc), 1, _ffi.ptr(payload), payload.size)
        ms = 1e3 * (time.perf_counter() - t0)
        assert code == 0, r.lib.r3n_last_error(r.ctx)
        if rep >= 0:
            uploads.append(ms)
        r.close()
    print("LEG " + json.dumps(dict(leg="host", convert_ms=convert_ms, upload_ms=uploads, payload_bytes=int(payload.size))))


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
    ap.add_argument("--make-parent-tree", default=None, metavar="REV")
    ap.add_argument("--leg", default=None, choices=("device", "host"))
    ap.add_argument("--size", default=f"{W}x{H}x{N}", help="WxHxN of the panorama and the cube")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equirect.md"))
    args = ap.parse_args()
    w, h, n = (int(v) for v in args.size.split("x"))
    if args.make_parent_tree:
        return make_parent_tree(args.make_parent_tree)
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
    import equirect_reference as Q
    moved = moved_bytes(w, h, n)
    hbm = dev["hbm_gb_s"]
    ideal = moved["total"] / (hbm * 1e9) * 1e3
    text = [f"# Cubes from panoramas: cost of a {w} x {h} RGBE8 panorama -> N = {n}, {n.bit_length()} levels", "",
            "`python tools/equirect_cost.py` on one MI355X, one session.  Every row is the median (min - max) of "
            f"{REPS} fresh contexts; one more context ran first, uncounted.  Host: wall time of r3n_texture_cubes_write_sources, which ends in a "
            "synchronise.  The other columns: between device events on the call's stream (r3n_timing_enable).", "",
            "| equirect_tail | launches | host ms | copies ms | k_equirect_faces ms | chain ms | k_cube_assemble ms |", "|---|---|---|---|---|---|---|"]

    def col(runs, key):
        v = [x[key] for x in runs]
        return f"{med(v):.3f} ({min(v):.3f} - {max(v):.3f})"

    by_tail = {}
    for tail in (Q.TAIL_DEFAULT, 0):
        runs = [x for x in dev["runs"] if x["tail"] == tail]
        by_tail[tail] = runs
        text.append(f"| {tail} | {runs[0]['launches']} | " + " | ".join(col(runs, k) for k in ("host_ms", "copy_ms", "faces_ms", "chain_ms", "assemble_ms")) + " |")
    d = by_tail[Q.TAIL_DEFAULT]
    kernels = med([x["faces_ms"] + x["chain_ms"] + x["assemble_ms"] for x in d])
    text += ["", f"The call must move {moved['total'] / 1e6:.1f} MB on the device: the source read once ({moved['source'] / 1e6:.1f} MB), every dense level written and "
             f"read once (2 x {moved['dense'] / 1e6:.1f} MB), the bordered pool written once ({moved['pool'] / 1e6:.1f} MB).  At the session's r3n_hbm_copy_rate of "
             f"{hbm:.0f} GB/s that is {ideal:.3f} ms; the three kernel phases take {kernels:.3f} ms: **{kernels / ideal:.2f} x** the time of moving the bytes.  "
             f"The host-to-device copy of the {moved['source'] / 1e6:.1f} MB payload (pageable memory) is in the copies column.", "",
             "## The tail in one launch against a launch per level", "",
             f"chain, equirect_tail = {Q.TAIL_DEFAULT}: {col(by_tail[Q.TAIL_DEFAULT], 'chain_ms')} ms; equirect_tail = 0: {col(by_tail[0], 'chain_ms')} ms.  "
             f"Host time of the call: {col(by_tail[Q.TAIL_DEFAULT], 'host_ms')} against {col(by_tail[0], 'host_ms')} ms.", "",
             "## The host alternative", "",
             f"The numpy reference conversion of the same panorama: {host['convert_ms']:.0f} ms (once).  Its result, {host['payload_bytes'] / 1e6:.1f} MB of Rgba32Float faces with "
             f"their chain, through r3n_texture_cubes_write_encoded: {med(host['upload_ms']):.3f} ({min(host['upload_ms']):.3f} - {max(host['upload_ms']):.3f}) ms per call "
             f"-- against {med([x['host_ms'] for x in d]):.3f} ms for the whole device path."]
    if parent:
        text += ["", "## bench.py, this commit against its parent", "",
                 f"`python bench.py {' '.join(BENCH)}`, alternating, ms per step: parent {' / '.join(f'{v:.4f}' for v in parent)} (spread "
                 f"{max(parent) - min(parent):.4f}); this commit {' / '.join(f'{v:.4f}' for v in this)}.  Medians {med(parent):.4f} and {med(this):.4f}: "
                 f"a difference of {med(this) - med(parent):+.4f} ms.  The default frame launches nothing new."]
    text.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write("\n".join(text))
    print("\n".join(text))
    print(json.dumps(dict(device=dev, host=host, bench_parent=parent, bench_this=this)))


if __name__ == "__main__":
    main()
