#!/usr/bin/env python3
"""GPU box: what ordering the transparent pass costs, on the device and on the host it replaces.

For n translucent objects (one triangle each: only the ordering is timed), n in 256 / 4 096 / 65 536 / 1 048 576:
  (a) the `blend_sort` stage of r3n_stage_times: HIP events around the launches of one r3n_blend_sort, the camera moving
      between calls, median over the repeats after warm-up calls;
  (b) the host path of blend_sort="host", wall clock: host.blend_draw_order (the Python mirror of the CPU batcher's sort) +
      r3n_blend_order_write (scan + two uploads); and (b') the same with the Python loop replaced by a vectorised numpy key + lexsort,
      which stands for a compiled host sort such as the reference's;
  (c) the wall clock of the r3n_blend_sort call itself (enqueue only, timing taps off, the queue drained between calls).
Also the one-off r3n_blend_objects_write.  Every figure is a median; the spread (min .. max) is printed beside it.

usage: python tools/blend_sort_cost.py [--repeats 30] [--warmup 5] [--out profiles/blend_sort.txt]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rend3_amd import _ffi, host

f32 = np.float32
SIZES = (256, 4096, 65536, 1048576)


def camera(k):
    return np.array([3.0 + 0.37 * k, -2.0 + 0.11 * k, 5.0 - 0.23 * k], dtype=f32)


def numpy_order(cam, slots, loc):
    """blend_draw_order's result by vectorised f32 arithmetic and one lexsort"""
    with np.errstate(over="ignore"):
        d = cam[None, :] - loc
        dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return slots[np.lexsort((slots, -dist))]


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return f"{np.median(xs):10.1f} us  ({xs.min():.1f} .. {xs.max():.1f})"


def measure(lib, n, repeats, warmup, lines):
    ctx = lib.r3n_create(0, None)
    if not ctx:
        raise RuntimeError("r3n_create failed")

    def ok(code, what):
        _ffi.check(ctx, code, what)
    rng = np.random.default_rng(n)
    slots = np.arange(n, dtype=np.uint32)
    rec = np.zeros((n, 32), dtype=np.uint32)
    rec.view(f32)[:, [0, 5, 10, 15]] = 1.0
    rec[:, 21], rec[:, 29] = 3, 1
    ok(lib.r3n_objects_write(ctx, _ffi.ptr(slots), _ffi.ptr(rec), n, max(n, 16)), "r3n_objects_write")
    loc = np.ascontiguousarray(rng.uniform(-200.0, 200.0, (n, 3)).astype(f32))
    t0 = time.perf_counter()
    ok(lib.r3n_blend_objects_write(ctx, _ffi.ptr(slots), _ffi.ptr(loc), n), "r3n_blend_objects_write")
    upload_us = 1e6 * (time.perf_counter() - t0)
    ok(lib.r3n_sync(ctx), "r3n_sync")
    ms, launches = np.zeros(len(_ffi.STAGE_TABLE)), np.zeros(len(_ffi.STAGE_TABLE), dtype=np.uint64)
    stage = _ffi.STAGES.index("blend_sort")
    # (c) the call on the host, taps off
    call_us = []
    for k in range(warmup + repeats):
        cam = camera(k)
        t0 = time.perf_counter()
        code = lib.r3n_blend_sort(ctx, _ffi.ptr(cam))
        t1 = time.perf_counter()
        ok(code, "r3n_blend_sort")
        ok(lib.r3n_sync(ctx), "r3n_sync")
        if k >= warmup:
            call_us.append(1e6 * (t1 - t0))
    # (a) the stage on the device
    ok(lib.r3n_timing_enable(ctx, 1), "r3n_timing_enable")
    stage_us = []
    for k in range(warmup + repeats):
        cam = camera(k)
        ok(lib.r3n_blend_sort(ctx, _ffi.ptr(cam)), "r3n_blend_sort")
        ok(lib.r3n_sync(ctx), "r3n_sync")
        ok(lib.r3n_stage_times(ctx, _ffi.ptr(ms), _ffi.ptr(launches), 1), "r3n_stage_times")
        if k >= warmup:
            stage_us.append(1e3 * ms[stage])
    ok(lib.r3n_timing_enable(ctx, 0), "r3n_timing_enable")
    # the device's answer is the host's (last camera)
    order, rank = np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    ok(lib.r3n_readback_blend_order(ctx, _ffi.ptr(order), _ffi.ptr(rank), n), "r3n_readback_blend_order")
    assert np.array_equal(order, numpy_order(camera(warmup + repeats - 1), slots, loc)) and np.array_equal(rank, np.arange(n + 1))
    # (b) the host path it replaces (this switches the context to host order mode); the Python loop is slow, so fewer repeats
    host_reps = max(1, min(repeats, 250_000 // n))
    host_warm = 1 if n <= 65536 else 0
    host_us, vec_us = [], []
    for k in range(host_warm + host_reps):
        cam = camera(k)
        t0 = time.perf_counter()
        arr = np.asarray(host.blend_draw_order(cam, slots, loc), dtype=np.uint32)
        ok(lib.r3n_blend_order_write(ctx, _ffi.ptr(arr), n), "r3n_blend_order_write")
        t1 = time.perf_counter()
        if k >= host_warm:
            host_us.append(1e6 * (t1 - t0))
    for k in range(warmup + repeats):
        cam = camera(k)
        t0 = time.perf_counter()
        arr = np.ascontiguousarray(numpy_order(cam, slots, loc))
        ok(lib.r3n_blend_order_write(ctx, _ffi.ptr(arr), n), "r3n_blend_order_write")
        t1 = time.perf_counter()
        if k >= warmup:
            vec_us.append(1e6 * (t1 - t0))
    assert n > 65536 or np.array_equal(arr, np.asarray(host.blend_draw_order(cam, slots, loc), dtype=np.uint32))
    ok(lib.r3n_sync(ctx), "r3n_sync")
    lib.r3n_destroy(ctx)
    path = "one workgroup" if n <= 4096 else "radix, %d tiles" % ((n + 4095) // 4096)
    lines.append(f"n = {n} ({path}; {repeats} repeats after {warmup} warm-up calls)")
    lines.append(f"  (a) blend_sort stage, device            {stats(stage_us)}")
    lines.append(f"  (b) blend_draw_order + order_write, host {stats(host_us)}  [{len(host_us)} repeats]")
    lines.append(f"  (b') numpy lexsort + order_write, host   {stats(vec_us)}")
    lines.append(f"  (c) r3n_blend_sort call, host            {stats(call_us)}")
    lines.append(f"      r3n_blend_objects_write, once        {upload_us:10.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("blend_sort_cost: needs the GPU (a timing taken anywhere else says nothing)")
    lib = _ffi.lib()
    lines = ["tools/blend_sort_cost.py: ordering n translucent objects, device sort against the host path"]
    for n in args.sizes:
        measure(lib, n, args.repeats, args.warmup, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
