#!/usr/bin/env python3
"""GPU box: what handing textures over costs, whole-array re-send against the streamed path (r3n_textures_update).

N BC7 textures of SIZE x SIZE with their full stored chains (random block data: the decode cost of a block does not depend much
on its bits, the copy cost not at all), two ways of loading them:
  (a) one texture per frame -- a viewer streaming a scene in: add one, evaluate the textures (Renderer._flush_textures, where
      TextureManager::evaluate sits), draw a frame of the street scene (scenes.bistro_like: 600 objects, 100 000 triangles, four
      shadow views, 1280 x 720; not read back, so it is in flight during the next hand-over) -- with
      Renderer(texture_upload="whole") against "stream", `--repeats` loads each, alternated.  Timed: the host wall time of every
      hand-over (it ends in the call's own device synchronise) and of the whole load, frames included; medians and ranges over
      the loads.
  (b) the whole set in ONE call: r3n_textures_write_encoded against r3n_textures_update on fresh contexts, host wall time around
      the call (each synchronises before it returns), `--repeats` times each, alternated; medians and ranges.  Both calls plan
      the same job tables and run the same kernels, so what is left between them is the host side: the whole write's staging
      block of its own (allocated and freed in the call) and its full wait, the update's resident buffers and allocator.
Next to the times: what the program counts -- bytes copied and kernels launched.  The streamed path's come from r3n_texture_stats;
the whole-array path's are ARITHMETIC from the shapes (it copies every texture present on every re-send and decodes one kernel
family -- every texture here is BC7 -- with one launch: k textures present -> k * bytes, one launch), not measurements.  After (a) the two renderers' decoded
texels are compared word for word.

usage: python tools/texture_stream_cost.py [--textures 256] [--size 256] [--repeats 3] [--out profiles/texture_stream.md]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

f32 = np.float32
BC7 = 14  # R3N_TEXTURE_BC7_RGBA_UNORM
FRAME, AMBIENT = (1280, 720), (0.1, 0.1, 0.1, 1.0)


def chain(size, rng):
    levels = []
    for k in range(size.bit_length()):
        s = max(1, size >> k)
        levels.append(rng.integers(0, 256, ((s + 3) // 4) ** 2 * 16, dtype=np.uint8).tobytes())
    return levels


def stream_in(r3, mode, textures, size):
    """(a): one texture per frame.  Returns (hand-over seconds per texture, total seconds, renderer)."""
    import rend3_amd.scenes as S
    hm = r3.host
    r = r3.Renderer(hm.RIGHT, f32(FRAME[0]) / f32(FRAME[1]), texture_upload=mode)
    info = S.bistro_like(r, hm, r3.material_record, n_objects=600, target_tris=100_000, shadow_res=512)
    quad = r.add_mesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=f32), np.array([0, 2, 1, 0, 3, 2], dtype=np.uint32),
                      normals=np.tile(np.array([[0, 1, 0]], dtype=f32), (4, 1)), uv0=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=f32),
                      tangents=np.tile(np.array([[1, 0, 0]], dtype=f32), (4, 1)))
    r.set_camera_data(*info["camera"])
    for _ in range(3):  # warm-up: code objects, buffers, the temporal culling history
        r.render(*FRAME, ambient=AMBIENT, readback=False)
    r.sync()
    hand_over = []
    t_all = time.perf_counter()
    for k, levels in enumerate(textures):
        t = r.add_texture_2d_encoded(BC7, size, size, levels)
        if k == 0:
            m = r.add_material(r3.material_record(albedo_mode="texture", albedo_texture=t, roughness=0.5))
            r.add_object(quad, m, hm.identity())
        t0 = time.perf_counter()
        r._flush_textures()
        hand_over.append(time.perf_counter() - t0)
        r.render(*FRAME, ambient=AMBIENT, readback=False)
    r.sync()
    return np.array(hand_over), time.perf_counter() - t_all, r


def one_call(r3, textures, size, update):
    """(b): the whole set in one call on a fresh context.  Returns (seconds, stats dict or None)."""
    from rend3_amd import _ffi
    lib = _ffi.lib()
    ctx = lib.r3n_create(0, None)
    assert ctx, lib.r3n_create_error()
    descs = np.zeros((len(textures), 8), dtype=np.uint32)
    at, parts = 0, []
    for row, levels in zip(descs, textures):
        row[:6] = (at, size, size, len(levels), BC7, 0)
        parts += levels
        at += sum(len(lv) for lv in levels)
    payload = np.frombuffer(b"".join(parts), dtype=np.uint8)
    slots = np.arange(len(textures), dtype=np.uint32)
    stats = None
    t0 = time.perf_counter()
    if update:
        code = lib.r3n_textures_update(ctx, _ffi.ptr(slots), _ffi.ptr(descs), len(slots), _ffi.ptr(payload), at)
    else:
        code = lib.r3n_textures_write_encoded(ctx, _ffi.ptr(descs), len(textures), _ffi.ptr(payload), at)
    dt = time.perf_counter() - t0
    _ffi.check(ctx, code, "one call")
    if update:
        out = _ffi.TextureCounters()
        _ffi.check(ctx, lib.r3n_texture_stats(ctx, ctypes.byref(out), 0), "r3n_texture_stats")
        stats = {name: int(getattr(out, name)) for name, _ in _ffi.TextureCounters._fields_}
    lib.r3n_destroy(ctx)
    return dt, stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--textures", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("texture_stream_cost: needs the GPU (times are not measured anywhere else)")
    import rend3_amd as r3
    rng = np.random.default_rng(0x7E87)
    n, size = args.textures, args.size
    textures = [chain(size, rng) for _ in range(n)]
    levels = len(textures[0])
    tex_bytes = sum(len(lv) for lv in textures[0])
    lines = [f"# Handing textures over: whole-array re-send against the streamed path", "",
             f"`python tools/texture_stream_cost.py --textures {n} --size {size} --repeats {args.repeats}` on one MI355X: {n} BC7 textures of "
             f"{size} x {size} with full stored chains ({levels} levels, {tex_bytes} B each, {n * tex_bytes / 1e6:.1f} MB in all), random block data.  "
             "Times are host wall clock around calls that end in their own device synchronise.  Bytes and launches of the streamed path are "
             "`r3n_texture_stats` counters; those of the whole-array path are arithmetic from the shapes (k textures present: k x bytes, "
             "one launch per re-send -- one kernel family), not measured.", ""]

    # (a) one texture per frame
    stream_in(r3, "stream", textures[:4], size)  # warm-up of both paths' kernels and of the allocator's first growth
    stream_in(r3, "whole", textures[:4], size)
    rows, loads = {}, {"whole": [], "stream": []}
    for _ in range(args.repeats):
        for mode in ("whole", "stream"):
            hand, total, r = stream_in(r3, mode, textures, size)
            rows[mode] = (hand, total, r)  # (the last load's renderer: its texels and counters are read below)
            loads[mode].append((hand.sum(), np.median(hand), total))
    same = all(np.array_equal(a, b) for a, b in zip(rows["whole"][2].readback_texels(per_texture=True), rows["stream"][2].readback_texels(per_texture=True)))
    st = rows["stream"][2].texture_stats()
    lines += ["## One texture per frame", "",
              f"Medians (ranges) over {args.repeats} loads per mode, alternated; a frame of the street scene (600 objects, 100 000 triangles, four "
              f"shadow views, {FRAME[0]} x {FRAME[1]}) is enqueued after every hand-over and not waited for.", "",
              "| mode | hand-over, all textures | median hand-over | whole load with frames | bytes copied | kernel launches | waits for every frame |",
              "|---|---|---|---|---|---|---|"]

    def spread(values, scale=1e3, digits=1):
        v = np.array(values) * scale
        return f"{np.median(v):.{digits}f} ({v.min():.{digits}f} - {v.max():.{digits}f}) ms"
    for mode in ("whole", "stream"):
        if mode == "whole":
            copied, launches, waits = f"{n * (n + 1) // 2 * tex_bytes / 1e6:.1f} MB (arithmetic)", f"{n} (arithmetic)", f"{n} (one per re-send)"
        else:
            copied, launches, waits = f"{st['bytes_staged'] / 1e6:.1f} MB", str(st["kernel_launches"]), f"{st['full_syncs']} ({st['pool_grows']} growths)"
        sums, medians, totals = zip(*loads[mode])
        lines.append(f"| {mode} | {spread(sums)} | {spread(medians, digits=3)} | {spread(totals)} | {copied} | {launches} | {waits} |")
    ratio_a = np.median([x[0] for x in loads["whole"]]) / np.median([x[0] for x in loads["stream"]])
    lines += ["", f"Hand-over time, whole over stream: {ratio_a:.1f} x (measured).  Decoded texels of the two renderers equal word for word: {'yes' if same else 'NO'}.",
              f"Streamed path after the load: {st}.", ""]

    # (b) the whole set in one call
    one_call(r3, textures[:4], size, False)
    one_call(r3, textures[:4], size, True)
    t = {False: [], True: []}
    stats = None
    for _ in range(args.repeats):
        for update in (False, True):
            dt, s = one_call(r3, textures, size, update)
            t[update].append(dt)
            stats = s or stats
    lines += ["## The whole set in one call", "", "| call | host wall time, median (range) | kernel launches |", "|---|---|---|"]
    for update, name in ((False, "r3n_textures_write_encoded"), (True, "r3n_textures_update")):
        a = np.array(t[update]) * 1e3
        launches = str(stats["kernel_launches"]) if update else "1 (arithmetic)"
        lines.append(f"| `{name}` | {np.median(a):.2f} ms ({a.min():.2f} - {a.max():.2f}) | {launches} |")
    ratio_b = np.median(t[False]) / np.median(t[True])
    lines += ["", f"Whole-array write over update, medians of {args.repeats} alternated calls on fresh contexts: {ratio_b:.2f} x (measured).  "
              f"Update call: {stats}.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    assert same, "the two paths decoded different texels"


if __name__ == "__main__":
    main()
