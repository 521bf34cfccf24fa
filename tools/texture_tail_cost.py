#!/usr/bin/env python3
"""GPU box: what dropping a texture's top level costs -- r3n_textures_from_texture (a copy of the tail inside the texel pool)
against what there was before it, r3n_textures_update of the same tails from the host.

N BC7 textures of SIZE x SIZE with their full stored chains (random block data, as tools/texture_stream_cost.py), loaded with one
r3n_textures_update into a fresh context.  Measured: start_mip = 1 for all N in ONE call, into N new slots.
  SIZE 256   level 1 starts 65536 words into a texture: every source starts on a 16-byte boundary;
  SIZE 255   level 1 starts 65025 words in: every source starts one word behind a 16-byte boundary -- the misaligned path.
Timed: host wall clock around the call (it waits for the frames when a buffer grows -- none are in flight here -- places, uploads its
table and the new rows, launches once and waits for its own work), `--repeats` times, EACH on a freshly loaded context; and,
alternated with it, around r3n_textures_update of the same levels (BC7, sliced from the host's chains) on a context loaded the same
way.  Median and range.  Next to the times what the program counts: payload bytes staged and kernels launched (r3n_texture_stats for
the update, r3n_texture_tail_result for the copy).  After each copy every derived texture's words are compared with the source
tail's.

The kernel alone: run the tool under `rocprofv3 --kernel-trace` in a run of its own and give the trace to a second, unprofiled run
with --kernel-trace: the dispatches of k_copy_tails are told apart by their grid (the two sizes differ in wave slots), the warm-up
dispatch of each is dropped, and the traffic -- 2 x the copied bytes, read once and written once -- over the median duration stands
beside r3n_hbm_copy_rate from the same process for the same byte count (64 MiB at least: it measures no less).  Without a trace
the kernel columns say "not measured".

usage: python tools/texture_tail_cost.py [--textures 256] [--repeats 5] [--kernel-trace CSV] [--out profiles/texture_tail.md]"""
import argparse
import csv
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

BC7 = 14  # R3N_TEXTURE_BC7_RGBA_UNORM


def level_bytes(size, k):
    return ((max(1, size >> k) + 3) // 4) ** 2 * 16


def chain(size, rng):
    return b"".join(rng.integers(0, 256, level_bytes(size, k), dtype=np.uint8).tobytes() for k in range(size.bit_length()))


def pack(entries):
    """entries: (format, w, h, mips, bytes) -> (descs, payload, payload bytes)"""
    descs = np.zeros((len(entries), 8), dtype=np.uint32)
    at, parts = 0, []
    for row, (fmt, w, h, mips, data) in zip(descs, entries):
        row[:6] = (at, w, h, mips, fmt, 0)
        parts.append(data)
        at += len(data)
    return descs, np.frombuffer(b"".join(parts), dtype=np.uint8), at


def chain_words(size, first, mips):
    return sum(max(1, size >> k) ** 2 for k in range(first, mips))


class Loaded:
    """A fresh context holding the N textures in slots 0 .. N - 1."""

    def __init__(self, ffi, lib, textures, size):
        self.ffi, self.lib, self.size, self.n = ffi, lib, size, len(textures)
        self.mips = size.bit_length()
        self.ctx = lib.r3n_create(0, None)
        assert self.ctx, lib.r3n_create_error()
        descs, payload, n_bytes = pack([(BC7, size, size, self.mips, data) for data in textures])
        slots = np.arange(self.n, dtype=np.uint32)
        self.check(lib.r3n_textures_update(self.ctx, ffi.ptr(slots), ffi.ptr(descs), self.n, ffi.ptr(payload), n_bytes), "load")
        self.check(lib.r3n_sync(self.ctx), "sync")

    def check(self, code, what):
        self.ffi.check(self.ctx, code, what)

    def stats(self):
        out = self.ffi.TextureCounters()
        self.check(self.lib.r3n_texture_stats(self.ctx, ctypes.byref(out), 0), "stats")
        return {name: int(getattr(out, name)) for name, _ in self.ffi.TextureCounters._fields_}

    def copy_tails(self):
        items = (self.ffi.TextureTail16 * self.n)(*[self.ffi.TextureTail16(self.n + i, i, 1, 0) for i in range(self.n)])
        out = self.ffi.TextureTailResult()
        t0 = time.perf_counter()
        code = self.lib.r3n_textures_from_texture(self.ctx, items, self.n, ctypes.byref(out))
        dt = time.perf_counter() - t0
        self.check(code, "r3n_textures_from_texture")
        return dt, {name: int(getattr(out, name)) for name, _ in self.ffi.TextureTailResult._fields_}

    def upload_tails(self, textures):
        skip = level_bytes(self.size, 0)
        descs, payload, n_bytes = pack([(BC7, self.size >> 1, self.size >> 1, self.mips - 1, data[skip:]) for data in textures])
        slots = np.arange(self.n, 2 * self.n, dtype=np.uint32)
        before = self.stats()
        t0 = time.perf_counter()
        code = self.lib.r3n_textures_update(self.ctx, self.ffi.ptr(slots), self.ffi.ptr(descs), self.n, self.ffi.ptr(payload), n_bytes)
        dt = time.perf_counter() - t0
        self.check(code, "r3n_textures_update")
        after = self.stats()
        return dt, after["bytes_staged"] - before["bytes_staged"], after["kernel_launches"] - before["kernel_launches"]

    def tails_equal_sources(self):
        n = ctypes.c_uint32(0)
        self.check(self.lib.r3n_readback_texture_descs(self.ctx, None, 0, ctypes.byref(n)), "descs")
        d = np.zeros((n.value, 8), dtype=np.uint32)
        self.check(self.lib.r3n_readback_texture_descs(self.ctx, self.ffi.ptr(d), n.value, ctypes.byref(n)), "descs")
        words, first = chain_words(self.size, 1, self.mips), self.size * self.size
        a, b = np.zeros(words, dtype=np.uint32), np.zeros(words, dtype=np.uint32)
        for i in range(self.n):
            if d[self.n + i][1:4].tolist() != [self.size >> 1, self.size >> 1, self.mips - 1]:
                return False
            self.check(self.lib.r3n_readback_texels(self.ctx, int(d[i][0]) + first, self.ffi.ptr(a), words), "texels")
            self.check(self.lib.r3n_readback_texels(self.ctx, int(d[self.n + i][0]), self.ffi.ptr(b), words), "texels")
            if not np.array_equal(a, b):
                return False
        return True

    def close(self):
        self.lib.r3n_destroy(self.ctx)


def kernel_durations(path, blocks):
    """ns of every k_copy_tails dispatch of `blocks` workgroups of 256, in start order"""
    rows = [r for r in csv.DictReader(open(path)) if "k_copy_tails" in r["Kernel_Name"] and int(r["Grid_Size_X"]) in (blocks, blocks * 256)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--textures", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-trace", default=None, help="kernel-trace CSV of a profiled run of this tool with the same arguments")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("texture_tail_cost: needs the GPU (times are not measured anywhere else)")
    from rend3_amd import _ffi
    lib = _ffi.lib()
    n = args.textures
    lines = ["# Dropping a level: a texture's mip tail copied on the GPU against the same levels uploaded again", "",
             f"`python tools/texture_tail_cost.py --textures {n} --repeats {args.repeats}` on one MI355X: {n} BC7 textures with full stored chains "
             "(random block data), loaded with one `r3n_textures_update`; then `start_mip = 1` for all of them in ONE call into new slots.  Host "
             "wall clock around calls that end in their own device synchronise; every value from a freshly loaded context, the two calls "
             "alternated.  Kernel time: `k_copy_tails` from a `rocprofv3 --kernel-trace` run of its own of the same command; its traffic is 2 x "
             "the copied bytes.  `r3n_hbm_copy_rate` from the same process, for the copied byte count or 64 MiB, the least it measures, whichever is "
             "larger -- the copy kernel moves a third of that, so its launch ramp weighs more.", "",
             "| textures | source alignment | words copied | `r3n_textures_from_texture`, median (range) | bytes staged / launches | `r3n_textures_update` of the tails, median (range) | bytes staged / launches | kernel, median (range) | kernel rate | `r3n_hbm_copy_rate` | of it |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    same, every, kernel = True, [], {}
    for size in (256, 255):
        rng = np.random.default_rng(0x7E87 + size)
        textures = [chain(size, rng) for _ in range(n)]
        warm = Loaded(_ffi, lib, textures[:8], size)  # code objects, the first allocations; in a trace: the first dispatch of its grid
        warm.copy_tails()
        warm.close()
        warm = Loaded(_ffi, lib, textures[:8], size)
        warm.upload_tails(textures[:8])
        warm.close()
        t_copy, t_up, res, staged, launches = [], [], None, 0, 0
        for _ in range(args.repeats):
            a = Loaded(_ffi, lib, textures, size)
            dt, res = a.copy_tails()
            t_copy.append(dt)
            same = same and a.tails_equal_sources()
            a.close()
            b = Loaded(_ffi, lib, textures, size)
            dt, staged, launches = b.upload_tails(textures)
            t_up.append(dt)
            b.close()
        nbytes = res["words_copied"] * 4
        ctx = lib.r3n_create(0, None)
        rate = ctypes.c_double(0.0)
        _ffi.check(ctx, lib.r3n_hbm_copy_rate(ctx, max(nbytes, 64 << 20), 5, ctypes.byref(rate)), "r3n_hbm_copy_rate")  # (it takes no less)
        lib.r3n_destroy(ctx)
        c, u = np.array(t_copy) * 1e3, np.array(t_up) * 1e3
        every.append(f"{size} x {size}: copy " + " ".join(f"{v:.3f}" for v in c) + "; upload " + " ".join(f"{v:.3f}" for v in u))
        tail_words = chain_words(size, 1, size.bit_length())
        waves = n * (-(-tail_words // 1024))
        cells = ["not measured", "not measured", "not measured"]
        if args.kernel_trace:
            ns = kernel_durations(args.kernel_trace, (waves + 3) // 4)
            assert len(ns) == args.repeats, f"{len(ns)} dispatches of {(waves + 3) // 4} workgroups in the trace, {args.repeats} expected"
            k = np.array(ns) / 1e3
            gbs = 2 * nbytes / (np.median(k) * 1e-6) / 1e9
            kernel[size] = (np.median(k), k.min(), k.max())
            cells = [f"{np.median(k):.1f} us ({k.min():.1f} - {k.max():.1f})", f"{gbs:.0f} GB/s", f"{100 * gbs / rate.value:.0f} %"]
        lines.append(f"| {n} x {size} x {size} | {(size * size) & 3} | {res['words_copied']} | {np.median(c):.3f} ms ({c.min():.3f} - {c.max():.3f}) | "
                     f"0 B / {res['kernel_launches']} | {np.median(u):.3f} ms ({u.min():.3f} - {u.max():.3f}) | {staged} B / {launches} | {cells[0]} | {cells[1]} | "
                     f"{rate.value:.0f} GB/s | {cells[2]} |")
    lines += ["", "Every host value in ms, in call order: " + ".  ".join(every) + ".", ""]
    if kernel:
        al, mis = kernel[256], kernel[255]
        lines += [f"Misaligned against aligned sources, kernel alone: {mis[0]:.1f} us ({mis[1]:.1f} - {mis[2]:.1f}) for {chain_words(255, 1, 8) * n * 4 / 1e6:.1f} MB "
                  f"against {al[0]:.1f} us ({al[1]:.1f} - {al[2]:.1f}) for {chain_words(256, 1, 9) * n * 4 / 1e6:.1f} MB.", ""]
    lines += [f"Every derived texture's descriptor and words equal to its source's tail: {'yes' if same else 'NO'}.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    assert same, "a derived texture differs from its source's tail"


if __name__ == "__main__":
    main()
