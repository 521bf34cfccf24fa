#!/usr/bin/env python3
"""GPU box: what the pooled mesh path costs, each figure beside the alternative measured in the same run.

  A. Handing over meshes one per call with a frame in flight: a street-scene frame (scenes.bistro_like: 600 objects, 100 000
     triangles, four 512^2 shadow views) at 1280 x 720 is enqueued, then ONE mesh (a 33 x 33 grid, 1 089 vertices) is added -- MESHES
     times, Renderer(mesh_upload="append") against "stream", `--repeats` loads each, alternated.  Timed: the host wall time of every
     add_mesh (both paths return after their own copy has executed).  The full waits come from r3n_mesh_stats ("stream"); the
     append path waits for the main stream -- behind every frame in flight -- in every call, by construction.
  B. r3n_mesh_compact of a buffer with every second block removed (BLOCKS blocks of 4 096 words) against what a caller can do
     without it: a fresh upload of the surviving blocks through r3n_mesh_buffer_write plus r3n_objects_write of every record, at
     3 000 and at 1 048 576 object records.  Host wall clock around calls that end in their own device synchronise, `--repeats`
     times, the two alternated.  Every record is compared with the numpy-relocated one afterwards.
  C. The relocation kernel alone (r3n_mesh_compact_result.relocate_ns: two device events around the launch), median of
     `--repeats`, at 1 048 576 slots with move tables of 1, 1 000 and 100 000 entries; every record names moved blocks, so every
     record is read and written.  Traffic: 128 B of line read + 128 B of line written back per slot (36 + 28 B of them asked
     for), against r3n_hbm_copy_rate from the same process.

usage: python tools/mesh_stream_cost.py [--meshes 64] [--blocks 3000] [--repeats 5] [--out profiles/mesh_stream.md]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

f32 = np.float32
FRAME, AMBIENT = (1280, 720), (0.1, 0.1, 0.1, 1.0)
INVALID = 0xFFFFFFFF


def grid(n, rng):
    u, w = np.meshgrid(np.linspace(-1.0, 1.0, n), np.linspace(-1.0, 1.0, n))
    pos = np.stack([u.reshape(-1), w.reshape(-1), rng.uniform(-0.2, 0.2, n * n)], axis=1).astype(f32)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    idx = np.stack([a, a + 1, a + n, a + 1, a + n + 1, a + n], axis=1).reshape(-1).astype(np.uint32)
    return pos, idx


def spread(values, scale=1e3, digits=3):
    v = np.array(values) * scale
    return f"{np.median(v):.{digits}f} ({v.min():.{digits}f} - {v.max():.{digits}f})"


# ------------------------------------------------------------------ A
def hand_over(r3, mode, meshes):
    import rend3_amd.scenes as S
    hm = r3.host
    r = r3.Renderer(hm.RIGHT, f32(FRAME[0]) / f32(FRAME[1]), mesh_upload=mode)
    info = S.bistro_like(r, hm, r3.material_record, n_objects=600, target_tris=100_000, shadow_res=512)
    r.set_camera_data(*info["camera"])
    for _ in range(3):
        r.render(*FRAME, ambient=AMBIENT, readback=False)
    r.sync()
    r.mesh_stats(reset=True)
    times = []
    for pos, idx in meshes:
        r.render(*FRAME, ambient=AMBIENT, readback=False)  # a frame in flight
        t0 = time.perf_counter()
        r.add_mesh(pos, idx)
        times.append(time.perf_counter() - t0)
    r.sync()
    st = r.mesh_stats()
    r.close()
    return times, st


# ------------------------------------------------------------------ B, C: contexts of the C ABI
class Ctx:
    def __init__(self, ffi, lib):
        self.ffi, self.lib = ffi, lib
        self.ctx = lib.r3n_create(0, None)
        assert self.ctx, lib.r3n_create_error()

    def check(self, code, what):
        self.ffi.check(self.ctx, code, what)

    def add(self, words, payload=None):
        """blocks of `words` words each: uploaded from `payload` (back to back) or zero-filled"""
        recs = (self.ffi.MeshBlock24 * len(words))()
        at = 0
        for r, w in zip(recs, words):
            r.words = int(w)
            if payload is None:
                r.flags = self.ffi.MESH_BLOCK_ZERO
            else:
                r.payload_offset, at = at, at + 4 * int(w)
        out = np.zeros(len(words), dtype=np.uint64)
        self.check(self.lib.r3n_mesh_blocks_add(self.ctx, recs, len(words), self.ffi.ptr(payload), at, self.ffi.ptr(out)), "r3n_mesh_blocks_add")
        return out

    def remove(self, offsets):
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.check(self.lib.r3n_mesh_blocks_remove(self.ctx, self.ffi.ptr(o), len(o)), "r3n_mesh_blocks_remove")

    def objects_write(self, recs):
        slots = np.arange(len(recs), dtype=np.uint32)
        return self.lib.r3n_objects_write(self.ctx, self.ffi.ptr(slots), self.ffi.ptr(recs), len(recs), len(recs))

    def objects(self, n):
        out = np.zeros((n, 32), dtype=np.uint32)
        self.check(self.lib.r3n_readback_objects(self.ctx, 0, self.ffi.ptr(out), n), "r3n_readback_objects")
        return out

    def compact(self, capacity):
        moves = (self.ffi.MeshMove24 * capacity)()
        out = self.ffi.MeshCompactResult()
        t0 = time.perf_counter()
        code = self.lib.r3n_mesh_compact(self.ctx, None, ctypes.byref(out), moves, capacity)
        dt = time.perf_counter() - t0
        self.check(code, "r3n_mesh_compact")
        res = {name: int(getattr(out, name)) for name, _ in self.ffi.MeshCompactResult._fields_}
        mv = np.frombuffer(moves, dtype=np.uint64).reshape(-1, 3)[: res["blocks_moved"]].copy()
        return dt, res, mv

    def close(self):
        self.lib.r3n_destroy(self.ctx)


def records(n, starts, words, rng):
    """n records, each naming one block with all seven fields (a plain object), index_count small, disabled (never drawn)"""
    recs = np.zeros((n, 32), dtype=np.uint32)
    b = rng.integers(0, len(starts), n)
    base = (np.asarray(starts, dtype=np.uint64) // 4)[b]
    room = np.asarray(words, dtype=np.uint64)[b]
    recs[:, 20] = (base + rng.integers(0, 1 << 30, n).astype(np.uint64) % room).astype(np.uint32)
    for a in range(6):
        recs[:, 23 + a] = ((base + rng.integers(0, 1 << 30, n).astype(np.uint64) % room) * 4).astype(np.uint32)
    recs[:, 21] = 3
    return recs


def compaction_against_reupload(ffi, lib, n_blocks, n_objects, repeats, rng, relocate):
    words = np.full(n_blocks, 4096)
    payload = rng.integers(0, 2 ** 32, int(words.sum()), dtype=np.uint64).astype(np.uint32)
    keep = np.arange(1, n_blocks, 2)
    t_compact, t_alt, ok, res = [], [], True, None
    for _ in range(repeats):
        c = Ctx(ffi, lib)
        starts = c.add(words, payload)
        recs = records(n_objects, starts[keep], words[keep], rng)
        c.check(c.objects_write(recs), "r3n_objects_write")
        c.remove(starts[::2])
        c.check(lib.r3n_sync(c.ctx), "r3n_sync")
        dt, res, moves = c.compact(n_blocks)
        t_compact.append(dt)
        ok = ok and np.array_equal(c.objects(n_objects)[:, 20:29], relocate_records(recs, moves, relocate)[:, 20:29]) and res["free_ranges_after"] == 0
        c.close()
        # the alternative: the surviving blocks again, packed, through the append call, and every record from the host
        a = Ctx(ffi, lib)
        a.check(lib.r3n_mesh_buffer_write(a.ctx, 0, ffi.ptr(payload), payload.nbytes), "r3n_mesh_buffer_write")
        a.check(a.objects_write(recs), "r3n_objects_write")
        packed = np.ascontiguousarray(payload.reshape(n_blocks, 4096)[keep].reshape(-1))
        fixed = relocate_records(recs, moves, relocate)
        a.check(lib.r3n_sync(a.ctx), "r3n_sync")
        t0 = time.perf_counter()
        code = lib.r3n_mesh_buffer_write(a.ctx, 0, ffi.ptr(packed), packed.nbytes)
        code2 = a.objects_write(fixed)
        t_alt.append(time.perf_counter() - t0)
        a.check(code, "r3n_mesh_buffer_write")
        a.check(code2, "r3n_objects_write")
        a.close()
    return t_compact, t_alt, res, ok


def relocate_records(recs, moves, relocate):
    out = recs.copy()
    out[:, 20] = relocate(recs[:, 20], moves, words=True)
    out[:, 23:29] = relocate(recs[:, 23:29], moves)
    return out


def kernel_alone(ffi, lib, entries, slots, repeats, rng, relocate):
    """`entries` moved 4-word blocks behind a 4-word hole, a hole behind every second one: `entries` table entries"""
    words, kept = [4], [False]
    for i in range(entries):
        words.append(4)
        kept.append(True)
        if i % 2:
            words.append(4)
            kept.append(False)
    kept = np.array(kept)
    c = Ctx(ffi, lib)
    times, ok, live = [], True, None
    for _ in range(repeats + 1):  # the first one warms up
        if live is not None:
            c.remove(live)
        starts = c.add(words)
        recs = records(slots, starts[kept], np.full(int(kept.sum()), 4), rng)
        c.check(c.objects_write(recs), "r3n_objects_write")
        c.remove(starts[~kept])
        _dt, res, moves = c.compact(len(words))
        assert res["blocks_moved"] == entries, res
        times.append(res["relocate_ns"] * 1e-9)
        ok = ok and np.array_equal(c.objects(slots)[:, 20:29], relocate_records(recs, moves, relocate)[:, 20:29])
        live = moves[:, 1].copy()
    c.close()
    return times[1:], ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--meshes", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_stream_cost: needs the GPU (times are not measured anywhere else)")
    import rend3_amd as r3
    from rend3_amd import _ffi
    from rend3_amd.renderer import relocate_offsets
    lib = _ffi.lib()
    rng = np.random.default_rng(0x3E57)
    ctx = lib.r3n_create(0, None)
    rate = ctypes.c_double(0.0)
    _ffi.check(ctx, lib.r3n_hbm_copy_rate(ctx, 1 << 30, 5, ctypes.byref(rate)), "r3n_hbm_copy_rate")
    lib.r3n_destroy(ctx)
    lines = ["# Pooled mesh blocks: hand-over, compaction and relocation, each beside its alternative", "",
             f"`python tools/mesh_stream_cost.py --meshes {args.meshes} --blocks {args.blocks} --repeats {args.repeats}` on one MI355X.  Host times are "
             "wall clock around calls that end in their own device synchronise; the kernel time is between two device events.  Median "
             f"(range).  `r3n_hbm_copy_rate` (1 GiB) in the same process: {rate.value:.0f} GB/s.", ""]

    # ---- A
    meshes = [grid(33, rng) for _ in range(args.meshes)]
    hand_over(r3, "stream", meshes[:4])  # warm-up: code objects, first allocations
    per = {"append": [], "stream": []}
    totals = {"append": [], "stream": []}
    waits = []
    for _ in range(args.repeats):
        for mode in ("append", "stream"):
            t, st = hand_over(r3, mode, meshes)
            per[mode] += t
            totals[mode].append(sum(t))
            if mode == "stream":
                waits.append((st["full_waits"], st["growths"], st["add_calls"]))
    lines += [f"## A. {args.meshes} meshes (33 x 33 grids, 1 089 vertices, 12.5 k words each) handed over one per call, a 1280 x 720 frame in flight", "",
              "| path | all hand-overs, ms | one hand-over, ms | full waits |", "|---|---|---|---|",
              f"| `append` (`r3n_mesh_buffer_write`) | {spread(totals['append'], digits=2)} | {spread(per['append'])} | every call waits for the main stream, behind the frame in flight (by construction; not counted by `r3n_mesh_stats`) |",
              f"| `stream` (`r3n_mesh_blocks_add`) | {spread(totals['stream'], digits=2)} | {spread(per['stream'])} | "
              + ", ".join(f"{w} in {a} calls ({g} growths)" for w, g, a in waits) + " |", "",
              "The full waits of the stream path are the growths of the device block (x 2, behind a full wait each); between them a "
              "hand-over waits for its own copy alone.", ""]

    # ---- B
    lines += [f"## B. `r3n_mesh_compact`, every second of {args.blocks} blocks of 4 096 words removed, against re-uploading", "",
              "| object records | `r3n_mesh_compact`, ms | `r3n_mesh_buffer_write` of the survivors + `r3n_objects_write` of every record, ms | words moved | passes | launches | relocation kernel |",
              "|---|---|---|---|---|---|---|"]
    all_ok = True
    for n_objects in (3000, 1 << 20):
        tc, ta, res, ok = compaction_against_reupload(_ffi, lib, args.blocks, n_objects, args.repeats, rng, relocate_offsets)
        all_ok = all_ok and ok
        lines.append(f"| {n_objects} | {spread(tc)} | {spread(ta)} | {res['words_moved']} | {res['passes']} | {res['kernel_launches']} | {res['relocate_ns'] / 1e3:.1f} us |")
    lines += ["", "Each compaction runs in a fresh context, so its scratch block and job table are allocated inside the timed call.", ""]

    # ---- C
    slots = 1 << 20
    lines += [f"## C. `k_relocate_objects` alone, {slots} slots, every record names moved blocks", "",
              "| table entries | form | kernel, us | lines read + written (256 B per slot) | of the copy rate | bytes asked for (64 B per slot) |", "|---|---|---|---|---|---|"]
    for entries in (1, 1000, 100000):
        t, ok = kernel_alone(_ffi, lib, entries, slots, args.repeats, rng, relocate_offsets)
        all_ok = all_ok and ok
        med = float(np.median(t))
        lines.append(f"| {entries} | {'LDS' if entries <= 256 else 'global'} | {spread(t, 1e6, 1)} | {slots * 256 / med / 1e9:.0f} GB/s | "
                     f"{100 * slots * 256 / med / 1e9 / rate.value:.0f} % | {slots * 64 / med / 1e9:.0f} GB/s |")
    lines += ["", f"Every record equal to the numpy-relocated one after every compaction above: {'yes' if all_ok else 'NO'}.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    assert all_ok, "a compaction left a record that differs from the rule"


if __name__ == "__main__":
    main()
