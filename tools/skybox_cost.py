#!/usr/bin/env python3
"""GPU box: what the skybox node costs on the bench scene (bistro_like, 3840x2160), one and four samples.

Per sample count: the same camera path with no skybox bound and with one bound, stage timing on (HIP events around every launch,
single stream), the stage table read and reset after EVERY frame; medians over the timed frames.  Reported: the `skybox` stage, the
frame's GPU time (sum of the stages) both ways and their difference, the share of pixels that took the sky, and the kernel against
its traffic floor -- algorithmic bytes (8 B of key per sample read; per sky pixel 8 B of Rgba16Float + 4 B of Rgba8 written and up
to four texel words read) over the copy rate measured on this device (r3n_hbm_copy_rate).

usage: python tools/skybox_cost.py [--frames 24] [--warmup 6] [--out profiles/skybox_cost.txt]

--mips: the cost of cubes with levels and of float cubes instead (profiles/skybox_mips.md).  An EMPTY world at 3840x2160, so the sky
is on every pixel; the `skybox` stage of
  case 1  a 1024^2 one-level Rgba8UnormSrgb cube through r3n_texture_cubes_write (what the parent commit can load as well),
  case 2  the same cube with its full chain (box-filtered here) through r3n_texture_cubes_write_encoded,
  case 3  a 1024^2 Bc6hRgbUfloat cube with a full chain (random blocks: there is no encoder here; the fetches do not depend on
          the values),
each in --runs fresh processes, the median stage time per process (the camera's field of view is 60 degrees, which magnifies such a
cube: every pixel stays on level 0, so cases 2 and 3 show the cost of selecting the level, not of fetching two).  With --parent-tree DIR (a checkout of the parent commit with its
library built) case 1 alternates between the two trees, so that both spreads come from one session.  Then the host time of ONE
r3n_texture_cubes_write_encoded call for case 3 and of ONE r3n_texture_cubes_write call for case 1, each in five fresh contexts
(both entries decode on the device and border the faces with k_cube_assemble; a parent commit that still built the plain entry's
borders on the host is measured beside it: with --parent-tree the plain call is timed in this tree, then in the parent's, in the same
session).
       python tools/skybox_cost.py --mips [--runs 5] [--parent-tree DIR] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

# (--tree DIR: import the package and bench.py from another checkout -- the parent commit's, for --mips --parent-tree)
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import numpy as np

import bench
import rend3_amd as r3
import rend3_amd.scenes

W, H = 3840, 2160


def sky_cube(n=1024):
    """a smooth gradient per face plus a little noise: neighbouring pixels read neighbouring texels, as with a photographed sky"""
    rng = np.random.default_rng(0x5C1)
    u = np.linspace(0.0, 1.0, n, dtype=np.float32)
    faces = np.zeros((6, n, n, 4), dtype=np.uint8)
    for f in range(6):
        base = 40.0 + 30.0 * f
        img = base + 90.0 * u[None, :, None] * np.array([1.0, 0.6, 0.3], dtype=np.float32) + 60.0 * u[:, None, None]
        faces[f, ..., :3] = np.clip(img + rng.integers(0, 8, (n, n, 3)), 0, 255).astype(np.uint8)
    faces[..., 3] = 255
    return faces


def timed_frames(r, info, base, first, count, samples):
    per_frame = []
    for k in range(first, first + count):
        r.set_camera_data(bench.camera_path(r3.host, info["camera"][0], k), info["camera"][1])
        r.render(W, H, samples=samples, ambient=bench.AMBIENT, clear_color=bench.CLEAR, readback=False, base=base)
        r.sync()
        per_frame.append(r.stage_times(reset=True))
    return per_frame


def median(per_frame, stage=None):
    if stage is None:
        return float(np.median([sum(ms for ms, _ in st.values()) for st in per_frame]))
    return float(np.median([st[stage][0] for st in per_frame]))


def measure(samples, frames, warmup, lines):
    r = r3.Renderer(r3.host.RIGHT, np.float32(W / H))
    info = r3.scenes.bistro_like(r, r3.host, r3.material_record, textured=True)
    base = r3.BaseRenderGraph(r)
    cube = r.add_texture_cube(sky_cube(), srgb=True)
    copy_gbs = r.hbm_copy_rate()
    r.set_multi_stream(False)
    r.timing_enable(True)
    result = {}
    for bound in (False, True, False, True):  # alternating: the two states see the same drift
        r.set_background_texture(cube if bound else None)
        timed_frames(r, info, base, 0, warmup, samples)
        result.setdefault(bound, []).extend(timed_frames(r, info, base, warmup, frames, samples))
    # the share of pixels the sky reached, on the last timed camera
    vis = np.zeros((H, W) if samples == 1 else (H, W, samples), dtype=np.uint64)
    r._check(r.lib.r3n_readback_visibility(r.ctx, r3._ffi.ptr(vis)), "r3n_readback_visibility")
    took = (vis >> np.uint64(32)).astype(np.uint32).view(np.float32) <= 0.0
    share = float((took if samples == 1 else took.any(axis=2)).mean())
    sky_ms = median(result[True], "skybox")
    launches = result[True][-1]["skybox"][1]
    off, on = median(result[False]), median(result[True])
    px = W * H
    floor_bytes = 8.0 * samples * px + share * px * (8 + 4 + 16)
    floor_ms = 1e3 * floor_bytes / (copy_gbs * 1e9)
    lines.append(f"samples {samples}: {info.get('objects', '?')} objects, {2 * frames} timed frames per state after {warmup} warm-up frames each, copy rate {copy_gbs:.0f} GB/s")
    lines.append(f"  skybox stage            {sky_ms * 1e3:8.1f} us  (median per frame, {launches} launch per frame)")
    lines.append(f"  pixels that took the sky {100.0 * share:7.2f} %")
    lines.append(f"  frame, no skybox bound  {off * 1e3:8.1f} us  (sum of the stages, single stream)")
    lines.append(f"  frame, skybox bound     {on * 1e3:8.1f} us  (delta {1e3 * (on - off):+.1f} us)")
    lines.append(f"  traffic floor           {floor_ms * 1e3:8.1f} us  ({floor_bytes / 1e6:.1f} MB algorithmic); kernel / floor = {sky_ms / floor_ms:.2f}x")
    assert result[False][-1]["skybox"][1] == 0, "a frame without a skybox launched the node"
    r.close()


# ---------------------------------------------------------------------------------------------- --mips
BC6H_UF, RGBA8_SRGB = 32, 1


def box_chain(faces):
    """the full chain of uint8[6, N, N, 4] faces (N a power of two): 2 x 2 averages, level by level"""
    levels = [faces]
    while levels[-1].shape[1] > 1:
        a = levels[-1].astype(np.uint16)
        levels.append(((a[:, 0::2, 0::2] + a[:, 1::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 1::2] + 2) // 4).astype(np.uint8))
    return [[lv[f].tobytes() for lv in levels] for f in range(6)]


def bc6h_chain(n):
    rng = np.random.default_rng(0xBC6)
    mips = n.bit_length()
    return [[rng.integers(0, 256, ((max(1, n >> k) + 3) // 4) ** 2 * 16, dtype=np.uint8).tobytes() for k in range(mips)] for _ in range(6)]


def add_case_cube(r, case, n=1024):
    if case == 1:
        return r.add_texture_cube(sky_cube(n), srgb=True)
    if case == 2:
        return r.add_texture_cube_encoded(RGBA8_SRGB, n, box_chain(sky_cube(n)))
    return r.add_texture_cube_encoded(BC6H_UF, n, bc6h_chain(n))


def child_stage(case, frames, warmup):
    """one fresh process: the median `skybox` stage over an empty world"""
    r = r3.Renderer(r3.host.RIGHT, np.float32(W / H))
    r.set_background_texture(add_case_cube(r, case))
    r.set_camera_data(r3.host.look_at_rh((0, 0, 0), (1.0, 0.4, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    r.set_multi_stream(False)
    r.timing_enable(True)
    out = {}
    for samples in (1, 4):
        per_frame = []
        for k in range(warmup + frames):
            r.render(W, H, samples=samples, clear_color=bench.CLEAR, readback=False)
            r.sync()
            st = r.stage_times(reset=True)
            if k >= warmup:
                per_frame.append(st["skybox"][0])
        out[str(samples)] = float(np.median(per_frame)) * 1e3
    out["copy_gbs"] = r.hbm_copy_rate()
    r.close()
    print("RESULT " + json.dumps(out))


def child_upload(entry, contexts=5, n=1024):
    """the host time of one upload call, a fresh context each: "encoded" = r3n_texture_cubes_write_encoded for case 3, "plain" =
    r3n_texture_cubes_write for case 1"""
    if entry == "plain":
        payload = np.ascontiguousarray(sky_cube(n)).reshape(-1).view(np.uint32)
        desc = np.array([[0, n, n, 1, RGBA8_SRGB, 0, 0, 0]], dtype=np.uint32)
    else:
        faces = bc6h_chain(n)
        payload = np.frombuffer(b"".join(b"".join(levels) for levels in faces), dtype=np.uint8)
        desc = np.array([[0, n, n, n.bit_length(), BC6H_UF, 0, 0, 0]], dtype=np.uint32)
    write = r3._ffi.lib().r3n_texture_cubes_write if entry == "plain" else r3._ffi.lib().r3n_texture_cubes_write_encoded
    ms = []
    for _ in range(contexts):
        r = r3.Renderer(r3.host.RIGHT, np.float32(W / H))
        r.sync()
        t0 = time.perf_counter()
        code = write(r.ctx, r3._ffi.ptr(desc), 1, r3._ffi.ptr(payload), payload.size)  # (payload.size: texels there, bytes here)
        ms.append(1e3 * (time.perf_counter() - t0))
        assert code == 0
        copy_gbs = r.hbm_copy_rate()
        r.close()
    print("RESULT " + json.dumps({"ms": ms, "payload_bytes": int(payload.nbytes), "copy_gbs": copy_gbs}))


def run_child(args, tree=None):
    env = dict(os.environ)
    if tree:
        args = args + ["--tree", os.path.abspath(tree)]
        env["R3N_LIB"] = os.path.join(os.path.abspath(tree), "rend3_amd", "librend3_amd.so")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise RuntimeError(f"child {args} failed ({res.returncode}):\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
    return json.loads(next(line for line in res.stdout.splitlines() if line.startswith("RESULT "))[7:])


def mips_report(args):
    lines = [f"tools/skybox_cost.py --mips: empty world at {W}x{H} (sky on every pixel), 1024^2 cubes, {args.runs} fresh processes per row, "
             f"median `skybox` stage of {args.frames} frames after {args.warmup} warm-up frames per process"]

    def row(name, runs):
        for samples in ("1", "4"):
            v = sorted(x[samples] for x in runs)
            lines.append(f"  {name:<44} samples {samples}: median {np.median(v):8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  ({' '.join(f'{x:.1f}' for x in v)})")

    child = ["--child-stage", "1", "--frames", str(args.frames), "--warmup", str(args.warmup)]
    this, parent = [], []
    for _ in range(args.runs):  # alternating: both libraries see the same drift
        this.append(run_child(child))
        if args.parent_tree:
            parent.append(run_child(child, args.parent_tree))
    row("case 1, one-level sRGB cube, this tree", this)
    if parent:
        row("case 1, one-level sRGB cube, parent commit", parent)
    for case, name in ((2, "case 2, sRGB cube, full chain"), (3, "case 3, BC6H cube, full chain")):
        child[1] = str(case)
        row(name, [run_child(child) for _ in range(args.runs)])
    def upload_row(name, up):
        lines.append(f"  {name} ({up['payload_bytes'] / 1e6:.1f} MB payload), five fresh contexts: median {np.median(up['ms']):.2f} ms  "
                     f"min {min(up['ms']):.2f}  max {max(up['ms']):.2f}  ({' '.join(f'{x:.2f}' for x in up['ms'])}); copy rate {up['copy_gbs']:.0f} GB/s")

    upload_row("r3n_texture_cubes_write_encoded, case 3", run_child(["--child-upload", "encoded"]))
    this_up = run_child(["--child-upload", "plain"])
    parent_up = run_child(["--child-upload", "plain"], args.parent_tree) if args.parent_tree else None
    upload_row("r3n_texture_cubes_write, case 1, this tree", this_up)
    if parent_up:
        upload_row("r3n_texture_cubes_write, case 1, parent commit", parent_up)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12, help="timed frames per block; every state is measured in two blocks")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mips", action="store_true", help="the cost of cubes with levels and of float cubes (see above)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="--mips: a checkout of the parent commit, its library built; measured on case 1 in alternation")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-stage", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-upload", choices=("encoded", "plain"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_stage is not None:
        return child_stage(args.child_stage, args.frames, args.warmup)
    if args.child_upload:
        return child_upload(args.child_upload)
    if args.mips:
        return mips_report(args)
    lines = [f"tools/skybox_cost.py: bistro_like at {W}x{H}, 1024^2 Rgba8UnormSrgb cube"]
    for samples in (1, 4):
        measure(samples, args.frames, args.warmup, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
