#!/usr/bin/env python3
"""GPU box: what the skybox node costs on the bench scene (bistro_like, 3840x2160), one and four samples.

Per sample count: the same camera path with no skybox bound and with one bound, stage timing on (HIP events around every launch,
single stream), the stage table read and reset after EVERY frame; medians over the timed frames.  Reported: the `skybox` stage, the
frame's GPU time (sum of the stages) both ways and their difference, the share of pixels that took the sky, and the kernel against
its traffic floor -- algorithmic bytes (8 B of key per sample read; per sky pixel 8 B of Rgba16Float + 4 B of Rgba8 written and up
to four texel words read) over the copy rate measured on this device (r3n_hbm_copy_rate).

usage: python tools/skybox_cost.py [--frames 24] [--warmup 6] [--out profiles/skybox_cost.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12, help="timed frames per block; every state is measured in two blocks")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
