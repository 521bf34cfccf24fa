#!/usr/bin/env python3
"""GPU box: one 4096 x 4096 level per block format through r3n_textures_write_encoded (csrc/texture_decode.hip), one renderer
each.  Prints the host wall time of the hand-over (add_texture_2d_encoded, the array's re-send, sync) per format.  Run under
`rocprofv3 --kernel-trace --stats`, tools/texture_decode_rate.py --report <kernel_trace.csv> then prints the decode kernel's
(k_decode_block_jobs) HBM rate per format (algorithmic bytes: block bytes in + 64 B of RGBA8 out per block; the first row of
the trace is the 64 x 64 warm-up and is left out)."""
import csv
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FORMATS = [(6, "BC1", 8), (10, "BC3", 16), (12, "BC4", 8), (13, "BC5", 16), (14, "BC7", 16)]
W = H = 4096

if len(sys.argv) > 2 and sys.argv[1] == "--report":
    rows = [r for r in csv.DictReader(open(sys.argv[2])) if "k_decode_block_jobs" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[1:]
    blocks = (W // 4) * (H // 4)
    for (fid, name, bb), r in zip(FORMATS, rows):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        gb = blocks * (bb + 64) / 1e9
        print(f"{name}: {us:8.1f} us  {gb / (us * 1e-6) / 1e3:6.2f} TB/s  ({blocks * 16 / us:.0f} Mtexel/s)")
    sys.exit(0)

import rend3_amd as r3
rng = np.random.default_rng(3)
warm = r3.Renderer()  # the first hand-over of a process loads the code object: a 64 x 64 one, not timed
warm.add_texture_2d_encoded(6, 64, 64, [bytes(16 * 16 * 8)])
warm._flush_textures()
warm.sync()
warm.close()
for fid, name, bb in FORMATS:
    p = r3.Renderer()
    data = rng.integers(0, 256, (W // 4) * (H // 4) * bb, dtype=np.uint8)
    if name == "BC7":
        data.reshape(-1, 16)[:, 0] |= 1 << (np.arange(len(data) // 16) % 8).astype(np.uint8)  # every mode, evenly
    levels = [data.tobytes()]
    p.sync()
    t0 = time.perf_counter()
    p.add_texture_2d_encoded(fid, W, H, levels)
    p._flush_textures()  # where TextureManager::evaluate sits: the whole-array re-send
    p.sync()
    print(f"{name}: hand-over {1e3 * (time.perf_counter() - t0):.3f} ms")
    p.close()
