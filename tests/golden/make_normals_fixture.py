#!/usr/bin/env python3
"""Writes tests/golden/morph-nonormal.glb: a synthetic glTF 2.0 asset with morph targets and NO normals, generated from a seed
(nothing in it comes from any other asset).   usage: python tests/golden/make_normals_fixture.py [--check]

  mesh 0: a 9 x 9 grid in the XY plane (81 vertices, 128 triangles), POSITION only -- no NORMAL, no TANGENT -- two morph targets,
          both POSITION only:
            target 0  a bulge towards +z with noise
            target 1  a fold along the diagonal with noise
          mesh.weights = [0.5, 0.25]
  node 0: the mesh at x = -1.2 (draws with the mesh's weights)
  node 1: the mesh at x = +1.2 with node.weights = [0, 1]
  animation 0 "weights": node 1 LINEAR, three keys (0, 0.5, 1.25 s); node 0 STEP, two keys (0, 0.75 s)

The lighting of such a file follows its shape only if the normals are recomputed from the morphed positions.
"""
import json
import os
import struct
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "morph-nonormal.glb")
SEED = 0x6E6F726D  # "norm"
N = 9


def arrays():
    rng = np.random.Generator(np.random.PCG64(SEED))
    f32 = np.float32
    u, v = np.meshgrid(np.linspace(-1.0, 1.0, N), np.linspace(-1.0, 1.0, N))
    pos = np.stack([u.reshape(-1), v.reshape(-1), np.zeros(N * N)], axis=1).astype(f32)
    idx = []
    for j in range(N - 1):
        for i in range(N - 1):
            a = j * N + i
            idx += [a, a + 1, a + N, a + 1, a + N + 1, a + N]
    idx = np.array(idx, dtype=np.uint16)
    bulge = 0.7 * (1.0 - pos[:, 0] * pos[:, 0]) * (1.0 - pos[:, 1] * pos[:, 1])  # (arithmetic only: no libm in the bytes)
    t0_pos = np.stack([np.zeros(N * N), np.zeros(N * N), bulge], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    fold = 0.5 * np.abs(pos[:, 0] + pos[:, 1])
    t1_pos = np.stack([0.1 * pos[:, 1], np.zeros(N * N), fold], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    return dict(pos=pos, idx=idx, t0_pos=t0_pos.astype(f32), t1_pos=t1_pos.astype(f32),
                lin_t=np.array([0.0, 0.5, 1.25], dtype=f32),
                lin_w=np.array([[0.0, 1.0], [1.5, -0.5], [0.25, 0.75]], dtype=f32),
                step_t=np.array([0.0, 0.75], dtype=f32),
                step_w=np.array([[0.5, 0.25], [1.0, 0.0]], dtype=f32))


def build():
    a = arrays()
    blob = bytearray()
    views, accessors = [], []

    def view(data):
        while len(blob) % 4:
            blob.append(0)
        views.append(dict(buffer=0, byteOffset=len(blob), byteLength=len(data)))
        blob.extend(data)
        return len(views) - 1

    def accessor(arr, kind, minmax=False):
        comp = {np.dtype(np.float32): 5126, np.dtype(np.uint16): 5123}[arr.dtype]
        acc = dict(bufferView=view(arr.tobytes()), componentType=comp, count=len(arr), type=kind)
        if minmax:
            acc["min"], acc["max"] = [float(x) for x in np.atleast_1d(arr.min(axis=0))], [float(x) for x in np.atleast_1d(arr.max(axis=0))]
        accessors.append(acc)
        return len(accessors) - 1

    pos = accessor(a["pos"], "VEC3", minmax=True)
    idx = accessor(a["idx"], "SCALAR")
    t0p, t1p = accessor(a["t0_pos"], "VEC3", minmax=True), accessor(a["t1_pos"], "VEC3", minmax=True)
    lin_t, lin_w = accessor(a["lin_t"], "SCALAR", minmax=True), accessor(a["lin_w"].reshape(-1), "SCALAR")
    step_t, step_w = accessor(a["step_t"], "SCALAR", minmax=True), accessor(a["step_w"].reshape(-1), "SCALAR")
    doc = dict(
        asset=dict(version="2.0", generator="tests/golden/make_normals_fixture.py"),
        scene=0, scenes=[dict(nodes=[0, 1])],
        nodes=[dict(name="default weights", mesh=0, translation=[-1.2, 0.0, 0.0]),
               dict(name="own weights", mesh=0, translation=[1.2, 0.0, 0.0], weights=[0.0, 1.0])],
        materials=[dict(pbrMetallicRoughness=dict(baseColorFactor=[0.8, 0.6, 0.3, 1.0], metallicFactor=0.0, roughnessFactor=0.6),
                        doubleSided=True)],
        meshes=[dict(weights=[0.5, 0.25],
                     primitives=[dict(attributes=dict(POSITION=pos), indices=idx, material=0,
                                      targets=[dict(POSITION=t0p), dict(POSITION=t1p)])])],
        animations=[dict(name="weights",
                         samplers=[dict(input=lin_t, output=lin_w, interpolation="LINEAR"),
                                   dict(input=step_t, output=step_w, interpolation="STEP")],
                         channels=[dict(sampler=0, target=dict(node=1, path="weights")),
                                   dict(sampler=1, target=dict(node=0, path="weights"))])],
        accessors=accessors, bufferViews=views, buffers=[dict(byteLength=0)])
    while len(blob) % 4:
        blob.append(0)
    doc["buffers"][0]["byteLength"] = len(blob)
    js = json.dumps(doc, separators=(",", ":"), sort_keys=True).encode()
    js += b" " * (-len(js) % 4)
    body = struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(blob), 0x004E4942) + bytes(blob)
    return b"glTF" + struct.pack("<II", 2, 12 + len(body)) + body


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT, "rb").read() == data else 1)
    open(OUT, "wb").write(data)
    print(OUT, len(data), "bytes")
