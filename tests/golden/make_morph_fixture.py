#!/usr/bin/env python3
"""Writes tests/golden/morph-plane.glb: a synthetic glTF 2.0 asset with morph targets, generated from a seed (nothing in it
comes from any other asset).   usage: python tests/golden/make_morph_fixture.py [--check]

  mesh 0: a 9 x 9 grid in the XY plane (81 vertices: neither a multiple of 64 nor of 4), NORMAL (0, 0, 1), TANGENT (1, 0, 0, 1),
          128 triangles, three morph targets:
            target 0  POSITION + NORMAL             a bulge towards +z with noise
            target 1  POSITION only, SPARSE         seven vertices displaced, stored through a sparse accessor without buffer view
            target 2  POSITION + NORMAL + TANGENT   a sideways shear with noise (tangent deltas are vec3)
          mesh.weights = [0.25, 0, 0.5]
  node 0: the mesh at x = -1.2 (draws with the mesh's weights)
  node 1: the mesh at x = +1.2 with node.weights = [0, 1, 0.25]
  animation 0 "weights": node 1 LINEAR, three keys (0, 0.5, 1.25 s); node 0 STEP, two keys (0, 0.75 s)
"""
import json
import os
import struct
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "morph-plane.glb")
SEED = 0x6D6F7270  # "morp"
N = 9
SPARSE_VERTICES = [4, 13, 22, 40, 41, 58, 80]


def arrays():
    rng = np.random.Generator(np.random.PCG64(SEED))
    f32 = np.float32
    u, v = np.meshgrid(np.linspace(-1.0, 1.0, N), np.linspace(-1.0, 1.0, N))
    pos = np.stack([u.reshape(-1), v.reshape(-1), np.zeros(N * N)], axis=1).astype(f32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], dtype=f32), (N * N, 1))
    tan = np.tile(np.array([1.0, 0.0, 0.0, 1.0], dtype=f32), (N * N, 1))
    idx = []
    for j in range(N - 1):
        for i in range(N - 1):
            a = j * N + i
            idx += [a, a + 1, a + N, a + 1, a + N + 1, a + N]
    idx = np.array(idx, dtype=np.uint16)
    bulge = 0.6 * (1.0 - pos[:, 0] * pos[:, 0]) * (1.0 - pos[:, 1] * pos[:, 1])  # (arithmetic only: no libm in the bytes)
    t0_pos = np.stack([np.zeros(N * N), np.zeros(N * N), bulge], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    t0_nrm = np.stack([-0.5 * pos[:, 0], -0.5 * pos[:, 1], np.zeros(N * N)], axis=1) + rng.uniform(-0.05, 0.05, (N * N, 3))
    t1_pos = rng.uniform(-0.3, 0.3, (len(SPARSE_VERTICES), 3))
    t2_pos = np.stack([0.4 * pos[:, 1], np.zeros(N * N), 0.2 * pos[:, 0]], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    t2_nrm = rng.uniform(-0.1, 0.1, (N * N, 3))
    t2_tan = rng.uniform(-0.1, 0.1, (N * N, 3))
    return dict(pos=pos, nrm=nrm, tan=tan, idx=idx, t0_pos=t0_pos.astype(f32), t0_nrm=t0_nrm.astype(f32),
                t1_idx=np.array(SPARSE_VERTICES, dtype=np.uint16), t1_val=t1_pos.astype(f32), t2_pos=t2_pos.astype(f32),
                t2_nrm=t2_nrm.astype(f32), t2_tan=t2_tan.astype(f32),
                lin_t=np.array([0.0, 0.5, 1.25], dtype=f32),
                lin_w=np.array([[0.0, 1.0, 0.25], [1.5, 0.0, -0.5], [0.0, 0.75, 1.0]], dtype=f32),
                step_t=np.array([0.0, 0.75], dtype=f32),
                step_w=np.array([[0.25, 0.0, 0.5], [1.0, 0.5, 0.0]], dtype=f32))


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

    def accessor(arr, kind, minmax=False, **extra):
        comp = {np.dtype(np.float32): 5126, np.dtype(np.uint16): 5123}[arr.dtype]
        acc = dict(bufferView=view(arr.tobytes()), componentType=comp, count=len(arr), type=kind, **extra)
        if minmax:
            acc["min"], acc["max"] = [float(x) for x in np.atleast_1d(arr.min(axis=0))], [float(x) for x in np.atleast_1d(arr.max(axis=0))]
        accessors.append(acc)
        return len(accessors) - 1

    pos = accessor(a["pos"], "VEC3", minmax=True)
    nrm = accessor(a["nrm"], "VEC3")
    tan = accessor(a["tan"], "VEC4")
    idx = accessor(a["idx"], "SCALAR")
    t0p, t0n = accessor(a["t0_pos"], "VEC3", minmax=True), accessor(a["t0_nrm"], "VEC3")
    # target 1: no buffer view of its own, every value comes from the sparse block
    dense = np.zeros((N * N, 3), dtype=np.float32)
    dense[a["t1_idx"]] = a["t1_val"]
    accessors.append(dict(componentType=5126, count=N * N, type="VEC3", min=[float(x) for x in dense.min(axis=0)],
                          max=[float(x) for x in dense.max(axis=0)],
                          sparse=dict(count=len(a["t1_idx"]), indices=dict(bufferView=view(a["t1_idx"].tobytes()), componentType=5123),
                                      values=dict(bufferView=view(a["t1_val"].tobytes())))))
    t1p = len(accessors) - 1
    t2p, t2n, t2t = accessor(a["t2_pos"], "VEC3", minmax=True), accessor(a["t2_nrm"], "VEC3"), accessor(a["t2_tan"], "VEC3")
    lin_t, lin_w = accessor(a["lin_t"], "SCALAR", minmax=True), accessor(a["lin_w"].reshape(-1), "SCALAR")
    step_t, step_w = accessor(a["step_t"], "SCALAR", minmax=True), accessor(a["step_w"].reshape(-1), "SCALAR")
    doc = dict(
        asset=dict(version="2.0", generator="tests/golden/make_morph_fixture.py"),
        scene=0, scenes=[dict(nodes=[0, 1])],
        nodes=[dict(name="default weights", mesh=0, translation=[-1.2, 0.0, 0.0]),
               dict(name="own weights", mesh=0, translation=[1.2, 0.0, 0.0], weights=[0.0, 1.0, 0.25])],
        materials=[dict(pbrMetallicRoughness=dict(baseColorFactor=[0.8, 0.6, 0.3, 1.0], metallicFactor=0.0, roughnessFactor=0.6),
                        doubleSided=True)],
        meshes=[dict(weights=[0.25, 0.0, 0.5],
                     primitives=[dict(attributes=dict(POSITION=pos, NORMAL=nrm, TANGENT=tan), indices=idx, material=0,
                                      targets=[dict(POSITION=t0p, NORMAL=t0n), dict(POSITION=t1p),
                                               dict(POSITION=t2p, NORMAL=t2n, TANGENT=t2t)])])],
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
