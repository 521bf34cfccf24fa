#!/usr/bin/env python3
"""Writes tests/golden/morph-notangent.glb: a synthetic glTF 2.0 asset with morph targets, texture coordinates, a normal map and NO
tangents, generated from a seed (nothing in it comes from any other asset).
usage: python tests/golden/make_tangents_fixture.py [--check]

  mesh 0: a 9 x 9 grid in the XY plane (81 vertices, 128 triangles), POSITION and TEXCOORD_0 -- no NORMAL, no TANGENT -- two morph
          targets, both POSITION only:
            target 0  a bulge towards +z with noise
            target 1  a fold along the diagonal with noise
          TEXCOORD_0 is the grid's own parametrisation, sheared and with noise, so that no triangle's uv footprint is degenerate
          mesh.weights = [0.5, 0.25]
  material 0: a base colour factor and a normalTexture: an 8 x 8 RGBA8 PNG of tilted tangent-space normals (stored, not deflated,
          so that the bytes do not depend on a compression library's version)
  node 0: the mesh at x = -1.2 (draws with the mesh's weights)
  node 1: the mesh at x = +1.2 with node.weights = [0, 1]

What the normal map does to such a file's lighting follows its shape only if the tangents are generated, as the reference's
MeshBuilder generates them, and regenerated from the morphed positions.
"""
import json
import os
import struct
import sys
import zlib

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "morph-notangent.glb")
SEED = 0x74616E67  # "tang"
N = 9
TEXTURE = 8


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
    uv = np.stack([0.5 + 0.45 * pos[:, 0] + 0.1 * pos[:, 1], 0.5 - 0.4 * pos[:, 1]], axis=1) + rng.uniform(-0.01, 0.01, (N * N, 2))
    bulge = 0.7 * (1.0 - pos[:, 0] * pos[:, 0]) * (1.0 - pos[:, 1] * pos[:, 1])  # (arithmetic only: no libm in the bytes)
    t0_pos = np.stack([np.zeros(N * N), np.zeros(N * N), bulge], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    fold = 0.5 * np.abs(pos[:, 0] + pos[:, 1])
    t1_pos = np.stack([0.1 * pos[:, 1], np.zeros(N * N), fold], axis=1) + rng.uniform(-0.02, 0.02, (N * N, 3))
    # tangent-space normals tilted up to ~40 degrees: x, y in [-0.6, 0.6], z made up to about unit length (integer bytes, no libm)
    xy = rng.integers(-76, 77, (TEXTURE, TEXTURE, 2))
    z2 = 127 * 127 - (xy * xy).sum(axis=2)
    z = np.array([[int(np.floor(np.sqrt(float(q)))) for q in row] for row in z2])
    texels = np.stack([128 + xy[..., 0], 128 + xy[..., 1], 128 + z, np.full((TEXTURE, TEXTURE), 255)], axis=2).astype(np.uint8)
    return dict(pos=pos, idx=idx, uv=uv.astype(f32), t0_pos=t0_pos.astype(f32), t1_pos=t1_pos.astype(f32), texels=texels)


def png(rgba):
    """An RGBA8 PNG whose IDAT holds ONE stored (uncompressed) deflate block."""
    h, w, _c = rgba.shape
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))
    assert len(raw) < 65536
    stream = b"\x78\x01" + b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw + struct.pack(">I", zlib.adler32(raw))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", stream) + chunk(b"IEND", b""))


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
    uv = accessor(a["uv"], "VEC2")
    idx = accessor(a["idx"], "SCALAR")
    t0p, t1p = accessor(a["t0_pos"], "VEC3", minmax=True), accessor(a["t1_pos"], "VEC3", minmax=True)
    image = view(png(a["texels"]))
    doc = dict(
        asset=dict(version="2.0", generator="tests/golden/make_tangents_fixture.py"),
        scene=0, scenes=[dict(nodes=[0, 1])],
        nodes=[dict(name="default weights", mesh=0, translation=[-1.2, 0.0, 0.0]),
               dict(name="own weights", mesh=0, translation=[1.2, 0.0, 0.0], weights=[0.0, 1.0])],
        images=[dict(bufferView=image, mimeType="image/png")],
        textures=[dict(source=0)],
        materials=[dict(pbrMetallicRoughness=dict(baseColorFactor=[0.8, 0.6, 0.3, 1.0], metallicFactor=0.0, roughnessFactor=0.6),
                        normalTexture=dict(index=0), doubleSided=True)],
        meshes=[dict(weights=[0.5, 0.25],
                     primitives=[dict(attributes=dict(POSITION=pos, TEXCOORD_0=uv), indices=idx, material=0,
                                      targets=[dict(POSITION=t0p), dict(POSITION=t1p)])])],
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
