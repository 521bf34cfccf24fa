"""What tests/test_skybox_lod.py (CPU) and tests/test_skybox_lod_gpu.py share: the cubes, the cameras and targets of the frame
cases, and writers of KTX2 / DDS cube files.  The CPU file proves that these cases reach every path the classifier of
tests/skybox_lod_reference.py names; the GPU file renders them."""
import struct

import numpy as np

from oracle import host as oh
from rend3_amd import containers as C

f32 = np.float32

# one format per decode family and pool class
FORMATS = [C.RGBA8_SRGB, C.R8, C.BC1, C.BC7_SRGB, C.BC6H_UF, C.BC6H_SF, C.RGBA16F, C.RG11B10F, C.RGB9E5]


def full_chain(n):
    return int(n).bit_length()


def level_payload(fmt, n, rng, nonfinite=False):
    """random bytes of one n x n level.  Block formats and the packed formats take any bits; Rgba16Float gets finite halfs in
    [-4, 12) (nonfinite: a sprinkling of +-inf and NaN as well); Rg11b10Float keeps its exponents below 31 (finite)."""
    size = C.level_bytes(fmt, n, n)
    if fmt == C.RGBA16F:
        v = (rng.random((n * n, 4)) * 16.0 - 4.0).astype(np.float16)
        if nonfinite:
            pick = rng.random((n * n, 4)) < 0.08
            v[pick] = rng.choice(np.array([np.inf, -np.inf, np.nan], dtype=np.float16), size=int(pick.sum()))
        return v.tobytes()
    raw = rng.integers(0, 256, size, dtype=np.uint8)
    if fmt == C.RG11B10F:
        words = raw.view(np.uint32) & np.uint32(~((1 << 6) | (1 << 17) | (1 << 27)) & 0xFFFFFFFF)
        return words.tobytes()
    return raw.tobytes()


def random_cube(fmt, n, mips, seed, nonfinite=False):
    """faces[f][k]: the bytes of face f level k"""
    rng = np.random.default_rng(seed)
    return [[level_payload(fmt, max(1, n >> k), rng, nonfinite) for k in range(mips)] for _ in range(6)]


def constant_level_cube(n, mips, value_of):
    """an Rgba16Float cube whose level k is the one colour (value_of(k), 0, 0, 1) on every face"""
    faces = []
    for _ in range(6):
        levels = []
        for k in range(mips):
            nk = max(1, n >> k)
            t = np.zeros((nk * nk, 4), dtype=np.float16)
            t[:, 0], t[:, 3] = value_of(k), 1.0
            levels.append(t.tobytes())
        faces.append(levels)
    return faces


def inverse_matrix(hand, view, proj, width, height):
    cam = oh.CameraState(view, proj, hand, f32(width) / f32(height))
    return oh.mat4_inverse(cam.origin_view_proj)


# ---- the frame cases: (name, N, mips (0 = the full chain), (width, height), handedness, view, projection)
def frame_cases():
    lh, rh = oh.look_at_lh, oh.look_at_rh
    up = (0, 1, 0)
    return [
        ("magnified face", 4, 0, (64, 48), oh.LEFT, lh((0, 0, 0), (0.2, -0.1, 1.0), up), ("perspective", 60.0, 0.1)),
        ("corner, small levels", 4, 0, (24, 16), oh.RIGHT, rh((0, 0, 0), (-1.0, 1.0, -1.0), up), ("perspective", 100.0, 0.1)),
        ("two levels", 16, 0, (9, 7), oh.LEFT, lh((1, 2, 3), (2.0, 2.0, 4.0), up), ("perspective", 90.0, 0.5)),
        ("partial chain, clamped", 16, 2, (5, 4), oh.RIGHT, rh((0, 5, 0), (0.3, -1.0, 0.2), (0, 0, 1)), ("perspective", 120.0, 0.1)),
        ("behind the axis", 8, 0, (2, 2), oh.LEFT, lh((0, 0, 0), (0.1, 0.05, 1.0), up), ("perspective", 170.0, 0.1)),
        ("odd extent 5", 5, 0, (16, 12), oh.LEFT, lh((0, 0, 0), (1.0, 0.4, 1.0), up), ("perspective", 110.0, 0.1)),
        ("odd extent 3, ortho", 3, 0, (12, 8), oh.RIGHT, rh((0, 0, 0), (1.0, 0.4, 1.0), up), ("orthographic", (3.0, 2.0, 4.0))),
        ("extent 2", 2, 0, (7, 5), oh.LEFT, lh((0, 0, 0), (-1.0, -0.6, 0.4), up), ("perspective", 140.0, 0.1)),
        ("extent 1", 1, 0, (6, 4), oh.RIGHT, rh((0, 0, 0), (0.2, 0.9, 0.3), up), ("perspective", 90.0, 0.1)),
        ("N 64 on 8 x 8", 64, 0, (8, 8), oh.LEFT, lh((0, 0, 0), (-1.0, 1.0, -1.0), up), ("perspective", 100.0, 0.1)),
    ]


# ---- cube files
_VK = {C.RGBA8_SRGB: 43, C.RGBA8: 37, C.R8: 9, C.BC1: 131, C.BC7_SRGB: 146, C.BC6H_UF: 143, C.BC6H_SF: 144, C.RGBA16F: 97, C.RG11B10F: 122,
       C.RGB9E5: 123}
_DXGI = {C.RGBA8_SRGB: 29, C.RGBA8: 28, C.R8: 61, C.BC1: 71, C.BC7_SRGB: 99, C.BC6H_UF: 95, C.BC6H_SF: 96, C.RGBA16F: 10, C.RG11B10F: 26,
         C.RGB9E5: 67}


def write_ktx2_cube(fmt, width, faces, face_count=6, layers=0, scheme=0, height=None):
    """KTX2: header, level index, then per level the faces back to back (levels stored smallest first, as the format asks)"""
    mips = len(faces[0])
    head = 80 + 24 * mips
    blobs, at, index = [], head, [None] * mips
    for k in reversed(range(mips)):
        blob = b"".join(faces[f][k] for f in range(len(faces)))
        at = (at + 15) & ~15
        index[k] = (at, len(blob))
        blobs.append((at, blob))
        at += len(blob)
    out = bytearray(at)
    out[:12] = C.KTX2_MAGIC
    struct.pack_into("<9I", out, 12, _VK[fmt], 1, width, width if height is None else height, 0, layers, face_count, mips, scheme)
    for k, (off, length) in enumerate(index):
        struct.pack_into("<3Q", out, 80 + 24 * k, off, length, length)
    for off, blob in blobs:
        out[off:off + len(blob)] = blob
    return bytes(out)


def write_dds_cube(fmt, width, faces, dx10=True, caps2=0xFE00, array_size=1, misc=0x4, height=None):
    """DDS: per face its levels back to back.  dx10=False writes the legacy header (Rgba8 / DXT1 only)."""
    mips = len(faces[0])
    head = bytearray(128)
    head[:4] = b"DDS "
    struct.pack_into("<7I", head, 4, 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x20000, width if height is None else height, width, 0, 0, mips)
    if dx10:
        struct.pack_into("<II4s5I", head, 76, 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    elif fmt in (C.BC1, C.BC1_SRGB):
        struct.pack_into("<II4s5I", head, 76, 32, 0x4, b"DXT1", 0, 0, 0, 0, 0)
    else:
        struct.pack_into("<II4s5I", head, 76, 32, 0x41, b"\0\0\0\0", 32, 0xFF, 0xFF00, 0xFF0000, 0xFF000000)
    struct.pack_into("<2I", head, 108, 0x1008 | 0x400000, caps2)
    out = bytes(head)
    if dx10:
        out += struct.pack("<5I", _DXGI[fmt], 3, misc, array_size, 0)
    return out + b"".join(b"".join(levels) for levels in faces)
