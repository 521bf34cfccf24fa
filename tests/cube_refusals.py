"""What the cube-upload entries refuse, ONCE: the rows tests/test_skybox_lod_gpu.py sends to r3n_texture_cubes_write_encoded and
tests/test_equirect_gpu.py sends to r3n_texture_cubes_write_sources on the device, and tests/test_cube_plan.py sends to the planner
(rend3_amd/csrc/cube_plan.h) through tests/cube_plan_check.cpp on the CPU.

A row is (what, cubes, payload_bytes, code, message): `cubes` = one dict per cube of the call, over the entry's defaults below;
`message` = the tail of r3n_last_error behind the entry's name.  A row that breaks several rules states the code of the check that
comes first: the first offending cube in array order, and within a cube the order of checks of its entry --
    encoded: format id, square, extent, chain (no mips / more than the extent has), stored_mips, alignment, payload, pool capacity
    sources: kind, format id, zero extent, source extent, face extent, square (stored faces), mips, alignment, payload, pool and
             scratch capacity
-- with a cube's capacity check behind all of its own checks and in front of every check of the next cube."""
from rend3_amd import containers as C

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = -1, -5, -6
RGBE8 = 0x100
PAYLOAD_BYTES = 4096  # of the buffer the GPU tests pass; a larger payload_bytes is a lie the call must refuse before it reads

ENCODED_DEFAULTS = dict(width=4, height=4, mips=1, fmt=C.RGBA8, offset=0, stored=0)
SOURCE_DEFAULTS = dict(kind=1, fmt=RGBE8, width=8, height=4, extent=4, mips=1, offset=0)

SQUARE, EXTENT, FORMAT, POOL = "a cube's faces are square", "bad extent", "unknown format id", "the cube pool exceeds 2^32 words"
GENERATED = "a cube carries all its levels (no MipmapSource::Generated for cubes, rend3/src/managers/texture.rs:147)"
ENCODED_ALIGN, ENCODED_OUTSIDE = "face +X level 0 must start on a 4-byte boundary", "faces outside the payload"
MIPS, SOURCE_ALIGN, SOURCE_OUTSIDE = "more mips than the extent has", "a source must start on a 4-byte boundary", "data outside the payload"
ZERO, STORED_SQUARE = "zero extent", "a cube's faces are square, of the face extent"

ENCODED = [
    ("not square", [dict(height=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, SQUARE),
    ("extent 0", [dict(width=0, height=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, EXTENT),
    ("extent past 16384", [dict(width=16385, height=16385, fmt=C.R8)], 1 << 40, ERR_INVALID_ARG, EXTENT),
    ("more mips than the extent has", [dict(mips=4)], PAYLOAD_BYTES, ERR_INVALID_ARG, MIPS),
    ("no mips", [dict(mips=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, EXTENT),
    ("a face outside the payload", [dict()], 6 * 64 - 1, ERR_INVALID_ARG, ENCODED_OUTSIDE),
    ("the chain outside the payload", [dict(mips=3, fmt=C.BC1)], 6 * 24 - 1, ERR_INVALID_ARG, ENCODED_OUTSIDE),
    ("a misaligned offset", [dict(offset=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, ENCODED_ALIGN),
    ("an unknown format", [dict(fmt=C.FORMAT_COUNT)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("a generated chain", [dict(mips=3, stored=1)], PAYLOAD_BYTES, ERR_UNSUPPORTED, GENERATED),
    ("stored beyond mips", [dict(mips=2, stored=3)], PAYLOAD_BYTES, ERR_UNSUPPORTED, GENERATED),
    ("a pool past 2^32 words", [dict(width=16384, height=16384, fmt=C.R8_SNORM)], 1 << 40, ERR_CAPACITY, POOL),
    ("a pool past 2^32 words, three cubes", [dict(width=16384, height=16384, fmt=C.R8)] * 3, 1 << 40, ERR_CAPACITY, POOL),
    # ---- two rules at once
    ("not square AND a generated chain: square comes first", [dict(height=2, mips=2, stored=1)], PAYLOAD_BYTES, ERR_INVALID_ARG, SQUARE),
    ("a generated chain AND misaligned: stored_mips comes first", [dict(mips=3, stored=1, offset=2)], PAYLOAD_BYTES, ERR_UNSUPPORTED, GENERATED),
    ("more mips than the extent has AND a generated chain: the chain comes first", [dict(mips=4, stored=1)], PAYLOAD_BYTES, ERR_INVALID_ARG, MIPS),
    ("an unknown format AND misaligned: the format comes first", [dict(fmt=C.FORMAT_COUNT, offset=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("misaligned AND outside the payload: alignment comes first", [dict(offset=2)], 6 * 64, ERR_INVALID_ARG, ENCODED_ALIGN),
    ("a valid cube, then a generated chain", [dict(), dict(mips=3, stored=1, offset=384)], PAYLOAD_BYTES, ERR_UNSUPPORTED, GENERATED),
    ("a misaligned cube, then a pool past 2^32 words", [dict(offset=2), dict(width=16384, height=16384, fmt=C.R8_SNORM)], 1 << 40,
     ERR_INVALID_ARG, ENCODED_ALIGN),
    ("a pool past 2^32 words, then a misaligned cube", [dict(width=16384, height=16384, fmt=C.R8_SNORM), dict(offset=2)], 1 << 40,
     ERR_CAPACITY, POOL),
]

SOURCES = [
    ("an unknown kind", [dict(kind=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, "unknown source kind"),
    ("an unknown format", [dict(fmt=C.FORMAT_COUNT)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("an unknown encoding", [dict(fmt=RGBE8 + 1)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("RGBE8 is no format of stored faces", [dict(kind=0, width=4, height=4)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("zero width", [dict(width=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, ZERO),
    ("zero height", [dict(height=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, ZERO),
    ("zero face extent", [dict(extent=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, ZERO),
    ("a source extent above 65535", [dict(width=65536, height=1)], 1 << 40, ERR_INVALID_ARG, "a source extent above 65535"),
    ("a face extent above 16384", [dict(extent=16385)], PAYLOAD_BYTES, ERR_INVALID_ARG, "a face extent above 16384"),
    ("more mips than N has", [dict(extent=4, mips=4)], PAYLOAD_BYTES, ERR_INVALID_ARG, MIPS),
    ("no mips", [dict(mips=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, MIPS),
    ("data outside the payload", [dict()], 8 * 4 * 4 - 1, ERR_INVALID_ARG, SOURCE_OUTSIDE),
    ("an offset outside the payload", [dict(offset=1 << 33)], PAYLOAD_BYTES, ERR_INVALID_ARG, SOURCE_OUTSIDE),
    ("a decoded source outside the payload", [dict(fmt=C.BC6H_UF, width=9, height=5)], 6 * 16 - 1, ERR_INVALID_ARG, SOURCE_OUTSIDE),
    ("a misaligned offset", [dict(offset=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, SOURCE_ALIGN),
    ("stored faces that are not square", [dict(kind=0, fmt=C.RGBA8, width=4, height=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, STORED_SQUARE),
    ("stored faces of another extent", [dict(kind=0, fmt=C.RGBA8, width=4, height=4, extent=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, STORED_SQUARE),
    ("a pool past 2^32 words", [dict(extent=16384)], PAYLOAD_BYTES, ERR_CAPACITY, POOL),
    ("a pool past 2^32 words, four cubes", [dict(extent=8192)] * 4, PAYLOAD_BYTES, ERR_CAPACITY, POOL),
    # ---- two rules at once
    ("an unknown format AND misaligned: the format comes first", [dict(fmt=C.FORMAT_COUNT, offset=2)], PAYLOAD_BYTES, ERR_INVALID_ARG, FORMAT),
    ("an unknown kind AND a zero extent: the kind comes first", [dict(kind=2, width=0)], PAYLOAD_BYTES, ERR_INVALID_ARG, "unknown source kind"),
    ("stored faces not square AND no mips: square comes first", [dict(kind=0, fmt=C.RGBA8, width=4, height=2, mips=0)], PAYLOAD_BYTES,
     ERR_INVALID_ARG, STORED_SQUARE),
    ("a valid panorama, then a misaligned one", [dict(), dict(offset=130)], PAYLOAD_BYTES, ERR_INVALID_ARG, SOURCE_ALIGN),
    ("a misaligned panorama, then a pool past 2^32 words", [dict(offset=2), dict(extent=16384)], PAYLOAD_BYTES, ERR_INVALID_ARG, SOURCE_ALIGN),
    ("a pool past 2^32 words, then a misaligned panorama", [dict(extent=16384), dict(offset=2)], PAYLOAD_BYTES, ERR_CAPACITY, POOL),
]


def encoded_cubes(row):
    """the cubes of an ENCODED row as r3n_texture_desc32 words: offset, width, height, mips, format, stored_mips, 0, 0"""
    out = []
    for cube in row[1]:
        d = dict(ENCODED_DEFAULTS, **cube)
        out.append([d["offset"], d["width"], d["height"], d["mips"], d["fmt"], d["stored"], 0, 0])
    return out


def source_cubes(row):
    """the cubes of a SOURCES row as r3n_cube_source fields: kind, format, width, height, face_extent, mips, offset"""
    out = []
    for cube in row[1]:
        d = dict(SOURCE_DEFAULTS, **cube)
        out.append((d["kind"], d["fmt"], d["width"], d["height"], d["extent"], d["mips"], d["offset"]))
    return out
