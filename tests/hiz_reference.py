"""numpy restatement of the Hi-Z pyramid (hi_z.wgsl:19-32) and of the multisample depth resolve (resolve_depth_min.wgsl:19-27),
independent of the oracle and of the product; the judge of tests/test_hiz.py and tests/test_hiz_gpu.py.

 1. Level k of a w x h target is max(1, w >> k) x max(1, h >> k); there are bit_length(max(w, h)) levels, level 0 is the depth plane.
 2. Texel (x, y) of level k is  nearest = 1.0;  for ix < 2 + (sw & 1): for iy < 2 + (sh & 1): nearest = min(nearest, load(2x + ix, 2y + iy))
    over level k - 1 (sw x sh).  A load past the source reads 0.0 -- which only happens where a source side is 1.
 3. The resolve of a multisampled target is  nearest = 1.0;  for every sample: nearest = min(nearest, depth)  with depth = the high
    32 bits of the sample's visibility key.

Values are compared as u32 words, so the planes the recipes below produce hold positive normal floats plus exact 0.0 and 1.0 only:
min() of negative zero, NaN or subnormals is not defined alike on both sides (and WGSL permits flushing).

launch_plan() restates the HOST's choice of kernels in r3n_hi_z; it judges nothing, the tests use it to assert that their extents
reach every path.
"""
import numpy as np

f32 = np.float32

# width x height of every target the pyramid tests build, by context group (tests/test_hiz_gpu.py makes one context per group)
EXTENT_GROUPS = {
    "sides": [(1, 1), (2, 2), (16, 16), (1, 7), (5, 1), (256, 2)],
    "head": [(37, 19), (202, 118), (204, 116), (200, 120), (256, 160), (48, 32)],
    "grid": [(201, 121), (401, 241), (801, 481), (20001, 1)],
}
EXTENTS = [e for group in EXTENT_GROUPS.values() for e in group]


def mip_count(w, h):
    return int(max(w, h)).bit_length()


def mip_shape(w, h, k):
    """(rows, columns) of level k"""
    return max(1, h >> k), max(1, w >> k)


def mip_offsets(w, h):
    """element offset of every level in the concatenated pyramid, and the total"""
    off, at = [], 0
    for k in range(mip_count(w, h)):
        off.append(at)
        r, c = mip_shape(w, h, k)
        at += r * c
    return off, at


def downsample(src):
    """one level from the (sh, sw) f32 level before it"""
    src = np.asarray(src, dtype=f32)
    sh, sw = src.shape
    dh, dw = max(1, sh >> 1), max(1, sw >> 1)
    nx, ny = 2 + (sw & 1), 2 + (sh & 1)
    padded = np.zeros((2 * dh + ny, 2 * dw + nx), dtype=f32)  # loads past the source read 0.0
    padded[:sh, :sw] = src
    nearest = np.ones((dh, dw), dtype=f32)
    for ix in range(nx):
        for iy in range(ny):
            nearest = np.minimum(nearest, padded[iy:iy + 2 * dh:2, ix:ix + 2 * dw:2])
    return nearest


def levels(plane):
    """[level 0, level 1, ...] as 2-D arrays"""
    plane = np.ascontiguousarray(plane, dtype=f32)
    h, w = plane.shape
    out = [plane]
    for k in range(1, mip_count(w, h)):
        out.append(downsample(out[-1]))
        assert out[-1].shape == mip_shape(w, h, k)
    return out


def pyramid(plane):
    """the whole chain, levels concatenated the way Renderer.readback_hiz returns them"""
    return np.concatenate([l.reshape(-1) for l in levels(plane)])


def resolve_depth_min(keys, samples):
    """keys: u64[n * samples], the samples of a pixel adjacent.  Returns f32[n]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(f32).reshape(-1, samples)
    nearest = np.ones(len(depth), dtype=f32)
    for s in range(samples):
        nearest = np.minimum(nearest, depth[:, s])
    return nearest


def first_difference(expected, got, w, h):
    """None, or a description of the first word that differs between two pyramids of a w x h target"""
    e, g = np.asarray(expected).view(np.uint32), np.asarray(got).view(np.uint32)
    if e.shape != g.shape:
        return f"{w}x{h}: {g.size} words, expected {e.size}"
    bad = np.flatnonzero(e != g)
    if not len(bad):
        return None
    off, _ = mip_offsets(w, h)
    i = int(bad[0])
    k = int(np.searchsorted(off, i, side="right")) - 1
    _, cols = mip_shape(w, h, k)
    y, x = divmod(i - off[k], cols)
    return (f"{w}x{h}: {len(bad)} words differ, first at level {k} ({cols} wide) texel ({x}, {y}): "
            f"expected {np.asarray(expected, dtype=f32)[i]!r} ({int(e[i]):#010x}), got {np.asarray(got, dtype=f32)[i]!r} ({int(g[i]):#010x})")


# ------------------------------------------------------------------ plane recipes (seeded; (h, w) f32)
def distinct(w, h, seed):
    """A random permutation of 1 .. w*h scaled into (0, 1]: no two texels are equal, so every texel of every level names the one
    source texel it came from and a wrong window is a wrong value."""
    n = w * h
    assert n < (1 << 23), "k / n must stay distinct in f32"
    perm = np.random.default_rng(seed).permutation(n).astype(np.float64) + 1.0
    return (perm / n).astype(f32).reshape(h, w)


def planted(w, h, seed):
    """distinct with about 20 % of the texels at 0.0 (background) and 10 % at 1.0"""
    plane = distinct(w, h, seed)
    u = np.random.default_rng([seed, 1]).random((h, w))
    plane[u < 0.2] = f32(0.0)
    plane[u >= 0.9] = f32(1.0)
    return plane


def blocks(w, h, seed, b, top):
    """One random value in (0, top) per b x b block, times (0.9 + 0.1 * distinct): occluders as large as the triangles of the
    test scenes and as near, so the cull's decisions depend on which texels it reads."""
    rng = np.random.default_rng([seed, 2])
    by, bx = (h + b - 1) // b, (w + b - 1) // b
    level = (top * rng.uniform(2.0 ** -10, 1.0, size=(by, bx))).astype(f32)
    coarse = np.repeat(np.repeat(level, b, axis=0), b, axis=1)[:h, :w]
    return (coarse * (f32(0.9) + f32(0.1) * distinct(w, h, seed))).astype(f32)


RECIPES = {
    "distinct": distinct,
    "planted": planted,
    "blocks4": lambda w, h, seed: blocks(w, h, seed, 4, 0.03),
}


# ------------------------------------------------------------------ the host's choice of kernels
HEAD_MAX_LEVELS = 4
GRID_MIN_TEXELS = 2304   # k_hiz_downsample builds the level behind the head only when it has more texels than this
TAIL_SMALL_TEXELS = 2304  # first tail level at most this: 256 threads, else 1024
LDS_A, LDS_B = 8192, 2304  # R3N_HIZ_LDS_A / R3N_HIZ_LDS_B (kernels_raster.h)


def launch_plan(w, h, samples=1):
    """Follows r3n_hi_z (rend3_amd/csrc/r3n.hip) and hiz_tail_body (csrc/kernels_raster.h): UPDATE IT WITH THEM.  Used only to
    assert that the tests' extents cover every path, never to judge a value.

    head_levels: levels k_hiz_head builds beyond level 0;  head_stop: why it stopped ("cap" = 4 levels, "mips" = the pyramid has
    no more, "odd" = the next source level has an odd or unit side);  mip0: where level 0 comes from without an injected plane;
    downsample: k_hiz_downsample runs;  tail_threads: None without k_hiz_tail;  tail: per tail level (level, placement) with
    placement "A" / "B" = kept in that LDS array, "miss_A" / "miss_B" = too large for the array whose turn it was."""
    mips = mip_count(w, h)
    n = 0
    stop = None
    while stop is None:
        if n >= HEAD_MAX_LEVELS:
            stop = "cap"
        elif n + 1 >= mips:
            stop = "mips"
        elif (w >> n) % 2 or (h >> n) % 2 or (w >> n) < 2 or (h >> n) < 2:
            stop = "odd"
        else:
            n += 1
    first = n + 1
    grid = False
    if first < mips:
        r, c = mip_shape(w, h, first)
        if r * c > GRID_MIN_TEXELS:
            grid = True
            first += 1
    threads, tail = None, []
    if first < mips:
        r, c = mip_shape(w, h, first)
        threads = 256 if r * c <= TAIL_SMALL_TEXELS else 1024
        to_a = True
        for k in range(first, mips):
            r, c = mip_shape(w, h, k)
            fits = r * c <= (LDS_A if to_a else LDS_B)
            tail.append((k, ("A" if to_a else "B") if fits else ("miss_A" if to_a else "miss_B")))
            to_a = not to_a
    return dict(head_levels=n, head_stop=stop, mip0="keys" if samples == 1 else "resolve", downsample=grid, tail_threads=threads,
                tail=tail)
