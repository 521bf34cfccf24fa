"""A plain numpy restatement of the triangle cull (rend3_amd/csrc/kernels_cull.h k_triangle_cull): the decision of
cull.wgsl:264-324 with the Hi-Z read of cull.wgsl:243-262 as DESIGN.md states the contract, the sets and the lists a camera's cull
must leave, and the launch structure that produces them.  Nothing of the product or of oracle/ is imported.

The arithmetic is f32, ONE operation per numpy operation: the product is compiled without contraction, so every product, sum and
quotient rounds once, in the order written here.  np.fmin / np.fmax ignore a NaN operand as fminf / fmaxf do, np.rint rounds ties
to even as WGSL's round() does.

  verdict()          pass / reject of every triangle of an array
  trace()            the same with every intermediate and the rule that decided
  expected_lists()   a frame's pass set, residual set and, per material key, the entries each list must hold
  slot_plan()        wave slots, pairs and singles, chunks, sub-lists and loop trips of the launch that culls a list of objects"""
import os
import re

import numpy as np

f32, u32, i64 = np.float32, np.uint32, np.int64
POSITIVE_AREA_VISIBLE, MULTISAMPLED = 1, 2
INVALID = 0xFFFFFFFF
OPAQUE, CUTOUT, BLEND = 0, 1, 2

# the launch structure's constants; tests/test_triangle_cull.py reads the sources as text and compares
CHUNK_ITERS = 4        # wave slots a wavefront owns in a chunk
CHUNK_WAVES = 16       # wave slots of a chunk: four wavefronts x CHUNK_ITERS
SUBQ = 32              # sub-lists per (list, material key): a chunk appends to sub-list chunk % SUBQ
GRID_CAP = 4096        # blocks of the persistent launch: block b takes chunks b, b + grid, ...
RULES = ("backface", "rint_x", "rint_y", "shadow", "occluded", "visible")


def source_constants():
    """{name: [values found]} as the sources spell them"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    def read(*p):
        return open(os.path.join(root, *p)).read()
    cull, hip, hdr = read("rend3_amd", "csrc", "kernels_cull.h"), read("rend3_amd", "csrc", "r3n.hip"), read("include", "r3n.h")
    out = {"CHUNK_ITERS": [int(v) for v in re.findall(r"^#define\s+R3N_CHUNK_ITERS\s+(\d+)u?\b", cull, flags=re.M)],
           "SUBQ": [int(v) for v in re.findall(r"^#define\s+R3N_SUBQ\s+(\d+)u?\b", hdr, flags=re.M)],
           "GRID_CAP": [int(v) for v in re.findall(r"grid = std::max\(1u, std::min\(chunks, (\d+)u\)\)", hip)]}
    m = re.findall(r"^#define\s+R3N_CHUNK_WAVES\s+\((\d+)u \* R3N_CHUNK_ITERS\)", cull, flags=re.M)
    out["CHUNK_WAVES"] = [int(v) * c for v in m for c in out["CHUNK_ITERS"]]
    return out


# ------------------------------------------------------------------ the decision
def hiz_desc(width, height):
    """the pyramid's shape: levels max(d >> k, 1) of a width x height plane, concatenated, level 0 first"""
    mips = int(max(width, height)).bit_length()
    off, at = [], 0
    for k in range(mips):
        off.append(at)
        at += max(width >> k, 1) * max(height >> k, 1)
    return dict(width=int(width), height=int(height), mips=mips, offsets=np.asarray(off, dtype=i64), total=at)


def ceil_log2_ge1(x):
    """ceil(log2(max(x, 1))) from the exponent bits; NaN -> 0, +inf -> 1000"""
    x = np.fmax(np.asarray(x, dtype=f32), f32(1.0))
    b = x.view(u32).astype(i64)
    e = (b >> 23) & 0xFF
    l = e - 127 + ((b & 0x7FFFFF) != 0)
    return np.where(e == 0xFF, 1000, l).astype(i64)


def clamp_texel(v, dim):
    """float -> texel index: negative or NaN -> 0, at or above dim - 1 -> dim - 1, else truncated"""
    v = np.asarray(v, dtype=f32)
    dim = np.asarray(dim, dtype=i64)
    top = (dim - 1).astype(f32)
    ok = v >= f32(0.0)
    high = ok & (v >= top)
    mid = np.where(ok & ~high, v, f32(0.0)).astype(i64)
    return np.where(high, dim - 1, mid)


def trace(flags, shadow, resolution, mvp, positions, pyramid=None, desc=None):
    """Every intermediate of the decision for triangles positions[n, 3 vertices, xyz] under the column-major matrix `mvp` (16
    floats, or one row of 16 per triangle).  `pyramid` / `desc` (hiz_desc): the viewport's Hi-Z chain; a shadow view reads none.
    Returns arrays over the triangles: det, smin / smax [n, 2], longest, mip, lx, ly, hx, hy, occ, depth, rule (index into RULES),
    visible."""
    pos = np.asarray(positions, dtype=f32).reshape(-1, 3, 3)
    n = len(pos)
    m = np.broadcast_to(np.asarray(mvp, dtype=f32).reshape(-1, 16), (n, 16))
    with np.errstate(all="ignore"):
        x, y, z = pos[:, :, 0], pos[:, :, 1], pos[:, :, 2]
        # clip-space point, row r: ((c0 * x + c1 * y) + c2 * z) + c3
        p = np.stack([((m[:, r, None] * x + m[:, 4 + r, None] * y) + m[:, 8 + r, None] * z) + m[:, 12 + r, None] for r in range(4)], axis=2)
        ax, ay, az = p[:, 0, 0], p[:, 0, 1], p[:, 0, 3]
        bx, by, bz = p[:, 1, 0], p[:, 1, 1], p[:, 1, 3]
        cx, cy, cz = p[:, 2, 0], p[:, 2, 1], p[:, 2, 3]
        det = (ax * (by * cz - cy * bz) - bx * (ay * cz - cy * az)) + cx * (ay * bz - by * az)
        back = det <= f32(0.0) if flags & POSITIVE_AREA_VISIBLE else det >= f32(0.0)
        ndc = p[:, :, :3] / p[:, :, 3:4]
        mn = np.fmin(ndc[:, 0, :2], np.fmin(ndc[:, 1, :2], ndc[:, 2, :2]))
        mx = np.fmax(ndc[:, 0, :2], np.fmax(ndc[:, 1, :2], ndc[:, 2, :2]))
        half = np.asarray(resolution, dtype=f32) / f32(2.0)
        smin = (mn + f32(1.0)) * half
        smax = (mx + f32(1.0)) * half
        same = np.rint(smin) == np.rint(smax)
        if flags & MULTISAMPLED:
            same = np.zeros_like(same)
        rule = np.full(n, RULES.index("visible"), dtype=i64)
        out = dict(det=det, smin=smin, smax=smax, clip=p, ndc=ndc)
        if shadow:
            rule[:] = RULES.index("shadow")
        else:
            mintc = (mn + f32(1.0)) / f32(2.0)
            maxtc = (mx + f32(1.0)) / f32(2.0)
            mintc[:, 1] = f32(1.0) - mintc[:, 1]
            maxtc[:, 1] = f32(1.0) - maxtc[:, 1]
            uv = (maxtc + mintc) / f32(2.0)
            edges = smax - smin
            longest = np.fmax(edges[:, 0], edges[:, 1])
            mip = np.minimum(ceil_log2_ge1(longest), desc["mips"] - 1)
            depth = np.fmax(np.fmax(ndc[:, 0, 2], ndc[:, 1, 2]), ndc[:, 2, 2])
            mw = np.maximum(desc["width"] >> mip, 1)
            mh = np.maximum(desc["height"] >> mip, 1)
            px = uv[:, 0] * mw.astype(f32) - f32(0.5)
            py = uv[:, 1] * mh.astype(f32) - f32(0.5)
            lx = clamp_texel(np.fmax(np.floor(px), f32(0.0)), mw)
            ly = clamp_texel(np.fmax(np.floor(py), f32(0.0)), mh)
            hx = clamp_texel(np.fmin(np.ceil(px), mw.astype(f32) - f32(1.0)), mw)
            hy = clamp_texel(np.fmin(np.ceil(py), mh.astype(f32) - f32(1.0)), mh)
            tex = np.asarray(pyramid, dtype=f32).reshape(-1)
            assert len(tex) == desc["total"]
            base = desc["offsets"][mip]
            texels = np.stack([tex[base + ly * mw + lx], tex[base + ly * mw + hx], tex[base + hy * mw + lx], tex[base + hy * mw + hx]], axis=1)
            occ = np.fmin(np.fmin(np.fmin(texels[:, 0], texels[:, 1]), texels[:, 2]), texels[:, 3])
            rule[depth < occ] = RULES.index("occluded")
            out.update(uv=uv, longest=longest, mip=mip, depth=depth, mw=mw, mh=mh, px=px, py=py, lx=lx, ly=ly, hx=hx, hy=hy,
                       texels=texels, occ=occ)
        rule[same[:, 1]] = RULES.index("rint_y")
        rule[same[:, 0]] = RULES.index("rint_x")
        rule[back] = RULES.index("backface")
    out.update(rule=rule, visible=(rule == RULES.index("visible")) | (rule == RULES.index("shadow")))
    return out


def verdict(flags, shadow, resolution, mvp, positions, pyramid=None, desc=None):
    """does each triangle pass the cull: bool[n]"""
    return trace(flags, shadow, resolution, mvp, positions, pyramid, desc)["visible"]


# ------------------------------------------------------------------ sets and lists
def material_key(material_index, keys):
    """the key byte of a slot's material; an index beyond the table reads 0; a byte above 2 counts as 2"""
    mi = np.asarray(material_index, dtype=i64)
    keys = np.asarray(keys, dtype=i64)
    k = np.where(mi < len(keys), keys[np.minimum(mi, len(keys) - 1)], 0)
    return np.minimum(k, 2)


def expected_lists(ntri, key, drawn, passes, shadow=False, prev=None):
    """What a camera's cull must leave.  Per object slot: `ntri` (0 for a disabled slot), `key` (material_key) and `drawn` (the
    object pass listed it); `passes`: the decision per canonical triangle -- (object o, triangle t) sits at tri_base[o] + t, tri_base
    the exclusive sum of ntri -- read only where the object is drawn.  `prev`: what this function returned for the camera's last
    frame, None without history.  A slot has history when it was drawn last frame with the triangle count it has now (a slot beyond
    last frame's capacity, not drawn then, or rewritten with another count since has none): all of its passing triangles are
    residual.  Shadow views keep no residual list.
      pass, residual    u8 per canonical triangle
      predicted[k]      (object, triangle) rows the predicted list holds under key k, sorted; residual_list[k] likewise
      calls             the six vertex counts"""
    ntri = np.asarray(ntri, dtype=i64)
    key = np.asarray(key, dtype=i64)
    drawn = np.asarray(drawn, dtype=bool) & (ntri > 0)
    n = len(ntri)
    tri_base = np.zeros(n, dtype=i64)
    tri_base[1:] = np.cumsum(ntri[:-1])
    total = int(ntri.sum())
    obj = np.repeat(np.arange(n), ntri)
    tri = np.arange(total) - tri_base[obj]
    ps = np.asarray(passes, dtype=bool)[:total] & drawn[obj]
    before = np.zeros(total, dtype=bool)
    if prev is not None and not shadow:
        m = min(n, len(prev["ntri"]))
        has = np.zeros(n, dtype=bool)
        has[:m] = prev["drawn"][:m] & (prev["ntri"][:m] == ntri[:m])
        sel = has[obj]
        before[sel] = prev["pass"][prev["tri_base"][obj[sel]] + tri[sel]] != 0
    rs = ps & ~before & (not shadow)
    rows = np.stack([obj, tri], axis=1).astype(u32)
    predicted = [rows[ps & (key[obj] == k)] for k in range(3)]
    resid = [rows[rs & (key[obj] == k)] for k in range(3)]
    calls = np.array([3 * len(r) for r in predicted + resid], dtype=i64)
    return dict(ntri=ntri, key=key, drawn=drawn, tri_base=tri_base, total=total, object=obj, triangle=tri, residual=rs.astype(np.uint8),
                predicted=predicted, residual_list=resid, calls=calls, **{"pass": ps.astype(np.uint8)})


# ------------------------------------------------------------------ the launch
PAIR_FIRST, PAIR_SECOND, SINGLE = "pair first", "pair second", "single"
WHY_LAST_ITERATION, WHY_NEXT_OBJECT, WHY_LAST_SLOT = "it == 3", "the next slot is another object's", "the last slot"


def slot_plan(ntri_of_drawn_objects, grid_cap=GRID_CAP):
    """The launch that culls the drawn objects (in slot order, each with its triangle count >= 1).  Object e owns the wave slots
    [wave_start[e], wave_start[e + 1]), 64 triangles each; chunk c holds the wave slots [16 c, 16 c + 16), wavefront v of its block
    the four from 16 c + 4 v; a wavefront walks its four slots taking two at a time when the next one is its own (it + 1 < 4) and
    the same object's, else one.  Chunk c is handled by block c % grid in that block's trip c // grid and appends to sub-list
    c % SUBQ.  Returns arrays over the wave slots of all chunks (the last chunk's slots beyond total_waves are padding):
      wave_start[e], total_waves, nchunks, grid
      entry, wrel       the object (index into the drawn list) and the slot's number inside it; -1 for padding
      kind              PAIR_FIRST / PAIR_SECOND / SINGLE; None for padding       why: for a single, the reason
      lanes             triangles in the slot (1 .. 64; 0 for padding)
      chunk, sublist, trip, block, wavefront, iteration"""
    nt = np.asarray(ntri_of_drawn_objects, dtype=i64)
    assert (nt >= 1).all()
    waves = (nt + 63) // 64
    wave_start = np.zeros(len(nt) + 1, dtype=i64)
    wave_start[1:] = np.cumsum(waves)
    total = int(wave_start[-1])
    nchunks = (total + CHUNK_WAVES - 1) // CHUNK_WAVES
    grid = max(1, min(nchunks, grid_cap))
    nslots = nchunks * CHUNK_WAVES
    w = np.arange(nslots)
    entry = np.full(nslots, -1, dtype=i64)
    entry[:total] = np.repeat(np.arange(len(nt)), waves)
    wrel = np.where(entry >= 0, w - wave_start[np.maximum(entry, 0)], -1)
    lanes = np.where(entry >= 0, np.minimum(nt[np.maximum(entry, 0)] - 64 * wrel, 64), 0)
    it = w % CHUNK_ITERS
    kind = np.full(nslots, None, dtype=object)
    why = np.full(nslots, None, dtype=object)
    same_next = np.zeros(nslots, dtype=bool)
    same_next[:-1] = (entry[:-1] >= 0) & (entry[1:] == entry[:-1])
    for g in range(0, nslots, CHUNK_ITERS):  # one wavefront's walk
        i = 0
        while i < CHUNK_ITERS:
            s = g + i
            if entry[s] < 0:
                i += 1
            elif i + 1 < CHUNK_ITERS and same_next[s]:
                kind[s], kind[s + 1] = PAIR_FIRST, PAIR_SECOND
                i += 2
            else:
                kind[s] = SINGLE
                why[s] = WHY_LAST_ITERATION if i + 1 == CHUNK_ITERS else WHY_LAST_SLOT if s + 1 == total else WHY_NEXT_OBJECT
                i += 1
    chunk = w // CHUNK_WAVES
    return dict(wave_start=wave_start, total_waves=total, nchunks=nchunks, grid=grid, entry=entry, wrel=wrel, kind=kind, why=why,
                lanes=lanes, chunk=chunk, sublist=chunk % SUBQ, trip=chunk // grid, block=chunk % grid,
                wavefront=(w % CHUNK_WAVES) // CHUNK_ITERS, iteration=it, continues=same_next)


def describe_slot(plan, s):
    """a wave slot in the plan's terms, for failure messages"""
    k = plan["kind"][s]
    return (f"wave slot {s} ({'padding' if k is None else k}{'' if plan['why'][s] is None else ': ' + plan['why'][s]}), chunk {int(plan['chunk'][s])} "
            f"(block {int(plan['block'][s])}, trip {int(plan['trip'][s])}, sub-list {int(plan['sublist'][s])}), wavefront {int(plan['wavefront'][s])}, "
            f"iteration {int(plan['iteration'][s])}")
