"""A plain numpy restatement of the object pass (rend3_amd/csrc/kernels_cull.h: frustum test, visible-object scan, work-list
scatter, uniform-bake set) and of the host logic that picks one of its three launch plans (rend3_amd/csrc/r3n.hip:
run_object_pass, chained_rounds, chained_pass_fits) -- and the worlds tests/test_object_pass.py and
tests/test_object_pass_gpu.py run through it.

The worlds are arrays, not per-object Python state: `records()` turns one into r3n_object128 rows that go up with ONE
r3n_objects_write, so a 2 M-slot world costs about a second.  A record's bounding sphere is host-computed INPUT of the ABI, so it is
chosen freely here, decoupled from the geometry: every object draws `ntri` copies of one small front-facing triangle (one shared
index run; first_index / index_count select any count), moved by one of PALETTE_N translations, so the triangle cull's verdict
depends on (palette entry, camera) alone and rasterising costs nothing."""
import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32

# kernels_cull.h; tests/test_object_pass.py reads the #defines as text and compares
FUSED_OBJECT_PASS_MAX = 1024
CHAINED_OBJECT_PASS_MAX_BLOCKS = 512
CHAINED_OBJECT_PASS_MAX_ROUNDS = 16
CHUNK_ITERS = 4
DEFINES = {"R3N_FUSED_OBJECT_PASS_MAX": FUSED_OBJECT_PASS_MAX, "R3N_CHAINED_OBJECT_PASS_MAX_BLOCKS": CHAINED_OBJECT_PASS_MAX_BLOCKS,
           "R3N_CHAINED_OBJECT_PASS_MAX_ROUNDS": CHAINED_OBJECT_PASS_MAX_ROUNDS, "R3N_CHUNK_ITERS": CHUNK_ITERS}
VIS_DRAWN, VIS_INSIDE = 1, 2
META_NTRI_MASK, META_KEY_SHIFT = 0x3FFFFFFF, 30
OPAQUE, CUTOUT, BLEND = 0, 1, 2


def _ceil_div(a, b):
    return (a + b - 1) // b


def launch_plan(capacity, one_call):
    """What the host launches for a camera's object pass over `capacity` slots: on the per-node frame (r3n_cull ->
    run_object_pass) or on the one-call frame (r3n_render_frame -> run_bake_and_object_pass while chained_pass_fits, else the
    per-node form).  `canonical` names the plan of the tri_base pass, which is run_object_pass on either path."""
    nblocks = _ceil_div(capacity, 256)
    node = "fused" if capacity <= FUSED_OBJECT_PASS_MAX else "three_launch"
    plan = dict(plan=node, canonical=node, scan_width=None, scan_iterations=None, rounds=None, grid=None, fits=None)
    if one_call:
        rounds = max(1, _ceil_div(nblocks, CHAINED_OBJECT_PASS_MAX_BLOCKS))
        plan["fits"] = capacity >= 1 and rounds <= CHAINED_OBJECT_PASS_MAX_ROUNDS
        if plan["fits"]:
            plan.update(plan="chained", rounds=rounds, grid=_ceil_div(nblocks, rounds))
    if "three_launch" in (plan["plan"], plan["canonical"]):
        plan.update(scan_width=64 if nblocks <= 64 else 1024, scan_iterations=1 if nblocks <= 64 else _ceil_div(nblocks, 1024))
    return plan


# ------------------------------------------------------------------ the object pass
def meta_words(recs, material_keys):
    """ObjSoA.meta of every record: (enabled ? index_count / 3 : 0) | Material::key() << 30 (a material index beyond the table
    reads key 0)."""
    recs = np.asarray(recs, dtype=u32)
    keys = np.asarray(material_keys, dtype=u32)
    mi = recs[:, 22]
    key = np.where(mi < len(keys), keys[np.minimum(mi, len(keys) - 1)], 0).astype(u32)
    ntri = np.where(recs[:, 29] != 0, recs[:, 21] // 3, 0).astype(u32)
    return ntri | (key << u32(META_KEY_SHIFT))


def flags_exact(planes, spheres, meta, owned):
    """The two vis_flags bits of every slot (object_visible), computed in float64: d = n . c + w >= -radius on all five planes.
    THE answer only where every product and sum is exact in f32 whatever the order (the exact tier below); NaN compares false."""
    pl = np.asarray(planes, dtype=f64).reshape(5, 4)
    s = np.asarray(spheres, dtype=f64).reshape(-1, 4)
    meta = np.asarray(meta, dtype=u32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((s[:, 0:1] * pl[:, 0] + s[:, 1:2] * pl[:, 1]) + s[:, 2:3] * pl[:, 2]) + pl[:, 3]
        inside = (d >= -s[:, 3:4]).all(axis=1)
    inside &= (meta & u32(META_NTRI_MASK)) != 0
    return flags_from_inside(inside, meta, owned)


def flags_from_inside(inside, meta, owned):
    """R3N_VIS_INSIDE: has triangles and passes the frustum test, whoever owns it; R3N_VIS_DRAWN: ... and this rank owns it or
    its key is blend (drawn by every rank)."""
    inside = np.asarray(inside).astype(bool)
    key = np.asarray(meta, dtype=u32) >> u32(META_KEY_SHIFT)
    drawn = inside & (np.asarray(owned, dtype=bool) | (key == BLEND))
    return (inside * VIS_INSIDE + drawn * VIS_DRAWN).astype(np.uint8)


def expected(meta, flags, verdict, prev=None):
    """What a camera's object pass + triangle cull must leave, from the flags of every slot and the triangle cull's verdict
    (per slot: all triangles of an object are the same triangle).  `prev`: None, or the dict this function returned for the
    camera's previous frame (the viewport with history; a world that has grown since is padded).
      tri_base   canonical: exclusive cumsum of ntri over the enabled slots
      pass       per canonical triangle: the object's drawn bit AND the verdict
      residual   pass AND NOT last frame's pass bit (objects not drawn last frame carry no history)
      calls      the six indirect calls' vertex counts: 3 x |pass|, 3 x |residual| per material key
      baked      the slots whose baked matrices are defined: inside now, or -- with history -- inside last frame"""
    meta = np.asarray(meta, dtype=u32)
    flags = np.asarray(flags, dtype=np.uint8)
    n = len(meta)
    ntri = (meta & u32(META_NTRI_MASK)).astype(np.int64)
    key = (meta >> u32(META_KEY_SHIFT)).astype(np.int64)
    tri_base = np.zeros(n, dtype=u32)
    tri_base[1:] = np.cumsum(ntri[:-1]).astype(u32)
    slot_pass = ((flags & VIS_DRAWN) != 0) & np.asarray(verdict, dtype=bool)
    slot_resid = slot_pass.copy()
    baked = (flags & VIS_INSIDE) != 0
    if prev is not None:
        m = len(prev["slot_pass"])
        assert m <= n and np.array_equal(prev["ntri"], ntri[:m]), "history: the slots keep their triangle counts"
        slot_resid[:m] &= ~prev["slot_pass"]
        baked = baked.copy()
        baked[:m] |= (prev["flags"] & VIS_INSIDE) != 0
        baked &= ntri != 0
    calls = np.zeros(6, dtype=np.int64)
    for k in range(3):
        calls[k] = 3 * ntri[slot_pass & (key == k)].sum()
        calls[3 + k] = 3 * ntri[slot_resid & (key == k)].sum()
    return dict(tri_base=tri_base, total=int(ntri.sum()), ntri=ntri, flags=flags, slot_pass=slot_pass,
                residual=np.repeat(slot_resid, ntri).astype(np.uint8), calls=calls, baked=baked,
                **{"pass": np.repeat(slot_pass, ntri).astype(np.uint8)})


# ------------------------------------------------------------------ geometry and cameras
MAX_NTRI = 5000
NTRI_VALUES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 2112, 5000)  # 2 048 triangles = 32 wave slots = 8 first-entry words: above it
#                                                                   write_first_entries goes wavefront-wide
TRIANGLE = np.array([(0.05, -0.05, 0.0), (-0.05, -0.05, 0.0), (0.0, 0.05, 0.0)], dtype=f32)  # front-facing for a LEFT viewport
INDICES = np.tile(np.arange(3, dtype=u32), MAX_NTRI)
BLEND_NTRI = 2  # blend-key objects draw a mesh of their own (the oracle's transparent pass takes the count from the mesh)
PALETTE_N = 64
TARGET = 128    # the frames are TARGET x TARGET
TIERS = ("exact", "random")


def palette(tier):
    """PALETTE_N translations: an 8 x 8 grid in x, y; the exact tier stays in the plane z = 0."""
    k = np.arange(PALETTE_N)
    t = np.zeros((PALETTE_N, 3), dtype=f32)
    t[:, 0] = (-0.7 + 0.2 * (k % 8)).astype(f32)
    t[:, 1] = (-0.7 + 0.2 * (k // 8)).astype(f32)
    if tier == "random":
        t[:, 2] = (0.25 * (k % 3)).astype(f32)
    return t


def cameras(tier, hm):
    """(view, projection) of frame 0 and frame 1.  Exact tier: identity view and a raw diagonal projection with dyadic entries --
    the five normalised planes are (+-1, 0, 0, 1/sx), (0, -+1, 0, 1/sy), (0, 0, -1, 1/sz), exactly.  Random tier: perspective."""
    if tier == "exact":
        m1 = hm.identity().copy()
        m1[0], m1[10] = 0.5, 0.25
        return [(hm.identity(), ("raw", hm.identity())), (hm.identity(), ("raw", m1))]
    return [(hm.look_at_lh((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1)),
            (hm.look_at_lh((1.5, 0.8, -3.2), (0.0, 0.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))]


EXACT_PLANES = [np.array([1, 0, 0, 1, -1, 0, 0, 1, 0, -1, 0, 1, 0, 1, 0, 1, 0, 0, -1, 1], dtype=f32),
                np.array([1, 0, 0, 2, -1, 0, 0, 2, 0, -1, 0, 1, 0, 1, 0, 1, 0, 0, -1, 4], dtype=f32)]

INSIDE_SPHERE = np.array([0.0, 0.0, 0.0, 0.5], dtype=f32)       # inside under all four cameras
OUTSIDE_SPHERE = np.array([900.0, 0.0, 0.0, 0.5], dtype=f32)    # outside under all four


def exact_specials():
    """(name, sphere) rows of the exact tier, for frame 0's planes (x, y in [-1 - r, 1 + r], z <= 1 + r).
    Ties d == -r on each of the five planes are INSIDE (the >= of object_visible); the same centre with the radius one ulp
    smaller is outside.  NaN / inf: a NaN distance or radius compares false -> outside; an infinite centre component gives
    inf x 0 = NaN on the planes that ignore it."""
    inf, nan = np.inf, np.nan
    rows = []
    r = f32(0.5)
    below = np.nextafter(r, f32(0.0))
    for name, c in (("left", (-1.5, 0.25, 0.0)), ("right", (1.5, -0.25, 0.125)), ("top", (0.0, 1.5, 0.0)), ("bottom", (0.125, -1.5, 0.0)),
                    ("near", (0.0, 0.0, 1.5))):
        rows.append((f"tie_{name}", (*c, r)))
        rows.append((f"ulp_outside_{name}", (*c, below)))
    rows += [("radius0_inside", (0.0, 0.0, 0.0, 0.0)), ("radius0_on_plane", (1.0, 0.0, 0.0, 0.0)), ("radius0_corner", (-1.0, 1.0, 1.0, 0.0)),
             ("radius0_outside", (1.125, 0.0, 0.0, 0.0)), ("far_corner", (1024.0, -1024.0, -1024.0, 2.0)), ("no_far_plane", (0.0, 0.0, -1024.0, 0.125)),
             ("negative_radius", (0.75, 0.0, 0.0, -0.5)), ("huge_radius", (1024.0, 1024.0, 1024.0, 2048.0)),
             ("nan_centre", (nan, 0.0, 0.0, 1.0)), ("nan_radius", (0.0, 0.0, 0.0, nan)), ("inf_centre", (inf, 0.0, 0.0, 1.0)),
             ("neg_inf_centre", (0.0, -inf, 0.0, 1.0)), ("inf_radius", (0.0, 0.0, 0.0, inf)), ("neg_inf_radius", (0.0, 0.0, 0.0, -inf)),
             ("inf_radius_far", (1000.0, 0.0, 0.0, inf)), ("inf_both", (inf, 0.0, 0.0, inf)), ("neg_zero", (-0.0, -0.0, -0.0, 0.0))]
    return [(n, np.array(s, dtype=f32)) for n, s in rows]


# ------------------------------------------------------------------ worlds
PATTERNS = ("mix", "tier", "all", "none", "first", "last")


def pattern_mask(capacity, pattern):
    """+1: the slot is forced drawn (INSIDE_SPHERE, enabled, triangles); -1: forced culled (far sphere, disabled or no triangles,
    in turn); 0: the tier's own sphere decides.  "mix" by 256-slot block b: b % 4 == 0 alternates all-drawn and all-culled
    64-slot waves, 1 is a drawn block, 3 a culled block, 2 is left to the tier."""
    i = np.arange(capacity)
    m = np.zeros(capacity, dtype=np.int8)
    if pattern == "mix":
        b, w = (i // 256) % 4, (i // 64) % 2
        m[(b == 0) & (w == 0)] = 1
        m[(b == 0) & (w == 1)] = -1
        m[b == 1] = 1
        m[b == 3] = -1
    elif pattern == "all":
        m[:] = 1
    elif pattern in ("none", "first", "last"):
        m[:] = -1
        if pattern == "first":
            m[0] = 1
        if pattern == "last":
            m[-1] = 1
    else:
        assert pattern == "tier", pattern
    return m


def build_world(capacity, tier, pattern="mix", seed=1, blend=False, big_ntri_every=1):
    """Arrays of a `capacity`-slot world.  ntri: NTRI_VALUES in turn on every `big_ntri_every`-th slot, 1 .. 3 elsewhere (a large
    world keeps its triangle count down, not its capacity); the objects above 2 048 triangles also sit in slot 0, in the last
    slot and three in one wave where the world has one.  Keys: opaque and cutout mixed; `blend`: every 61st slot is a blend object."""
    rng = np.random.default_rng([seed, capacity, TIERS.index(tier), PATTERNS.index(pattern)])
    n = capacity
    i = np.arange(n)
    mask = pattern_mask(n, pattern)
    if tier == "exact":
        centre = (rng.integers(-20, 21, size=(n, 3)) / 8.0).astype(f32)
        radius = rng.choice(np.array([0.0, 0.125, 0.25, 0.5, 1.0, 2.0], dtype=f32), size=n)
        spheres = np.concatenate([centre, radius[:, None]], axis=1).astype(f32)
        sp = exact_specials()
        free = np.flatnonzero(mask == 0)  # the special rows go where the pattern leaves the sphere alone
        at = free[(np.arange(len(sp)) * 7 + 3) % len(free)] if len(free) >= 8 * len(sp) else free[: len(sp)]
        for (_name, s), k in zip(sp, at):
            spheres[k] = s
    else:
        centre = rng.uniform((-4.0, -4.0, -5.0), (4.0, 4.0, 5.0), size=(n, 3))
        spheres = np.concatenate([centre, rng.uniform(0.0, 1.5, size=(n, 1))], axis=1).astype(f32)
    ntri = rng.integers(1, 4, size=n).astype(u32)
    sel = i % big_ntri_every == 0
    ntri[sel] = np.asarray(NTRI_VALUES, dtype=u32)[(i[sel] // big_ntri_every) % len(NTRI_VALUES)]
    enabled = rng.random(n) >= 0.06
    ntri[rng.random(n) < 0.04] = 0
    if pattern == "mix":
        # the wavefront-wide path of write_first_entries in the first and in the last slot, and three times in one wave
        for k, v in ((0, 5000), (n - 1, 2049)) + (((130, 2112), (131, 2049), (160, 5000)) if n > 192 else ()):
            ntri[k], mask[k] = v, 1
    cull_kind = i % 3
    spheres[mask == 1] = INSIDE_SPHERE
    enabled[mask == 1] = True
    ntri[(mask == 1) & (ntri == 0)] = 1
    spheres[(mask == -1) & (cull_kind == 0)] = OUTSIDE_SPHERE
    enabled[(mask == -1) & (cull_kind == 1)] = False
    ntri[(mask == -1) & (cull_kind == 2)] = 0
    spheres[(mask == -1) & (cull_kind == 2)] = INSIDE_SPHERE  # no triangles: not inside whatever the sphere says
    material = rng.integers(0, 2, size=n).astype(u32)  # 0 opaque, 1 cutout
    if blend:
        b = i % 61 == 5
        material[b] = BLEND
        ntri[b] = BLEND_NTRI
        enabled[b] = True
        spheres[b] = np.where((i[b] % 2 == 0)[:, None], INSIDE_SPHERE, OUTSIDE_SPHERE)
    return dict(capacity=n, tier=tier, pattern=pattern, spheres=np.ascontiguousarray(spheres), ntri=ntri, enabled=enabled,
                material=material, pal=rng.integers(0, PALETTE_N, size=n), big_ntri_every=big_ntri_every)


def grow_world(world, capacity, seed=2):
    """`world` with a tail of new slots up to `capacity`; the old slots keep their records."""
    tail = build_world(capacity, world["tier"], world["pattern"], seed=seed, big_ntri_every=world["big_ntri_every"])
    n = world["capacity"]
    out = dict(world, capacity=capacity)
    for k in ("spheres", "ntri", "enabled", "material", "pal"):
        out[k] = np.concatenate([world[k], tail[k][n:]])
    return out


def records(world, mesh, blend_mesh=None, first=0):
    """r3n_object128 rows (32 words) of the world's slots [first, capacity).  `mesh`: the renderer's mesh record of the shared
    index run (first_index, attr_off), `blend_mesh` of the blend objects' mesh."""
    sl = slice(first, world["capacity"])
    n = world["capacity"] - first
    rec = np.zeros((n, 32), dtype=u32)
    rf = rec.view(f32)
    rf[:, 0] = rf[:, 5] = rf[:, 10] = rf[:, 15] = 1.0
    rf[:, 12:15] = palette(world["tier"])[world["pal"][sl]]
    rf[:, 16:20] = world["spheres"][sl]
    rec[:, 20] = mesh.first_index
    rec[:, 21] = 3 * world["ntri"][sl]
    rec[:, 22] = world["material"][sl]
    rec[:, 23:29] = np.asarray(mesh.attr_off, dtype=u32)
    is_blend = world["material"][sl] == BLEND
    if is_blend.any():
        rec[is_blend, 20] = blend_mesh.first_index
        rec[is_blend, 23:29] = np.asarray(blend_mesh.attr_off, dtype=u32)
    rec[:, 29] = world["enabled"][sl]
    return rec


def setup_renderer(r, mk):
    """The shared geometry and the three materials (index == key) on an oracle or product renderer; returns (mesh, blend mesh)."""
    m = r.add_mesh(TRIANGLE, INDICES, mesh_handedness=0)
    mb = r.add_mesh(TRIANGLE, INDICES[: 3 * BLEND_NTRI], mesh_handedness=0)
    r.add_material(mk(albedo=(0.2, 0.6, 0.9, 1.0), albedo_mode="value", unlit=True), OPAQUE)
    r.add_material(mk(albedo=(0.9, 0.5, 0.1, 1.0), albedo_mode="value", unlit=True, cutout=0.5), CUTOUT)
    r.add_material(mk(albedo=(0.3, 0.9, 0.3, 0.5), albedo_mode="value", unlit=True), BLEND)
    return r.meshes[m], r.meshes[mb]


MATERIAL_KEYS = np.array([OPAQUE, CUTOUT, BLEND], dtype=np.uint8)


def load_oracle(o, world, meshes):
    """The world's records as the oracle's object buffer (any capacity: it is an array); blend objects get the bookkeeping
    the transparent pass sorts by."""
    recs = records(world, *meshes)
    o.objects = recs
    o.capacity = world["capacity"]
    o.object_meta = {int(h): dict(mesh=1, material=BLEND, enabled=True, location=recs[h].view(f32)[16:19].copy())
                     for h in np.flatnonzero((world["material"] == BLEND) & world["enabled"])}
    return recs


# ------------------------------------------------------------------ the triangle cull's verdict, from the oracle
def palette_world(tier):
    return dict(capacity=PALETTE_N, tier=tier, pattern="all", spheres=np.tile(INSIDE_SPHERE, (PALETTE_N, 1)),
                ntri=np.ones(PALETTE_N, dtype=u32), enabled=np.ones(PALETTE_N, dtype=bool),
                material=np.zeros(PALETTE_N, dtype=u32), pal=np.arange(PALETTE_N))


_VERDICTS = {}
LIGHT = {"exact": dict(color=(1, 1, 1), intensity=1.0, direction=(0.1, -0.2, -1.0), distance=4.0, resolution=128),
         "random": dict(color=(1, 1, 1), intensity=1.0, direction=(0.1, -0.2, -1.0), distance=12.0, resolution=128)}


def verdicts(tier, zero_plane=False, light=False):
    """verdict[k][palette entry]: does the entry's triangle pass the oracle's triangle cull in frame k of a world of one object
    per palette entry, over three frames with camera 0, 1, 0 -- so verdict[c] is camera c's for c in (0, 1), and frames 1 and 2
    cull against the pyramid of everything the palette can draw.  `zero_plane`: against an all-zero Hi-Z pyramid instead (it
    occludes nothing).  A world that draws a SUBSET of the palette's triangles builds a pyramid between the two (the depth plane
    is a MAX over what is drawn, a level a MIN over texels, and a triangle is rejected when its depth is below the level's
    value): where the two verdicts agree -- tests/test_object_pass.py asserts it -- the verdict holds in every such world, with
    or without history.  `light`: with LIGHT[tier] in the world, the verdicts of its shadow view instead (no Hi-Z there)."""
    if (tier, zero_plane, light) not in _VERDICTS:
        from oracle import host as oh
        from oracle.world import OracleRenderer, material_record
        o = OracleRenderer(oh.LEFT, f32(1.0))
        load_oracle(o, palette_world(tier), setup_renderer(o, material_record))
        if light:
            o.add_directional_light(**LIGHT[tier])

        def hook(what, buf, **_kw):
            if what == "pass1_depth" and zero_plane:
                buf[:] = 0.0
        out = []
        cams = cameras(tier, oh)
        for view, proj in (cams[0], cams[1], cams[0]):
            o.set_camera_data(view, proj)
            fo = o.render(TARGET, TARGET, exchange=hook)
            out.append((fo["shadows"][0] if light else fo)["pass"][:PALETTE_N].astype(bool))
        _VERDICTS[(tier, zero_plane, light)] = out
    return _VERDICTS[(tier, zero_plane, light)]


# ------------------------------------------------------------------ the oracle's object-level functions on a record array
class NoMesh:
    """records() for the calls that read no geometry (r3o_frustum_cull, r3o_uniform_bake)"""
    first_index, attr_off = 0, [0] * 6


def oracle_header(view, proj, capacity, camera=None, shadow_index=None, size=TARGET):
    from oracle import host as oh
    from oracle.lib import get as get_lib
    cam = oh.CameraState(view, proj, oh.LEFT, f32(1.0)) if camera is None else camera
    return oh.camera_header(cam, shadow_index, (size, size), 1, capacity, get_lib())


def oracle_inside(hdr, recs):
    """r3o_frustum_cull: enabled, has a triangle, sphere passes the five planes"""
    from oracle.lib import get as get_lib
    lib = get_lib()
    out = np.zeros(len(recs), dtype=np.uint8)
    lib.r3o_frustum_cull(lib.ptr(hdr), lib.ptr(np.ascontiguousarray(recs)), lib.ptr(out))
    return out.astype(bool)


def oracle_baked(hdr, recs):
    """r3o_uniform_bake: model_view and model_view_proj of every enabled slot, (capacity, 32) f32"""
    from oracle.lib import get as get_lib
    lib = get_lib()
    out = np.zeros((len(recs), 32), dtype=f32)
    lib.r3o_uniform_bake(lib.ptr(hdr), lib.ptr(np.ascontiguousarray(recs)), lib.ptr(out))
    return out


# ------------------------------------------------------------------ the capacities the GPU tests run
# per-node frame (R3N_FRAME_NODES=1: run_object_pass) and one-call frame (r3n_render_frame: the chained pass while it fits)
NODE_CAPACITIES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16_384, 16_385, 262_144, 262_145)
ONE_CALL_CAPACITIES = (1, 255, 256, 257, 1024, 1025, 131_072, 131_073, 262_145, 524_289, 1_966_081, 2_097_152, 2_097_153)
BOUNDARY_CAPACITIES = (1025, 16_385, 131_073, 262_145, 2_097_153)  # the first capacity of every plan / scan / rounds change
ORACLE_FRAME_MAX = 4096  # worlds up to here are also compared against a whole oracle frame


def big_ntri_every(capacity):
    """a world's triangle count stays below about three million: the large counts thin out as the world grows"""
    return 1 if capacity <= 257 else 8 if capacity <= ORACLE_FRAME_MAX else 64 if capacity <= 300_000 else 4096
