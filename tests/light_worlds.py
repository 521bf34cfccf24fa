"""
The stage and the light sets of tests/test_lights.py (oracle alone) and tests/test_lights_gpu.py (HIP against the oracle): directed
inputs for the fragment stage's light loop -- the light limits, and the edge of every shortcut the kernel takes where the oracle
evaluates every light in full (kernels_shade.h fragment_stage, stage_lights, shadow_pcf5 / shadow_pcf5_general).

Like tests/scenes.py every builder takes a renderer `r` of the Renderer-shaped API, its host-math module `hm` and its material
constructor `mk`; the light sets are plain data (lists of keyword dicts), so both renderers are given the same numbers.

The stage (about 1 500 triangles; left-handed): a tessellated 8 x 8 floor spanning +-6 at y = 0; four icospheres of subdivision 2
at y = 1.2 -- roughness 0.5, metallic with roughness 0.3, roughness 0.0 (the nl == 0 shortcut is not valid there: D * V is
0 * inf), ao = 0.0 (shadow * ao == 0 whatever the shadow); a box with ao = 0.5; a box of albedo 3e30 (the magnitude sum of the
pixel inputs passes the bound below which a zero term may be skipped); optionally a slab above everything and a near-mirror
quad (build_stage).  The ao = 0 materials are emissive: a pixel whose every light term is zero shows the emission, one that a
0 * inf poisoned shows ambient * albedo -- without emission both would show ambient * albedo and nothing could be told apart.
"""
import math

import numpy as np

from scenes import BLEND, CUTOUT, OPAQUE, box, grid_plane, icosphere

f32 = np.float32
W, H = 128, 80
AMBIENT = (0.1, 0.1, 0.1, 1.0)
CLEAR = (0.02, 0.03, 0.05, 1.0)
EYE, TARGET = (0.0, 4.0, -9.0), (0.0, 1.0, 0.0)
HUGE_ALBEDO = 3e30

ZERO_BELOW_DIRECTION = (-1.0, 0.45, 0.15)
MIRROR_CENTRE, MIRROR_ALBEDO = (4.5, 1.2, -4.0), (0.5, 0.5, 0.5)

SPHERES = ("rough05", "metal", "rough0", "ao0")
SPHERE_X = (-4.5, -1.5, 1.5, 4.5)


def aspect():
    return f32(W) / f32(H)


def set_camera(r, hm):
    r.set_camera_data(hm.look_at_lh(EYE, TARGET, (0, 1, 0)), ("perspective", 60.0, 0.1))


def build_stage(r, hm, mk, textured=False, blend=False, cutout=False, slab=False, mirror=False):
    """Returns {name: object handle}.  textured: the floor samples an 8 x 8 RGBA8 albedo texture (n_textures > 0: the TEX
    instantiations, the per-class kernels); blend: two translucent quads in front of the spheres (unsplit four-sample resolve,
    k_blend_apply's own walk of the light lists); cutout: the first sphere's material is a cutout one; slab: a slab at y = 4.4 over
    the whole stage; mirror: a quad with ao = 0, roughness 0.1 and reflectance 1.4e15 (f0 = 3.1e29), turned so that the highlight of
    the zero_paths light from below lies on it as seen from the camera.  In the highlight (fd + fr) * colour overflows f32 already
    for a light colour of 1e6, which the kernel takes for harmless: the term is inf * 0 = NaN, not +0, and a kernel may skip it
    only if it also bounds f0 (test_lights.py holds the pixel counts)."""
    out = {}
    p, i, n = grid_plane(8, 6.0)
    if textured:
        rng = np.random.default_rng(8)
        img = rng.integers(40, 256, (8, 8, 4), dtype=np.uint8)
        img[..., 3] = 255
        tex = r.add_texture_2d(img, srgb=True, mip_count="maximum", mip_source="generated")
        uv = (p[:, [0, 2]] * f32(0.25) + f32(0.5)).astype(f32)
        floor_mesh = r.add_mesh(p, i, normals=n, uv0=uv)
        floor_mat = r.add_material(mk(albedo_mode="texture", albedo_texture=tex, roughness=0.6), OPAQUE)
    else:
        floor_mesh = r.add_mesh(p, i, normals=n)
        floor_mat = r.add_material(mk(albedo=(0.8, 0.8, 0.8, 1.0), albedo_mode="value", roughness=0.6), OPAQUE)
    out["floor"] = r.add_object(floor_mesh, floor_mat, hm.identity())

    p, i, n = icosphere(2)
    i = i.reshape(-1, 3)[:, ::-1].reshape(-1)  # outward faces clockwise: front faces of a left-handed renderer
    sphere = r.add_mesh(p, i, normals=n)
    first = mk(albedo=(0.9, 0.5, 0.3, 0.75), albedo_mode="value", roughness=0.5, cutout=0.5) if cutout else \
        mk(albedo=(0.9, 0.5, 0.3, 1.0), albedo_mode="value", roughness=0.5)
    mats = [
        r.add_material(first, CUTOUT if cutout else OPAQUE),
        r.add_material(mk(albedo=(0.9, 0.8, 0.4, 1.0), albedo_mode="value", roughness=0.3, metallic=1.0), OPAQUE),
        r.add_material(mk(albedo=(0.4, 0.7, 0.9, 1.0), albedo_mode="value", roughness=0.0), OPAQUE),
        r.add_material(mk(albedo=(0.5, 0.9, 0.5, 1.0), albedo_mode="value", roughness=0.5, ao=0.0, emissive=(0.3, 0.2, 0.1)), OPAQUE),
    ]
    for name, x, mat in zip(SPHERES, SPHERE_X, mats):
        out[name] = r.add_object(sphere, mat, hm.translation((x, 1.2, 0.5)))

    p, i, n = box()
    cube = r.add_mesh(p, i, normals=n)
    half_ao = r.add_material(mk(albedo=(0.8, 0.4, 0.8, 1.0), albedo_mode="value", roughness=0.4, ao=0.5), OPAQUE)
    huge = r.add_material(mk(albedo=(HUGE_ALBEDO, HUGE_ALBEDO, HUGE_ALBEDO, 1.0), albedo_mode="value", roughness=0.5), OPAQUE)
    out["ao05"] = r.add_object(cube, half_ao, hm.mat4_mul(hm.translation((-2.5, 0.6, -3.0)), hm.scale((0.6, 0.6, 0.6))))
    out["huge"] = r.add_object(cube, huge, hm.mat4_mul(hm.translation((2.5, 0.6, -3.0)), hm.scale((0.6, 0.6, 0.6))))
    if slab:
        slab_mat = r.add_material(mk(albedo=(0.6, 0.6, 0.7, 1.0), albedo_mode="value", roughness=0.7), OPAQUE)
        out["slab"] = r.add_object(cube, slab_mat, hm.mat4_mul(hm.translation((0.0, 4.4, 0.0)), hm.scale((6.5, 0.1, 6.5))))
    if mirror:
        d = np.array(ZERO_BELOW_DIRECTION, dtype=np.float64)
        centre = np.array(MIRROR_CENTRE, dtype=np.float64)
        to_light = -d / np.linalg.norm(d)
        to_eye = (np.array(EYE, dtype=np.float64) - centre) / np.linalg.norm(np.array(EYE, dtype=np.float64) - centre)
        nrm = (to_eye + to_light) / np.linalg.norm(to_eye + to_light)  # the half vector at the centre
        t = np.cross(nrm, (0.0, 1.0, 0.0))
        t /= np.linalg.norm(t)
        b = np.cross(nrm, t)
        pos = np.array([centre - t - b, centre + t - b, centre + t + b, centre - t + b], dtype=f32)
        mesh = r.add_mesh(pos, [0, 1, 2, 0, 2, 3], normals=np.tile(nrm.astype(f32), (4, 1)))
        mat = r.add_material(mk(albedo=MIRROR_ALBEDO + (1.0,), albedo_mode="value", roughness=0.1, reflectance=1.4e15, ao=0.0,
                                emissive=(2.0, 1.5, 1.0)), OPAQUE)
        out["mirror"] = r.add_object(mesh, mat, hm.identity())
    if blend:
        quad = r.add_mesh([(-1, -1, 0), (-1, 1, 0), (1, 1, 0), (1, -1, 0)], [0, 1, 2, 0, 2, 3], normals=[(0, 0, -1)] * 4)
        for k, (x, col) in enumerate(((-3.0, (0.9, 0.2, 0.2, 0.5)), (3.0, (0.2, 0.3, 0.9, 0.35)))):
            mat = r.add_material(mk(albedo=col, albedo_mode="value", roughness=0.4), BLEND)
            out[f"quad{k}"] = r.add_object(quad, mat, hm.mat4_mul(hm.translation((x, 1.3, -1.5)), hm.scale((1.6, 1.1, 1.0))))
    return out


def apply_lights(r, dirs, points):
    for d in dirs:
        r.add_directional_light(**d)
    for p in points:
        r.add_point_light(**p)


def _colour(i, a, b, c):
    """a distinct colour per index: no two lights of a set can be swapped, none dropped, without the frame changing"""
    return (0.25 + 0.75 * ((i * a) % 7) / 6.0, 0.25 + 0.75 * ((i * b) % 5) / 4.0, 0.25 + 0.75 * ((i * c) % 3) / 2.0)


# ------------------------------------------------------------------ counts
COUNT_PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (3, 2), (5, 255), (15, 256), (16, 0), (16, 256)]
DIR_RESOLUTIONS = (128, 64, 64, 32)


def counts(n_dir, n_point):
    """n_dir directional lights spread over the upper hemisphere, resolutions cycling 128, 64, 64, 32 (the atlas is a real
    quadtree); n_point point lights of radius 3 on an 8 x 8 x 4 lattice 1 .. 3 above the floor, visited in a scattered order so
    that the first and the last lights of every count stand over the visible stage.  The limits are 16 and 256
    (R3N_MAX_DIR_LIGHTS, R3N_MAX_POINT_LIGHTS): at 256 the staging loop runs with one light per thread of the block."""
    dirs, points = [], []
    for i in range(n_dir):
        az = 2.0 * math.pi * ((i * 7) % 16) / 16.0 + 0.2
        tilt = 0.25 + 0.05 * i
        dirs.append(dict(color=_colour(i, 5, 3, 2), intensity=0.4 + 2.0 / n_dir,
                         direction=(tilt * math.cos(az), -1.0, tilt * math.sin(az)), distance=60.0,
                         resolution=DIR_RESOLUTIONS[i % 4]))
    for i in range(n_point):
        cell = (i * 37 + 99) % 256
        x, z, layer = cell % 8, (cell // 8) % 8, cell // 64
        points.append(dict(position=(-5.25 + 1.5 * x, 1.0 + 2.0 * layer / 3.0, -5.25 + 1.5 * z), color=_colour(i, 3, 2, 1),
                           intensity=0.5 + 6.0 / n_point, radius=3.0))
    return dirs, points


# ------------------------------------------------------------------ zero_paths
ZERO_COLOURS = [f32(3.0), f32(1e6), np.nextafter(f32(1e6), f32(np.inf)), f32(np.inf), f32(-np.inf), f32(np.nan), f32(-5.0), f32(1e7)]
ZERO_COLOUR_IDS = ["3", "1e6", "1e6_next", "inf", "-inf", "nan", "-5", "1e7"]
ZERO_STAGE = dict(slab=True, mirror=True)
ZERO_BELOW, ZERO_OCCLUDED = 1, 4  # indices into zero_paths()[0]


def zero_paths(which=None, value=3.0):
    """The stage with its slab and its mirror (ZERO_STAGE).  Directional lights: 0 an ordinary one from above, from the camera's side, under the slab's edge
    (always there: a dropped or poisoned term shows); 1 from below -- obliquely, (-1, 0.45, 0.15): straight up is parallel to the
    shadow camera's `up` and would only repeat light 3 -- (nl == 0 on the floor; its shadow box is too small to hold
    anything, so what faces it is lit); 2 grazing, (1, 0, 0); 3 direction (0, -1, 0), parallel to the `up` of the shadow camera:
    NaN shadow matrices; 4 from above the slab: shadow == 0 under it.  `which` (ZERO_BELOW | ZERO_OCCLUDED) has colour
    (value, value, value) with intensity 1, the other of the two has 3.0.
    Point lights: radius 0, a negative radius, radius +inf, one far beyond its radius, one exactly on a floor vertex."""
    col = {ZERO_BELOW: f32(3.0), ZERO_OCCLUDED: f32(3.0)}
    if which is not None:
        col[which] = f32(value)
    dirs = [
        dict(color=(1.0, 0.9, 0.8), intensity=1.5, direction=(0.3, -0.35, 1.0), distance=60.0, resolution=64),
        dict(color=(col[ZERO_BELOW],) * 3, intensity=1.0, direction=ZERO_BELOW_DIRECTION, distance=4.0, resolution=32),
        dict(color=(0.2, 0.5, 0.3), intensity=1.0, direction=(1.0, 0.0, 0.0), distance=60.0, resolution=32),
        dict(color=(0.3, 0.2, 0.4), intensity=1.0, direction=(0.0, -1.0, 0.0), distance=60.0, resolution=32),
        dict(color=(col[ZERO_OCCLUDED],) * 3, intensity=1.0, direction=(0.95, -1.0, -0.55), distance=60.0, resolution=64),
    ]
    points = [
        dict(position=(-3.0, 1.0, -2.0), color=(1.0, 0.5, 0.2), intensity=2.0, radius=0.0),
        dict(position=(0.0, 0.5, -2.5), color=(0.1, 0.2, 0.05), intensity=1.0, radius=-2.0),
        dict(position=(3.0, 2.5, 1.0), color=(0.02, 0.03, 0.06), intensity=1.0, radius=float("inf")),
        dict(position=(0.0, 40.0, 0.0), color=(0.5, 0.5, 1.0), intensity=5.0, radius=2.0),
        dict(position=(-1.5, 0.0, -3.0), color=(0.9, 0.9, 0.3), intensity=2.0, radius=2.5),  # a vertex of the 8 x 8 floor
    ]
    return dirs, points


# ------------------------------------------------------------------ frustum_edges
FRUSTUM_DISTANCES = (16.0, 16.0, 12.0)
FRUSTUM_DIRECTIONS = [(0.0, -1.0, 0.35), (1.0, -0.6, 0.0), (0.05, -1.0, 0.3)]
FRUSTUM_RESOLUTIONS = (64, 32, 32)


def frustum_edges(n_lights, distance=None):
    """1 .. 3 directional lights whose shadow box (centred on the camera, `distance` across; None: 16, 16, 12) ends inside the
    visible stage: its boundary crosses the floor in the light's y (light 0), in its x (light 1), in either and in both (light 2),
    and part of the stage lies outside [0, 1] in the light's depth (shadow_lookup_census below counts all that).  The bounds test of opaque.wgsl:509-514 (`any`, un-atlased coordinates against atlas-space
    bounds) then lets lookups leave the light's own map: with resolutions 64, 32, 32 they land in a neighbour's map or wrap
    round the atlas (Repeat addressing: shadow_pcf5_general)."""
    dirs = [dict(color=_colour(k + 1, 5, 3, 2), intensity=2.0, direction=FRUSTUM_DIRECTIONS[k],
                 distance=FRUSTUM_DISTANCES[k] if distance is None else distance,
                 resolution=FRUSTUM_RESOLUTIONS[k]) for k in range(n_lights)]
    return dirs, []


# ------------------------------------------------------------------ in_flight
IN_FLIGHT_FRAMES = 6


def in_flight_start():
    return counts(2, 3)


def in_flight_step(r, frame):
    """the world edit in front of frame `frame` (0 .. 5) of the in-flight sequence"""
    if frame == 0:
        r.add_point_light(position=(0.0, 1.5, -3.0), color=(0.2, 0.9, 0.4), intensity=3.0, radius=3.0)
    elif frame == 1:  # turned, and another resolution: the atlas is laid out again
        r.update_directional_light(0, direction=(-0.5, -1.0, 0.2), resolution=32)
    elif frame == 2:
        r.update_point_light(1, color=(1.0, 0.1, 0.1))
    elif frame == 3:  # an odd count
        r.add_directional_light(color=(0.3, 0.4, 1.0), intensity=1.5, direction=(0.1, -1.0, -0.6), distance=60.0, resolution=64)
    elif frame == 4:
        pass
    elif frame == 5:
        r.update_point_light(0, position=(-1.0, 1.2, -1.0))


# ------------------------------------------------------------------ reading a frame
def geometry_mask(frame):
    """pixels that show a triangle (single-sample frames)"""
    return (frame["vis"] & np.uint64(0xFFFFFFFF)) != 0


def object_mask(frame, handle):
    """pixels whose nearest triangle belongs to the object `handle` (single-sample frames)"""
    ids = (frame["vis"] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    obj = np.searchsorted(frame["tri_base"], np.maximum(ids, 0), side="right") - 1
    return (ids >= 0) & (obj == handle)


def world_positions(frame, camera):
    """(H, W, 3) float64 world position of every pixel's nearest fragment (NaN on the background), from the depth half of the
    visibility keys through the inverse of the camera's view_proj (single-sample frames)"""
    h, w = frame["vis"].shape
    depth = (frame["vis"] >> np.uint64(32)).astype(np.uint32).view(f32).astype(np.float64)
    m = np.asarray(camera.view_proj, dtype=np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:h, 0:w]
    ndc = np.stack([(xs + 0.5) / w * 2.0 - 1.0, 1.0 - (ys + 0.5) / h * 2.0, depth, np.ones_like(depth)], axis=-1)
    p = ndc @ np.linalg.inv(m).T
    with np.errstate(divide="ignore", invalid="ignore"):  # (the background: depth 0)
        p = p[..., :3] / p[..., 3:4]
    p[~geometry_mask(frame)] = np.nan
    return p


def shadow_lookup_census(frame, camera):
    """Per shadow view, how the geometry pixels fare in the bounds test of opaque.wgsl:509-514 as the oracle and the kernel
    restate it, recomputed in float64 (counts of pixels, robust against the last bit): looked_up; of those out_x_only / out_y_only /
    out_both (light-local coordinates outside [0, 1] in x, in y, in both: the lookup leaves the light's own map); wrapped (the 4 x 4
    block of texels leaves the ATLAS: Repeat addressing, shadow_pcf5_general); depth_out (outside [0, 1] in depth: no lookup)."""
    pos = world_positions(frame, camera)
    geo = geometry_mask(frame)
    aw, ah = frame["atlas_size"]
    hom = np.concatenate([pos, np.ones(pos.shape[:2] + (1,))], axis=-1)
    out = []
    for sh in frame["shadow_descs"]:
        m = np.asarray(sh["camera"].view_proj, dtype=np.float64).reshape(4, 4).T
        sn = hom @ m.T
        fx, fy = sn[..., 0] * 0.5 + 0.5, sn[..., 1] * 0.5 + 0.5
        lx, ly = fx, 1.0 - fy
        off = np.array(sh["offset"], dtype=np.float64) / (aw, ah)
        size = sh["size"] / np.array((aw, ah), dtype=np.float64)
        border = 1.5 / np.array((aw, ah), dtype=np.float64)
        tl, tr = off + border, off + size - border
        with np.errstate(invalid="ignore"):
            depth_in = (sn[..., 2] >= 0.0) & (sn[..., 2] <= 1.0)
            looked = geo & ((fx >= tl[0]) | (fy >= tl[1])) & ((fx <= tr[0]) | (fy <= tr[1])) & depth_in
            ox, oy = (lx < 0.0) | (lx > 1.0), (ly < 0.0) | (ly > 1.0)
            tx, ty = np.floor((off[0] + size[0] * lx) * aw - 0.5), np.floor((off[1] + size[1] * ly) * ah - 0.5)
            wrapped = looked & ((tx < 1.0) | (tx > aw - 3.0) | (ty < 1.0) | (ty > ah - 3.0))
        out.append(dict(looked_up=int(looked.sum()), out_x_only=int((looked & ox & ~oy).sum()), out_y_only=int((looked & oy & ~ox).sum()),
                        out_both=int((looked & ox & oy).sum()), wrapped=int(wrapped.sum()), depth_out=int((geo & ~depth_in).sum())))
    return out
