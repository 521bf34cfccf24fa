"""Host-side mirror of the reference's routine interface for the hot path, driving the HIP kernels through
the C ABI (include/r3n.h).  Names, argument meaning and the node order follow the reference:

  Renderer (world edits the path consumes)         rend3/src/renderer/mod.rs:126-424
  RenderGraph / node closures                      rend3/src/graph/graph.rs:81-519, graph/node.rs:59-213
  BaseRenderGraph::{new, add_to_graph}             rend3-routine/src/base.rs:110-186
  GpuCuller::{add_object_uniform_upload_to_graph,
              add_culling_to_graph}                rend3-routine/src/culling/culler.rs:661-713
  ForwardRoutine::add_forward_to_graph             rend3-routine/src/forward.rs:192-315
  PbrRoutine (5 forward routines + hi-z)           rend3-routine/src/pbr/routine.rs:35-133
  HiZRoutine::add_hi_z_to_graph                    rend3-routine/src/hi_z.rs:161-234
  TonemappingRoutine::add_to_graph                 rend3-routine/src/tonemapping.rs:108-147

The graph here is the fixed schedule only (the render-graph machinery itself is
out of scope); nodes are closures executed in declaration order by RenderGraph.execute.
This module never imports the oracle; without the native library it raises.
"""
import ctypes
import dataclasses
import math
import os

import numpy as np

from . import _ffi, host

f32 = np.float32
INVALID = 0xFFFFFFFF
OPAQUE, CUTOUT, BLEND = 0, 1, 2

# rend3-routine/shaders/src/material.wgsl:1-15
FLAGS_ALBEDO_ACTIVE = 0x0001
FLAGS_ALBEDO_BLEND = 0x0002
FLAGS_ALBEDO_VERTEX_SRGB = 0x0004
FLAGS_AOMR_COMBINED = 0x0040
FLAGS_AOMR_SPLIT = 0x0100
FLAGS_CC_GLTF_COMBINED = 0x0400
FLAGS_BICOMPONENT_NORMAL = 0x0008
FLAGS_SWIZZLED_NORMAL = 0x0010
FLAGS_YDOWN_NORMAL = 0x0020
FLAGS_AOMR_SWIZZLED_SPLIT = 0x0080
FLAGS_AOMR_BW_SPLIT = 0x0200
FLAGS_CC_GLTF_SPLIT = 0x0800
FLAGS_CC_BW_SPLIT = 0x1000
FLAGS_UNLIT = 0x2000
FLAGS_NEAREST = 0x4000

# r3n_sample_probe (include/r3n.h): r3n_sample_query40 / r3n_sample_result52 and the R3N_PROBE_* form ids
SAMPLE_QUERY = np.dtype([("id", np.uint32, 3), ("nearest", np.uint32), ("u", f32), ("v", f32), ("ddx", f32, 2), ("ddy", f32, 2)])
SAMPLE_RESULT = np.dtype([("rgba", f32, (3, 4)), ("flags", np.uint32)])
assert SAMPLE_QUERY.itemsize == 40 and SAMPLE_RESULT.itemsize == 52
# r3n_environment_probe (include/r3n.h r3n_env_query32 / r3n_env_sample32)
ENV_QUERY = np.dtype([("dir", f32, 3), ("roughness", f32), ("n", f32, 3), ("pad", f32)])
ENV_SAMPLE = np.dtype([("specular", f32, 3), ("irradiance", f32, 3), ("level", np.uint32), ("fraction", f32)])
assert ENV_QUERY.itemsize == 32 and ENV_SAMPLE.itemsize == 32
IBL_MAX_EXTENT, IBL_MAX_LEVELS = 256, 16  # csrc/ibl_rule.h
PROBE_FORMS = ("grad", "grad_rgb", "short", "short_rgb", "share", "alpha", "alpha_short", "batched")  # index = R3N_PROBE_*


def material_texture_slots(ru, normal_texture, normal_mode, normal_y_down, aomr, reflectance_texture,
                           clearcoat_textures, emissive_texture, anisotropy_texture):
    """Texture ids (handle + 1) of slots 1..9 of the 208-byte record and the flags of NormalTexture / AoMRTextures /
    ClearcoatTextures::to_flags (pbr/material.rs:201-222, 305-317, 354-364).  aomr: None | ("combined", tex) |
    ("swizzled_split", ao, mr) | ("split", ao, mr) | ("bw_split", ao, m, r); clearcoat_textures: None |
    ("gltf_combined", tex) | ("gltf_split", cc, ccr) | ("bw_split", cc, ccr); any texture may be None."""
    def put(slot, tex):
        if tex is not None:
            ru[slot] = int(tex) + 1
    flags = 0
    if normal_texture is not None:
        put(1, normal_texture)
        flags |= {"tricomponent": 0, "bicomponent": FLAGS_BICOMPONENT_NORMAL,
                  "bicomponent_swizzled": FLAGS_BICOMPONENT_NORMAL | FLAGS_SWIZZLED_NORMAL}[normal_mode]
        if normal_y_down:
            flags |= FLAGS_YDOWN_NORMAL
    if aomr is None:
        flags |= FLAGS_AOMR_COMBINED  # "so shader only checks roughness texture, then bails"
    elif aomr[0] == "combined":
        flags |= FLAGS_AOMR_COMBINED
        put(2, aomr[1])
    elif aomr[0] in ("swizzled_split", "split"):
        flags |= FLAGS_AOMR_SWIZZLED_SPLIT if aomr[0] == "swizzled_split" else FLAGS_AOMR_SPLIT
        put(9, aomr[1])
        put(2, aomr[2])
    elif aomr[0] == "bw_split":
        flags |= FLAGS_AOMR_BW_SPLIT
        put(9, aomr[1])
        put(3, aomr[2])
        put(2, aomr[3])
    else:
        raise ValueError(aomr)
    put(4, reflectance_texture)
    if clearcoat_textures is None or clearcoat_textures[0] == "gltf_combined":
        flags |= FLAGS_CC_GLTF_COMBINED
        if clearcoat_textures is not None:
            put(5, clearcoat_textures[1])
    elif clearcoat_textures[0] in ("gltf_split", "bw_split"):
        flags |= FLAGS_CC_GLTF_SPLIT if clearcoat_textures[0] == "gltf_split" else FLAGS_CC_BW_SPLIT
        put(5, clearcoat_textures[1])
        put(6, clearcoat_textures[2])
    else:
        raise ValueError(clearcoat_textures)
    put(7, emissive_texture)
    put(8, anisotropy_texture)
    return flags


def material_record(albedo=(0, 0, 0, 1), albedo_mode="value", unlit=False, roughness=0.0, metallic=0.0,
                    reflectance=0.5, emissive=(0, 0, 0), ao=1.0, clear_coat=0.0, clear_coat_roughness=0.0,
                    cutout=None, vertex_srgb=True, albedo_texture=None, nearest=False, uv_transform0=None,
                    normal_texture=None, normal_mode="tricomponent", normal_y_down=False, aomr=None,
                    reflectance_texture=None, clearcoat_textures=None, emissive_texture=None, anisotropy_texture=None):
    """ShaderMaterial::from_material (rend3-routine/src/pbr/material.rs:548-583) behind the 48-byte texture-id prefix
    (rend3/src/managers/material.rs:25-29).  208 bytes as f32[52].  albedo_mode (AlbedoComponent, material.rs:60-140):
    "none" | "vertex" | "value" | "value_vertex", or with `albedo_texture` (texture handle) "texture" |
    "texture_vertex" | "texture_value" | "texture_vertex_value".  nearest = SampleType::Nearest; uv_transform0 = Mat3
    (row-major nested list)."""
    rec = np.zeros(52, dtype=f32)
    ru = rec.view(np.uint32)
    for base in (12, 24):  # uv_transform0/1 = identity mat3 (3 x vec4 columns)
        rec[base + 0] = rec[base + 5] = rec[base + 10] = 1.0
    flags = material_texture_slots(ru, normal_texture, normal_mode, normal_y_down, aomr, reflectance_texture,
                                   clearcoat_textures, emissive_texture, anisotropy_texture)
    if albedo_mode == "none":
        alb = (0.0, 0.0, 0.0, 1.0)
    elif albedo_mode == "vertex":
        flags |= FLAGS_ALBEDO_ACTIVE | FLAGS_ALBEDO_BLEND | (FLAGS_ALBEDO_VERTEX_SRGB if vertex_srgb else 0)
        alb = (1.0, 1.0, 1.0, 1.0)
    elif albedo_mode == "value":
        flags |= FLAGS_ALBEDO_ACTIVE
        alb = albedo
    elif albedo_mode == "value_vertex":
        flags |= FLAGS_ALBEDO_ACTIVE | FLAGS_ALBEDO_BLEND | (FLAGS_ALBEDO_VERTEX_SRGB if vertex_srgb else 0)
        alb = albedo
    elif albedo_mode in ("texture", "texture_value"):
        flags |= FLAGS_ALBEDO_ACTIVE
        alb = albedo if albedo_mode == "texture_value" else (1.0, 1.0, 1.0, 1.0)
    elif albedo_mode in ("texture_vertex", "texture_vertex_value"):
        flags |= FLAGS_ALBEDO_ACTIVE | FLAGS_ALBEDO_BLEND | (FLAGS_ALBEDO_VERTEX_SRGB if vertex_srgb else 0)
        alb = albedo if albedo_mode == "texture_vertex_value" else (1.0, 1.0, 1.0, 1.0)
    else:
        raise ValueError(albedo_mode)
    if albedo_mode.startswith("texture"):
        if albedo_texture is None:
            raise ValueError("texture albedo modes need albedo_texture")
        ru[0] = int(albedo_texture) + 1  # NonZeroU32 index into the bindless array
    if nearest:
        flags |= FLAGS_NEAREST
    if uv_transform0 is not None:
        m = np.asarray(uv_transform0, dtype=f32).reshape(3, 3)
        for col in range(3):
            rec[12 + 4 * col: 12 + 4 * col + 3] = m[:, col]
    if unlit:
        flags |= FLAGS_UNLIT
    rec[36:40] = alb
    rec[40:43] = emissive
    rec[43], rec[44], rec[45], rec[46], rec[47] = roughness, metallic, reflectance, clear_coat, clear_coat_roughness
    rec[49] = ao
    rec[50] = 0.0 if cutout is None else cutout
    ru[51] = flags
    return rec


def morph_reach(position_deltas, n_targets):
    """reach[t] = max over the vertices of sqrt((dx * dx + dy * dy) + dz * dz), f32 with one rounding per operation: how far
    target t moves any vertex at weight 1.  Zeros without position deltas."""
    if position_deltas is None:
        return np.zeros(n_targets, dtype=f32)
    d = np.ascontiguousarray(position_deltas, dtype=f32).reshape(n_targets, -1, 3)
    if d.shape[1] == 0:
        return np.zeros(n_targets, dtype=f32)
    return np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).max(axis=1).astype(f32)


def morph_radius(radius, weights, reach):
    r = f32(radius)
    for w, rc in zip(np.asarray(weights, dtype=f32), np.asarray(reach, dtype=f32)):
        if w != 0.0:
            r = f32(r + f32(f32(abs(w)) * rc))
    return r


@dataclasses.dataclass
class AutoExposure:
    """Renderer.set_tonemapping(auto_exposure=...): the mean log-luminance of ranks [low, high) of the frame's sorted luminances is
    brought to `key`; the exposure stays within [min_ev, max_ev] stops and approaches its target at `speed` per second (inf:
    instantly)."""
    key: float = 0.18
    min_ev: float = -16.0
    max_ev: float = 16.0
    low: float = 0.5
    high: float = 0.95
    speed: float = 3.0


def tonemap_opts(operator="blit", exposure_ev=0.0, white=4.0, auto_exposure=None, dt=1.0 / 60.0):
    """Renderer.set_tonemapping's arguments as an r3n_tonemap_opts (every field valid whatever the mode, as r3n_tonemap_set
    wants it); what cannot be expressed raises here."""
    if operator not in _ffi.TONEMAP_OPS:
        raise ValueError(f"set_tonemapping: unknown operator {operator!r} (one of {sorted(_ffi.TONEMAP_OPS)})")
    o = _ffi.TonemapOpts()
    o.op, o.exposure_mode = _ffi.TONEMAP_OPS[operator], _ffi.EXPOSURE_MANUAL
    o.exposure_ev, o.white = float(exposure_ev), float(white)
    ae = auto_exposure if auto_exposure is not None else AutoExposure()
    if not isinstance(ae, AutoExposure):
        raise TypeError("set_tonemapping: auto_exposure is an AutoExposure or None")
    if not ae.key > 0.0 or not math.isfinite(ae.key):
        raise ValueError("set_tonemapping: AutoExposure.key is a positive luminance")
    if not (dt > 0.0 and ae.speed > 0.0):
        raise ValueError("set_tonemapping: dt and AutoExposure.speed are positive")
    o.key_log2, o.min_ev, o.max_ev = math.log2(ae.key), float(ae.min_ev), float(ae.max_ev)
    o.adapt = 1.0 if math.isinf(ae.speed) else min(1.0, max(-math.expm1(-float(dt) * float(ae.speed)), 2.0 ** -24))
    if not 0.0 <= ae.low < ae.high <= 1.0:
        raise ValueError("set_tonemapping: AutoExposure wants 0 <= low < high <= 1")
    o.low_permille, o.high_permille = int(round(ae.low * 1000)), int(round(ae.high * 1000))
    if auto_exposure is not None:
        o.exposure_mode = _ffi.EXPOSURE_AUTO
    return o


def bloom_opts(intensity=0.04, threshold=1.0, knee=0.5, scatter=0.7, max_levels=8):
    """Renderer.set_bloom's arguments as an r3n_bloom_opts; what r3n_bloom_set would refuse raises here."""
    vals = dict(intensity=intensity, threshold=threshold, knee=knee, scatter=scatter)
    for name, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or math.isnan(v):
            raise ValueError(f"set_bloom: {name} is a number, not {v!r}")
    if not 0.0 <= intensity <= 1024.0:
        raise ValueError("set_bloom: intensity lies within [0, 1024]")
    if not 0.0 <= threshold <= 65504.0:
        raise ValueError("set_bloom: threshold lies within [0, 65504] (exposed units: 1 is display white)")
    if not 0.0 <= knee <= threshold:
        raise ValueError("set_bloom: knee lies within [0, threshold]")
    if not 0.0 <= scatter <= 1.0:
        raise ValueError("set_bloom: scatter lies within [0, 1]")
    if isinstance(max_levels, bool) or int(max_levels) != max_levels or not 1 <= max_levels <= _ffi.BLOOM_MAX_LEVELS:
        raise ValueError(f"set_bloom: max_levels is an integer within [1, {_ffi.BLOOM_MAX_LEVELS}]")
    o = _ffi.BloomOpts()
    o.intensity, o.threshold, o.knee, o.scatter, o.max_levels = float(intensity), float(threshold), float(knee), float(scatter), int(max_levels)
    if not (0.0 <= o.knee <= o.threshold):  # (as the ABI compares them: after the rounding to f32)
        raise ValueError("set_bloom: knee lies within [0, threshold]")
    return o


class CameraSpecifier:
    """rend3-routine/src/common/camera.rs:3-35"""
    VIEWPORT = _ffi.CAMERA_VIEWPORT

    @staticmethod
    def shadow(i):
        assert i != 0xFFFFFFFF
        return i


class _Mesh:
    __slots__ = ("attr_off", "first_index", "index_count", "centre", "radius", "vertex_count", "joint_off", "weight_off",
                 "n_targets", "delta_off", "reach", "morph_weights", "adjacency_off", "left_handed", "morph_normals", "morph_tangents",
                 "block",  # block: mesh_upload="stream": byte offset of the mesh's pooled block (None in "append" mode)
                 "required_joint_count")  # highest joint index of any slot + 1 (mesh.rs:135-139); None without joint indices


def required_joint_count(joint_indices):
    """InternalMesh::required_joint_count (rend3/src/managers/mesh.rs:135-139): the highest joint index over all four slots of
    every vertex, plus one.  The weights play no part, as in the reference: a slot whose weight is zero counts too."""
    ji = np.asarray(joint_indices, dtype=np.uint16).reshape(-1)
    return int(ji.max()) + 1 if ji.size else 0


def checked_joint_matrices(required, joint_matrices):
    """SkeletonManager::validate_skeleton (rend3/src/managers/skeleton.rs:73-89): the matrices as (n, 16) f32; ValueError when
    the mesh has no joint indices or names more joints than there are matrices (NotEnoughJoints, with both counts)."""
    if required is None:
        raise ValueError("Mesh must have joint indices to be used in a skeleton")  # SkeletonCreationError
    mats = np.ascontiguousarray(joint_matrices, dtype=f32).reshape(-1, 16)
    if required > len(mats):
        raise ValueError(f"NotEnoughJoints: the mesh names {required} joints, but only {len(mats)} joint matrices were provided")
    return mats


def relocate_offsets(values, moves, words=False):
    """The rule of rend3_amd/csrc/mesh_reloc.h, restated for the host's mirrors after r3n_mesh_compact.  values: mesh-buffer
    addresses (byte offsets; words=True: word addresses), any shape; moves: rows (old byte offset, new byte offset, padded
    words).  An address whose word lies in [old, old + padded words) of a move follows it by old - new; every other address,
    INVALID always, is unchanged; a byte offset keeps its low two bits.  Returns a uint32 array of the same shape."""
    v = np.asarray(values, dtype=np.uint32)
    moves = np.asarray(moves, dtype=np.uint64).reshape(-1, 3)
    if not len(moves) or not v.size:
        return v.copy()
    moves = moves[np.argsort(moves[:, 0])]
    src = moves[:, 0] // 4
    end, shift = src + moves[:, 2], src - moves[:, 1] // 4
    word = v.astype(np.uint64) if words else v.astype(np.uint64) >> np.uint64(2)
    low = np.zeros_like(word) if words else v.astype(np.uint64) & np.uint64(3)
    e = np.searchsorted(src, word, side="right").astype(np.int64) - 1  # the last move that starts at or below the word
    k = np.maximum(e, 0)
    hit = (e >= 0) & (word < end[k]) & (v != INVALID)
    moved = word - np.where(hit, shift[k], np.uint64(0))
    out = moved if words else (moved << np.uint64(2)) | low
    return np.where(hit, out, v.astype(np.uint64)).astype(np.uint32)


def _shift_mesh(m, fn):
    """Every mesh-buffer address a _Mesh holds through fn(byte offset) -> byte offset: the block's start at add_mesh, the moves of
    a compaction afterwards.  INVALID stays."""
    def f(off):
        return INVALID if off == INVALID else int(fn(int(off)))
    m.attr_off = [f(o) for o in m.attr_off]
    m.joint_off, m.weight_off, m.adjacency_off = f(m.joint_off), f(m.weight_off), f(m.adjacency_off)
    m.delta_off = [f(o) for o in m.delta_off]
    m.first_index = f(4 * m.first_index) // 4


class EvalOutput:
    """What Renderer::evaluate_instructions hands the graph (rend3/src/renderer/eval.rs:157-187), path subset."""

    def __init__(self, shadows, shadow_target_size):
        self.shadows = shadows  # [dict(offset=(x, y), size, handle[, camera])] in shadow-view order
        self.shadow_target_size = shadow_target_size


class Renderer:
    """World bookkeeping feeding the object/mesh/material/light buffers of the C ABI."""

    def __init__(self, handedness=host.LEFT, aspect_ratio=None, device=0, max_big_items=None, blend_sort="host", texture_upload="whole",
                 texture_compact=None, mesh_upload="append", mesh_compact=None):
        self.lib = _ffi.lib()
        if blend_sort not in ("host", "gpu"):
            raise ValueError("blend_sort: 'host' or 'gpu'")
        if texture_upload not in ("whole", "stream"):
            raise ValueError("texture_upload: 'whole' or 'stream'")
        # how 2D textures reach the device: "whole" = the bindless array is re-sent when it changed (r3n_textures_write_encoded);
        # "stream" = single entries are added, replaced and removed in place (r3n_textures_update / r3n_textures_remove,
        # TextureManager::add / remove), the host keeps no copy of what it sent
        self._texture_upload = texture_upload
        self._tex_live = []       # "stream": per slot, True while the slot holds a texture (queued ones included)
        self._tex_queue = []      # "stream": (slot, desc row without offset, bytes) not yet sent
        self._tex_removals = []   # "stream": slots whose removal is not yet sent
        self._tex_tails = []      # "stream": (slot, source slot, start_mip, mip_count) of add_texture_2d_from_texture, not yet sent
        self._tex_mips = []       # "stream": per slot, the levels of the texture it holds
        # "stream": None = the pool is never compacted by itself; a fraction f in (0, 1] = r3n_textures_compact at a texture flush in
        # front of a frame, when more than f of the pool below its high-water mark is holes
        if texture_compact is not None and not (0.0 < float(texture_compact) <= 1.0):
            raise ValueError("texture_compact: None or a fraction in (0, 1]")
        self._texture_compact = None if texture_compact is None else float(texture_compact)
        # how mesh words reach the device: "append" = behind one cursor through r3n_mesh_buffer_write, nothing is ever given back;
        # "stream" = every mesh, skeleton and morph instance is ONE pooled block (r3n_mesh_blocks_add / _remove, MeshManager::add /
        # remove), removable one by one, and compact_meshes slides the live blocks together on the GPU
        if mesh_upload not in ("append", "stream"):
            raise ValueError("mesh_upload: 'append' or 'stream'")
        self._mesh_upload = mesh_upload
        # "stream": None = the mesh buffer is never compacted by itself; a fraction f in (0, 1] = r3n_mesh_compact in
        # evaluate_instructions when more than f of the buffer below its high-water mark is holes (the rule of texture_compact)
        if mesh_compact is not None and not (0.0 < float(mesh_compact) <= 1.0):
            raise ValueError("mesh_compact: None or a fraction in (0, 1]")
        self._mesh_compact = None if mesh_compact is None else float(mesh_compact)
        self._mesh_edits = False  # "stream": a block was added or removed since the last look at the holes
        self.object_writes = 0    # r3n_objects_write calls that carried records (the tests' "no resend" counts them)
        # where the transparent pass's back-to-front order is sorted: "host" = host.blend_draw_order + r3n_blend_order_write every
        # frame; "gpu" = the blend set goes up when the world changes (r3n_blend_objects_write), r3n_blend_sort orders it per frame
        self.blend_sort = blend_sort
        self._blend_sent = None  # "gpu": the (slots, locations) of the last r3n_blend_objects_write
        config = None
        if max_big_items is not None:  # r3n_config.max_big_items: raster work-queue capacity (the library keeps a floor, r3n.h)
            config = _ffi.Config(struct_size=ctypes.sizeof(_ffi.Config), max_big_items=int(max_big_items))
        self.ctx = self.lib.r3n_create(device, ctypes.byref(config) if config is not None else None)
        if not self.ctx:
            raise _ffi.R3nError("r3n_create failed: " + self.lib.r3n_create_error().decode())
        self.handedness = handedness
        self.aspect_ratio = aspect_ratio
        self.mesh_cursor = 0  # in u32 words
        self.meshes = []
        self.materials = []
        self._had_blend = False
        self._blend_cache = None
        self.tex_descs = np.zeros((0, 8), dtype=np.uint32)  # r3n_texture_desc32 rows
        self.tex_pool = np.zeros(4, dtype=np.uint8)   # every texture's levels in ITS format (bytes)
        self.tex_used = 0
        self._tex_dirty = False
        self.cubes = []            # (faces uint8[6, N, N, 4], srgb) per add_texture_cube handle
        self._cubes_dirty = False
        self._background = None    # SkyboxRoutine.set_background_texture: the cube handle bound as the skybox, or None
        self._background_sent = None
        self._skybox_level, self._skybox_level_sent = -1.0, None
        self._pose_state = {}      # skeleton handle -> (clip, time): rend3-anim poses re-evaluated in front of every skinning pass
        self._anim_sets = None     # concatenated rend3-anim tables of every AnimationData (animation_add)
        self.output_format = 0
        self.capacity = 16  # FreelistDerivedBuffer::STARTING_SIZE
        self.object_meta = {}
        self.free_handles, self.pending_free, self.deferred_removals = [], [], []
        self.next_handle = 0
        self.world_version = 0  # bumped by every object / skeleton edit
        self.dirty_objects = {}
        self.dir_lights, self.point_lights = [], []
        self._camera_inputs = (host.identity(), ("raw", host.identity()))
        self._camera = None
        self.object_range = None
        self.skeletons = []
        self.morphs = []           # add_morph_instance: dict(mesh, out_off[3], weights, objects)
        self._morph_dirty = set()  # instances never evaluated, or whose weights changed since: the next frame's one r3n_morph call
        # R3N_FRAME_NODES=1: render() issues the frame node by node through the graph mirror (one C call per reference node, what
        # a Rust integration's node closures do); default: Renderer::evaluate's CPU work and the whole node list behind ONE C call
        # each (r3n_host_evaluate_frame, r3n_render_frame)
        self.frame_nodes = os.environ.get("R3N_FRAME_NODES", "0") == "1"
        self._fc = None  # persistent ctypes blocks of the one-call path
        self._lights_version = 0
        self._capacity_sent = None
        self._resolution = (0, 0)
        # None: an R3N_ERR_CAPACITY return raises like every other error.  A list: it is recorded there as (call, code) instead -- the
        # report names an EARLIER frame, the call itself did its work (a read-back has filled its buffer) and no frame is refused
        self.capacity_reports = None
        self._write_objects([], force_capacity=True)

    def close(self):
        if self.ctx:
            self.lib.r3n_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, code, what):
        if code == _ffi.ERR_CAPACITY and self.capacity_reports is not None:
            self.capacity_reports.append((what, code))
            return
        _ffi.check(self.ctx, code, what)

    # ------------------------------------------------------------------ world edits
    def add_mesh(self, positions, indices=None, normals=None, colors=None, mesh_handedness=host.LEFT, tangents=None,
                 joint_indices=None, joint_weights=None, uv0=None, morph_targets=None, morph_weights=None, morph_normals="base",
                 build_tangents=False, morph_tangents="base"):
        """morph_targets: glTF morph targets as dict(positions=, normals=, tangents=), each f32[T, V, 3] or None (at least one
        given; a target that lacks an attribute the others have holds zeros there).  The deltas are written once, here, behind
        the mesh's own runs: per attribute T target-major runs of 3 V words, the block 16-byte aligned.  morph_weights: the
        mesh's default weights (T floats, default zeros).  A mesh without NORMAL gets the normals add_mesh computes from the BASE
        shape.  morph_normals: "base" (default) keeps those for every morphed shape (only NORMAL deltas move normals);
        "recompute" gives every morph instance of the mesh a private normal run that r3n_vertex_normals rewrites from the
        instance's morphed positions whenever its weights change -- what calculate_normals gives for those positions, bit for bit
        (DESIGN.md section 2 "Recomputed normals").  It needs normals=None, position deltas and no normal deltas (ValueError
        otherwise); the mesh's vertex adjacency (V + 1 + 3 T words) is built once, here, and stored behind the delta block.
        build_tangents: True is MeshBuilder::build's second half (rend3-types/src/lib.rs:505-509): a mesh with uv0 and without
        tangents gets the tangents calculate_tangents generates from its positions, normals (given or just computed) and uv0,
        over the same index run, as attribute 2 (DESIGN.md section 2 "Generated tangents").  With tangents given or without uv0
        it does nothing, as in the reference.  False (default) leaves such a mesh without a tangent run, as before; True is the
        reference's behaviour and becomes the default together with the oracle.  morph_tangents: "base" (default) lets the
        tangents of the bind shape serve every weight; "recompute" gives every morph instance a private tangent run that
        r3n_vertex_tangents rewrites from the instance's current positions and normals whenever its weights change.  It needs
        build_tangents=True, tangents=None, uv0, position deltas and no tangent deltas (ValueError otherwise) and shares the
        adjacency with morph_normals="recompute"."""
        if morph_normals not in ("base", "recompute"):
            raise ValueError("morph_normals: 'base' or 'recompute'")
        if morph_normals == "recompute":
            if normals is not None:
                raise ValueError("morph_normals='recompute': the mesh has normals of its own (normals=None)")
            if morph_targets is None or morph_targets.get("positions") is None:
                raise ValueError("morph_normals='recompute': the mesh needs morph targets with position deltas")
            if morph_targets.get("normals") is not None:
                raise ValueError("morph_normals='recompute': the targets carry normal deltas")
        if morph_tangents not in ("base", "recompute"):
            raise ValueError("morph_tangents: 'base' or 'recompute'")
        if morph_tangents == "recompute":
            if not build_tangents:
                raise ValueError("morph_tangents='recompute': the mesh's tangents are not generated (build_tangents=True)")
            if tangents is not None:
                raise ValueError("morph_tangents='recompute': the mesh has tangents of its own (tangents=None)")
            if uv0 is None:
                raise ValueError("morph_tangents='recompute': the mesh needs uv0")
            if morph_targets is None or morph_targets.get("positions") is None:
                raise ValueError("morph_tangents='recompute': the mesh needs morph targets with position deltas")
            if morph_targets.get("tangents") is not None:
                raise ValueError("morph_tangents='recompute': the targets carry tangent deltas")
        if joint_indices is not None and joint_weights is None:  # SkeletonCreationError::MissingAttributesJointWeights, refused here
            raise ValueError("MissingAttributesJointWeights: a mesh with joint indices needs joint weights")
        positions = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
        if indices is None:
            indices = np.arange(len(positions), dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        # (refuses a bad index; built once, shared by the two recomputing kernels)
        adjacency = host.vertex_adjacency(indices, len(positions)) if "recompute" in (morph_normals, morph_tangents) else None
        if normals is None:  # MeshBuilder::build (rend3-types/src/lib.rs:501-504)
            normals = host.calculate_normals(positions, indices, mesh_handedness == host.LEFT)
        normals = np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
        if build_tangents and tangents is None and uv0 is not None:  # MeshBuilder::build (rend3-types/src/lib.rs:505-509)
            tangents = host.calculate_tangents(positions, normals, uv0, indices)
        m = _Mesh()
        m.attr_off = [INVALID] * 6
        chunks = []
        stream = self._mesh_upload == "stream"
        cursor = 0 if stream else self.mesh_cursor  # "stream": offsets inside the blob first; the block's start is added below

        def push(words):
            nonlocal cursor
            start = cursor
            chunks.append(np.ascontiguousarray(words))
            cursor += len(words)
            return start

        m.attr_off[0] = 4 * push(positions.view(np.uint32).reshape(-1))
        m.attr_off[1] = 4 * push(normals.view(np.uint32).reshape(-1))
        if tangents is not None:
            m.attr_off[2] = 4 * push(np.ascontiguousarray(tangents, dtype=f32).reshape(-1).view(np.uint32))
        if uv0 is not None:  # VERTEX_ATTRIBUTE_TEXTURE_COORDINATES_0: vec2<f32>
            m.attr_off[3] = 4 * push(np.ascontiguousarray(uv0, dtype=f32).reshape(-1, 2).reshape(-1).view(np.uint32))
        if colors is not None:
            colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 4)
            m.attr_off[5] = 4 * push(colors.view(np.uint32).reshape(-1))
        m.vertex_count = len(positions)
        m.joint_off = m.weight_off = INVALID
        m.required_joint_count = None
        if joint_indices is not None:  # [u16; 4] per vertex + vec4<f32> weights (rend3-types/src/attribute.rs:97-135)
            m.required_joint_count = required_joint_count(joint_indices)
            m.joint_off = 4 * push(np.ascontiguousarray(joint_indices, dtype=np.uint16).reshape(-1, 4).view(np.uint32).reshape(-1))
            m.weight_off = 4 * push(np.ascontiguousarray(joint_weights, dtype=f32).reshape(-1, 4).view(np.uint32).reshape(-1))
        m.first_index = push(indices)
        m.index_count = len(indices)
        m.n_targets, m.delta_off, m.reach, m.morph_weights = 0, [INVALID] * 3, None, None
        m.adjacency_off, m.left_handed = INVALID, mesh_handedness == host.LEFT  # morph_normals / morph_tangents = "recompute"
        m.morph_normals, m.morph_tangents = morph_normals == "recompute", morph_tangents == "recompute"
        if morph_targets is not None:
            deltas = [morph_targets.get(k) for k in ("positions", "normals", "tangents")]
            shapes = {np.shape(d) for d in deltas if d is not None}
            if len(shapes) != 1 or next(iter(shapes))[1:] != (len(positions), 3):
                raise ValueError("morph_targets: every attribute given is [T, V, 3] with the mesh's V and one T")
            m.n_targets = int(next(iter(shapes))[0])
            if not 1 <= m.n_targets <= _ffi.MAX_MORPH_TARGETS:
                raise ValueError("morph_targets: 1 .. R3N_MAX_MORPH_TARGETS targets")
            if deltas[2] is not None and tangents is None:
                raise ValueError("morph_targets: tangent deltas need tangents")
            for a, d in enumerate(deltas):
                if d is None:
                    continue
                if cursor % 4:  # the delta block starts on a 16-byte boundary
                    push(np.zeros(4 - cursor % 4, dtype=np.uint32))
                m.delta_off[a] = 4 * push(np.ascontiguousarray(d, dtype=f32).reshape(-1).view(np.uint32))
            m.reach = morph_reach(deltas[0], m.n_targets)
            m.morph_weights = (np.zeros(m.n_targets, dtype=f32) if morph_weights is None
                               else np.ascontiguousarray(morph_weights, dtype=f32).reshape(-1).copy())
            if len(m.morph_weights) != m.n_targets:
                raise ValueError("morph_weights: one weight per target")
            if adjacency is not None:
                if cursor % 4:
                    push(np.zeros(4 - cursor % 4, dtype=np.uint32))
                m.adjacency_off = 4 * push(adjacency)
        blob = np.concatenate(chunks)
        m.block = None
        if stream:  # one block for the whole blob: its start is a multiple of 16 bytes, so every alignment inside is kept
            m.block = self._add_mesh_blocks([blob])[0]
            _shift_mesh(m, lambda off: off + m.block)
        else:
            self._check(self.lib.r3n_mesh_buffer_write(self.ctx, 4 * self.mesh_cursor, _ffi.ptr(blob), blob.nbytes),
                        "r3n_mesh_buffer_write")
            self.mesh_cursor = cursor
        m.centre, m.radius = host.bounding_sphere_from_mesh(positions)
        self.meshes.append(m)
        return len(self.meshes) - 1

    # ---- skeletons (rend3/src/managers/skeleton.rs:67-163)
    def add_skeleton(self, mesh, joint_matrices, morph=None):
        """morph: a morph instance of the same mesh -- the skeleton then skins from the instance's morphed runs (glTF: morph
        first, then skin) and its objects take the instance's widened bounding sphere.  ValueError, before anything is allocated,
        when the mesh names more joints than there are matrices (NotEnoughJoints, skeleton.rs:83-89).  The skeleton stores
        exactly the matrices given, for good: the reference truncates to the mesh's count (skeleton.rs:115-117), this mirror
        keeps the surplus -- never read by the skinning kernel -- so that a pose can write a whole rig."""
        m = self.meshes[mesh]
        matrices = checked_joint_matrices(m.required_joint_count, joint_matrices)
        if morph is not None and self.morphs[morph]["mesh"] != mesh:
            raise ValueError("add_skeleton: the morph instance belongs to another mesh")
        out_off = [INVALID] * 3
        if self._mesh_upload == "stream":
            return self._add_skeletons_stream(mesh, [matrices], morph)[0]
        for a in range(3):  # private position / normal / tangent copies (skeleton.rs:110-113)
            if m.attr_off[a] != INVALID:
                out_off[a] = 4 * self.mesh_cursor
                zeros = np.zeros(3 * m.vertex_count, dtype=np.uint32)
                self._check(self.lib.r3n_mesh_buffer_write(self.ctx, out_off[a], _ffi.ptr(zeros), zeros.nbytes), "r3n_mesh_buffer_write")
                self.mesh_cursor += len(zeros)
        self.skeletons.append(dict(mesh=mesh, out_off=out_off, matrices=matrices, morph=morph, block=None))
        self._skin_inputs = None
        return len(self.skeletons) - 1

    def add_skeletons_bulk(self, mesh, joint_matrices_per_skeleton):
        """Many skeletons of one mesh (config 5): one zero-fill upload for all private output ranges.  Every matrix list is
        checked as in add_skeleton before anything is allocated: one short list refuses the whole call."""
        m = self.meshes[mesh]
        matrices = [checked_joint_matrices(m.required_joint_count, mats) for mats in joint_matrices_per_skeleton]
        if self._mesh_upload == "stream":
            return self._add_skeletons_stream(mesh, matrices, None)
        n = len(matrices)
        n_attr = sum(1 for a in range(3) if m.attr_off[a] != INVALID)
        words = 3 * m.vertex_count
        zeros = np.zeros(n * n_attr * words, dtype=np.uint32)
        base = self.mesh_cursor
        self._check(self.lib.r3n_mesh_buffer_write(self.ctx, 4 * base, _ffi.ptr(zeros), zeros.nbytes), "r3n_mesh_buffer_write")
        self.mesh_cursor += len(zeros)
        first = len(self.skeletons)
        for i in range(n):
            out_off, k = [INVALID] * 3, 0
            for a in range(3):
                if m.attr_off[a] != INVALID:
                    out_off[a] = 4 * (base + (i * n_attr + k) * words)
                    k += 1
            self.skeletons.append(dict(mesh=mesh, out_off=out_off, morph=None, block=None, matrices=matrices[i]))
        self._skin_inputs = None
        return list(range(first, first + n))

    def _add_skeletons_stream(self, mesh, joint_matrices_per_skeleton, morph):
        """mesh_upload="stream": ONE r3n_mesh_blocks_add with one zero-filled block per skeleton (its private runs back to back), so
        that each can be retired on its own (SkeletonManager::remove, skeleton.rs:139-147).  The matrix lists come checked
        (checked_joint_matrices) from add_skeleton / add_skeletons_bulk."""
        m = self.meshes[mesh]
        attrs = [a for a in range(3) if m.attr_off[a] != INVALID]
        words = 3 * m.vertex_count
        blocks = self._add_mesh_blocks([len(attrs) * words] * len(joint_matrices_per_skeleton))
        first = len(self.skeletons)
        for block, mats in zip(blocks, joint_matrices_per_skeleton):
            out_off = [INVALID] * 3
            for k, a in enumerate(attrs):
                out_off[a] = block + 4 * k * words
            self.skeletons.append(dict(mesh=mesh, out_off=out_off, morph=morph, block=block, matrices=mats))
        self._skin_inputs = None
        return list(range(first, first + len(blocks)))

    # ---- morph targets (glTF 2.0 section 3.7.2.2; DESIGN.md section 2 "Morph targets")
    def add_morph_instance(self, mesh, weights=None):
        """One set of weights over a mesh's morph targets, with private output runs for the attributes that have deltas (an
        attribute without deltas keeps the mesh's own run).  weights: T floats, default the mesh's.  Bind it with
        add_object(None, material, transform, morph=handle) or add_skeleton(mesh, matrices, morph=handle)."""
        return self.add_morph_instances_bulk(mesh, [weights])[0]

    def add_morph_instances_bulk(self, mesh, weights_per_instance):
        """Many morph instances of one mesh: one zero-fill upload for all private output runs (16-byte aligned each)."""
        m = self.meshes[mesh]
        if not m.n_targets:
            raise ValueError("add_morph_instance: the mesh has no morph targets")
        n = len(weights_per_instance)
        # the attributes with a private run: those with deltas, the normals of a morph_normals="recompute" mesh and the tangents of a
        # morph_tangents="recompute" one
        attrs = [a for a in range(3) if m.delta_off[a] != INVALID or (a == 1 and m.morph_normals) or (a == 2 and m.morph_tangents)]
        words = (3 * m.vertex_count + 3) & ~3  # a run, padded to 16 bytes
        if self._mesh_upload == "stream":  # ONE call, one zero-filled block per instance: each can be retired on its own
            blocks = self._add_mesh_blocks([max(len(attrs) * words, 4)] * n)
            starts = [b // 4 for b in blocks]
        else:
            base = (self.mesh_cursor + 3) & ~3
            zeros = np.zeros(max(n * len(attrs) * words, 4), dtype=np.uint32)
            self._check(self.lib.r3n_mesh_buffer_write(self.ctx, 4 * base, _ffi.ptr(zeros), zeros.nbytes), "r3n_mesh_buffer_write")
            self.mesh_cursor = base + len(zeros)
            blocks, starts = [None] * n, [base + i * len(attrs) * words for i in range(n)]
        first = len(self.morphs)
        for i, w in enumerate(weights_per_instance):
            out_off = [INVALID] * 3
            for k, a in enumerate(attrs):
                out_off[a] = 4 * (starts[i] + k * words)
            self.morphs.append(dict(mesh=mesh, out_off=out_off, weights=self._morph_weights(m, m.morph_weights if w is None else w), objects=[],
                                    block=blocks[i]))
            self._morph_dirty.add(first + i)
        return list(range(first, first + n))

    @staticmethod
    def _morph_weights(m, weights):
        w = np.ascontiguousarray(weights, dtype=f32).reshape(-1).copy()
        if len(w) != m.n_targets:
            raise ValueError(f"morph weights: the mesh has {m.n_targets} targets, got {len(w)} weights")
        return w

    def set_morph_weights(self, handle, weights):
        """The instance is evaluated again in front of the next frame; the objects bound to it (directly or through a skeleton)
        get the bounding sphere of the new weights through the dirty-object path."""
        inst = self.morphs[handle]
        inst["weights"] = self._morph_weights(self.meshes[inst["mesh"]], weights)
        self._morph_dirty.add(handle)
        self.world_version += 1
        for h in inst["objects"]:
            meta = self.object_meta.get(h)
            if meta is None or meta.get("morph_instance") != handle:
                continue  # (the handle was freed, perhaps given to another object)
            rec = self._object_record(h)
            meta["sphere"] = rec.view(f32)[16:20].copy()
            self._mark(h, rec)

    def morph_radius(self, handle):
        """radius' = (((r + |w0| reach0) + |w1| reach1) + ...) over the non-zero weights in target order, f32."""
        inst = self.morphs[handle]
        m = self.meshes[inst["mesh"]]
        return morph_radius(m.radius, inst["weights"], m.reach)

    def _flush_morphs(self):
        """ONE r3n_morph call for the instances never evaluated or whose weights changed, then ONE r3n_vertex_normals call for those
        of them whose mesh recomputes its normals, then ONE r3n_vertex_tangents call for those whose mesh recomputes its tangents;
        none when there are none."""
        if not self._morph_dirty:
            return
        handles = sorted(self._morph_dirty)
        inputs = np.full((len(handles), 12), INVALID, dtype=np.uint32)
        weights, at = [], 0
        for i, hd in enumerate(handles):
            inst = self.morphs[hd]
            m = self.meshes[inst["mesh"]]
            for a in range(3):
                if m.delta_off[a] != INVALID:
                    inputs[i, a], inputs[i, 3 + a], inputs[i, 6 + a] = m.attr_off[a], m.delta_off[a], inst["out_off"][a]
            inputs[i, 9:12] = (at, m.n_targets, m.vertex_count)
            weights.append(inst["weights"])
            at += m.n_targets
        weights = np.ascontiguousarray(np.concatenate(weights), dtype=f32)
        self._check(self.lib.r3n_morph(self.ctx, _ffi.ptr(inputs), len(inputs), _ffi.ptr(weights), len(weights)), "r3n_morph")
        recs = []
        for hd in handles:
            inst = self.morphs[hd]
            m = self.meshes[inst["mesh"]]
            if m.morph_normals:  # r3n_normals_input32
                recs.append((inst["out_off"][0], inst["out_off"][1], 4 * m.first_index, m.index_count, m.adjacency_off, m.vertex_count,
                             1 if m.left_handed else 0, 0))
        if recs:
            recs = np.array(recs, dtype=np.uint32)
            self._check(self.lib.r3n_vertex_normals(self.ctx, _ffi.ptr(recs), len(recs)), "r3n_vertex_normals")
        recs = []
        for hd in handles:
            inst = self.morphs[hd]
            m = self.meshes[inst["mesh"]]
            if m.morph_tangents:  # r3n_tangents_input32: the instance's current positions and normals, the mesh's uv0
                out = inst["out_off"]
                recs.append((out[0], out[1] if out[1] != INVALID else m.attr_off[1], m.attr_off[3], out[2], 4 * m.first_index,
                             m.index_count, m.adjacency_off, m.vertex_count))
        if recs:
            recs = np.array(recs, dtype=np.uint32)
            self._check(self.lib.r3n_vertex_tangents(self.ctx, _ffi.ptr(recs), len(recs)), "r3n_vertex_tangents")
        self._morph_dirty.clear()

    def set_skeleton_joint_matrices(self, sk, joint_matrices):
        """SkeletonManager::set_joint_matrices (skeleton.rs:151-163) against the count the skeleton stores, which is fixed at its
        creation: fewer matrices raise ValueError (the reference's assert), more are truncated to it.  So the matrix bases in
        the cached skinning records, the running sums of the stored counts, cannot go stale."""
        stored = len(self.skeletons[sk]["matrices"])
        mats = np.ascontiguousarray(joint_matrices, dtype=f32).reshape(-1, 16)
        if len(mats) < stored:
            raise ValueError(f"Not enough joints to update this skeleton. The skeleton stores {stored} joint matrices, "
                             f"but only {len(mats)} joint matrices were provided.")
        self.world_version += 1  # skinned vertices may leave the bounds the partition was built from
        self._pose_state.pop(sk, None)
        self.skeletons[sk]["matrices"] = np.ascontiguousarray(mats[:stored])

    def animation_add(self, rigs, joints, clips, tracks, times, values):
        """Register one AnimationData's tables (anim.AnimationData builds them; record layouts in include/r3n.h).  The
        library holds ONE table set (r3n_animation_write), so the sets of all scene instances are concatenated here with
        their indices rebased.  Returns the index of the set's first clip."""
        sets = self._anim_sets
        if sets is None:
            sets = self._anim_sets = [[np.zeros(0, dtype=a.dtype) for a in (rigs, joints, clips, tracks)] + [np.zeros(0, f32), np.zeros(0, f32)]]
        cur = sets[0]
        rigs, clips, tracks = rigs.copy(), clips.copy(), tracks.copy()
        rigs["first"] += len(cur[1])
        clips["rig"] += len(cur[0])
        clips["track"] += len(cur[3])
        tracks["kf"] += np.where(tracks["kc"] > 0, len(cur[4]), 0).astype(np.uint32)
        tracks["vf"] += np.where(tracks["kc"] > 0, len(cur[5]), 0).astype(np.uint32)
        clip_base = len(cur[2])
        sets[0] = [np.concatenate([a, b]) for a, b in zip(cur, (rigs, joints, clips, tracks, np.asarray(times, f32), np.asarray(values, f32)))]
        arrs = [np.ascontiguousarray(a) for a in sets[0]]
        args = []
        for a, rec in zip(arrs, (16, 80, 16, 80, 4, 4)):
            args += [_ffi.ptr(a) if a.size else None, a.nbytes // rec]
        self._check(self.lib.r3n_animation_write(self.ctx, *args), "r3n_animation_write")
        return clip_base

    def pose_skeletons(self, requests):
        """rend3-anim poses: requests = [(clip, time, skeleton handle)].  The joint matrices are evaluated on the GPU
        (csrc/anim.hip) in front of every skinning pass, straight into the buffer the skinning kernel reads, until the
        skeleton gets another pose or explicit matrices (Renderer::set_skeleton_joint_matrices semantics: the last
        value set stays).  The pose kernel writes the clip's whole rig at the skeleton's matrix base: ValueError, before any
        request is taken, when a clip's rig has more joints than its skeleton stores (it would overwrite the next skeleton's)."""
        requests = list(requests)
        sets = self._anim_sets
        for clip, _time, sk in requests:
            if sets is None or not 0 <= int(clip) < len(sets[0][2]):
                raise ValueError(f"pose_skeletons: clip {clip} is not registered (animation_add)")
            if not 0 <= int(sk) < len(self.skeletons) or self.skeletons[int(sk)] is None:
                raise ValueError(f"pose_skeletons: skeleton {sk} does not exist (a bad handle, or removed)")
            rig_joints = int(sets[0][0]["n"][int(sets[0][2]["rig"][int(clip)])])
            stored = len(self.skeletons[int(sk)]["matrices"])
            if rig_joints > stored:
                raise ValueError(f"pose_skeletons: the rig of clip {clip} has {rig_joints} joints, but skeleton {sk} stores only "
                                 f"{stored} joint matrices")
        self.world_version += 1
        for clip, time, sk in requests:
            self._pose_state[sk] = (int(clip), np.float32(time))

    def _pose_requests(self):
        state = self._pose_state
        rq = np.zeros(len(state), dtype=[("clip", np.uint32), ("time", np.float32), ("base", np.uint32), ("pad", np.uint32)])
        for i, (sk, (clip, time)) in enumerate(sorted(state.items())):
            rq[i] = (clip, time, int(self._skin_inputs[self._skin_row[sk]][8]), 0)
        return rq

    def skinning_buffers(self):
        """build_gpu_skinning_input_buffers (rend3-routine/src/skinning.rs:54-139)"""
        if getattr(self, "_skin_inputs", None) is None:
            live = [(h, sk) for h, sk in enumerate(self.skeletons) if sk is not None]  # (remove_skeleton leaves None: handles are not reused)
            inputs = np.zeros((len(live), 10), dtype=np.uint32)
            self._skin_row = {h: i for i, (h, _) in enumerate(live)}
            base = 0
            for i, (_, sk) in enumerate(live):
                m = self.meshes[sk["mesh"]]
                src = list(m.attr_off[:3])
                if sk["morph"] is not None:  # morph, then skin: the base runs are the morph instance's outputs where it has some
                    src = [o if o != INVALID else b for o, b in zip(self.morphs[sk["morph"]]["out_off"], src)]
                inputs[i] = [src[0], src[1], src[2], m.joint_off, m.weight_off, sk["out_off"][0],
                             sk["out_off"][1], sk["out_off"][2], base, m.vertex_count]
                base += len(sk["matrices"])
            self._skin_inputs = inputs
        mats = np.ascontiguousarray(np.concatenate([sk["matrices"] for sk in self.skeletons if sk is not None]))
        return self._skin_inputs, mats

    def _has_skeletons(self):
        return any(sk is not None for sk in self.skeletons)

    # ---- pooled mesh blocks (mesh_upload="stream"; MeshManager::add / remove, rend3/src/managers/mesh.rs:123-211)
    @property
    def mesh_upload(self):
        return self._mesh_upload

    @mesh_upload.setter
    def mesh_upload(self, mode):
        if mode not in ("append", "stream"):
            raise ValueError("mesh_upload: 'append' or 'stream'")
        if mode != self._mesh_upload and (self.meshes or self.skeletons or self.morphs):
            raise ValueError("mesh_upload cannot change once meshes exist")
        self._mesh_upload = mode

    @property
    def mesh_compact(self):
        return self._mesh_compact

    @mesh_compact.setter
    def mesh_compact(self, fraction):
        if fraction is not None and not (0.0 < float(fraction) <= 1.0):
            raise ValueError("mesh_compact: None or a fraction in (0, 1]")
        self._mesh_compact = None if fraction is None else float(fraction)

    def _add_mesh_blocks(self, items):
        """ONE r3n_mesh_blocks_add: items are uint32 arrays (uploaded) or word counts (zero-filled on the device).  Returns the
        blocks' byte offsets."""
        recs = (_ffi.MeshBlock24 * len(items))()
        chunks, at = [], 0
        for i, it in enumerate(items):
            if isinstance(it, np.ndarray):
                recs[i].payload_offset, recs[i].words, recs[i].flags = at, len(it), 0
                chunks.append(np.ascontiguousarray(it, dtype=np.uint32))
                at += 4 * len(it)
            else:
                recs[i].payload_offset, recs[i].words, recs[i].flags = 0, int(it), _ffi.MESH_BLOCK_ZERO
        payload = np.concatenate(chunks) if chunks else None
        out = np.zeros(len(items), dtype=np.uint64)
        self._check(self.lib.r3n_mesh_blocks_add(self.ctx, recs, len(items), _ffi.ptr(payload), at, _ffi.ptr(out)), "r3n_mesh_blocks_add")
        self._mesh_edits = True
        return [int(b) for b in out]

    def _remove_mesh_block(self, what, block):
        if self._mesh_upload != "stream":
            raise ValueError(f"{what} needs Renderer(mesh_upload='stream'): the append path gives no words back")
        offs = np.array([block], dtype=np.uint64)
        self._check(self.lib.r3n_mesh_blocks_remove(self.ctx, _ffi.ptr(offs), 1), "r3n_mesh_blocks_remove")
        self._mesh_edits = True

    def _enabled_objects(self):
        return [meta for meta in self.object_meta.values() if meta.get("enabled")]

    def remove_mesh(self, h):
        """MeshManager::remove (mesh.rs:197-211): the mesh's words are given back and may be reused.  ValueError while an enabled
        object, a skeleton or a morph instance still names the handle (the reference keeps a mesh alive while anything holds its
        handle).  Handles are not reused.  mesh_upload="stream" only."""
        if self._mesh_upload != "stream":
            raise ValueError("remove_mesh needs Renderer(mesh_upload='stream'): the append path gives no words back")
        if self.meshes[h] is None:
            raise ValueError("remove_mesh: the mesh was removed already")
        if (any(meta.get("mesh") == h for meta in self._enabled_objects()) or any(sk is not None and sk["mesh"] == h for sk in self.skeletons)
                or any(inst is not None and inst["mesh"] == h for inst in self.morphs)):
            raise ValueError("remove_mesh: an enabled object, a skeleton or a morph instance still names the mesh")
        self._remove_mesh_block("remove_mesh", self.meshes[h].block)
        self.meshes[h] = None

    def remove_skeleton(self, h):
        """SkeletonManager::remove (skeleton.rs:139-147): the skeleton's private runs are given back.  ValueError while an enabled
        object is bound to it.  mesh_upload="stream" only."""
        if self._mesh_upload != "stream":
            raise ValueError("remove_skeleton needs Renderer(mesh_upload='stream'): the append path gives no words back")
        if self.skeletons[h] is None:
            raise ValueError("remove_skeleton: the skeleton was removed already")
        if any(meta.get("skeleton") == h for meta in self._enabled_objects()):
            raise ValueError("remove_skeleton: an enabled object is still bound to the skeleton")
        self._remove_mesh_block("remove_skeleton", self.skeletons[h]["block"])
        self.skeletons[h] = None
        self._pose_state.pop(h, None)
        self._skin_inputs = None
        self.world_version += 1

    def remove_morph_instance(self, h):
        """The instance's private runs are given back.  ValueError while an enabled object or a skeleton is bound to it.
        mesh_upload="stream" only."""
        if self._mesh_upload != "stream":
            raise ValueError("remove_morph_instance needs Renderer(mesh_upload='stream'): the append path gives no words back")
        if self.morphs[h] is None:
            raise ValueError("remove_morph_instance: the instance was removed already")
        if (any(h in (meta.get("morph"), meta.get("morph_instance")) for meta in self._enabled_objects())
                or any(sk is not None and sk["morph"] == h for sk in self.skeletons)):
            raise ValueError("remove_morph_instance: an enabled object or a skeleton is still bound to the instance")
        self._remove_mesh_block("remove_morph_instance", self.morphs[h]["block"])
        self.morphs[h] = None
        self._morph_dirty.discard(h)
        self.world_version += 1

    def compact_meshes(self, max_words=0, stage_words=0):
        """Slides the live mesh blocks towards word 0 on the GPU and patches the object records there (r3n_mesh_compact): no record
        is re-sent.  Afterwards every mirror of a mesh-buffer address the renderer holds follows the returned moves through
        relocate_offsets -- the meshes, the skeletons' and morph instances' private runs, the cached skinning inputs (the morph,
        normals and tangents inputs are built from those per call) and the records still waiting in the dirty-object mirror.
        max_words / stage_words: as compact_textures.  mesh_upload="stream" only.  Returns r3n_mesh_compact_result as a dict,
        plus moves = uint64[n, 3] rows (old byte offset, new byte offset, padded words)."""
        if self._mesh_upload != "stream":
            raise ValueError("compact_meshes needs Renderer(mesh_upload='stream'): the append path lays its buffer out densely")
        capacity = max(self.mesh_stats()["blocks_live"], 1)
        moves = (_ffi.MeshMove24 * capacity)()
        opts = _ffi.MeshCompactOpts(max_words=int(max_words), stage_words=int(stage_words))
        out = _ffi.MeshCompactResult()
        self._check(self.lib.r3n_mesh_compact(self.ctx, ctypes.byref(opts), ctypes.byref(out), moves, capacity), "r3n_mesh_compact")
        res = {name: int(getattr(out, name)) for name, _ in _ffi.MeshCompactResult._fields_}
        res["moves"] = np.array([(mv.old_byte_offset, mv.new_byte_offset, mv.padded_words) for mv in moves[:res["blocks_moved"]]],
                                dtype=np.uint64).reshape(-1, 3)
        if res["blocks_moved"]:
            self._apply_mesh_moves(res["moves"])
        return res

    def _apply_mesh_moves(self, moves):
        def one(off):
            return int(relocate_offsets(np.uint32(off), moves))
        for m in self.meshes:
            if m is not None:
                _shift_mesh(m, one)
                m.block = one(m.block)
        for entry in list(self.skeletons) + list(self.morphs):
            if entry is not None:
                entry["out_off"] = [int(o) for o in relocate_offsets(entry["out_off"], moves)]
                entry["block"] = one(entry["block"])
        if getattr(self, "_skin_inputs", None) is not None:  # columns 0..7 are byte offsets (r3n_skinning_input40)
            self._skin_inputs[:, :8] = relocate_offsets(self._skin_inputs[:, :8], moves)
        # records not sent yet go up with the new addresses; the device has patched the ones it holds
        for rec in self.dirty_objects.values():
            rec[20] = relocate_offsets(rec[20], moves, words=True)
            rec[23:29] = relocate_offsets(rec[23:29], moves)

    def mesh_stats(self, reset=False):
        """Counters of the pooled mesh path (r3n_mesh_stats) as a dict; reset=True zeroes them after the read."""
        out = _ffi.MeshCounters()
        self._check(self.lib.r3n_mesh_stats(self.ctx, ctypes.byref(out), 1 if reset else 0), "r3n_mesh_stats")
        return {name: int(getattr(out, name)) for name, _ in _ffi.MeshCounters._fields_}

    def shadow_occlusion_stats(self, view):
        """Figures of the last frame's two-phase depth draw of shadow view `view` (r3n_shadow_occlusion_stats) as a dict."""
        out = _ffi.ShadowOcclusionCounters()
        self._check(self.lib.r3n_shadow_occlusion_stats(self.ctx, int(view), ctypes.byref(out)), "r3n_shadow_occlusion_stats")
        return {name: int(getattr(out, name)) for name, _ in _ffi.ShadowOcclusionCounters._fields_}

    def readback_objects(self, first_slot=0, n=None):
        """r3n_readback_objects: the 128-byte records as the device holds them, uint32[n, 32]."""
        n = self.capacity - first_slot if n is None else int(n)
        out = np.zeros((max(n, 1), 32), dtype=np.uint32)
        if n:
            self._check(self.lib.r3n_readback_objects(self.ctx, int(first_slot), _ffi.ptr(out), n), "r3n_readback_objects")
        return out[:n]

    @property
    def texture_upload(self):
        return self._texture_upload

    @texture_upload.setter
    def texture_upload(self, mode):
        if mode not in ("whole", "stream"):
            raise ValueError("texture_upload: 'whole' or 'stream'")
        if mode != self._texture_upload and (len(self.tex_descs) or self._tex_live):
            raise ValueError("texture_upload cannot change once textures exist")
        self._texture_upload = mode

    @property
    def texture_compact(self):
        return self._texture_compact

    @texture_compact.setter
    def texture_compact(self, fraction):
        if fraction is not None and not (0.0 < float(fraction) <= 1.0):
            raise ValueError("texture_compact: None or a fraction in (0, 1]")
        self._texture_compact = None if fraction is None else float(fraction)

    def add_texture_2d(self, rgba8, srgb=True, mip_count=1, mip_source="uploaded"):
        """Renderer::add_texture_2d with Texture{data, format, size, mip_count, mip_source}: rgba8 = (H, W, 4) u8;
        format Rgba8UnormSrgb | Rgba8Unorm; mip_count int or "maximum"; mip_source "uploaded" | "generated".
        texture_upload="whole": the whole bindless array is re-sent (r3n_textures_write_encoded); "stream": the entry alone is sent
        (r3n_textures_update) and takes the lowest free slot.  Returns the texture handle (index)."""
        data, w, h, mips, stored = host.prepare_texture(rgba8, srgb, mip_count, mip_source)
        return self._append_texture(data, w, h, mips, 1 if srgb else 0, stored)

    def add_texture_2d_encoded(self, fmt, width, height, levels, generate_mips=False):
        """Renderer::add_texture_2d for the other formats rend3-gltf's loader produces (containers.py ids = R3N_TEXTURE_*):
        `levels` = the stored levels' bytes, largest first.  generate_mips: MipmapCount::Maximum + MipmapSource::Generated
        (single-level uncompressed files, rend3-gltf/src/lib.rs:1031-1036); the chain is then built from the expanded
        RGBA8 level (on the GPU, like the expansion itself), which gives every channel the values the format's own blit
        chain would.  Block-compressed data goes to the GPU as stored and is decoded there."""
        from . import containers
        if generate_mips:
            if not containers.generate_mips_allowed(fmt) or len(levels) != 1:
                raise ValueError("mips are generated for single-level 8-bit uncompressed textures only")
            mips = int(max(width, height)).bit_length()
            return self._append_texture(np.frombuffer(levels[0], dtype=np.uint8), width, height, mips, fmt, 1 if mips > 1 else 0)
        for k, lv in enumerate(levels):
            if len(lv) != containers.level_bytes(fmt, max(1, width >> k), max(1, height >> k)):
                raise ValueError(f"level {k}: wrong byte count for its extent")
        return self._append_texture(np.frombuffer(b"".join(levels), dtype=np.uint8), width, height, len(levels), fmt)

    def _append_texture(self, data_u8, w, h, mips, fmt, stored=0):
        if self._texture_upload == "stream":
            # the lowest free slot (TextureManager's handle allocator); sent with everything else queued when the next frame is
            # evaluated (TextureManager::evaluate)
            if self._tex_tails:
                # uploads go in front of the queued add_texture_2d_from_texture copies, in one call that may open at most as many
                # slots as it has entries: an upload behind a queued copy's slot would be past that bound
                self._flush_textures()
            slot = self._take_texture_slot(mips)
            self._tex_queue.append((slot, (w, h, mips, fmt, stored), np.array(data_u8, dtype=np.uint8)))
            return slot
        start = (self.tex_used + 3) & ~3  # level 0 of every texture starts on a 4-byte boundary
        end = start + len(data_u8)
        if end > len(self.tex_pool):
            grown = np.zeros(max(2 * len(self.tex_pool), end), dtype=np.uint8)
            grown[: self.tex_used] = self.tex_pool[: self.tex_used]
            self.tex_pool = grown
        self.tex_pool[start:end] = data_u8
        self.tex_used = end
        desc = np.array([[start, w, h, mips, fmt, stored, 0, 0]], dtype=np.uint32)
        self.tex_descs = np.ascontiguousarray(np.concatenate([self.tex_descs, desc]))
        self._tex_dirty = True  # the array is re-sent once, when the next frame is evaluated (TextureManager::evaluate)
        return len(self.tex_descs) - 1

    def _take_texture_slot(self, mips):
        slot = self._tex_live.index(False) if False in self._tex_live else len(self._tex_live)
        if slot == len(self._tex_live):
            self._tex_live.append(True)
            self._tex_mips.append(0)
        self._tex_live[slot] = True
        self._tex_mips[slot] = int(mips)
        return slot

    def add_texture_2d_from_texture(self, src, start_mip, mip_count=None):
        """Renderer::add_texture_2d_from_texture with TextureFromTexture{src, start_mip, mip_count}: a new texture of the size of
        level start_mip of `src` whose levels are copies of levels start_mip .. of it, mip_count of them (None = all that remain) --
        copied on the GPU inside the texel pool (r3n_textures_from_texture), nothing is sent from the host.  texture_upload="stream"
        only.  `src` may be a texture that is itself still queued.  Takes the lowest free slot; returns the new handle."""
        if self._texture_upload != "stream":
            raise ValueError("add_texture_2d_from_texture needs Renderer(texture_upload='stream'): the whole-array path keeps no resident pool to copy from")
        src, start_mip = int(src), int(start_mip)
        if not (0 <= src < len(self._tex_live)) or not self._tex_live[src]:
            raise ValueError(f"add_texture_2d_from_texture: handle {src} holds no texture")
        mips = self._tex_mips[src]
        count = mips - start_mip if mip_count is None else int(mip_count)
        if not (0 <= start_mip < mips) or not (1 <= count <= mips - start_mip):
            raise ValueError(f"add_texture_2d_from_texture: levels [{start_mip}, {start_mip + count}) of a texture with {mips}")
        if any(t[0] == src for t in self._tex_tails):
            self._flush_textures()  # sources are resolved against the table in front of the call: a queued tail goes first
        slot = self._take_texture_slot(count)
        self._tex_tails.append((slot, src, start_mip, count))
        return slot

    def remove_texture(self, handle):
        """TextureManager::remove (the reference drops a texture with its handle): the slot's texels become reusable, the handle
        may be handed out again.  texture_upload="stream" only.  Materials that still name the handle read an unspecified texel."""
        if self._texture_upload != "stream":
            raise ValueError("remove_texture needs Renderer(texture_upload='stream'): the whole-array path has no removal")
        handle = int(handle)
        if not (0 <= handle < len(self._tex_live)) or not self._tex_live[handle]:
            raise ValueError(f"remove_texture: handle {handle} holds no texture")
        if any(slot == handle for slot, _, _ in self._tex_queue) or any(handle in t[:2] for t in self._tex_tails):
            # it was never sent, or a queued add_texture_2d_from_texture makes or reads it: send, then remove (keeps the table the
            # library's; removals go in front of everything else queued)
            self._flush_textures()
        self._tex_live[handle] = False
        self._tex_removals.append(handle)

    def compact_textures(self, max_words=0, stage_words=0):
        """Slides the live textures towards pool word 0 on the GPU (r3n_textures_compact), so that what removals left free is reused
        and the pool stops growing.  texture_upload="stream" only.  max_words: stop after that many words (0 = all); stage_words:
        scratch words the call may use (0 = the library's default).  Pending textures and removals are sent first.  Returns
        r3n_texture_compact_result as a dict."""
        if self._texture_upload != "stream":
            raise ValueError("compact_textures needs Renderer(texture_upload='stream'): the whole-array path lays its pool out densely")
        self._flush_textures()
        opts = _ffi.TextureCompactOpts(max_words=int(max_words), stage_words=int(stage_words))
        out = _ffi.TextureCompactResult()
        self._check(self.lib.r3n_textures_compact(self.ctx, ctypes.byref(opts), ctypes.byref(out)), "r3n_textures_compact")
        return {name: int(getattr(out, name)) for name, _ in _ffi.TextureCompactResult._fields_}

    def sample_probe(self, form, queries):
        """r3n_sample_probe: the frame kernels' texture sampler on a list of queries, over this renderer's textures (pending ones are
        sent first).  form: an R3N_PROBE_* id; queries: array of SAMPLE_QUERY (40-byte records; 64 consecutive ones are one
        wavefront).  Returns an array of SAMPLE_RESULT."""
        self._flush_textures()
        q = np.ascontiguousarray(queries, dtype=SAMPLE_QUERY)
        out = np.zeros(len(q), dtype=SAMPLE_RESULT)
        self._check(self.lib.r3n_sample_probe(self.ctx, int(form), _ffi.ptr(q), len(q), _ffi.ptr(out)), "r3n_sample_probe")
        return out

    def _flush_textures(self, before_frame=False):
        changed = bool(self._tex_removals or self._tex_queue or self._tex_tails)
        self._send_textures()
        if before_frame and changed and self._texture_compact is not None and self._texture_upload == "stream":
            st = self.texture_stats()
            if st["pool_words"] - st["live_words"] > self._texture_compact * st["pool_words"]:
                self.compact_textures()

    def _send_textures(self):
        if self._tex_removals:
            slots = np.array(self._tex_removals, dtype=np.uint32)
            self._check(self.lib.r3n_textures_remove(self.ctx, _ffi.ptr(slots), len(slots)), "r3n_textures_remove")
            self._tex_removals = []
        if self._tex_queue:
            slots = np.array([q[0] for q in self._tex_queue], dtype=np.uint32)
            descs = np.zeros((len(slots), 8), dtype=np.uint32)
            at, parts = 0, []
            for row, (_, d, data) in zip(descs, self._tex_queue):
                row[0], row[1:6] = at, d
                parts.append(data)
                pad = -len(data) & 3  # level 0 of every texture starts on a 4-byte boundary
                if pad:
                    parts.append(np.zeros(pad, dtype=np.uint8))
                at += len(data) + pad
            payload = np.ascontiguousarray(np.concatenate(parts)) if at else np.zeros(4, dtype=np.uint8)
            self._check(self.lib.r3n_textures_update(self.ctx, _ffi.ptr(slots), _ffi.ptr(descs), len(slots), _ffi.ptr(payload), at),
                        "r3n_textures_update")
            self._tex_queue = []  # nothing sent is kept on the host
        if self._tex_tails:  # behind the updates: a tail may name a texture queued in the same flush
            items = (_ffi.TextureTail16 * len(self._tex_tails))(*[_ffi.TextureTail16(*t) for t in self._tex_tails])
            self._check(self.lib.r3n_textures_from_texture(self.ctx, items, len(self._tex_tails), None), "r3n_textures_from_texture")
            self._tex_tails = []
        if self._tex_dirty:
            self._check(self.lib.r3n_textures_write_encoded(self.ctx, _ffi.ptr(self.tex_descs), len(self.tex_descs),
                                                            _ffi.ptr(self.tex_pool), self.tex_used), "r3n_textures_write_encoded")
            self._tex_dirty = False

    def add_texture_cube(self, faces, srgb=True):
        """Renderer::add_texture_cube with Texture{format: Rgba8UnormSrgb | Rgba8Unorm, mip_count: ONE}: faces = uint8[6, N, N, 4]
        in layer order +X, -X, +Y, -Y, +Z, -Z (scene_viewer's right, left, top, bottom, front, back).  The cube array is re-sent
        when the next frame is evaluated (r3n_texture_cubes_write).  Returns the cube handle (index)."""
        faces = np.ascontiguousarray(faces, dtype=np.uint8)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[3] != 4:
            raise ValueError("a cube texture is uint8[6, N, N, 4]")
        self._drop_derived_cubes()
        self.cubes.append((faces, bool(srgb)))
        self._cubes_dirty = True
        return len(self.cubes) - 1

    def add_texture_cube_encoded(self, fmt, width, faces):
        """Renderer::add_texture_cube with any TextureFormat and MipmapCount::Specific(n), MipmapSource::Uploaded: fmt = an
        R3N_TEXTURE_* id (containers.py), faces[f][k] = the bytes of level k of face f, faces in layer order +X, -X, +Y, -Y, +Z,
        -Z, every face with the same number of levels; level k is max(1, width >> k) texels square.  What
        containers.parse_ktx2_cube / parse_dds_cube return fits: add_texture_cube_encoded(c["format"], c["width"], c["faces"]).
        The cube array is re-sent when the next frame is evaluated (r3n_texture_cubes_write_encoded).  Returns the cube handle."""
        from . import containers
        fmt, width = int(fmt), int(width)
        if not 0 <= fmt < containers.FORMAT_COUNT:
            raise ValueError(f"add_texture_cube_encoded: unknown format id {fmt}")
        if not 1 <= width <= 16384:
            raise ValueError("add_texture_cube_encoded: a cube's extent is 1 .. 16384")
        if len(faces) != 6:
            raise ValueError("add_texture_cube_encoded: a cube has six faces")
        mips = len(faces[0])
        if mips < 1 or mips > width.bit_length():
            raise ValueError(f"add_texture_cube_encoded: {mips} levels, an extent of {width} has 1 .. {width.bit_length()}")
        kept = []
        for f, levels in enumerate(faces):
            if len(levels) != mips:
                raise ValueError(f"add_texture_cube_encoded: face {f} has {len(levels)} levels, face 0 has {mips}")
            row = []
            for k, level in enumerate(levels):
                level = bytes(level)
                n = max(1, width >> k)
                if len(level) != containers.level_bytes(fmt, n, n):
                    raise ValueError(f"add_texture_cube_encoded: face {f} level {k} has {len(level)} bytes, "
                                     f"{containers.FORMAT_NAMES[fmt]} {n} x {n} takes {containers.level_bytes(fmt, n, n)}")
                row.append(level)
            kept.append(row)
        self._drop_derived_cubes()
        self.cubes.append(_EncodedCube(fmt, width, mips, kept))
        self._cubes_dirty = True
        return len(self.cubes) - 1

    def add_texture_cube_equirect(self, data, width, height, fmt="rgbe8", face_extent=None, mips="maximum"):
        """A cube built on the GPU from ONE equirectangular (latitude / longitude) panorama of width x height texels: `data` = its
        bytes (or a uint8 array), fmt = "rgbe8" (Radiance RGBE as containers.parse_hdr returns it: add_texture_cube_equirect(p["rgbe"],
        p["width"], p["height"])) or an R3N_TEXTURE_* id (one level, as a 2D container stores it).  face_extent = the cube's N
        (default max(1, height // 2)), mips = "maximum" or a level count in 1 .. floor(log2 N) + 1.  The cube holds f32 texels
        whatever the source format.  The cube array is re-sent when the next frame is evaluated
        (r3n_texture_cubes_write_sources).  Returns the cube handle."""
        from . import containers
        width, height = int(width), int(height)
        if not (1 <= width <= 65535 and 1 <= height <= 65535):
            raise ValueError("add_texture_cube_equirect: a panorama's sides are 1 .. 65535")
        if isinstance(fmt, str):
            if fmt != "rgbe8":
                raise ValueError(f"add_texture_cube_equirect: unknown encoding {fmt!r}")
            fmt, need = _ffi.CUBE_ENCODING_RGBE8, width * height * 4
        else:
            fmt = int(fmt)
            if not 0 <= fmt < containers.FORMAT_COUNT:
                raise ValueError(f"add_texture_cube_equirect: unknown format id {fmt}")
            need = containers.level_bytes(fmt, width, height)
        n = max(1, height // 2) if face_extent is None else int(face_extent)
        if not 1 <= n <= 16384:
            raise ValueError("add_texture_cube_equirect: a cube's extent is 1 .. 16384")
        mips = n.bit_length() if mips == "maximum" else int(mips)
        if not 1 <= mips <= n.bit_length():
            raise ValueError(f"add_texture_cube_equirect: {mips} levels, an extent of {n} has 1 .. {n.bit_length()}")
        data = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
        if len(data) != need:
            raise ValueError(f"add_texture_cube_equirect: {len(data)} bytes, a {width} x {height} panorama of this format has {need}")
        self._drop_derived_cubes()
        self.cubes.append(_EquirectCube(fmt, width, height, data, n, mips))
        self._cubes_dirty = True
        return len(self.cubes) - 1

    def environment_mean(self, cube):
        """The mean colour of a cube: the mean of the six 1 x 1 faces of its LAST level (r3n_readback_cube_face), which a cube with a
        full chain has box-filtered down from every texel.  It weighs every texel of a face alike: the box-filtered mean, NOT a
        solid-angle integral (texels near a face's corners cover less of the sphere).  Needs a cube whose last level is 1 x 1.
        environment_lights returns the solid-angle mean (its `ambient`, with max_lights = 0 the mean of the whole level), for any
        cube and pool class."""
        self._flush_cubes()
        if not 0 <= cube < len(self.cubes):
            raise ValueError("environment_mean: no such cube")
        c = self.cubes[cube]
        width, mips = self._cube_extent_and_mips(cube)
        if max(1, width >> (mips - 1)) != 1:
            raise ValueError("environment_mean: the cube's last level is not 1 x 1")
        faces = [self.readback_cube_face(cube, mips - 1, f) for f in range(6)]
        if faces[0].dtype != np.float32:
            raise ValueError("environment_mean: a cube of float texels (an HDR environment)")
        total = np.zeros(4, dtype=np.float32)
        for f in faces:
            total = total + f[1, 1]
        return total / np.float32(6.0)

    def _cube_extent_and_mips(self, cube):
        c = self.cubes[cube]
        return (c.width, c.mips) if isinstance(c, (_EncodedCube, _EquirectCube, _DerivedCube)) else (c[0].shape[1], 1)

    def _drop_derived_cubes(self):
        """A whole-array write replaces the array, the cubes prefilter_environment appended included: they leave the host's list
        when a cube is added (their handles die; a background bound to one is unbound, as the library does)."""
        kept = [c for c in self.cubes if not isinstance(c, _DerivedCube)]
        if len(kept) != len(self.cubes):
            if self._background is not None and self._background < len(self.cubes) and isinstance(self.cubes[self._background], _DerivedCube):
                self._background = None
            self.cubes = kept
            self._cubes_dirty = True

    def prefilter_environment(self, cube, level=None, levels=None):
        """The roughness-prefiltered specular chain and the SH9 irradiance of an environment, built on the GPU from the STORED levels
        of `cube` (r3n_environment_prefilter; DESIGN.md section 2 "Environment prefilter").  level=None: the finest stored level of
        extent <= 256; levels=None: all that fit (the stored levels from `level` on, at most floor(log2 extent) + 1 and 16).  Returns
        (handle, sh): the handle of a NEW cube of float texels appended to the array -- level k filtered for the roughness
        k / (levels - 1), level 0 the source itself -- and sh = float32[9, 3], the radiance coefficients L_lm.  The new cube lives
        until the array is re-sent (any add_texture_cube*).  Not lighting yet: no frame reads it but the skybox node
        (set_background_texture(handle), set_skybox_level)."""
        self._flush_cubes()
        if not 0 <= cube < len(self.cubes):
            raise ValueError("prefilter_environment: no such cube")
        width, mips = self._cube_extent_and_mips(cube)
        if level is None:
            level = next((k for k in range(mips) if max(1, width >> k) <= IBL_MAX_EXTENT), None)
            if level is None:
                raise ValueError(f"prefilter_environment: the cube stores no level of extent <= {IBL_MAX_EXTENT} (its last is {max(1, width >> (mips - 1))})")
        level = int(level)
        if not 0 <= level < mips:
            raise ValueError("prefilter_environment: the cube has no such level")
        extent = max(1, width >> level)
        if levels is None:
            levels = min(mips - level, extent.bit_length(), IBL_MAX_LEVELS)
        params = _ffi.EnvPrefilterParams(int(cube), level, int(levels))
        out = _ffi.EnvPrefilterResult()
        self._check(self.lib.r3n_environment_prefilter(self.ctx, ctypes.addressof(params), ctypes.addressof(out)), "r3n_environment_prefilter")
        self.cubes.append(_DerivedCube(int(out.extent), int(out.levels), cube, level))
        assert int(out.cube_id) == len(self.cubes) - 1
        sh = np.array([[out.sh[m][ch] for ch in range(3)] for m in range(9)], dtype=np.float32)
        return len(self.cubes) - 1, sh

    def environment_probe(self, cube, sh, queries):
        """r3n_environment_probe: the lookups a resolve will call (csrc/ibl_lookup.h) on a list of queries.  sh: float32[9, 3] (or
        [9, 4]) as prefilter_environment returns it; queries: array of ENV_QUERY (dir, roughness, n).  Returns an array of
        ENV_SAMPLE: specular = the cube at lod = roughness * (levels - 1), irradiance = E(n) / pi, and the level and fraction."""
        self._flush_cubes()
        if not 0 <= cube < len(self.cubes):
            raise ValueError("environment_probe: no such cube")
        coeff = np.zeros((9, 4), dtype=np.float32)
        sh = np.asarray(sh, dtype=np.float32)
        if sh.shape not in ((9, 3), (9, 4)):
            raise ValueError("environment_probe: sh is float32[9, 3]")
        coeff[:, :3] = sh[:, :3]
        q = np.ascontiguousarray(queries, dtype=ENV_QUERY)
        out = np.zeros(len(q), dtype=ENV_SAMPLE)
        self._check(self.lib.r3n_environment_probe(self.ctx, int(cube), _ffi.ptr(coeff), _ffi.ptr(q), len(q), _ffi.ptr(out)), "r3n_environment_probe")
        return out

    def set_skybox_level(self, level=None):
        """Which level of the background cube the skybox node draws (r3n_skybox_set_level): None or a negative number = selected
        per pixel, as ever; level >= 0 = that level, clamped to the cube's last, fractions mixing two levels.  A one-level cube
        ignores it.  Sent when the next frame is evaluated."""
        level = -1.0 if level is None else float(level)
        if level != level:
            raise ValueError("set_skybox_level: NaN")
        self._skybox_level = -1.0 if level < 0 else level

    def environment_lights(self, cube, max_lights=4, cone_degrees=6.0, min_share=0.02, level=None, raw=False):
        """Directional lights and an ambient term read out of one level of a cube on the GPU (r3n_environment_lights; DESIGN.md
        section 2 "Environment lights"): at most max_lights (0 .. 16) times the brightest texel not yet taken seeds a cone of
        half-angle cone_degrees (in (0, 60]), which is moved onto the energy centroid of its texels and becomes a light unless it
        holds less than min_share (in [0, 1)) of the level's energy.  level=None: the finest level of extent <= 1024.  Returns
        (lights, ambient): lights = [dict(direction=unit vector TOWARDS the light, irradiance=rgb, solid_angle, texels, seed)],
        brightest seed first; ambient = float32[4], the solid-angle mean radiance of what no light took, alpha 1.  raw=True returns
        the whole _ffi.EnvLightsResult (the integer sums included) instead.  Light extraction, not image-based lighting."""
        self._flush_cubes()
        if not 0 <= cube < len(self.cubes):
            raise ValueError("environment_lights: no such cube")
        if not 0 <= int(max_lights) <= _ffi.ENV_MAX_LIGHTS:
            raise ValueError(f"environment_lights: max_lights is 0 .. {_ffi.ENV_MAX_LIGHTS}")
        if not 0.0 < float(cone_degrees) <= 60.0:
            raise ValueError("environment_lights: cone_degrees is in (0, 60]")
        if not 0.0 <= float(min_share) < 1.0:
            raise ValueError("environment_lights: min_share is in [0, 1)")
        width, mips = self._cube_extent_and_mips(cube)
        if level is None:
            level = next((k for k in range(mips) if max(1, width >> k) <= 1024), None)
            if level is None:
                raise ValueError(f"environment_lights: the cube stores no level of extent <= 1024 (its last is {max(1, width >> (mips - 1))})")
        cone_cos = min(np.float32(math.cos(math.radians(float(cone_degrees)))), np.nextafter(np.float32(1), np.float32(0)))
        params = _ffi.EnvLightsParams(cube, int(level), int(max_lights), float(max(cone_cos, np.float32(0.5))), float(np.float32(min_share)))
        out = _ffi.EnvLightsResult()
        self._check(self.lib.r3n_environment_lights(self.ctx, ctypes.addressof(params), ctypes.addressof(out)), "r3n_environment_lights")
        if raw:
            return out
        lights = [dict(direction=np.array(l.direction[:], dtype=np.float32), irradiance=np.array(l.irradiance[:], dtype=np.float32),
                       solid_angle=float(l.solid_angle), texels=int(l.texels), seed=int(l.seed)) for l in out.lights[:out.n_lights]]
        return lights, np.array(out.ambient[:], dtype=np.float32)

    def add_environment_lights(self, cube, max_lights=4, cone_degrees=6.0, min_share=0.02, level=None, scale=1.0, distance=100.0, resolution=2048):
        """environment_lights, then one add_directional_light(color=irradiance, intensity=scale, direction=-direction to the light)
        per record.  Returns (light ids, scale * ambient): pass the second as `ambient=` to render."""
        lights, ambient = self.environment_lights(cube, max_lights, cone_degrees, min_share, level)
        if len(self.dir_lights) + len(lights) > 16:
            raise ValueError(f"add_environment_lights: {len(lights)} lights on top of {len(self.dir_lights)}: a frame shades at most 16 directional lights")
        ids = [self.add_directional_light(color=tuple(float(v) for v in l["irradiance"]), intensity=float(scale),
                                          direction=tuple(-float(v) for v in l["direction"]), distance=distance, resolution=resolution) for l in lights]
        scaled = ambient * np.float32(scale)
        scaled[3] = np.float32(1.0)
        return ids, scaled

    @staticmethod
    def _pack_cube(payload, cube):
        """appends a cube's bytes to `payload` at a 4-byte boundary -- a stored cube LayerMajor (face by face, a face's levels back to
        back), a panorama as its one level -- and returns the offset"""
        payload += bytes(-len(payload) % 4)
        at = len(payload)
        if isinstance(cube, _EquirectCube):
            payload += cube.data
        elif isinstance(cube, _EncodedCube):
            for levels in cube.faces:
                for level in levels:
                    payload += level
        else:
            payload += cube[0].tobytes()
        return at

    def _flush_cubes_sources(self):
        """the whole array through r3n_texture_cubes_write_sources: stored cubes LayerMajor, panoramas as one level"""
        src = (_ffi.CubeSource * max(len(self.cubes), 1))()
        payload = bytearray()
        for i, cube in enumerate(self.cubes):
            at = self._pack_cube(payload, cube)
            if isinstance(cube, _EquirectCube):
                src[i] = _ffi.CubeSource(_ffi.CUBE_SOURCE_EQUIRECT, cube.fmt, cube.src_width, cube.src_height, cube.width, cube.mips, at)
            elif isinstance(cube, _EncodedCube):
                src[i] = _ffi.CubeSource(_ffi.CUBE_SOURCE_CUBE, cube.fmt, cube.width, cube.width, cube.width, cube.mips, at)
            else:
                faces, srgb = cube
                src[i] = _ffi.CubeSource(_ffi.CUBE_SOURCE_CUBE, 1 if srgb else 0, faces.shape[2], faces.shape[1], faces.shape[1], 1, at)
        data = np.frombuffer(bytes(payload) + bytes(4), dtype=np.uint8)
        self._check(self.lib.r3n_texture_cubes_write_sources(self.ctx, ctypes.addressof(src), len(self.cubes), _ffi.ptr(data), len(payload)),
                    "r3n_texture_cubes_write_sources")

    def replace_texture_cubes(self, cubes):
        """Replaces the whole cube array: `cubes` = [(faces, srgb), ...]; handles are indices into it."""
        if self._background is not None and self._background < len(self.cubes) and isinstance(self.cubes[self._background], _DerivedCube):
            self._background = None
        self.cubes = []
        for faces, srgb in cubes:
            self.add_texture_cube(faces, srgb)
        self._cubes_dirty = True
        if self._background is not None and self._background >= len(self.cubes):
            self._background = None  # (as the library does: a skybox whose cube left the array is unbound)

    def set_background_texture(self, cube):
        """SkyboxRoutine::set_background_texture(Option<TextureCubeHandle>) (rend3-routine/src/skybox.rs): None = no skybox."""
        self._background = cube

    def _flush_cubes_encoded(self):
        """the whole array through r3n_texture_cubes_write_encoded: LayerMajor payload, every cube on a 4-byte boundary"""
        descs = np.zeros((max(len(self.cubes), 1), 8), dtype=np.uint32)
        payload = bytearray()
        for i, cube in enumerate(self.cubes):
            at = self._pack_cube(payload, cube)
            if isinstance(cube, _EncodedCube):
                descs[i, :5] = (at, cube.width, cube.width, cube.mips, cube.fmt)
            else:
                faces, srgb = cube
                descs[i, :5] = (at, faces.shape[2], faces.shape[1], 1, 1 if srgb else 0)
        data = np.frombuffer(bytes(payload) + bytes(4), dtype=np.uint8)
        self._check(self.lib.r3n_texture_cubes_write_encoded(self.ctx, _ffi.ptr(descs), len(self.cubes), _ffi.ptr(data), len(payload)),
                    "r3n_texture_cubes_write_encoded")

    def _flush_cubes(self):
        if self._cubes_dirty and any(isinstance(cube, _EquirectCube) for cube in self.cubes):
            self._flush_cubes_sources()
            self._cubes_dirty = False
            self._background_sent = None
        if self._cubes_dirty and any(isinstance(cube, _EncodedCube) for cube in self.cubes):
            self._flush_cubes_encoded()
            self._cubes_dirty = False
            self._background_sent = None
        if self._cubes_dirty:  # plain cubes only: the RGBA8 entry, as ever
            descs = np.zeros((max(len(self.cubes), 1), 8), dtype=np.uint32)
            at = 0
            for i, (faces, srgb) in enumerate(self.cubes):
                descs[i, :5] = (at, faces.shape[2], faces.shape[1], 1, 1 if srgb else 0)
                at += faces.size // 4
            texels = (np.concatenate([f.reshape(-1) for f, _ in self.cubes]) if self.cubes else np.zeros(4, dtype=np.uint8)).view(np.uint32)
            self._check(self.lib.r3n_texture_cubes_write(self.ctx, _ffi.ptr(descs), len(self.cubes), _ffi.ptr(np.ascontiguousarray(texels)), at),
                        "r3n_texture_cubes_write")
            self._cubes_dirty = False
            self._background_sent = None  # (the library unbinds a skybox whose cube left the array)
        if self._background_sent is None or self._background_sent[0] != self._background:
            self._check(self.lib.r3n_skybox_set(self.ctx, 0 if self._background is None else int(self._background) + 1), "r3n_skybox_set")
            self._background_sent = (self._background,)
        if self._skybox_level_sent != self._skybox_level:
            self._check(self.lib.r3n_skybox_set_level(self.ctx, float(self._skybox_level)), "r3n_skybox_set_level")
            self._skybox_level_sent = self._skybox_level

    def add_material(self, record, key=OPAQUE):
        idx = len(self.materials)
        self.materials.append((np.asarray(record, dtype=f32), key))
        slots = np.array([idx], dtype=np.uint32)
        rec = np.ascontiguousarray(record, dtype=f32).reshape(1, 52)
        keys = np.array([key], dtype=np.uint8)
        self._check(self.lib.r3n_materials_write(self.ctx, _ffi.ptr(slots), _ffi.ptr(rec), _ffi.ptr(keys), 1),
                    "r3n_materials_write")
        return idx

    def update_material(self, handle, record, key=None):
        """Renderer::update_material: rewrites the material's 208-B record in place (r3n_materials_write orders itself
        after a resolve still in flight)."""
        key = self.materials[handle][1] if key is None else key
        if key != self.materials[handle][1]:
            self._blend_cache = None  # the material moved into / out of the transparent pass
        self.materials[handle] = (np.asarray(record, dtype=f32), key)
        slots = np.array([handle], dtype=np.uint32)
        rec = np.ascontiguousarray(record, dtype=f32).reshape(1, 52)
        keys = np.array([key], dtype=np.uint8)
        self._check(self.lib.r3n_materials_write(self.ctx, _ffi.ptr(slots), _ffi.ptr(rec), _ffi.ptr(keys), 1), "r3n_materials_write")

    def update_directional_light(self, handle, **changes):
        """Renderer::update_directional_light with a DirectionalLightChange (only the given fields change)."""
        self.dir_lights[handle].update(changes)
        self._lights_version += 1

    def update_point_light(self, handle, **changes):
        self.point_lights[handle].update(changes)
        self._lights_version += 1

    def _alloc_handle(self):
        if self.free_handles:
            return self.free_handles.pop(0)
        h = self.next_handle
        self.next_handle += 1
        return h

    def _use_index(self, idx):
        cap = self.capacity
        if idx > cap:  # freelist/buffer.rs:48-52
            cap = 1 << (int(idx) - 1).bit_length()
        while cap <= idx:
            cap *= 2
        self.capacity = cap

    def _object_record(self, h):
        meta = self.object_meta[h]
        mesh = self.meshes[meta["mesh"]]
        rec = np.zeros(32, dtype=np.uint32)
        rf = rec.view(f32)
        rf[0:16] = meta["transform"]
        radius = mesh.radius if meta.get("morph_instance") is None else self.morph_radius(meta["morph_instance"])
        c, r = host.bounding_sphere_apply_transform(mesh.centre, radius, meta["transform"])
        rf[16:19] = c
        rf[19] = r
        rec[20], rec[21], rec[22] = mesh.first_index, mesh.index_count, meta["material"]
        rec[23:29] = mesh.attr_off
        if meta.get("morph") is not None:  # the morph instance's runs override the mesh's, as a skeleton's do
            for a, off in enumerate(self.morphs[meta["morph"]]["out_off"]):
                if off != INVALID:
                    rec[23 + a] = off
        if meta.get("skeleton") is not None:  # object.rs:250-258: skeleton ranges override the mesh's
            for a, off in enumerate(self.skeletons[meta["skeleton"]]["out_off"]):
                if off != INVALID:
                    rec[23 + a] = off
        rec[29] = 1 if meta["enabled"] else 0
        return rec

    def _mark(self, h, rec):
        self.world_version += 1  # an object was added / moved / removed (parallel.Exchange: host-side bounds are stale)
        self._blend_cache = None
        self._use_index(h)
        self.dirty_objects[h] = rec

    def _write_objects(self, items, force_capacity=False):
        if not items and not force_capacity:
            return
        slots = np.array([h for h, _ in items], dtype=np.uint32)
        recs = np.ascontiguousarray(np.stack([r for _, r in items]) if items else np.zeros((0, 32), dtype=np.uint32))
        self.object_writes += 1 if len(slots) else 0
        self._check(self.lib.r3n_objects_write(self.ctx, _ffi.ptr(slots) if len(slots) else None,
                                               _ffi.ptr(recs) if len(slots) else None, len(slots), self.capacity),
                    "r3n_objects_write")

    def write_object_records(self, slots, records, capacity, blend=None):
        """Bulk edit for tests and tools: r3n_object128 rows (32 u32 words each) written as they are to `slots` with ONE
        r3n_objects_write, the object buffer then `capacity` slots long (any number).  The per-object mirror is REPLACED, not
        updated: afterwards it knows only `blend` -- {slot: (material index, sorting location)} of the enabled objects the
        transparent pass has to order -- so a context written this way is not edited through add_object / remove_object."""
        if self.dirty_objects or self.pending_free or self.deferred_removals:
            raise RuntimeError("write_object_records: the context has object edits of its own pending")
        slots = np.ascontiguousarray(slots, dtype=np.uint32).reshape(-1)
        records = np.ascontiguousarray(records, dtype=np.uint32).reshape(len(slots), 32)
        if len(slots):
            self.object_writes += 1
            self._check(self.lib.r3n_objects_write(self.ctx, _ffi.ptr(slots), _ffi.ptr(records), len(slots), int(capacity)), "r3n_objects_write")
        self.capacity = self._capacity_sent = int(capacity)
        self.object_meta = {int(h): dict(enabled=True, material=int(m), location=np.asarray(loc, dtype=f32).copy())
                            for h, (m, loc) in (blend or {}).items()}
        self._blend_cache = None
        self.world_version += 1

    def add_object(self, mesh, material, transform, skeleton=None, morph=None):
        """morph: a morph instance (add_morph_instance) -- the object draws the instance's runs; with skeleton= the skeleton's
        own morph instance (add_skeleton(..., morph=)) applies instead."""
        if skeleton is not None and morph is not None:
            raise ValueError("add_object: bind the morph instance to the skeleton (add_skeleton(..., morph=))")
        h = self._alloc_handle()
        if skeleton is not None:
            mesh = self.skeletons[skeleton]["mesh"]
        elif morph is not None:
            mesh = self.morphs[morph]["mesh"]
        # morph_instance: the instance whose weights widen this object's bounding sphere
        morph_instance = morph if skeleton is None else self.skeletons[skeleton]["morph"]
        self.object_meta[h] = dict(mesh=mesh, material=material, transform=np.asarray(transform, dtype=f32).copy(),
                                   enabled=True, skeleton=skeleton, morph=morph, morph_instance=morph_instance)
        if morph_instance is not None:
            self.morphs[morph_instance]["objects"].append(h)
        rec = self._object_record(h)
        self._mark(h, rec)
        # object.rs:273: a new object's sorting location is its transformed bounding-sphere centre
        self.object_meta[h]["location"] = rec.view(f32)[16:19].copy()
        self.object_meta[h]["sphere"] = rec.view(f32)[16:20].copy()  # world-space bounding sphere (multi-GPU partitioning)
        return h

    def add_objects_bulk(self, mesh_ids, material_ids, transforms):
        """Vectorised add_object for large synthetic scenes (same records as add_object, built by the C++ host mirror)."""
        n = len(mesh_ids)
        transforms = np.ascontiguousarray(transforms, dtype=f32).reshape(n, 16)
        desc = np.zeros((n, 4), dtype=f32)
        mu = np.zeros((n, 8), dtype=np.uint32)
        for i, mid in enumerate(mesh_ids):
            m = self.meshes[mid]
            desc[i, :3], desc[i, 3] = m.centre, m.radius
            mu[i, 0], mu[i, 1] = m.first_index, m.index_count
            mu[i, 2:8] = m.attr_off
        mats = np.ascontiguousarray(material_ids, dtype=np.uint32)
        recs = np.zeros((n, 32), dtype=np.uint32)
        self.lib.r3n_host_build_object_records(n, _ffi.ptr(transforms), _ffi.ptr(desc), _ffi.ptr(mu), _ffi.ptr(mats), _ffi.ptr(recs))
        handles = []
        for i in range(n):
            h = self._alloc_handle()
            self.object_meta[h] = dict(mesh=int(mesh_ids[i]), material=int(material_ids[i]), transform=transforms[i], enabled=True,
                                       location=recs[i].view(f32)[16:19].copy(), sphere=recs[i].view(f32)[16:20].copy())
            self._mark(h, recs[i])
            handles.append(h)
        return handles

    def set_object_transform(self, h, transform):
        self.object_meta[h]["transform"] = np.asarray(transform, dtype=f32).copy()
        rec = self._object_record(h)
        self.object_meta[h]["sphere"] = rec.view(f32)[16:20].copy()
        self._mark(h, rec)
        # object.rs:313: after a transform update the sorting location is the translation
        self.object_meta[h]["location"] = self.object_meta[h]["transform"][12:15].copy()

    def remove_object(self, h):
        self.object_meta[h]["enabled"] = False  # object.rs:330-342: disabled now, removed next frame
        self._mark(h, self._object_record(h))
        self.deferred_removals.append(h)

    def add_directional_light(self, color=(1, 1, 1), intensity=1.0, direction=(0, -1, 0), distance=100.0,
                              resolution=2048):
        self.dir_lights.append(dict(color=color, intensity=intensity, direction=direction, distance=distance,
                                    resolution=resolution))
        self._lights_version += 1
        return len(self.dir_lights) - 1

    def add_point_light(self, position, color=(1, 1, 1), intensity=1.0, radius=1.0):
        self.point_lights.append(dict(position=position, color=color, intensity=intensity, radius=radius))
        self._lights_version += 1
        return len(self.point_lights) - 1

    def set_camera_data(self, view, projection):
        """Renderer::set_camera_data: the CameraState (camera.rs:23-85) is derived when something asks for it -- in the one-call
        frame path that is r3n_host_evaluate_frame, in C++."""
        self._camera_inputs = (view, projection)
        self._camera = None

    @property
    def camera(self):
        if self._camera is None:
            self._camera = host.CameraState(self._camera_inputs[0], self._camera_inputs[1], self.handedness, self.aspect_ratio)
        return self._camera

    def current_view_proj(self):
        """view_proj of the camera the last evaluated frame used (f32[16], column-major)."""
        if self._fc is not None and not self.frame_nodes:
            return np.array(self._fc["frame"].view_proj[:], dtype=f32)
        return self.camera.view_proj

    def current_resolution(self):
        return self._resolution

    def set_object_owners(self, owners, rank):
        """Multi-GPU sharding by owner byte (parallel.partition_objects_spatial): this rank culls / draws the slots it owns."""
        owners = np.ascontiguousarray(owners, dtype=np.uint8)
        self._check(self.lib.r3n_set_object_owners(self.ctx, owners.ctypes.data if len(owners) else None, len(owners), rank), "r3n_set_object_owners")

    def comm_init(self, rank, world, share):
        """Multi-GPU, native (r3n_comm_init): the sort-first exchanges are issued by the library itself over RCCL inside
        r3n_render_frame -- no exchange object, no host-language collective on the frame path.  `share(ids or None) -> ids`: hands
        rank 0's communicator ids (bytes) to every rank (comm_init_torch passes them through torch.distributed).  Collective."""
        n = _ffi.COMM_IDS * _ffi.COMM_ID_BYTES
        ids = None
        if rank == 0:
            buf = (ctypes.c_uint8 * n)()
            for k in range(_ffi.COMM_IDS):
                self._check(self.lib.r3n_comm_unique_id(ctypes.byref(buf, k * _ffi.COMM_ID_BYTES)), "r3n_comm_unique_id")
            ids = bytes(buf)
        ids = share(ids)
        assert isinstance(ids, (bytes, bytearray)) and len(ids) == n
        self._check(self.lib.r3n_comm_init(self.ctx, (ctypes.c_uint8 * n).from_buffer_copy(ids), rank, world), "r3n_comm_init")
        self._comm = (int(rank), int(world))

    def comm_init_torch(self, group=None):
        import torch.distributed as dist

        def share(ids):
            box = [ids]
            dist.broadcast_object_list(box, src=0 if group is None else dist.get_global_rank(group, 0), group=group)
            return box[0]
        self.comm_init(dist.get_rank(group), dist.get_world_size(group), share)

    def comm_set_split(self, by_objects):
        """The split the library's own exchanges implement (r3n_comm_set_split): False = sort-first rows (what comm_init selects),
        True = object ranges (set_object_range / owners): depth MAX all-reduce in front of Hi-Z + key MAX reduce-scatter behind
        pass 2, issued by r3n_render_frame."""
        self._check(self.lib.r3n_comm_set_split(self.ctx, 0 if by_objects else 1), "r3n_comm_set_split")

    def comm_destroy(self):
        self._check(self.lib.r3n_comm_destroy(self.ctx), "r3n_comm_destroy")
        self._comm = None

    def set_object_range(self, begin, end):
        """Multi-GPU sharding (not in the reference): this rank culls/draws object slots [begin, end)."""
        self._check(self.lib.r3n_set_object_range(self.ctx, begin, end), "r3n_set_object_range")

    def set_camera_object_range(self, camera, begin, end):
        """This camera's own object range (a shadow view owned whole by one rank draws every slot there)."""
        self._check(self.lib.r3n_set_camera_object_range(self.ctx, camera, begin, end), "r3n_set_camera_object_range")

    # ------------------------------------------------------------------ per-frame evaluation
    def evaluate_instructions(self):
        self._flush_textures(before_frame=True)
        self._flush_cubes()
        self._compact_meshes_before_frame()
        return self._evaluate_instructions()

    def _compact_meshes_before_frame(self):
        """mesh_compact=f: after a block was added or removed, r3n_mesh_compact when more than f of the buffer below its mark is holes"""
        if self._mesh_compact is None or not self._mesh_edits:
            return
        self._mesh_edits = False
        st = self.mesh_stats()
        if st["pool_words"] - st["live_words"] > self._mesh_compact * st["pool_words"]:
            self.compact_meshes()

    def _flush_objects(self):
        """ObjectManager::evaluate (object.rs:344-364): last frame's removals become real, dirty records are scattered."""
        for h in self.pending_free:
            self.dirty_objects[h] = np.zeros(32, dtype=np.uint32)  # unwrap_or_default(), object.rs:363
            self.object_meta.pop(h, None)
            self.free_handles.append(h)
        self.pending_free = self.deferred_removals
        self.deferred_removals = []
        if self.dirty_objects or self._capacity_sent != self.capacity:
            self._write_objects(sorted(self.dirty_objects.items()), force_capacity=True)
            self.dirty_objects = {}
            self._capacity_sent = self.capacity

    def _evaluate_instructions(self):
        """Renderer::evaluate_instructions (rend3/src/renderer/eval.rs:9-187), path subset: flush dirty objects,
        evaluate lights -> shadow cameras + atlas + light buffers."""
        self._flush_objects()
        size, shadows, dir_buf = host.evaluate_directional_lights(self.dir_lights, self.camera)
        point_buf = host.point_light_buffer(self.point_lights)
        self._check(self.lib.r3n_lights_write(self.ctx, _ffi.ptr(dir_buf), dir_buf.nbytes, _ffi.ptr(point_buf),
                                              point_buf.nbytes), "r3n_lights_write")
        self._dir_buf, self._point_buf = dir_buf, point_buf
        self._write_blend_order(self.camera.location)
        return EvalOutput(shadows, size)

    def _sort_blend_order(self, camera_location):
        """blend_sort == "gpu": the blend set is sent when it changed -- a blend object came, went or moved --, and the order is
        sorted on the device for this frame's camera location.  No per-object work in a frame without a world edit."""
        if self._blend_cache is None or self._blend_sent is None:  # the world was edited / the mode was switched to "gpu"
            self._blend_cache = [h for h, m in sorted(self.object_meta.items())
                                 if m["enabled"] and self.materials[m["material"]][1] == BLEND]
            slots = np.asarray(self._blend_cache, dtype=np.uint32)
            locs = np.ascontiguousarray([self.object_meta[h]["location"] for h in self._blend_cache], dtype=f32).reshape(-1, 3)
            sent = self._blend_sent
            if sent is None or not (np.array_equal(sent[0], slots) and np.array_equal(sent[1].view(np.uint32), locs.view(np.uint32))):
                if len(slots) or self._had_blend:
                    self._check(self.lib.r3n_blend_objects_write(self.ctx, _ffi.ptr(slots) if len(slots) else None,
                                                                 _ffi.ptr(locs) if len(slots) else None, len(slots)),
                                "r3n_blend_objects_write")
                self._blend_sent = (slots, locs)
        if self._blend_cache:
            cam = np.ascontiguousarray(camera_location, dtype=f32)
            self._check(self.lib.r3n_blend_sort(self.ctx, _ffi.ptr(cam)), "r3n_blend_sort")
        self._had_blend = bool(self._blend_cache)

    def readback_blend_order(self):
        """(order, rank_base): the draw order the transparent pass reads and the scan of its triangle counts (parity tap)."""
        n = len(self._blend_cache or ())
        order, rank = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        self._check(self.lib.r3n_readback_blend_order(self.ctx, _ffi.ptr(order), _ffi.ptr(rank), n), "r3n_readback_blend_order")
        return order[:n], rank

    def _write_blend_order(self, camera_location):
        if self.blend_sort == "gpu":
            return self._sort_blend_order(camera_location)
        self._blend_sent = None  # (host order mode replaces whatever set the library holds)
        # the CPU batcher's back-to-front order of the blend-key objects (batching.rs:146-176), every frame
        if self._blend_cache is None:  # rebuilt only after objects / materials changed
            self._blend_cache = [h for h, m in sorted(self.object_meta.items())
                                 if m["enabled"] and self.materials[m["material"]][1] == BLEND]
        blend = self._blend_cache
        order = host.blend_draw_order(camera_location, blend, [self.object_meta[h]["location"] for h in blend]) if blend else []
        if order or self._had_blend:
            arr = np.asarray(order, dtype=np.uint32)
            self._check(self.lib.r3n_blend_order_write(self.ctx, _ffi.ptr(arr) if len(arr) else None, len(arr)), "r3n_blend_order_write")
        self._had_blend = bool(order)

    # ------------------------------------------------------------------ convenience: one whole frame
    def render(self, width, height, samples=1, ambient=(0, 0, 0, 0), clear_color=(0, 0, 0, 0), readback=True,
               base=None, exchange=None):
        """The reference's per-frame driver (rend3-test/src/runner.rs:121-169): evaluate, build the graph with
        BaseRenderGraph::add_to_graph, execute.  `readback` additionally pulls the parity taps."""
        self._resolution = (width, height)
        comm = getattr(self, "_comm", None)
        if comm is not None and (self.frame_nodes or exchange is not None):
            raise RuntimeError("comm_init: the library issues the exchanges inside r3n_render_frame (no exchange object, no per-node frame)")
        if not self.frame_nodes:
            eval_output = self.render_frame(width, height, samples, ambient, clear_color, exchange,
                                            viewport_first=bool(base is not None and base.viewport_first))
            if not readback:
                return None
            owned = None
            if exchange is not None and hasattr(exchange, "owns_shadow_view"):
                owned = {si for si in range(len(eval_output.shadows)) if exchange.owns_shadow_view(si)}
            elif comm is not None:
                owned = {si for si in range(len(eval_output.shadows)) if si % comm[1] == comm[0]}
            return self.readback_frame(eval_output, width, height, samples, owned)
        eval_output = self.evaluate_instructions()
        base = base or BaseRenderGraph(self)
        graph = RenderGraph()
        inputs = BaseRenderGraphInputs(eval_output, base.default_routines(), (width, height), samples)
        base.add_to_graph(graph, inputs, BaseRenderGraphSettings(ambient, clear_color), exchange=exchange)
        graph.execute(self, eval_output)
        if not readback:
            return None
        owned = None
        if exchange is not None and hasattr(exchange, "owns_shadow_view"):
            owned = {si for si in range(len(eval_output.shadows)) if exchange.owns_shadow_view(si)}
        return self.readback_frame(eval_output, width, height, samples, owned)

    # ------------------------------------------------------------------ the frame in two C calls
    def render_frame(self, width, height, samples=1, ambient=(0, 0, 0, 0), clear_color=(0, 0, 0, 0), exchange=None,
                     viewport_first=False):
        """evaluate_instructions + BaseRenderGraph::add_to_graph + RenderGraph::execute with the host out of the loop: the CPU
        half (camera state, shadow cameras + atlas, light buffer, frame uniforms, camera headers) is r3n_host_evaluate_frame, the
        node list r3n_render_frame.  Same inputs, same results as the node-by-node path (R3N_FRAME_NODES=1); returns the
        EvalOutput (shadow layout) the read-backs want."""
        import ctypes as ct
        lib = self.lib
        fc = self._fc
        if fc is None:
            fc = self._fc = dict(cam=_ffi.HostCamera144(), frame=_ffi.HostFrame(), desc=_ffi.FrameDesc(), lights=None, lights_version=-1,
                                 point=None, ambient=(ct.c_float * 4)(), cb=None, cb_for=None, error=None)
            d = fc["desc"]
            d.struct_size = ct.sizeof(_ffi.FrameDesc)
            fr = fc["frame"]
            base = ct.addressof(fr)
            d.uniforms = base + _ffi.HostFrame.uniforms.offset
            d.viewport_header = base + _ffi.HostFrame.viewport_header.offset
            d.shadow_views = base + _ffi.HostFrame.shadow_views.offset
            d.directional_buffer = base + _ffi.HostFrame.directional_buffer.offset
        self._flush_textures(before_frame=True)
        self._flush_cubes()
        self._compact_meshes_before_frame()
        self._flush_objects()
        self._flush_morphs()  # morph, then skin (the skinning node is inside r3n_render_frame)
        cam, fr, d = fc["cam"], fc["frame"], fc["desc"]
        view, projection = self._camera_inputs
        ct.memmove(cam.view, np.ascontiguousarray(view, dtype=f32).ctypes.data, 64)
        kind = projection[0]
        cam.handedness = 1 if self.handedness == host.RIGHT else 0
        cam.aspect_ratio = 0.0 if self.aspect_ratio is None else float(self.aspect_ratio)
        if kind == "perspective":
            cam.projection_kind = 1
            cam.projection_params[0], cam.projection_params[1] = projection[1], projection[2]
        elif kind == "orthographic":
            cam.projection_kind = 0
            cam.projection_params[0], cam.projection_params[1], cam.projection_params[2] = projection[1]
        elif kind == "raw":
            cam.projection_kind = 2
            ct.memmove(cam.projection_params, np.ascontiguousarray(projection[1], dtype=f32).ctypes.data, 64)
        else:
            raise ValueError(kind)
        if fc["lights_version"] != self._lights_version:
            la = np.zeros((max(len(self.dir_lights), 1), 12), dtype=f32)
            for i, l in enumerate(self.dir_lights):
                if l is None:
                    continue
                la[i, 0:3], la[i, 3] = l["color"], l["intensity"]
                la[i, 4:7], la[i, 7] = l["direction"], l["distance"]
                la[i, 8:9].view(np.uint32)[0] = l["resolution"]
            fc["lights"] = la
            fc["point"] = np.ascontiguousarray(host.point_light_buffer(self.point_lights))
            fc["lights_version"] = self._lights_version
        amb = fc["ambient"]
        amb[0], amb[1], amb[2], amb[3] = ambient
        if lib.r3n_host_evaluate_frame(ct.byref(cam), fc["lights"].ctypes.data, len(self.dir_lights), 16384, amb, width, height, samples,
                                       self.capacity, ct.byref(fr)) != 0:
            raise _ffi.R3nError("r3n_host_evaluate_frame: more shadow-casting lights than R3N_MAX_SHADOW_VIEWS")
        n_views = fr.n_shadow_views
        shadows = [dict(offset=(fr.shadow_views[k].x, fr.shadow_views[k].y), size=fr.shadow_views[k].size, handle=fr.shadow_handles[k])
                   for k in range(n_views)]
        ev = EvalOutput(shadows, (fr.shadow_atlas_width, fr.shadow_atlas_height))
        if self._blend_cache is None or self._blend_cache or self._had_blend:
            self._write_blend_order(np.array(fr.camera_location[:], dtype=f32))
        d.flags = _ffi.FRAME_VIEWPORT_FIRST if viewport_first else 0
        d.width, d.height, d.samples = width, height, samples
        d.shadow_atlas_width, d.shadow_atlas_height, d.n_shadow_views = fr.shadow_atlas_width, fr.shadow_atlas_height, n_views
        d.clear_color[0], d.clear_color[1], d.clear_color[2], d.clear_color[3] = clear_color
        d.directional_bytes = fr.directional_bytes
        d.point_buffer, d.point_bytes = fc["point"].ctypes.data, fc["point"].nbytes
        d.shadow_view_mask = 0
        if exchange is not None and hasattr(exchange, "owns_shadow_view"):
            d.flags |= _ffi.FRAME_SHADOW_MASK
            d.shadow_view_mask = sum(1 << v for v in range(n_views) if exchange.owns_shadow_view(v))
        keep = None
        if self._has_skeletons():  # skinning (base.rs:145, skinning.rs:211-226)
            sk_in, sk_m = self.skinning_buffers()
            poses = self._pose_requests()
            if len(poses):
                self._check(lib.r3n_pose_skeletons(self.ctx, _ffi.ptr(np.ascontiguousarray(poses)), len(poses)), "r3n_pose_skeletons")
            keep = (sk_in, sk_m)
            d.skin_inputs, d.n_skeletons, d.joint_matrices, d.n_joint_matrices = sk_in.ctypes.data, len(sk_in), sk_m.ctypes.data, len(sk_m)
        else:
            d.skin_inputs, d.n_skeletons, d.joint_matrices, d.n_joint_matrices = None, 0, None, 0
        if exchange is not None:
            state = dict(ev=ev, samples=samples)
            fc["cb_state"] = state
            if fc["cb_for"] is not exchange:
                def callback(_user, site, _self=self, _fc=fc, _exchange=exchange):
                    try:
                        st = _fc["cb_state"]
                        _exchange(_ffi.EXCHANGE_SITES[site], _self, ev=st["ev"], samples=st["samples"])
                        return 0
                    except BaseException as e:  # never unwind through the C frames
                        _fc["error"] = e
                        return -1
                fc["cb"], fc["cb_for"] = _ffi.EXCHANGE_FN(callback), exchange
            d.exchange = fc["cb"]
        else:
            d.exchange = _ffi.EXCHANGE_FN()
        code = lib.r3n_render_frame(self.ctx, ct.byref(d))
        del keep
        if fc["error"] is not None:
            err, fc["error"] = fc["error"], None
            raise err
        self._check(code, "r3n_render_frame")
        return ev

    def readback_frame(self, eval_output, width, height, samples=1, owned_views=None):
        lib, ctx = self.lib, self.ctx
        cap = self.capacity
        out = {"capacity": cap, "shadows": []}
        total = int(sum(self.meshes[m["mesh"]].index_count // 3 for m in self.object_meta.values() if m["enabled"]))

        def cam_sets(cam):
            visible = np.zeros(cap, dtype=np.uint8)
            self._check(lib.r3n_readback_visible_objects(ctx, cam, _ffi.ptr(visible), cap), "readback_visible_objects")
            p = np.zeros(max(total, 1), dtype=np.uint8)
            r = np.zeros(max(total, 1), dtype=np.uint8)
            self._check(lib.r3n_readback_triangle_sets(ctx, cam, _ffi.ptr(p), _ffi.ptr(r), len(p)), "readback_triangle_sets")
            calls = np.zeros((6, 5), dtype=np.uint32)
            self._check(lib.r3n_readback_draw_calls(ctx, cam, _ffi.ptr(calls)), "readback_draw_calls")
            baked = np.zeros((cap, 32), dtype=f32)
            self._check(lib.r3n_readback_baked(ctx, cam, _ffi.ptr(baked), cap), "readback_baked")
            return dict(visible=visible, residual=r, draw_calls=calls, baked=baked, **{"pass": p})

        if cap and self.object_meta:
            for si in range(len(eval_output.shadows)):
                # (multi-GPU: a shadow view this rank does not own was never culled here)
                out["shadows"].append(cam_sets(si) if owned_views is None or si in owned_views else None)
            out.update(cam_sets(_ffi.CAMERA_VIEWPORT))
        vis = np.zeros((height, width) if samples == 1 else (height, width, samples), dtype=np.uint64)
        self._check(lib.r3n_readback_visibility(ctx, _ffi.ptr(vis)), "readback_visibility")
        aw, ah = eval_output.shadow_target_size
        atlas = np.zeros((ah, aw), dtype=f32)
        self._check(lib.r3n_readback_shadow_atlas(ctx, _ffi.ptr(atlas)), "readback_shadow_atlas")
        hdr16 = np.zeros((height, width, 4), dtype=np.uint16)
        self._check(lib.r3n_readback_hdr(ctx, _ffi.ptr(hdr16)), "readback_hdr")
        rgba8 = np.zeros((height, width, 4), dtype=np.uint8)
        rgba_f = np.zeros((height, width, 4), dtype=f32)
        self._check(lib.r3n_readback_output(ctx, _ffi.ptr(rgba8), _ffi.ptr(rgba_f)), "readback_output")
        out.update(vis=vis, atlas=atlas, atlas_size=(aw, ah), hdr16=hdr16, rgba8=rgba8, rgba_f32=rgba_f)
        return out

    def readback_triangle_lists(self, cam, which):
        """r3n_readback_triangle_lists (a test and diagnostic entry): the predicted (`which` 0) or residual (1) list of `cam`'s last
        cull as the device holds it.  Returns (refs, counts, subcap): refs (n, 2) u32 rows (object, triangle), the regions'
        entries concatenated in (material key, sub-list) order and never re-sorted; counts (3, R3N_SUBQ) u32; the entries
        reserved per region.  A count above subcap leaves the rows beyond the region 0xFFFFFFFF."""
        counts, subcap = np.zeros((3, 32), dtype=np.uint32), ctypes.c_uint32()
        lib, args = self.lib, (self.ctx, int(cam), int(which))
        self._check(lib.r3n_readback_triangle_lists(*args, None, 0, _ffi.ptr(counts), ctypes.byref(subcap)), "r3n_readback_triangle_lists")
        n = int(counts.sum(dtype=np.uint64))
        refs = np.full((n, 2), 0xFFFFFFFF, dtype=np.uint32)
        if n:
            self._check(lib.r3n_readback_triangle_lists(*args, _ffi.ptr(refs), n, _ffi.ptr(counts), ctypes.byref(subcap)), "r3n_readback_triangle_lists")
        return refs, counts, int(subcap.value)

    def raster_stats(self):
        """r3n_readback_raster_stats: work items each r3n_forward call of the last frame queued, [0..16) the viewport's, then 12 per
        shadow lane -- counted as requested, so a call above 32 x the sub-queue capacity overflowed a sub-queue."""
        out = np.zeros(64, dtype=np.uint32)
        self._check(self.lib.r3n_readback_raster_stats(self.ctx, _ffi.ptr(out)), "r3n_readback_raster_stats")
        return out

    def readback_mesh_words(self, byte_offset, n_words):
        out = np.zeros(n_words, dtype=np.uint32)
        self._check(self.lib.r3n_readback_mesh(self.ctx, byte_offset, _ffi.ptr(out), out.nbytes), "r3n_readback_mesh")
        return out

    def set_output_format(self, fmt):
        """TonemappingRoutine's output_format: 0 Rgba8UnormSrgb (default), 1 Bgra8UnormSrgb, 2 Rgba8Unorm, 3 Bgra8Unorm."""
        self._check(self.lib.r3n_set_output_format(self.ctx, int(fmt)), "r3n_set_output_format")
        self.output_format = int(fmt)

    def set_tonemapping(self, operator="blit", exposure_ev=0.0, white=4.0, auto_exposure=None, dt=1.0 / 60.0):
        """What rend3-routine/src/tonemapping.rs:1-10 announces: an exposure and an operator ("blit" | "reinhard" | "aces") in front
        of the blit's transfer (r3n_tonemap_set).  exposure_ev: stops (with auto_exposure: compensation added to the metered value);
        white: Reinhard's white point; auto_exposure: an AutoExposure, metered on the GPU from a luminance histogram of the HDR
        target -- its `speed` per second and the frame interval `dt` give the share of the distance to the target covered per
        frame, adapt = 1 - exp(-dt * speed).  Between frames only; setting anything restarts the adaptation (the next frame adapts
        instantly).  set_tonemapping() with the defaults is the reference's behaviour: the blit stays fused into the resolve."""
        o = tonemap_opts(operator, exposure_ev, white, auto_exposure, dt)
        self._check(self.lib.r3n_tonemap_set(self.ctx, ctypes.byref(o)), "r3n_tonemap_set")

    def readback_exposure(self):
        """What the last tonemapping node produced (waits for it): dict(histogram (256,) uint32, excluded, valid, mean_log2,
        target_ev, current_ev, scale)."""
        st = _ffi.ExposureState()
        self._check(self.lib.r3n_readback_exposure(self.ctx, ctypes.byref(st)), "r3n_readback_exposure")
        return dict(histogram=np.array(st.histogram[:], dtype=np.uint32), excluded=int(st.excluded), valid=int(st.valid),
                    mean_log2=f32(st.mean_log2), target_ev=f32(st.target_ev), current_ev=f32(st.current_ev), scale=f32(st.scale))

    def set_bloom(self, intensity=0.04, threshold=1.0, knee=0.5, scatter=0.7, max_levels=8):
        """Bloom in front of the tonemapping operator (r3n_bloom_set; hangs on rend3-routine/src/tonemapping.rs:1-10 like the
        operators): what is brighter than `threshold` in exposed units (1 = display white, under auto-exposure too), with a soft
        `knee` around it, is spread through a pyramid of at most `max_levels` levels -- `scatter` is the share of each coarser level
        added on the way up -- and added back times `intensity`.  set_bloom(None), or an intensity of 0, switches it off: the
        frame is then what it is without it, launch for launch.  Between frames only; independent of set_tonemapping."""
        if intensity is None:
            self._check(self.lib.r3n_bloom_set(self.ctx, None), "r3n_bloom_set")
            return
        o = bloom_opts(intensity, threshold, knee, scatter, max_levels)
        self._check(self.lib.r3n_bloom_set(self.ctx, ctypes.byref(o)), "r3n_bloom_set")

    def readback_bloom(self, level):
        """Level `level` of the bloom pyramid as the last tonemapping node left it (waits for it): (h, w, 3) uint16 half bits.
        Levels past the last one read the down chain, which is kept under R3N_TUNE bloom_keep_down=1 only."""
        w, h, n = _ffi.u32(0), _ffi.u32(0), _ffi.u32(0)
        self._check(self.lib.r3n_readback_bloom(self.ctx, int(level), None, 0, ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)), "r3n_readback_bloom")
        out = np.zeros((h.value, w.value, 3), dtype=np.uint16)
        self._check(self.lib.r3n_readback_bloom(self.ctx, int(level), _ffi.ptr(out), out.size // 3, ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)),
                    "r3n_readback_bloom")
        return out

    def bloom_levels(self):
        """Number of levels of the pyramid the last tonemapping node built."""
        n = _ffi.u32(0)
        self._check(self.lib.r3n_readback_bloom(self.ctx, 0, None, 0, None, None, ctypes.byref(n)), "r3n_readback_bloom")
        return int(n.value)

    def set_skinning_mode(self, mode):
        """0 = R3N_SKIN_EXACT (vector ALU, default), 1 = R3N_SKIN_MFMA (matrix cores; rigs of at most four joints)."""
        self._check(self.lib.r3n_set_skinning_mode(self.ctx, int(mode)), "r3n_set_skinning_mode")

    def set_shade_mode(self, mode):
        """0 = R3N_SHADE_EXACT (default, bit-identical to the oracle), 1 = R3N_SHADE_FAST (fused / approximate shading arithmetic,
        framebuffer within 1e-3 after tonemap)."""
        self._check(self.lib.r3n_set_shade_mode(self.ctx, int(mode)), "r3n_set_shade_mode")

    def readback_joint_matrices(self):
        """The joint matrices the last skinning pass read (host-provided and GPU-posed), (n, 16) f32."""
        n = sum(len(sk["matrices"]) for sk in self.skeletons if sk is not None)
        out = np.zeros((max(n, 1), 16), dtype=f32)
        if n:
            self._check(self.lib.r3n_readback_joint_matrices(self.ctx, 0, _ffi.ptr(out), n), "r3n_readback_joint_matrices")
        return out[:n]

    def readback_cube_face(self, cube, level, face):
        """Bordered face `face` of level `level` of cube `cube` as the device holds it (r3n_readback_cube_face): (n + 2, n + 2)
        uint32 RGBA8 words, or (n + 2, n + 2, 4) float32 for a cube of a float-decoded format; n = max(1, width >> level).  The
        four corner texels are zero."""
        self._flush_cubes()
        if not 0 <= cube < len(self.cubes):
            raise ValueError("readback_cube_face: no such cube")
        c = self.cubes[cube]
        width = c.width if isinstance(c, (_EncodedCube, _EquirectCube, _DerivedCube)) else c[0].shape[1]
        p = max(1, width >> level) + 2
        words = np.zeros(p * p * 4, dtype=np.uint32)
        cls = np.zeros(1, dtype=np.uint32)
        self._check(self.lib.r3n_readback_cube_face(self.ctx, int(cube), int(level), int(face), _ffi.ptr(words), words.size, _ffi.ptr(cls)),
                    "r3n_readback_cube_face")
        if int(cls[0]) == 2:
            return words.view(np.float32).reshape(p, p, 4)
        return words[:p * p].reshape(p, p).copy()

    def readback_texels(self, per_texture=False):
        """The decoded texels of every texture (levels back to back, array order): RGBA8 textures as (n, 4) u8, textures
        of the float-decoded formats as (n, 4) f32.  per_texture=False concatenates them into one (n, 4) u8 array (a float
        texel is then four rows).  In the library's pool every texture starts on a 4-word boundary
        (r3n_textures_write_encoded); the gaps are dropped here."""
        from . import containers
        self._flush_textures()
        if self._texture_upload == "stream":
            descs = self.readback_texture_descs()
            parts = []
            for d in descs:
                if d[1] == 0:  # a removed slot
                    parts.append(None)
                    continue
                fl = int(d[4]) == 2  # R3N_POOL_FLOAT
                n = sum(max(1, int(d[1]) >> k) * max(1, int(d[2]) >> k) for k in range(int(d[3]))) * (4 if fl else 1)
                words = np.zeros(n, dtype=np.uint32)
                self._check(self.lib.r3n_readback_texels(self.ctx, int(d[0]), _ffi.ptr(words), n), "r3n_readback_texels")
                parts.append(words.view(np.float32).reshape(-1, 4) if fl else words.view(np.uint8).reshape(-1, 4))
            if per_texture:
                return parts
            live = [p.view(np.uint8).reshape(-1, 4) for p in parts if p is not None]
            return np.concatenate(live) if live else np.zeros((0, 4), dtype=np.uint8)
        is_float = [containers.is_float_format(int(d[4])) for d in self.tex_descs]
        sizes = [sum(max(1, int(d[1]) >> k) * max(1, int(d[2]) >> k) for k in range(int(d[3]))) * (4 if fl else 1)
                 for d, fl in zip(self.tex_descs, is_float)]
        starts, cur = [], 0
        for n in sizes:
            cur = (cur + 3) & ~3
            starts.append(cur)
            cur += n
        pool = np.zeros(max(cur, 1), dtype=np.uint32)
        if cur:
            self._check(self.lib.r3n_readback_texels(self.ctx, 0, _ffi.ptr(pool), cur), "r3n_readback_texels")
        parts = [pool[s0:s0 + n] for s0, n in zip(starts, sizes)]
        if per_texture:
            return [p.view(np.float32).reshape(-1, 4) if fl else p.view(np.uint8).reshape(-1, 4) for p, fl in zip(parts, is_float)]
        return (np.concatenate(parts) if parts else pool[:0]).view(np.uint8).reshape(-1, 4)

    def readback_texture_descs(self):
        """The texture table as the device holds it (r3n_readback_texture_descs): (n, 8) u32 rows of r3n_texture_desc32 -- offset in
        pool words, width, height, mips, pool format class (0 RGBA8, 1 RGBA8 sRGB, 2 four f32 per texel); removed slots have
        width = height = 0."""
        self._flush_textures()
        n = ctypes.c_uint32(0)
        self._check(self.lib.r3n_readback_texture_descs(self.ctx, None, 0, ctypes.byref(n)), "r3n_readback_texture_descs")  # the length alone
        descs = np.zeros((n.value, 8), dtype=np.uint32)
        if n.value:
            self._check(self.lib.r3n_readback_texture_descs(self.ctx, _ffi.ptr(descs), n.value, ctypes.byref(n)), "r3n_readback_texture_descs")
        return descs

    def texture_stats(self, reset=False):
        """Counters of the streamed texture path (r3n_texture_stats) as a dict; reset=True zeroes them after the read."""
        out = _ffi.TextureCounters()
        self._check(self.lib.r3n_texture_stats(self.ctx, ctypes.byref(out), 1 if reset else 0), "r3n_texture_stats")
        return {name: int(getattr(out, name)) for name, _ in _ffi.TextureCounters._fields_}

    def readback_hiz(self, width, height):
        n = 0
        k = 0
        m = max(width, height)
        while m:
            n += max(1, width >> k) * max(1, height >> k)
            k += 1
            m >>= 1
        pyr = np.zeros(n, dtype=f32)
        self._check(self.lib.r3n_readback_hiz(self.ctx, _ffi.ptr(pyr), n), "readback_hiz")
        return pyr

    # ------------------------------------------------------------------ timing taps
    def timing_enable(self, on=True):
        self._check(self.lib.r3n_timing_enable(self.ctx, 1 if on else 0), "r3n_timing_enable")

    def set_multi_stream(self, on=True):
        self._check(self.lib.r3n_set_multi_stream(self.ctx, 1 if on else 0), "r3n_set_multi_stream")

    def stage_times(self, reset=True):
        ms = np.zeros(len(_ffi.STAGE_TABLE), dtype=np.float64)
        n = np.zeros(len(_ffi.STAGE_TABLE), dtype=np.uint64)
        self._check(self.lib.r3n_stage_times(self.ctx, _ffi.ptr(ms), _ffi.ptr(n), 1 if reset else 0), "r3n_stage_times")
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(_ffi.STAGE_TABLE)}

    def hbm_copy_rate(self, nbytes=1 << 30, repeats=5):
        """GB/s of a float4 copy of `nbytes` on this device (read + write bytes): the measured HBM roofline denominator."""
        out = ctypes.c_double(0.0)
        self._check(self.lib.r3n_hbm_copy_rate(self.ctx, int(nbytes), int(repeats), ctypes.byref(out)), "r3n_hbm_copy_rate")
        return float(out.value)

    def sync(self):
        self._check(self.lib.r3n_sync(self.ctx), "r3n_sync")


# ---------------------------------------------------------------------------------------------------- graph
class RenderGraph:
    """Fixed-order stand-in for rend3::graph::RenderGraph: nodes are (name, closure) run in declaration order."""

    def __init__(self):
        self.nodes = []

    def add_node(self, name, body):
        self.nodes.append((name, body))

    def execute(self, renderer, eval_output):
        for _name, body in self.nodes:
            body(renderer, eval_output)


class BaseRenderGraphSettings:
    """rend3-routine/src/base.rs:94-98"""

    def __init__(self, ambient_color=(0, 0, 0, 0), clear_color=(0, 0, 0, 0)):
        self.ambient_color = ambient_color
        self.clear_color = clear_color


class BaseRenderGraphInputs:
    """rend3-routine/src/base.rs:72-92 (eval_output, routines, target{resolution, samples})"""

    def __init__(self, eval_output, routines, resolution, samples=1):
        self.eval_output = eval_output
        self.routines = routines
        self.resolution = resolution
        self.samples = samples


class GpuCuller:
    """rend3-routine/src/culling/culler.rs:185-714"""

    def add_object_uniform_upload_to_graph(self, graph, camera_specifier, resolution, samples, name):
        def body(r, ev):
            cam = r.camera if camera_specifier == CameraSpecifier.VIEWPORT else ev.shadows[camera_specifier]["camera"]
            hdr = host.camera_header(cam, None if camera_specifier == CameraSpecifier.VIEWPORT else camera_specifier,
                                     resolution, samples, r.capacity)
            r._check(r.lib.r3n_uniform_bake(r.ctx, camera_specifier, _ffi.ptr(hdr)), "r3n_uniform_bake")

        graph.add_node(name, body)

    def add_culling_to_graph(self, graph, camera_specifier, name):
        graph.add_node(name, lambda r, ev: r._check(r.lib.r3n_cull(r.ctx, camera_specifier), "r3n_cull"))


class ForwardRoutine:
    """rend3-routine/src/forward.rs:135-316: one (routine type, material key) pipeline."""

    def __init__(self, routine_type, material_key):
        self.routine_type = routine_type
        self.material_key = material_key

    def add_forward_to_graph(self, graph, label, camera, culling_source):
        def body(r, ev):
            r._check(r.lib.r3n_forward(r.ctx, camera, self.routine_type, culling_source, self.material_key), "r3n_forward")

        graph.add_node(label, body)


class HiZRoutine:
    """rend3-routine/src/hi_z.rs:18-235"""

    def add_hi_z_to_graph(self, graph):
        graph.add_node("HiZ", lambda r, ev: r._check(r.lib.r3n_hi_z(r.ctx), "r3n_hi_z"))


class PbrRoutine:
    """rend3-routine/src/pbr/routine.rs:17-133"""

    def __init__(self):
        self.opaque_depth = ForwardRoutine(_ffi.PASS_DEPTH, OPAQUE)
        self.cutout_depth = ForwardRoutine(_ffi.PASS_DEPTH, CUTOUT)
        self.opaque_routine = ForwardRoutine(_ffi.PASS_FORWARD, OPAQUE)
        self.cutout_routine = ForwardRoutine(_ffi.PASS_FORWARD, CUTOUT)
        self.blend_routine = ForwardRoutine(_ffi.PASS_FORWARD, BLEND)
        self.hi_z = HiZRoutine()


class TonemappingRoutine:
    """rend3-routine/src/tonemapping.rs:29-148"""

    def set_tonemapping(self, renderer, *args, **kwargs):
        """Renderer.set_tonemapping through the routine (the operators tonemapping.rs:1-10 announces)."""
        renderer.set_tonemapping(*args, **kwargs)

    def set_bloom(self, renderer, *args, **kwargs):
        """Renderer.set_bloom through the routine."""
        renderer.set_bloom(*args, **kwargs)

    def add_to_graph(self, graph):
        def body(r, ev):
            r._check(r.lib.r3n_tonemap(r.ctx, None, 0), "r3n_tonemap")

        graph.add_node("Tonemapping", body)


class _DerivedCube:
    """a cube prefilter_environment appended on the device: nothing of it is kept on the host"""

    def __init__(self, width, mips, source, level):
        self.width, self.mips, self.source, self.level = width, mips, source, level


class _EncodedCube:
    """a cube of add_texture_cube_encoded: faces[f][k] = the bytes of face f level k"""

    def __init__(self, fmt, width, mips, faces):
        self.fmt, self.width, self.mips, self.faces = fmt, width, mips, faces


class _EquirectCube:
    """a cube of add_texture_cube_equirect: one panorama of src_width x src_height texels, built into `width`^2 faces on the GPU"""

    def __init__(self, fmt, src_width, src_height, data, width, mips):
        self.fmt, self.src_width, self.src_height, self.data, self.width, self.mips = fmt, src_width, src_height, data, width, mips


class SkyboxRoutine:
    """rend3-routine/src/skybox.rs: holds the background cube; its node draws it where nothing nearer was drawn."""

    def __init__(self, renderer):
        self.renderer = renderer

    def set_background_texture(self, cube):
        self.renderer.set_background_texture(cube)

    def evaluate(self, renderer=None):
        """SkyboxRoutine::evaluate: makes the bound cube current (the reference rebuilds its bind group here)."""
        (renderer or self.renderer)._flush_cubes()

    def add_to_graph(self, graph):
        graph.add_node("Skybox", lambda r, _ev: r._check(r.lib.r3n_skybox(r.ctx), "r3n_skybox"))


class BaseRenderGraphRoutines:
    def __init__(self, pbr, tonemapping, skybox=None):
        self.pbr, self.tonemapping, self.skybox = pbr, tonemapping, skybox


class BaseRenderGraph:
    """rend3-routine/src/base.rs:103-186: owns the culler; add_to_graph declares the frame's nodes in order."""

    def __init__(self, renderer):
        self.renderer = renderer
        self.gpu_culler = GpuCuller()
        # measured on the bench scene: handing the GPU the viewport pass 1 before the shadow views costs 7 % (1.29 vs
        # 1.20 ms/frame): the shadow views are the longer chain and want the early start
        self.viewport_first = False

    def default_routines(self):
        return BaseRenderGraphRoutines(PbrRoutine(), TonemappingRoutine(), SkyboxRoutine(self.renderer))

    def add_to_graph(self, graph, inputs, settings, exchange=None):
        """Node order == base.rs:135-185.  `exchange` (multi-GPU only, not in the reference) is called with
        ("shadow" | "pass1" | "pass2", renderer) at the points where ranks must merge their depth keys."""
        ev = inputs.eval_output
        w, h = inputs.resolution
        pbr = inputs.routines.pbr
        VP = CameraSpecifier.VIEWPORT

        # clear_shadow_buffers + create_frame_uniforms (base.rs:139,142)
        def begin(r, _ev):
            fu = host.frame_uniforms(r.camera, settings.ambient_color, (w, h))
            clear = np.asarray(settings.clear_color, dtype=f32)
            aw, ah = ev.shadow_target_size
            r._check(r.lib.r3n_frame_begin(r.ctx, _ffi.ptr(fu), w, h, inputs.samples, _ffi.ptr(clear), aw, ah),
                     "r3n_frame_begin")
            for si, sh in enumerate(ev.shadows):
                r._check(r.lib.r3n_shadow_viewport(r.ctx, si, sh["offset"][0], sh["offset"][1], sh["size"]),
                         "r3n_shadow_viewport")

        graph.add_node("Frame Uniforms", begin)
        # morph targets, in front of skinning (glTF: morph first, then skin); not in the reference (rend3-gltf/src/lib.rs:761-763)
        graph.add_node("Morph", lambda r, _ev: r._flush_morphs())
        # skinning (base.rs:145, skinning.rs:211-226)
        def skin(r, _ev):
            if r._has_skeletons():
                sk_in, sk_m = r.skinning_buffers()
                poses = r._pose_requests()
                if len(poses):
                    r._check(r.lib.r3n_pose_skeletons(r.ctx, _ffi.ptr(np.ascontiguousarray(poses)), len(poses)), "r3n_pose_skeletons")
                r._check(r.lib.r3n_skinning(r.ctx, _ffi.ptr(sk_in), len(sk_in), _ffi.ptr(sk_m), len(sk_m)), "r3n_skinning")

        graph.add_node("Skinning", skin)
        def shadow_nodes():
            # multi-GPU: shadow views are sharded by view -- a rank renders the views it owns (whole) and receives the others
            sharded = exchange is not None and hasattr(exchange, "owns_shadow_view")
            mine = [si for si in range(len(ev.shadows)) if not sharded or exchange.owns_shadow_view(si)]
            if sharded:
                # an owned view is drawn WHOLE here (every object slot), whatever the viewport's object range is; set every frame
                # next to the ownership test so the two cannot disagree (r3n_render_frame does the same from its view mask)
                def ranges(r, _ev):
                    for si in range(len(ev.shadows)):
                        r.set_camera_object_range(si, *((0, 0xFFFFFFFE) if si in mine else (0xFFFFFFFF, 0xFFFFFFFF)))
                graph.add_node("shadow view ownership", ranges)
            # shadow_object_uniform_upload (base.rs:148)
            for si in mine:
                sh = ev.shadows[si]
                self.gpu_culler.add_object_uniform_upload_to_graph(graph, si, (sh["size"], sh["size"]), 1, f"Shadow Culling S{si}")
            # pbr_shadow_culling (base.rs:150)
            for si in mine:
                self.gpu_culler.add_culling_to_graph(graph, si, f"Shadow Culling S{si}")
            # pbr_shadow_rendering (base.rs:153,366-396)
            for si in mine:
                for routine in (pbr.opaque_depth, pbr.cutout_depth):
                    routine.add_forward_to_graph(graph, f"pbr shadow renderering S{si}", si, _ffi.SOURCE_RESIDUAL)
            if exchange is not None and len(ev.shadows):
                graph.add_node("exchange shadow atlas", lambda r, _ev: exchange("shadow", r, ev=ev, samples=inputs.samples))

        def viewport_pass1_nodes():
            # object_uniform_upload (base.rs:156)
            self.gpu_culler.add_object_uniform_upload_to_graph(graph, VP, (w, h), inputs.samples, "Uniform Bake")
            # pbr_render_opaque_predicted_triangles (base.rs:159)
            for routine in (pbr.opaque_routine, pbr.cutout_routine):
                routine.add_forward_to_graph(graph, "PBR Forward Pass 1", VP, _ffi.SOURCE_PREDICTED)

        # The two groups are independent (the shadow atlas is first read by the resolve), so their relative order
        # only decides what the GPU is handed first.  Reference order: shadows, then the viewport (base.rs:148-159).
        if self.viewport_first:
            viewport_pass1_nodes()
            shadow_nodes()
        else:
            shadow_nodes()
            viewport_pass1_nodes()
        if exchange is not None:
            graph.add_node("exchange pass-1 depth", lambda r, _ev: exchange("pass1", r, ev=ev, samples=inputs.samples))
        # hi_z (base.rs:162)
        pbr.hi_z.add_hi_z_to_graph(graph)
        # pbr_culling (base.rs:169)
        self.gpu_culler.add_culling_to_graph(graph, VP, "Primary Culling")
        # pbr_render_opaque_residual_triangles (base.rs:172)
        for routine in (pbr.opaque_routine, pbr.cutout_routine):
            routine.add_forward_to_graph(graph, "PBR Forward Pass 2", VP, _ffi.SOURCE_RESIDUAL)
        if exchange is not None:
            graph.add_node("exchange pass-2 keys", lambda r, _ev: exchange("pass2", r, ev=ev, samples=inputs.samples))
        # the deferred evaluation of the opaque passes' fragments (this design's stand-in for their fragment shaders)
        graph.add_node("Resolve Opaque", lambda r, _ev: r._check(r.lib.r3n_resolve_opaque(r.ctx), "r3n_resolve_opaque"))
        # skybox (base.rs:175): `if let Some(skybox)`; with no background bound the node enqueues nothing
        if inputs.routines.skybox is not None:
            inputs.routines.skybox.add_to_graph(graph)
        # pbr_forward_rendering_transparent (base.rs:181)
        pbr.blend_routine.add_forward_to_graph(graph, "PBR Forward Transparent", VP, _ffi.SOURCE_RESIDUAL)
        # tonemapping (base.rs:184)
        inputs.routines.tonemapping.add_to_graph(graph)
        graph.add_node("Frame End", lambda r, _ev: r._check(r.lib.r3n_frame_end(r.ctx), "r3n_frame_end"))
