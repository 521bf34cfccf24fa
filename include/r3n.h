/*
 * r3n.h -- C ABI of the MI355X-native rend3 object pipeline (librend3_amd.so).
 *
 * rend3 has no FFI boundary of its own (100 % Rust + WGSL); its extension API is the set of
 * `add_*_to_graph` routine methods whose node bodies record wgpu work.  This header is the
 * boundary those node bodies would call instead.  Each entry point cites the reference
 * interface it replaces; INTEGRATION.md shows the Rust `extern "C"` block and the adaptor
 * structs (BaseRenderGraph / GpuCuller / ForwardRoutine / HiZRoutine / TonemappingRoutine)
 * a maintainer would add on the rend3 side.
 *
 * Conventions
 *   - opaque context, one HIP device + one HIP stream per context;
 *   - every call returns 0 on success, <0 on error (never unwinds); r3n_last_error() has text;
 *   - the caller owns every host pointer for the duration of the call only; the context owns
 *     all device memory; all calls are asynchronous on the context's stream except r3n_readback_*,
 *     r3n_sync and calls documented as synchronising;
 *   - byte layouts are rend3's own (encase std430), restated in SURVEY.md App. A and checked by
 *     static_asserts in rend3_amd/csrc/layouts.h;
 *   - calls are made from one thread at a time (the reference holds the data_core mutex for the
 *     whole graph execution, rend3/src/graph/graph.rs:265).
 */
#ifndef R3N_H
#define R3N_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3N_OK 0
#define R3N_ERR_INVALID_ARG (-1)
#define R3N_ERR_HIP (-2)
#define R3N_ERR_NO_DEVICE (-3)
#define R3N_ERR_STATE (-4)
#define R3N_ERR_UNSUPPORTED (-5)
#define R3N_ERR_CAPACITY (-6) /* a fixed-size internal buffer (raster work queue, blend fragment list) overflowed.  Raised by kernels, so it
                                * surfaces later: r3n_frame_end / r3n_render_frame / r3n_sync / a read-back return it ONCE for an EARLIER frame
                                * whose image is incomplete; the frame just closed is unaffected, and no frame is ever refused because of it */

/* CameraSpecifier (rend3-routine/src/common/camera.rs:3-35): shadow index, or R3N_CAMERA_VIEWPORT
 * (== CameraSpecifier::Viewport.to_shader_index() == u32::MAX). */
typedef uint32_t r3n_camera;
#define R3N_CAMERA_VIEWPORT 0xFFFFFFFFu
#define R3N_MAX_SHADOW_VIEWS 64u

/* RoutineType (rend3-routine/src/forward.rs:40-44) */
#define R3N_PASS_DEPTH 0u
#define R3N_PASS_FORWARD 1u
/* CullingSource (rend3-routine/src/forward.rs:64-70) */
#define R3N_SOURCE_PREDICTED 0u
#define R3N_SOURCE_RESIDUAL 1u
/* Material::key() of PbrMaterial = TransparencyType (rend3-routine/src/pbr/material.rs:383-392,497-499) */
#define R3N_KEY_OPAQUE 0u
#define R3N_KEY_CUTOUT 1u
#define R3N_KEY_BLEND 2u

typedef struct r3n_ctx r3n_ctx;

/* ShaderObject<PbrMaterial>, 128 B (rend3/src/managers/object.rs:23-36) */
typedef struct r3n_object128 {
    float transform[16];
    float bounding_sphere_center[3];
    float bounding_sphere_radius;
    uint32_t first_index;
    uint32_t index_count;
    uint32_t material_index;
    uint32_t vertex_attribute_start_offsets[6];
    uint32_t enabled;
    uint32_t _pad[2];
} r3n_object128;

/* GpuPoweredShaderWrapper<PbrMaterial> = 10 texture ids + ShaderMaterial, 208 B
 * (rend3/src/managers/material.rs:25-29, rend3-routine/src/pbr/material.rs:526-543) */
typedef struct r3n_material208 {
    uint32_t textures[10];
    uint32_t _pad[2];
    float uv_transform0[12];
    float uv_transform1[12];
    float albedo[4];
    float emissive[3];
    float roughness;
    float metallic;
    float reflectance;
    float clear_coat;
    float clear_coat_roughness;
    float anisotropy;
    float ambient_occlusion;
    float alpha_cutout;
    uint32_t flags;
} r3n_material208;

/* One entry of the bindless texture array (rend3/src/managers/texture.rs; Texture in rend3-types/src/lib.rs:
 * data, format, size, mip_count).  For r3n_textures_write: RGBA8 texels, `offset` = first texel (u32) of mip 0 in the texel
 * pool, the mips follow contiguously; material records refer to entry i as texture id i + 1 (0 = none). */
typedef struct r3n_texture_desc32 {
    uint32_t offset;
    uint32_t width, height, mips;
    uint32_t format; /* R3N_TEXTURE_* */
    uint32_t stored_mips; /* r3n_textures_write_encoded only: 0 = all `mips` levels are in the payload (MipmapSource::Uploaded);
                             k < mips = the first k levels are, the others are GENERATED on the GPU (MipmapSource::Generated,
                             rend3/src/util/mipmap.rs + mipmap.wgsl: Linear / ClampToEdge blit per level in the texture's
                             format); uncompressed 8-bit formats, 16-bit float formats and RGB10A2 only */
    uint32_t _pad[2];
} r3n_texture_desc32;
#define R3N_TEXTURE_RGBA8_UNORM 0u
#define R3N_TEXTURE_RGBA8_UNORM_SRGB 1u
/* formats accepted by r3n_textures_write_encoded only (rend3-types TextureFormat names; what rend3-gltf's
 * util::map_ktx2_format / map_dxgi_format / map_d3d_format / convert_dynamic_image produce for 8-bit colour data,
 * rend3-gltf/src/lib.rs:1157-1175,1176-1410).  R / RG read (r, 0, 0, 1) / (r, g, 0, 1) like a sampled texture. */
#define R3N_TEXTURE_R8_UNORM 2u
#define R3N_TEXTURE_RG8_UNORM 3u
#define R3N_TEXTURE_BGRA8_UNORM 4u
#define R3N_TEXTURE_BGRA8_UNORM_SRGB 5u
#define R3N_TEXTURE_BC1_RGBA_UNORM 6u
#define R3N_TEXTURE_BC1_RGBA_UNORM_SRGB 7u
#define R3N_TEXTURE_BC2_RGBA_UNORM 8u
#define R3N_TEXTURE_BC2_RGBA_UNORM_SRGB 9u
#define R3N_TEXTURE_BC3_RGBA_UNORM 10u
#define R3N_TEXTURE_BC3_RGBA_UNORM_SRGB 11u
#define R3N_TEXTURE_BC4_R_UNORM 12u
#define R3N_TEXTURE_BC5_RG_UNORM 13u
#define R3N_TEXTURE_BC7_RGBA_UNORM 14u
#define R3N_TEXTURE_BC7_RGBA_UNORM_SRGB 15u
/* formats whose values are not 8-bit unorm: decoded into four f32 per texel (16 B per texel in the pool instead of 4).
 * Missing channels read (0, 0, 1).  stored_mips < mips (generated levels) is accepted for R16 / RG16 / RGBA16_FLOAT and
 * RGB10A2_UNORM -- the ones rend3-gltf generates chains for (filterable render targets; the level is rounded to the format:
 * binary16 to nearest even); the others must carry every level.  rend3-gltf/src/lib.rs:1204-1330 (KTX2), :1480-1485 (D3D),
 * :1499-1597 (DXGI) produce them. */
#define R3N_TEXTURE_R8_SNORM 16u
#define R3N_TEXTURE_RG8_SNORM 17u
#define R3N_TEXTURE_RGBA8_SNORM 18u
#define R3N_TEXTURE_R16_FLOAT 19u
#define R3N_TEXTURE_RG16_FLOAT 20u
#define R3N_TEXTURE_RGBA16_FLOAT 21u
#define R3N_TEXTURE_R32_FLOAT 22u
#define R3N_TEXTURE_RG32_FLOAT 23u
#define R3N_TEXTURE_RGBA32_FLOAT 24u
#define R3N_TEXTURE_RGBA16_UNORM 25u
#define R3N_TEXTURE_RGBA16_SNORM 26u
#define R3N_TEXTURE_RGB10A2_UNORM 27u
#define R3N_TEXTURE_RG11B10_FLOAT 28u
#define R3N_TEXTURE_RGB9E5_UFLOAT 29u
#define R3N_TEXTURE_BC4_R_SNORM 30u
#define R3N_TEXTURE_BC5_RG_SNORM 31u
#define R3N_TEXTURE_BC6H_RGB_UFLOAT 32u
#define R3N_TEXTURE_BC6H_RGB_FLOAT 33u
#define R3N_TEXTURE_FORMAT_COUNT 34u

/* PerCameraUniform header, 240 B (rend3-routine/src/culling/culler.rs:158-175) */
typedef struct r3n_camera_header240 {
    float view[16];
    float view_proj[16];
    uint32_t shadow_index;
    uint32_t _pad[3];
    float frustum[20];
    float resolution[2];
    uint32_t flags; /* bit0 positive area visible, bit1 multisampled (culler.rs:151-156) */
    uint32_t object_count;
} r3n_camera_header240;

/* FrameUniforms, 496 B (rend3-routine/src/uniforms.rs:17-27) */
typedef struct r3n_frame_uniforms496 {
    float view[16];
    float view_proj[16];
    float origin_view_proj[16];
    float inv_view[16];
    float inv_view_proj[16];
    float inv_origin_view_proj[16];
    float frustum[20];
    float ambient[4];
    uint32_t resolution[2];
    uint32_t _pad[2];
} r3n_frame_uniforms496;

/* wgpu DrawIndexedIndirect as written by cull.wgsl:47-61 (structures.wgsl:20-26), 20 B.
 * One per region; here a region is one material key. */
typedef struct r3n_indirect_call {
    uint32_t vertex_count;
    uint32_t instance_count;
    uint32_t base_index;
    int32_t vertex_offset;
    uint32_t base_instance;
} r3n_indirect_call;

/* GpuSkinningInput, 40 B (rend3-routine/src/skinning.rs:23-46, shaders/src/skinning.wgsl:3-25).  Offsets are byte
 * offsets into the mesh buffer; 0xFFFFFFFF = attribute absent. */
typedef struct r3n_skinning_input40 {
    uint32_t base_position_offset, base_normal_offset, base_tangent_offset;
    uint32_t joint_indices_offset, joint_weight_offset;
    uint32_t updated_position_offset, updated_normal_offset, updated_tangent_offset;
    uint32_t joint_matrix_base_offset, vertex_count;
} r3n_skinning_input40;

/* One morph instance of r3n_morph, 48 B: a mesh's POSITION / NORMAL / TANGENT runs, the deltas of its glTF morph targets and the
 * instance's private output runs.  Byte offsets into the mesh buffer; 0xFFFFFFFF = absent.  An attribute is morphed when it has
 * deltas: base, delta and updated offset are then all present, else all three absent.  The deltas of one attribute are
 * `n_targets` runs of 3 * vertex_count f32 words, target-major, back to back. */
typedef struct r3n_morph_input48 {
    uint32_t base_position_offset, base_normal_offset, base_tangent_offset;
    uint32_t delta_position_offset, delta_normal_offset, delta_tangent_offset; /* target 0's run; target t at + t * 12 * vertex_count */
    uint32_t updated_position_offset, updated_normal_offset, updated_tangent_offset;
    uint32_t weight_base; /* first weight of this instance in `weights` */
    uint32_t n_targets, vertex_count;
} r3n_morph_input48;
#define R3N_MAX_MORPH_TARGETS 256u
/* One instance of r3n_vertex_normals, 32 B: the f32x3 position run to read (a morph instance's updated positions), the f32x3
 * normal run to write, the mesh's index run and its adjacency words (r3n_host_vertex_adjacency).  Byte offsets into the mesh
 * buffer, index_count in words. */
typedef struct r3n_normals_input32 {
    uint32_t position_offset;   /* f32x3 run to read: a morph instance's updated positions */
    uint32_t normal_offset;     /* f32x3 run to write */
    uint32_t index_offset, index_count;
    uint32_t adjacency_offset;  /* r3n_host_vertex_adjacency's words */
    uint32_t vertex_count, left_handed, _pad;
} r3n_normals_input32;
/* One instance of r3n_vertex_tangents, 32 B: the runs to READ -- the instance's current f32x3 positions and normals and the mesh's
 * f32x2 uv0 -- the f32x3 tangent run to WRITE, the mesh's index run and its adjacency words (r3n_host_vertex_adjacency).  Byte
 * offsets into the mesh buffer, index_count in words. */
typedef struct r3n_tangents_input32 {
    uint32_t position_offset, normal_offset, uv_offset; /* runs to read */
    uint32_t tangent_offset;                            /* f32x3 run to write */
    uint32_t index_offset, index_count;
    uint32_t adjacency_offset;                          /* r3n_host_vertex_adjacency's words */
    uint32_t vertex_count;
} r3n_tangents_input32;

/* ---- rend3-anim (rend3-anim/src/lib.rs) tables, row N4.  A RIG is one skin: its joints in the skin's order, each with
 * its parent joint and its depth in the joint hierarchy (AnimationData::from_gltf_scene, :77-145, flattened); a CLIP is
 * one animation applied to one rig: a track per joint with the key ranges of its translation / rotation / scale
 * channels and the bind components used where a channel is absent (pose_animation_frame, :226-236). */
typedef struct r3n_anim_rig16 {
    uint32_t first_joint, n_joints; /* into the joints array; n_joints <= 512 */
    uint32_t max_depth, _pad;
} r3n_anim_rig16;
typedef struct r3n_anim_joint80 {
    int32_t parent;  /* joint index inside the rig; -1: the node has no parent (global = local); -2: its parent node is
                        not a joint of this skin (global = IDENTITY * local), rend3-anim/src/lib.rs:246-256 */
    uint32_t depth;  /* 0 for parent < 0, else depth(parent) + 1 */
    uint32_t _pad[2];
    float inverse_bind[16];
} r3n_anim_joint80;
typedef struct r3n_anim_clip16 {
    uint32_t rig, first_track; /* tracks [first_track, first_track + rig.n_joints) */
    float duration;            /* Animation::duration: the time is clamped to [0, duration] (:189) */
    uint32_t _pad;
} r3n_anim_clip16;
typedef struct r3n_anim_track80 {
    uint32_t animated;        /* 0: the clip has no channel for this joint's node -> local matrix IDENTITY (:220); else nonzero */
    uint32_t key_first[3];    /* translation, rotation, scale: first key time (index into `times`) */
    uint32_t key_count[3];    /* 0: channel absent -> bind component */
    uint32_t value_first[3];  /* first value (index into `values`: 3 floats per vec3 key, 4 per quaternion key, xyzw) */
    float bind_t[3], bind_r[4], bind_s[3]; /* Mat4::to_scale_rotation_translation of the node's local transform */
} r3n_anim_track80;
typedef struct r3n_pose_request16 {
    uint32_t clip;
    float time;
    uint32_t matrix_base; /* first joint matrix of the skeleton (GpuSkinningInput.joint_matrix_base_offset) */
    uint32_t _pad;
} r3n_pose_request16;

/* Arithmetic of the PBR fragment stage (r3n_resolve_opaque).  EXACT (default): every f32 operation rounds once, IEEE division and
 * square root -- the contract under which visibility, HDR and framebuffer are bit-identical to the CPU oracle.  FAST (opt-in):
 * fused multiply-add and hardware reciprocal / rsqrt in interpolation, texture filtering and BRDF; coverage, depth, level of
 * detail, shadow coordinates and comparisons stay exact.  The framebuffer then stays within the north-star tolerance
 * (|delta| <= 1e-3 after tonemap), not bit-identical.  Honoured by the single-sample resolve; MSAA always runs EXACT. */
#define R3N_SHADE_EXACT 0u
#define R3N_SHADE_FAST 1u

typedef struct r3n_config {
    uint32_t struct_size;      /* sizeof(r3n_config) */
    uint32_t max_big_items;    /* raster work-queue capacity in items (0 = default 2 Mi: 32 sub-queues of 65 536).  Divided by 32 and
                                * raised to the floor of 1 024 per sub-queue; only the test hook R3N_BIG_CAPACITY goes below it */
    uint32_t shade_mode;       /* R3N_SHADE_EXACT | R3N_SHADE_FAST */
    uint32_t _pad;
    uint64_t reserved[2];
} r3n_config;

/* ---- lifetime (replaces rend3::create_iad + BaseRenderGraph::new / PbrRoutine::new state:
 *      rend3-routine/src/base.rs:111-124, culling/culler.rs:198-425) */
r3n_ctx *r3n_create(int hip_device, const r3n_config *config);
void r3n_destroy(r3n_ctx *ctx);
const char *r3n_last_error(const r3n_ctx *ctx);
/* text of the last error of a failed r3n_create (ctx == NULL) */
const char *r3n_create_error(void);
int r3n_sync(r3n_ctx *ctx);
/* the context's hipStream_t, so callers (torch, RCCL) can order work against it */
void *r3n_stream(r3n_ctx *ctx);

/* ---- world data uploads (the managers' GPU buffers the hot path reads)
 *      MeshManager::add upload, rend3/src/managers/mesh.rs:123-184 (layout: SoA attribute runs + u32 indices) */
int r3n_mesh_buffer_write(r3n_ctx *ctx, uint64_t byte_offset, const void *data, uint64_t bytes);
/* ---- pooled mesh blocks: the mesh buffer as a pool that gives words back (MeshManager sub-allocates every attribute and index
 *      range from a RangeAllocator, rend3/src/managers/mesh.rs:123-184 add, :228-258 allocate_range / free_range, and grows the
 *      buffer only when no hole fits, :232-308; skeletons take and return their private copies the same way,
 *      rend3/src/managers/skeleton.rs:105-113 and :139-147).  A BLOCK is one contiguous allocation of mesh-buffer words on a 4-word
 *      (16-byte) boundary -- a mesh's whole blob (attribute runs, indices, delta block, adjacency), one skeleton's private runs, or
 *      one morph instance's private runs; its padded length is a multiple of 4 words, so a slide by a multiple of 16 bytes keeps
 *      every alignment inside it.  The first r3n_mesh_blocks_add puts the context in POOLED mode: r3n_mesh_buffer_write then stays
 *      legal for ranges inside ONE live block (padding included; in-place edits, with its usual waits) and returns R3N_ERR_STATE
 *      elsewhere.  A context whose mesh buffer was written by r3n_mesh_buffer_write before refuses r3n_mesh_blocks_add with
 *      R3N_ERR_STATE.  All four calls below are refused between r3n_frame_begin and r3n_frame_end (R3N_ERR_STATE).
 *
 *      r3n_mesh_blocks_add (MeshManager::add / allocate_range, mesh.rs:123-184, :228-247): n blocks; block i takes blocks[i].words
 *      (>= 1) words from payload + blocks[i].payload_offset (a multiple of 4 bytes, the range inside payload_bytes), or, with
 *      R3N_MESH_BLOCK_ZERO, no payload: its words are zero-filled on the device (the private runs of skeletons and morph
 *      instances).  byte_offsets_out[i] = where the block starts.  Placement is first fit at the lowest address over the holes,
 *      else behind the high-water mark -- deterministic, so every rank that makes the same calls gets the same offsets.  Copies
 *      and fills run on the update path's own stream and the call waits for that stream alone: words no enqueued frame can name --
 *      behind the mark, or a hole that was free at the last full wait -- are written without waiting for a frame.  Words freed
 *      since the last full wait are parked; holes that were free before are preferred, and taking parked words costs ONE wait for
 *      every frame in flight.  Growth of the device block (x 2) is one device-to-device copy behind such a wait.  A block that
 *      would end past byte 2^32 -> R3N_ERR_CAPACITY; a bad record (words == 0, unknown flags, a payload range outside the
 *      payload or not 4-byte aligned) -> R3N_ERR_INVALID_ARG; both with nothing allocated or written.
 *
 *      r3n_mesh_blocks_remove (MeshManager::remove / free_range, mesh.rs:197-211, :249-258; SkeletonManager::remove,
 *      skeleton.rs:139-147): frees whole blocks by their start; the words are parked until the next full wait (a frame in flight
 *      may still read them).  An offset that is not the start of a live block, or one named twice -> R3N_ERR_INVALID_ARG with
 *      nothing changed.  Never waits for the GPU.  The caller disables (r3n_objects_write) every object that names the block
 *      first: the object pass never fetches geometry of a disabled slot.
 *
 *      r3n_mesh_compact (no counterpart in the reference, whose allocator never moves a range): slides the live blocks towards
 *      word 0 in ascending address order, each to the 4-word boundary behind the one before (opts as r3n_texture_compact_opts:
 *      max_words, stage_words, same meaning, defaults and refusals), and RELOCATES on the device every address the object buffer
 *      holds: in every record below the object capacity, enabled or not, first_index (words) and the six
 *      vertex_attribute_start_offsets (bytes) that lie inside a moved block follow it; nothing else of a record is written
 *      (csrc/mesh_reloc.h states the rule).  The call waits ONCE for every frame in flight (parked words become holes), enqueues
 *      the moves and the relocation, and waits for its own work; with nothing to move it returns without any wait.  moves_out
 *      receives the moves in ascending address order so that the caller can fix its own mirrors -- the inputs of r3n_skinning,
 *      r3n_morph, r3n_vertex_normals and r3n_vertex_tangents are the caller's; moves_capacity smaller than the number of moves ->
 *      R3N_ERR_INVALID_ARG with nothing changed (blocks_live of r3n_mesh_stats is always enough).  result (may be NULL): as
 *      r3n_texture_compact_result, kernel_launches counting the relocation launch, plus relocate_ns.  R3N_ERR_HIP: as
 *      r3n_textures_compact -- the context's allocator is the one from before the call, the words are unspecified.
 *
 *      r3n_mesh_stats: counters since creation or the last reset (add_calls, remove_calls, compact_calls, bytes_staged,
 *      launches = fills, move kernels and relocation kernels, full_waits = waits for every frame in flight the calls above made,
 *      growths) and the pool's state now (blocks_live, live_words unpadded, pool_words = the high-water mark, free_ranges,
 *      buffer_words = the device block's size).  `out` may be NULL with reset != 0. */
#define R3N_MESH_BLOCK_ZERO 1u
typedef struct r3n_mesh_block24 {
    uint64_t payload_offset; /* bytes into payload; ignored with R3N_MESH_BLOCK_ZERO */
    uint64_t words;
    uint32_t flags, _pad;
} r3n_mesh_block24;
typedef struct r3n_mesh_move24 {
    uint64_t old_byte_offset, new_byte_offset, padded_words;
} r3n_mesh_move24;
typedef struct r3n_mesh_compact_opts {
    uint64_t max_words, stage_words;
} r3n_mesh_compact_opts;
typedef struct r3n_mesh_compact_result {
    uint64_t blocks_moved, words_moved, passes, kernel_launches, full_syncs, pool_words_before, pool_words_after, free_ranges_after;
    uint64_t relocate_ns; /* the relocation kernel alone, between two device events on the call's stream (0: nothing launched) */
} r3n_mesh_compact_result;
typedef struct r3n_mesh_counters {
    uint64_t add_calls, remove_calls, compact_calls, bytes_staged, launches, full_waits, growths, blocks_live, live_words, pool_words,
        free_ranges, buffer_words;
} r3n_mesh_counters;
int r3n_mesh_blocks_add(r3n_ctx *ctx, const r3n_mesh_block24 *blocks, uint32_t n, const void *payload, uint64_t payload_bytes,
                        uint64_t *byte_offsets_out);
int r3n_mesh_blocks_remove(r3n_ctx *ctx, const uint64_t *byte_offsets, uint32_t n);
int r3n_mesh_compact(r3n_ctx *ctx, const r3n_mesh_compact_opts *opts, r3n_mesh_compact_result *result, r3n_mesh_move24 *moves_out,
                     uint32_t moves_capacity);
int r3n_mesh_stats(r3n_ctx *ctx, r3n_mesh_counters *out, int reset);
/*      ObjectManager::evaluate scatter upload, rend3/src/managers/object.rs:344-364.
 *      `capacity` = object-buffer capacity in records (FreelistDerivedBuffer, util/freelist/buffer.rs:48-52);
 *      growing it preserves existing records, new records are zero (enabled == 0). */
int r3n_objects_write(r3n_ctx *ctx, const uint32_t *slots, const r3n_object128 *records, uint32_t n,
                      uint32_t capacity);
/*      MaterialManager::evaluate, rend3/src/managers/material.rs:202-227.  `keys[i]` = Material::key()
 *      (R3N_KEY_*), which is host-side state in the reference (not part of the 208-byte record). */
int r3n_materials_write(r3n_ctx *ctx, const uint32_t *slots, const r3n_material208 *records,
                        const uint8_t *keys, uint32_t n);
/*      TextureManager (rend3/src/managers/texture.rs): replaces the whole bindless 2D texture array.  Material records
 *      sample entry `id - 1` (opaque.wgsl:151-160).  Formats other than RGBA8 -> R3N_ERR_UNSUPPORTED. */
int r3n_textures_write(r3n_ctx *ctx, const r3n_texture_desc32 *descs, uint32_t n_textures, const uint32_t *texels,
                       uint64_t n_texels);
/*      Same, for textures in the formats the loader produces (above): `payload` holds every texture's levels back to
 *      back in ITS OWN format (block-compressed levels: ceil(w/4) x ceil(h/4) blocks, 8 or 16 B each), desc.offset =
 *      BYTE offset of level 0 in `payload`.  The library expands / decodes everything on the GPU into its RGBA8 texel
 *      pool (the texture unit's job in the reference: formats go straight to wgpu, rend3/src/managers/texture.rs:59-
 *      150).  Snorm / float / 16-bit / ETC2 / ASTC / BC6H formats -> R3N_ERR_UNSUPPORTED.  Every stored level of the call is
 *      decoded by at most four launches, one per kernel family, as in r3n_textures_update; more than 2^31 wave slots (64 blocks
 *      or texels of one level each) in one family -> R3N_ERR_CAPACITY with nothing changed, which takes a pool near the 2^32-word
 *      limit filled with one-texel levels.  The call waits for every frame in flight first and returns when its work has run; its
 *      staging memory is freed before it returns. */
int r3n_textures_write_encoded(r3n_ctx *ctx, const r3n_texture_desc32 *descs, uint32_t n_textures, const void *payload,
                               uint64_t payload_bytes);
/*      TextureManager::add (rend3/src/managers/texture.rs: one texture per handle, handed over while frames are being drawn), for n
 *      entries at once: texture descs[i] goes into slot slots[i] of the bindless array (material texture id = slot + 1).  descs /
 *      payload exactly as r3n_textures_write_encoded takes them (offset = byte offset of level 0 in `payload`, 4-byte aligned;
 *      stored_mips as there; every format that call accepts).  A slot that holds a texture is replaced.  Only the call's own data
 *      is copied and decoded -- every stored level of every texture of the call in at most four launches -- into a texel pool that
 *      stays resident: a texture is one contiguous range of pool words on a 4-word boundary, first fit at the lowest address,
 *      appended behind the last one when no hole takes it (slots k, k + 1, ... updated in ascending order from an empty context or
 *      after a whole-array write get the offsets the whole-array write of the concatenated list gives).  The whole-array writes
 *      above reset the pool to their own layout; the two kinds of call can be mixed.
 *      Duplicate slots, a slot >= table length + n (the host allocates the lowest free index: it never needs more) and everything
 *      r3n_textures_write_encoded rejects are rejected before anything changes; a pool beyond 2^32 words -> R3N_ERR_CAPACITY.
 *      Frames in flight are waited for only when a buffer has to grow (geometric), when a written slot held a texture at any time
 *      since the last such wait, or when the data goes into words freed since then (ranges not recently freed are preferred);
 *      otherwise the call waits for its own copy and decode work alone, which runs on a stream of its own beside the frames (the
 *      caller owns `payload` for the duration of the call; what is enqueued after the call sees the new textures). */
int r3n_textures_update(r3n_ctx *ctx, const uint32_t *slots, const r3n_texture_desc32 *descs, uint32_t n, const void *payload,
                        uint64_t payload_bytes);
/*      TextureManager::remove (rend3/src/managers/texture.rs; the reference drops the texture with its handle): the slots' pool words
 *      become reusable; the slots stay in the table as removed entries -- on the device a 1 x 1, one-level RGBA8 entry at pool word
 *      0, so that a stale material id reads in bounds, with an unspecified value.  Removing a removed or never-written slot, or one
 *      slot twice -> R3N_ERR_INVALID_ARG, nothing changed.  Never waits for the GPU.  (After a raw r3n_textures_write whose ranges
 *      are not ascending, disjoint and 4-word aligned the slots own no words: removing them frees none.) */
int r3n_textures_remove(r3n_ctx *ctx, const uint32_t *slots, uint32_t n);
/*      Compaction of the streamed pool (no counterpart in the reference, which keeps one wgpu texture per handle and has no pool to
 *      fragment): slides the live textures towards pool word 0, in ascending address order, each to the 4-word boundary behind the
 *      one before, so that the holes below the high-water mark disappear and the mark comes down.  The decoded words are moved on the
 *      device; nothing is copied from the host or decoded again, no texture is reordered, and the words of every live texture are
 *      unchanged -- `offset` is the only field of its descriptor that changes.  Removed slots stay removed entries at pool word 0.
 *      The device block is neither shrunk nor freed: later textures reuse the words behind the lowered mark.
 *      opts (NULL = all zero): max_words != 0 stops in front of the first texture whose padded words would take the call past that
 *      many words moved -- the prefix is packed, one hole follows it, the rest is untouched and a later call goes on from there.
 *      stage_words = the most words of scratch memory the call may use, a multiple of 4 and at least 256 (anything else ->
 *      R3N_ERR_INVALID_ARG); 0 = 16 Mi words, 64 MiB: a launch never writes a word it reads elsewhere, so a stretch whose shift
 *      is shorter than itself goes through scratch in pieces of this size, two launches each: launches <= 2 * (ceil(words_moved /
 *      stage_words) + 1), which is 34 for a 1 GiB pool and 514 for a 16 GiB pool moved entirely through the default scratch.  The
 *      default bounds the scratch block, which stays resident like the update path's staging.
 *      When nothing would move the call returns R3N_OK without a wait or a launch (full_syncs == 0) and releases no removed range.
 *      Otherwise it waits ONCE for every frame in flight -- ranges removed since the last such wait then count as holes -- enqueues
 *      its passes, uploads the descriptor and level-offset rows of the moved slots, and waits for its own work before it returns;
 *      what is enqueued after the call sees the new offsets.  Between r3n_frame_begin and r3n_frame_end -> R3N_ERR_STATE; a live slot
 *      that owns no words (after a raw r3n_textures_write whose ranges are not ascending, disjoint and 4-word aligned) ->
 *      R3N_ERR_STATE; both with nothing changed.  R3N_ERR_HIP (a launch, a copy or the wait failed): the context's offsets, allocator
 *      and mark are the ones from before the call, but passes may have run, so the pool's words are unspecified -- re-send the
 *      textures with a whole-array write.
 *      out (may be NULL): textures_moved, words_moved (padded), passes (a pass is one launch, or two through scratch),
 *      kernel_launches, full_syncs (0 or 1), the high-water mark before and after, and the holes left below it (0 after a call
 *      without a budget).  r3n_texture_stats counts none of this: its counters stay the update path's. */
typedef struct r3n_texture_compact_opts {
    uint64_t max_words, stage_words;
} r3n_texture_compact_opts;
typedef struct r3n_texture_compact_result {
    uint64_t textures_moved, words_moved, passes, kernel_launches, full_syncs, pool_words_before, pool_words_after, free_ranges_after;
} r3n_texture_compact_result;
int r3n_textures_compact(r3n_ctx *ctx, const r3n_texture_compact_opts *opts, r3n_texture_compact_result *out);
/*      Renderer::add_texture_2d_from_texture (TextureManager::fill_from_texture, rend3/src/managers/texture.rs:198-242: a new texture
 *      of mip_level_size(start_mip) whose levels are GPU-side copies of levels start_mip .. of `src`), for n textures at once:
 *      slot items[i].dst_slot receives levels [start_mip, start_mip + mip_count) of the texture in items[i].src_slot (mip_count 0 =
 *      all that remain).  The new entry has the extents of level start_mip of the source, mip_count levels and the source's pool
 *      class (RGBA8, RGBA8 sRGB, or four f32 per texel); its words are placed exactly as r3n_textures_update places a texture and
 *      are copied from the source's inside the pool by ONE launch for the whole call -- a texture's levels lie back to back, so a
 *      tail is one word range, starting on any word.  Nothing is copied from the host but the call's table and the touched
 *      descriptor and level-offset rows; nothing is decoded or generated again, so the tail of a generated chain (stored_mips <
 *      mips), which the host never had, can be kept.  The source is unchanged and may be removed afterwards; two items may name
 *      one source.
 *      Sources are resolved against the table as it is before the call: src_slot must hold a live texture that owns its words
 *      (after a raw r3n_textures_write whose ranges are not ascending, disjoint and 4-word aligned no slot does).  dst_slot must
 *      hold NO live texture -- removed, never written, or past the table, below table length + n as in r3n_textures_update -- and
 *      may not be named twice: the reference only ever fills a freshly allocated handle, a live slot is not replaced.  start_mip >=
 *      the source's mips, or start_mip + mip_count > the source's mips -> refused.  Everything refused returns
 *      R3N_ERR_INVALID_ARG (a pool beyond 2^32 words, or more than 2^31 wave slots -- 256 16-byte units of one item each -- of copy
 *      work: R3N_ERR_CAPACITY) before anything changes; n == 0 returns R3N_OK without a wait or a launch.  (R3N_ERR_STATE: a
 *      destination range overlapping a source, which the allocator never hands out.)
 *      Frames in flight are waited for under exactly the conditions of r3n_textures_update -- a buffer has to grow (word offsets are
 *      kept), a destination slot held a texture at some time since the last such wait, or the words were freed since then;
 *      otherwise the call runs on the texture path's own stream beside the frames and waits for its own work alone.  What is
 *      enqueued after the call sees the new entries.  R3N_ERR_HIP (a copy, the launch or the wait failed): the context's table,
 *      allocator and mark are the ones from before the call; the device's rows of the destination slots are unspecified until the
 *      slots are written again.
 *      out (may be NULL): textures (n), words_copied (unpadded), kernel_launches (1), full_syncs (0 or 1), and the pool's
 *      high-water mark afterwards.  r3n_texture_stats counts none of this: its counters stay the update path's (bytes_staged does
 *      not move; pool_words, live_words and free_ranges describe the pool as always). */
typedef struct r3n_texture_tail16 {
    uint32_t dst_slot, src_slot, start_mip, mip_count; /* mip_count 0 = all that remain */
} r3n_texture_tail16;
typedef struct r3n_texture_tail_result {
    uint64_t textures, words_copied, kernel_launches, full_syncs, pool_words_after;
} r3n_texture_tail_result;
int r3n_textures_from_texture(r3n_ctx *ctx, const r3n_texture_tail16 *items, uint32_t n, r3n_texture_tail_result *out);
/*      Counters of the streamed texture path since creation or the last reset, and the pool's state now.  update_calls: successful
 *      r3n_textures_update calls; kernel_launches: every kernel they enqueued; bytes_staged: payload bytes they copied; full_syncs:
 *      waits for every frame in flight they made; pool_grows: calls in which the pool, the descriptor table or the level-offset
 *      table grew.  pool_words: the pool's high-water mark; live_words: words owned by live textures; free_ranges: holes below the
 *      mark.  `out` may be NULL with reset != 0.  (The staging and job-table blocks grow geometrically without a wait: an outgrown
 *      block is kept until the next full wait and freed there.) */
typedef struct r3n_texture_counters {
    uint64_t update_calls, kernel_launches, bytes_staged, full_syncs, pool_grows, pool_words, live_words, free_ranges;
} r3n_texture_counters;
int r3n_texture_stats(r3n_ctx *ctx, r3n_texture_counters *out, int reset);
/*      Test entry: the texture sampler of the frame's kernels (csrc/texture.h) on a list of queries, against the context's own
 *      texture state -- the pool, descriptors, level-offset table and decode tables the resolve and the rasterisers are handed, as
 *      they are at the call.  Query i is textureSampleGrad(textures[id[k] - 1], nearest ? nearest : linear, (u, v), ddx, ddy);
 *      result i holds up to three RGBA samples.  `form` names the instantiation the product launches (exact arithmetic only):
 *        R3N_PROBE_GRAD / _GRAD_RGB    the general entry with / without the alpha channel (takes its own short path when it applies)
 *        R3N_PROBE_SHORT / _SHORT_RGB  the short-path-only instantiations of the resolve's material classes
 *        R3N_PROBE_SHARE               short-path-only, id[0], id[1], id[2] in slot order through ONE level-of-detail / footprint cache
 *                                      that starts empty (the fragment stage); slots 0 and 1 with alpha, slot 2 without
 *        R3N_PROBE_ALPHA / _ALPHA_SHORT  the rasterisers' alpha-only sampler (cutout test): the value lands in rgba[0][3]
 *        R3N_PROBE_BATCHED             the PBR class's three maps in one pass; flags = 1 when it took the wave, 0 when it declined
 *                                      (rgba is then zero)
 *      Single-map forms sample id[0] into rgba[0].  A channel a form does not produce is zero: alpha of the _RGB forms and of
 *      slot 2 of SHARE / BATCHED, rgba[1..2] of the single-map forms, everything but rgba[0][3] of the ALPHA forms.
 *      ONE THREAD PER QUERY, QUERIES 64 i .. 64 i + 63 ARE ONE WAVEFRONT: the batched form declines or accepts per wavefront and
 *      takes its wave-uniform branches (second level, wrapping rows) by what any of those 64 queries needs; a last partial wave
 *      runs with its missing lanes idle.
 *      The short-path-only and batched forms have preconditions the kernels do not check (the resolve's material classes establish
 *      them): every id is 0 or a texture on the sampler's short path (power-of-two extents, RGBA8 pool texels, pool <= 2^30 words)
 *      and nearest == 0.  The call checks every query on the host and returns R3N_ERR_INVALID_ARG without a launch when one
 *      violates them, or when `form` is unknown.  The general forms take any id, one past the table or of a removed slot
 *      included, like the product.  Waits for every frame in flight, allocates and frees its scratch, waits for its own launch. */
#define R3N_PROBE_GRAD 0
#define R3N_PROBE_GRAD_RGB 1
#define R3N_PROBE_SHORT 2
#define R3N_PROBE_SHORT_RGB 3
#define R3N_PROBE_SHARE 4
#define R3N_PROBE_ALPHA 5
#define R3N_PROBE_ALPHA_SHORT 6
#define R3N_PROBE_BATCHED 7
#define R3N_PROBE_FORM_COUNT 8
typedef struct r3n_sample_query40 {
    uint32_t id[3];
    uint32_t nearest;
    float u, v, ddx[2], ddy[2];
} r3n_sample_query40;
typedef struct r3n_sample_result52 {
    float rgba[3][4];
    uint32_t flags;
} r3n_sample_result52;
int r3n_sample_probe(r3n_ctx *ctx, uint32_t form, const r3n_sample_query40 *queries, uint32_t n, r3n_sample_result52 *out);
/*      The cube textures (the reference's d2c_texture_manager, rend3/src/managers/texture.rs; Renderer::add_texture_cube): replaces
 *      the context's whole cube array, which is separate from the bindless 2D array.  A cube is six square faces of width x width
 *      RGBA8 texels, contiguous from desc.offset (in texels) in `texels`, in layer order +X, -X, +Y, -Y, +Z, -Z (what scene_viewer
 *      uploads as right, left, top, bottom, front, back).  width != height, width == 0 or > 16384, faces outside `texels`
 *      -> R3N_ERR_INVALID_ARG; formats other than R3N_TEXTURE_RGBA8_UNORM / _SRGB, or mips != 1 -> R3N_ERR_UNSUPPORTED (a cube's mip
 *      level would follow from the derivatives of the direction; scene_viewer uploads MipmapCount::ONE).  stored_mips is ignored.
 *      An array whose pool of bordered faces would pass 2^32 words -> R3N_ERR_CAPACITY; every refusal comes before anything changes.
 *      The call is r3n_texture_cubes_write_encoded of the same cubes as one-level RGBA8 faces, `texels` being the payload: the
 *      device expands the faces and k_cube_assemble builds their borders, as for every entry (csrc/skybox.h), in a scratch block
 *      that is freed before the call returns.
 *      Synchronises.  A skybox bound to a cube that no longer exists (r3n_skybox_set) is unbound. */
int r3n_texture_cubes_write(r3n_ctx *ctx, const r3n_texture_desc32 *descs, uint32_t n_cubes, const uint32_t *texels,
                            uint64_t n_texels);
/*      The same array from ENCODED faces with their mip chains: Renderer::add_texture_cube with any TextureFormat and
 *      MipmapCount::Specific(n), MipmapSource::Uploaded (TextureManager::add(.., cube = true), rend3/src/managers/texture.rs:98-196).
 *      Replaces the whole cube array like r3n_texture_cubes_write.  A cube is width == height == N, `mips` levels, in any format
 *      r3n_textures_write_encoded accepts.  desc.offset = byte offset in `payload` of face +X level 0, 4-byte aligned; the layout is
 *      the reference's LayerMajor: for face +X, -X, +Y, -Y, +Z, -Z its levels 0 .. mips - 1 back to back, every level in its
 *      format's own byte count (block formats: ceil(n / 4)^2 blocks), level k of extent n_k = max(1, N >> k).
 *      Refused before anything changes: width != height, N == 0 or N > 16384, more mips than the extent has, a face outside
 *      `payload`, a misaligned offset, an unknown format id -> R3N_ERR_INVALID_ARG; stored_mips neither 0 nor mips ->
 *      R3N_ERR_UNSUPPORTED (a cube's chain is never generated: the reference asserts it, texture.rs:147); a cube pool beyond 2^32
 *      words, or a job family beyond 2^31 wave slots -> R3N_ERR_CAPACITY.  Inside a frame -> R3N_ERR_STATE.
 *      Every (cube, face, level) is decoded on the device by the kernels of the 2D path (at most four launches for the call) into a
 *      scratch block that is freed before the call returns; one further launch builds the bordered faces (csrc/skybox.h).  The
 *      formats that decode to f32 (R3N_TEXTURE_R8_SNORM and above: BC6H, the float and the 16-bit formats ...) cost 16 bytes per
 *      texel, as in the 2D pool; all others 4.  Synchronises.  A skybox bound to a cube that no longer exists is unbound.  The
 *      skybox node selects the level from the direction's screen-space differences and filters trilinearly;
 *      a one-level RGBA8 cube gives the same device words and frames through either entry. */
int r3n_texture_cubes_write_encoded(r3n_ctx *ctx, const r3n_texture_desc32 *descs, uint32_t n_cubes, const void *payload,
                                    uint64_t payload_bytes);
/*      The same array from SOURCES of two kinds, so that an HDR environment can be uploaded as the file it ships as: one
 *      equirectangular (latitude / longitude) panorama.  Replaces the whole cube array like the two entries above.
 *      R3N_CUBE_SOURCE_CUBE: what r3n_texture_cubes_write_encoded takes -- width == height == face_extent == N, `mips` stored levels,
 *      LayerMajor from `offset`; the same refusals; an array of such sources gives the same pool words and descriptors as that entry.
 *      R3N_CUBE_SOURCE_EQUIRECT: ONE stored level of width x height texels at `offset` (4-byte aligned; any width, height in
 *      1 .. 65535, 2 : 1 is not required; row 0 is +Y, the panorama's centre column looks along +X), in R3N_CUBE_ENCODING_RGBE8
 *      (Radiance RGBE, four bytes r g b e per texel: a source encoding of this entry only, not a texture format) or in any format
 *      r3n_textures_write_encoded accepts.  The device resamples it into six faces of face_extent = N in 1 .. 16384 texels and builds
 *      `mips` in 1 .. floor(log2 N) + 1 levels of every face (DESIGN.md section 2 "Cubes from panoramas"; csrc/equirect_rule.h is the
 *      rule).  The cube lands in the f32 class, 16 bytes per texel, whatever the source format.
 *      Refused before anything changes: an unknown kind or format, a zero extent, a source extent above 65535, N above 16384, more
 *      mips than N has, data outside `payload`, a misaligned offset -> R3N_ERR_INVALID_ARG; a cube pool or scratch block beyond 2^32
 *      words, or more than 2^31 wave slots in one launch -> R3N_ERR_CAPACITY; inside a frame -> R3N_ERR_STATE.
 *      Synchronises; its scratch block is freed before it returns.  A skybox bound to a cube that no longer exists is unbound. */
#define R3N_CUBE_SOURCE_CUBE 0u
#define R3N_CUBE_SOURCE_EQUIRECT 1u
#define R3N_CUBE_ENCODING_RGBE8 0x100u /* `format` of an EQUIRECT source: Radiance RGBE8 */
typedef struct r3n_cube_source {   /* 32 B */
    uint32_t kind;          /* R3N_CUBE_SOURCE_* */
    uint32_t format;        /* R3N_TEXTURE_*, or R3N_CUBE_ENCODING_RGBE8 (EQUIRECT only) */
    uint32_t width, height; /* the stored level 0: N x N for CUBE, the panorama for EQUIRECT */
    uint32_t face_extent;   /* N */
    uint32_t mips;          /* levels of the cube */
    uint64_t offset;        /* bytes into payload */
} r3n_cube_source;
int r3n_texture_cubes_write_sources(r3n_ctx *ctx, const r3n_cube_source *sources, uint32_t n_cubes, const void *payload,
                                    uint64_t payload_bytes);
/*      SkyboxRoutine::set_background_texture (rend3-routine/src/skybox.rs): cube_id 0 = no skybox, i + 1 = cube i of the array
 *      above; an id past the array -> R3N_ERR_INVALID_ARG.  Between frames only (R3N_ERR_STATE inside one). */
int r3n_skybox_set(r3n_ctx *ctx, uint32_t cube_id);
/*      Environment lights: reads directional lights and an ambient term out of ONE level of ONE cube of the array above, on the
 *      device.  Not in the reference: rend3-routine/src/skybox.rs only draws the cube, and its lights are whatever the caller
 *      adds by hand.  Opt-in; changes nothing of the context that a frame reads.  This is light extraction, not image-based
 *      lighting: the records are meant for r3n_lights_write (direction = -direction) and `ambient` for the frame uniforms.
 *      The rule (DESIGN.md section 2 "Environment lights"; csrc/envlight_rule.h states it and proves its integer sums free of
 *      overflow): every interior texel of the level has a solid angle and a unit direction; at most max_lights times the
 *      brightest texel not yet taken seeds a cone of half-angle acos(cone_cos), the cone is moved onto the energy centroid
 *      of its texels, twice, and the texels of the moved cone become a light -- unless they hold less than min_share of the level's
 *      energy, which ends the search.  `ambient` is the solid-angle mean radiance of what no light took.  Every sum is an
 *      integer sum of texel quantities quantised to 2^-scale_exp, so the result does not depend on the launch plan
 *      (R3N_TUNE envlight_plane, envlight_blocks), word for word; a texel channel that is NaN, infinite or negative counts as 0.
 *      `cube`, `level`: as r3n_readback_cube_face; any pool class.  No such cube or level, max_lights > R3N_ENV_MAX_LIGHTS,
 *      cone_cos outside [0.5, 1) or NaN, min_share outside [0, 1) or NaN -> R3N_ERR_INVALID_ARG with a message that names the
 *      field; a level of extent above 1024 -> R3N_ERR_UNSUPPORTED with a message that names the finest level the entry takes;
 *      inside a frame -> R3N_ERR_STATE; all with nothing changed.  Synchronises, like the cube writes. */
#define R3N_ENV_MAX_LIGHTS 16u   /* most lights of one call (no counterpart in skybox.rs) */
typedef struct r3n_env_lights_params {   /* 20 B */
    uint32_t cube, level, max_lights;
    float cone_cos, min_share;
} r3n_env_lights_params;
typedef struct r3n_env_sums {   /* 48 B: raw integer sums over a set of texels */
    uint64_t q[3];     /* sum of floor(channel * solid angle * 2^scale_exp) */
    uint64_t qy;       /* sum of the energies (13933 q_r + 46871 q_g + 4732 q_b) >> 16 */
    uint64_t qw;       /* sum of floor(solid angle * 2^44) */
    uint64_t texels;
} r3n_env_sums;
typedef struct r3n_env_light {   /* 192 B */
    float direction[3];    /* unit vector from the scene TOWARDS the light */
    float solid_angle;     /* of the cone's texels, steradians */
    float irradiance[3];   /* sum of radiance * solid angle over them */
    uint32_t texels;
    uint32_t seed;         /* linear index (face * n + j) * n + i of the seed texel */
    uint32_t _pad[3];
    int64_t shift[2][6];   /* the two mean-shift steps' sums of energy * direction: [c] of (qy >> 20), [3 + c] of (qy & 0xFFFFF) */
    r3n_env_sums sums;     /* of the cone's texels */
} r3n_env_light;
typedef struct r3n_env_lights_result {   /* 3336 B */
    uint32_t n_lights;
    int32_t scale_exp;     /* the radiance sums are in units of 2^-scale_exp; 0 for a level without energy */
    uint32_t extent;       /* of the level */
    uint32_t emax_bits;    /* the f32 bits of the largest channel * solid angle of the level */
    float ambient[4];      /* mean radiance of the remainder; [3] = 1 */
    r3n_env_sums total;    /* the whole level */
    r3n_env_sums remainder;/* what no light took: total - the lights */
    uint64_t seeds[17];    /* the seed keys (luminance bits << 32 | ~index) found for light 0 .. 16, 0 where no search ran */
    r3n_env_light lights[16]; /* [0, n_lights): emitted; the record behind them keeps the raw fields (seed, shift, sums) of the
                                 candidate that was refused, everything else is 0 */
} r3n_env_lights_result;
int r3n_environment_lights(r3n_ctx *ctx, const r3n_env_lights_params *params, r3n_env_lights_result *out);
/*      Environment prefilter: builds, on the device, the two resources image-based lighting derives from an environment -- a chain
 *      of GGX-prefiltered specular levels and nine SH coefficients of its radiance -- from the STORED levels of one cube of the
 *      array above.  Not in the reference (rend3-routine/src/skybox.rs only draws the cube).  Opt-in.  This is still not lighting:
 *      no frame kernel reads either resource until the resolve consumes them; today the skybox node can draw a level of the new
 *      cube (r3n_skybox_set_level), and r3n_environment_probe evaluates the lookups a resolve will call (csrc/ibl_lookup.h).
 *      The rule (DESIGN.md section 2 "Environment prefilter"; csrc/ibl_rule.h states it with its error bound): with S the extent of
 *      `level` and L = `levels`, result level 0 is the decoded source level; result level k in 1 .. L - 1 (extent max(1, S >> k),
 *      perceptual roughness k / (L - 1)) is, per texel, the GGX-weighted mean over EVERY texel of the stored level `level` + k; the
 *      SH coefficients are taken from the first of those levels of extent <= 32 (else the last).  Every sum follows one fixed tree
 *      (per source row, per face, the six faces), so every launch plan (R3N_TUNE ibl_tile, ibl_block) gives the same words.  A texel
 *      channel that is NaN, infinite, negative or zero counts as 0 in every sum; level 0 is copied as it decodes.
 *      APPENDS one f32-class cube of extent S with L levels to the cube array: existing cubes keep their ids and their words, a
 *      bound skybox stays bound, result->cube_id is the old count (r3n_skybox_set takes cube_id + 1).  A later whole-array write
 *      (r3n_texture_cubes_write and its siblings) replaces the array, this cube included.
 *      Refused with nothing changed, the message naming the field: no such cube or level, levels < 2 or above
 *      min(floor(log2 S) + 1, 16) -> R3N_ERR_INVALID_ARG; S above 256 -> R3N_ERR_UNSUPPORTED with a message that names the finest
 *      level the entry takes (the pair loop is quadratic in the level's texels); more levels than the cube stores from `level` on
 *      -> R3N_ERR_UNSUPPORTED (chains are never generated here); a pool beyond 2^32 words -> R3N_ERR_CAPACITY; inside a frame ->
 *      R3N_ERR_STATE.  Synchronises; its scratch block is freed before it returns. */
typedef struct r3n_env_prefilter_params { uint32_t cube, level, levels; } r3n_env_prefilter_params;
typedef struct r3n_env_prefilter_result {   /* 160 B */
    uint32_t cube_id;   /* index of the new cube in the array */
    uint32_t extent, levels, sh_level;   /* sh_level: the source level (relative to params.level) the coefficients were taken from */
    float sh[9][4];     /* Llm rgb in the order Y00, Y1-1, Y10, Y11, Y2-2, Y2-1, Y20, Y21, Y22; [3] = 0 */
} r3n_env_prefilter_result;
int r3n_environment_prefilter(r3n_ctx *ctx, const r3n_env_prefilter_params *params, r3n_env_prefilter_result *out);
/*      A test and diagnostic entry in the manner of r3n_sample_probe: the two lookups of csrc/ibl_lookup.h, one thread per query.
 *      specular = ibl_specular(cube, dir, roughness): lod = roughness * (levels - 1) clamped to [0, levels - 1] (NaN gives 0), its
 *      floor and fraction, the seamless bilinear of the skybox node on that level and the next, mixed by the fraction; `dir` need
 *      not be normalised.  irradiance = ibl_irradiance(sh, n) = E(n) / pi of the nine coefficients.  `cube` may be any cube of the
 *      array, of any class.  No such cube -> R3N_ERR_INVALID_ARG.  Waits for every frame in flight and for its own launch. */
typedef struct r3n_env_query32 {
    float dir[3], roughness;
    float n[3], pad;
} r3n_env_query32;
typedef struct r3n_env_sample32 {
    float specular[3], irradiance[3];
    uint32_t level;     /* floor(lod) */
    float fraction;     /* lod - level */
} r3n_env_sample32;
int r3n_environment_probe(r3n_ctx *ctx, uint32_t cube, const float sh[9][4], const r3n_env_query32 *queries, uint32_t n, r3n_env_sample32 *out);
/*      Which level of the bound cube the skybox node draws.  A negative level (the default) selects the level per pixel from the
 *      direction's screen-space differences, as ever.  level >= 0 draws the bound cube at that level, clamped to its last one:
 *      floor(level) mixed with the next by the fraction, each filtered seamlessly -- a blurred backdrop when the cube is a
 *      prefiltered chain.  A one-level cube ignores it.  NaN -> R3N_ERR_INVALID_ARG.  Between frames only (R3N_ERR_STATE). */
int r3n_skybox_set_level(r3n_ctx *ctx, float level);
/*      Draw order of the blend-key objects for the transparent pass: object slots back to front, as the CPU batcher
 *      sorts them every frame (rend3-routine/src/culling/batching.rs:146-176, Sorting::BLENDING: -distance^2 from the
 *      camera location to the object location).  Call once per frame before r3n_resolve_opaque (n may be 0). */
int r3n_blend_order_write(r3n_ctx *ctx, const uint32_t *objects_back_to_front, uint32_t n);
/*      The same order, sorted ON THE DEVICE.  r3n_blend_objects_write uploads the BLEND SET -- the blend-key objects' slots and
 *      their sorting locations -- when the world changes; r3n_blend_sort orders it for one camera location every frame.  The
 *      location is host-side state in the reference, like Material::key(): the world bounding-sphere centre at add_object
 *      (rend3/src/managers/object.rs:273), the transform's translation after set_object_transform (:313); it is not in the
 *      128-byte record, so the caller supplies it (locations = 3 n floats).  `slots` strictly ascending and < the object
 *      capacity, else R3N_ERR_INVALID_ARG; 2^29 or more triangles in the set -> R3N_ERR_UNSUPPORTED (the limit of
 *      r3n_blend_order_write).  The triangle counts are those of the object records at the time of the call: send the set again
 *      after an r3n_objects_write that touches one of its objects.  n == 0 clears the set.  Uploads through pinned staging without
 *      waiting for the GPU and sizes the sort's scratch buffers.  Between frames only (R3N_ERR_STATE inside one).
 *      THE LAST of r3n_blend_order_write and r3n_blend_objects_write decides where the transparent pass takes its order from. */
int r3n_blend_objects_write(r3n_ctx *ctx, const uint32_t *slots, const float *locations, uint32_t n);
/*      Sorting::BLENDING on the device: key = -dist, dist = (d.x * d.x + d.y * d.y) + d.z * d.z in f32 with d = camera_location -
 *      location, ascending; equal keys by ascending slot (the reference's unstable sort leaves ties open).  +inf distances are
 *      legal and tie with each other; NaN locations are outside the contract (the order is then unspecified, nothing else).
 *      Call once per frame before r3n_resolve_opaque, where r3n_blend_order_write is called in host order mode.  Enqueues kernels
 *      on the main stream and nothing else: no host wait, no read-back, no per-object host work.  Without a set (or in host order
 *      mode) it does nothing and returns R3N_OK. */
int r3n_blend_sort(r3n_ctx *ctx, const float camera_location[3]);
/*      DirectionalLightManager / PointLightManager buffers, byte-identical:
 *      u32 count @0, array @16 (stride 128 / 32): rend3/src/managers/directional.rs:31-53,135-153, point.rs:14-74.
 *      At most 16 directional and 256 point lights; a longer list (R3N_ERR_UNSUPPORTED) or a count beyond its buffer
 *      (R3N_ERR_INVALID_ARG) is refused with a message that names the list, and a refused call changes neither list. */
int r3n_lights_write(r3n_ctx *ctx, const void *directional_buffer, uint64_t directional_bytes,
                     const void *point_buffer, uint64_t point_bytes);

/* TonemappingRoutine::new's output_format (rend3-routine/src/tonemapping.rs:29-106): *Srgb targets take the exact OETF of
 * the fixed-function store (blit.wgsl fs_main_scene), other targets the shader's srgb_scene_to_display approximation
 * (fs_main_monitor, math/color.wgsl:13-19, exponent 0.4166); Bgra8* targets hold blue first.  Default RGBA8_UNORM_SRGB. */
#define R3N_OUTPUT_RGBA8_UNORM_SRGB 0u
#define R3N_OUTPUT_BGRA8_UNORM_SRGB 1u
#define R3N_OUTPUT_RGBA8_UNORM 2u
#define R3N_OUTPUT_BGRA8_UNORM 3u
int r3n_set_output_format(r3n_ctx *ctx, uint32_t format);
/* Skinning kernel (r3n_skinning).  EXACT (default): vector ALU, every operation rounded once -- bit-identical to the oracle's
 * restatement of skinning.wgsl:37-94.  MFMA (opt-in): the joint-matrix x vertex-block contraction on the matrix cores
 * (v_mfma_f32_16x16x4_f32: four joint matrices x 16 vertices per instruction), for rigs of at most FOUR joints
 * (R3N_ERR_UNSUPPORTED otherwise); its f32 results follow the fused-multiply-add order of the instruction, bit-identical to
 * oracle/r3o.c::r3o_skinning_mfma_order, within 1e-6 relative of EXACT.  It weights joint slots, not influences; a slot that
 * no taken influence of a vertex names adds +0 to that vertex whatever its matrix holds, so a degenerate joint matrix (zero
 * column, NaN, inf) reaches exactly the vertices it reaches in EXACT. */
#define R3N_SKIN_EXACT 0u
#define R3N_SKIN_MFMA 1u
int r3n_set_skinning_mode(r3n_ctx *ctx, uint32_t mode);
/* switches the fragment-stage arithmetic (R3N_SHADE_*) for the resolves enqueued from now on */
int r3n_set_shade_mode(r3n_ctx *ctx, uint32_t mode);

/* ---- frame (node order of BaseRenderGraph::add_to_graph, rend3-routine/src/base.rs:135-185)
 * r3n_frame_begin: create_frame_uniforms (uniforms.rs:73-125) + render-target setup (base.rs:224-264) +
 * clear_shadow_buffers (clear.rs:4-20).  Clears colour to `clear_color`, depth and the shadow atlas to 0.0.
 * `samples` is SampleCount::One (1) or ::Four (4): the colour / depth targets of the viewport then hold 4 samples per pixel
 * (forward.rs:358, base.rs:236-258), Hi-Z starts from their depth-min resolve (resolve_depth_min.wgsl) and the HDR target
 * the tonemapper reads is the render pass's box resolve.  Shadow views are always single-sampled (base.rs:230).
 * width / height / samples may change from one frame to the next: the targets are re-created, the cameras' culling history (last
 * frame's result bits and predicted triangles) is KEPT, as the reference keeps a camera's culling buffers whatever the target's
 * size (CullingBufferMap is keyed by the CameraSpecifier alone, culler.rs:53-80). */
int r3n_frame_begin(r3n_ctx *ctx, const r3n_frame_uniforms496 *uniforms, uint32_t width, uint32_t height,
                    uint32_t samples, const float clear_color[4], uint32_t shadow_atlas_width,
                    uint32_t shadow_atlas_height);
/* skinning::add_skinning_to_graph (rend3-routine/src/skinning.rs:211-226): build_gpu_skinning_input_buffers (:54-139) +
 * GpuSkinner::execute_pass (:142-199) + skinning.wgsl.  `inputs`: one record per skeleton, `joint_matrices`: all
 * skeletons' joint matrices back to back (column-major mat4).  ONE launch covers every skeleton (the reference issues
 * one dispatch + one dynamic-offset bind per skeleton).  Must precede the frame's bakes (base.rs:145).
 * PRECONDITION, not checked here (the indices live in device memory): every joint index a skeleton's mesh holds, in any of the
 * four slots and whatever its weight, is below that skeleton's matrix count -- the distance from its joint_matrix_base_offset
 * to the next skeleton's, or to n_joint_matrices for the last.  A larger index reads another skeleton's matrices or past the
 * buffer.  The host mirror enforces it where skeletons are made (SkeletonManager::validate_skeleton's NotEnoughJoints,
 * rend3/src/managers/skeleton.rs:73-89: Renderer.add_skeleton / add_skeletons_bulk refuse a shorter list) and keeps a
 * skeleton's count fixed afterwards, so the bases of cached records stay the running sums of the counts.  R3N_SKIN_MFMA reads a
 * skeleton's joint count from the same distance. */
int r3n_skinning(r3n_ctx *ctx, const r3n_skinning_input40 *inputs, uint32_t n_skeletons, const float *joint_matrices,
                 uint32_t n_joint_matrices);
/* rend3-anim on the GPU.  r3n_animation_write replaces the rig / clip tables.  r3n_pose_skeletons queues
 * pose_animation_frame's per-skin work (rend3-anim/src/lib.rs:213-262) for `n` skeleton instances: the NEXT r3n_skinning
 * evaluates them on the GPU -- after copying its host `joint_matrices` (which may be NULL when every skeleton is posed
 * this way) -- and writes each skeleton's joint matrices (global * inverse bind) at its matrix_base: the clip's WHOLE rig,
 * rig.n_joints matrices.  Only the largest end is checked against n_joint_matrices; that the skeleton at matrix_base stores at
 * least rig.n_joints matrices is the caller's part (Renderer.pose_skeletons refuses a larger rig: it would overwrite the next
 * skeleton's matrices). */
int r3n_animation_write(r3n_ctx *ctx, const r3n_anim_rig16 *rigs, uint32_t n_rigs, const r3n_anim_joint80 *joints,
                        uint32_t n_joints, const r3n_anim_clip16 *clips, uint32_t n_clips, const r3n_anim_track80 *tracks,
                        uint32_t n_tracks, const float *times, uint32_t n_times, const float *values, uint32_t n_values);
int r3n_pose_skeletons(r3n_ctx *ctx, const r3n_pose_request16 *requests, uint32_t n);
/* glTF 2.0 morph targets (the reference stops at a TODO, rend3-gltf/src/lib.rs:761-763; the arithmetic is defined here and in
 * DESIGN.md section 2).  For each instance and each attribute that has deltas, every f32 word k of the run becomes
 *     acc = base[k];  for t = 0 .. n_targets - 1 with weights[weight_base + t] != 0.0f:  acc = fl(acc + fl(w[t] * delta[t][k]));  updated[k] = acc
 * one rounding per operation, no fused multiply-add.  Skipping the weights that compare equal to zero (+0 and -0; NaN does not) is
 * part of the definition: all-zero weights reproduce the base run bit for bit (a -0.0 word included).  Nothing is normalised.
 * ONE launch covers every instance of the call; instances and weights go through pinned staging, the call only enqueues on the
 * context's stream and does not wait for the GPU.  Callable between frames, or inside one in front of r3n_skinning: morph comes
 * first, a skeleton that skins a morphed instance takes the updated_* runs as its base_* runs.  It orders itself behind a resolve
 * still in flight, as r3n_skinning does.  n_instances == 0 returns R3N_OK and launches nothing.
 * R3N_ERR_INVALID_ARG: a run outside the mesh buffer or not 4-byte aligned; a delta without its base or its output, or a base or
 * an output without a delta; weight_base + n_targets > n_weights; n_targets outside 1 .. R3N_MAX_MORPH_TARGETS;
 * an instance that morphs nothing; an output run that overlaps a base or delta run of the same instance. */
int r3n_morph(r3n_ctx *ctx, const r3n_morph_input48 *inputs, uint32_t n_instances, const float *weights, uint32_t n_weights);
/* Vertex normals recomputed from an instance's positions, for morphed meshes that ship without NORMAL: what
 * Mesh::calculate_normals_for_buffers (rend3-types/src/lib.rs:662-704) gives for those positions, bit for bit (DESIGN.md section 2
 * "Recomputed normals").  With T = floor(index_count / 3) triangles t = (i0, i1, i2) (a remainder is ignored):
 *     e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  n_t = left_handed ? cross(e1, e2) : cross(e2, e1)
 *     acc = (+0, +0, +0);  for the triangles naming v, in ascending triangle number, once per occurrence: acc = fl(acc + n_t)
 *     rcp = 1 / sqrt((x * x + y * y) + z * z);  normal[v] = rcp finite and > 0 ? acc * rcp : (+0, +0, +0)
 * one rounding per operation, no fused multiply-add.  The order of the additions is the serial loop's, so there are no atomics: a
 * thread per vertex gathers its triangles through the adjacency words.  ONE launch covers every instance of the call; the records
 * go through pinned staging, the call only enqueues on the context's stream and does not wait for the GPU; it orders itself behind
 * a resolve still in flight, as r3n_morph does.  Call it after r3n_morph and before r3n_skinning (same stream, no other
 * synchronisation).  n_instances == 0 returns R3N_OK and launches nothing.
 * R3N_ERR_INVALID_ARG, nothing launched: a run outside the mesh buffer or not 4-byte aligned; vertex_count == 0; the normal run
 * overlapping the position, index or adjacency run of its record; left_handed > 1. */
int r3n_vertex_normals(r3n_ctx *ctx, const r3n_normals_input32 *inputs, uint32_t n_instances);
/* Vertex tangents generated from an instance's positions, normals and the mesh's uv0, for morphed meshes that ship without TANGENT:
 * what Mesh::calculate_tangents_for_buffers (rend3-types/src/lib.rs:784-837, zeroed = true, glam's scalar Vec3) gives for those
 * runs, bit for bit (DESIGN.md section 2 "Generated tangents").  With T = floor(index_count / 3) triangles t = (i0, i1, i2) (a
 * remainder is ignored):
 *     e1 = p[i1] - p[i0];  e2 = p[i2] - p[i0];  a = uv[i1] - uv[i0];  b = uv[i2] - uv[i0]
 *     r = 1 / (a.x * b.y - a.y * b.x);  g_t = e1 * b.y - (e2 * a.y) * r          per component; r multiplies the second product only
 *     acc = (+0, +0, +0);  for the triangles naming v, in ascending triangle number, once per occurrence: acc = fl(acc + g_t)
 *     d = (n.x * acc.x + n.y * acc.y) + n.z * acc.z;  q = acc - n * d            n = normal[v] as stored, not re-normalised
 *     rcp = 1 / sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);  tangent[v] = rcp finite and > 0 ? q * rcp : (+0, +0, +0)
 * one rounding per operation, no fused multiply-add.  A triangle with a degenerate uv footprint (every triangle that names a vertex
 * twice is one) has r = +-inf; its term is inf or NaN and every vertex it names ends as (+0, +0, +0).  No output word is NaN or inf;
 * handedness plays no part.  The order of the additions is the serial loop's, so there are no atomics: a thread per vertex gathers
 * its triangles through the adjacency words.  ONE launch covers every instance of the call; the records go through pinned staging,
 * the call only enqueues on the context's stream and does not wait for the GPU; it orders itself behind a resolve still in flight.
 * Call order inside a frame: r3n_morph -> r3n_vertex_normals -> r3n_vertex_tangents -> r3n_skinning (same stream, no other
 * synchronisation).  n_instances == 0 returns R3N_OK and launches nothing.
 * R3N_ERR_INVALID_ARG, nothing launched: a run outside the mesh buffer or not 4-byte aligned; vertex_count == 0; the tangent run
 * overlapping the position, normal, uv, index or adjacency run of its record. */
int r3n_vertex_tangents(r3n_ctx *ctx, const r3n_tangents_input32 *inputs, uint32_t n_instances);
/* GpuCuller::object_uniform_upload (culler.rs:427-529) + uniform_prep.wgsl.  Called on its own it bakes every enabled slot, like
 * the reference.  Inside r3n_render_frame the bake is fused into the object pass and covers only the slots a kernel reads: those
 * inside the frustum now or (viewport) in the camera's previous frame -- the others keep what they held. */
int r3n_uniform_bake(r3n_ctx *ctx, r3n_camera camera, const r3n_camera_header240 *header);
/* GpuCuller::add_culling_to_graph (culler.rs:682-713) = batch_objects (batching.rs:120-250, frustum cull +
 * slot assignment, done on the GPU here) + GpuCuller::cull (culler.rs:531-659) + cull.wgsl.
 * Owns the per-camera temporal state (previous-invocation map, ping-pong result bits, predicted lists). */
int r3n_cull(r3n_ctx *ctx, r3n_camera camera);
/* HiZRoutine::add_hi_z_to_graph (hi_z.rs:161-234) + hi_z.wgsl: pyramid from the viewport depth so far */
int r3n_hi_z(r3n_ctx *ctx);
/* Shadow viewport of a shadow camera inside the atlas (base.rs:369: ViewportRect(desc.map.offset, size)) */
int r3n_shadow_viewport(r3n_ctx *ctx, r3n_camera shadow_camera, uint32_t x, uint32_t y, uint32_t size);
/* ForwardRoutine::add_forward_to_graph (forward.rs:192-315) for one (camera, routine type, culling source,
 * material key): rasterises that draw-call range with depth test GreaterEqual + write (forward.rs:347-351).
 * FORWARD colour is resolved per pixel by r3n_resolve_opaque (each pixel shaded once, for its nearest fragment). */
int r3n_forward(r3n_ctx *ctx, r3n_camera camera, uint32_t pass, uint32_t source, uint32_t material_key);
/* Evaluates opaque.wgsl (VS :91-135 + FS :203-551) for the nearest fragment of every pixel -> Rgba16Float HDR.
 * Must follow the last opaque / cutout FORWARD r3n_forward of the frame (base.rs:172) and precede r3n_tonemap.
 * The transparent pass -- r3n_forward(R3N_CAMERA_VIEWPORT, R3N_PASS_FORWARD, R3N_SOURCE_RESIDUAL, R3N_KEY_BLEND),
 * base.rs:181 -- comes after it: this frame's passing triangles of the blend-key objects, in the order given to
 * r3n_blend_order_write (or sorted by r3n_blend_sort), depth-tested against the opaque depth (no depth write) and alpha-blended into the HDR target
 * (pbr/routine.rs:113-118). */
int r3n_resolve_opaque(r3n_ctx *ctx);
/* SkyboxRoutine::add_to_graph (rend3-routine/src/skybox.rs, skybox.wgsl; base.rs:175): every sample whose depth the sky's 0.0
 * passes GreaterEqual -- the cleared ones, and a triangle at depth exactly 0.0 -- takes the bound cube's colour in the direction of
 * its PIXEL CENTRE (bilinear, level 0, seamless across faces; alpha 1).  Legal after r3n_resolve_opaque and before the transparent
 * r3n_forward / r3n_tonemap of the same frame (else R3N_ERR_STATE); with no skybox bound it returns R3N_OK and enqueues nothing. */
int r3n_skybox(r3n_ctx *ctx);
/* TonemappingRoutine::add_to_graph (tonemapping.rs:108-147) + blit.wgsl into an Rgba8UnormSrgb target.
 * If `host_rgba8` is non-NULL the image is also copied out (synchronises), `pitch_bytes` per row. */
int r3n_tonemap(r3n_ctx *ctx, void *host_rgba8, uint64_t pitch_bytes);
/* The routine's `src` is any Rgba16Float target (tonemapping.rs:108-116: `src: RenderTargetHandle`), not only the
 * one r3n_resolve_opaque fills: this writes `n_pixels` RGBA half texels starting at `first_pixel` into the frame's HDR
 * target.  A following r3n_tonemap then runs the stand-alone blit kernel over the whole target. */
int r3n_hdr_write(r3n_ctx *ctx, const uint16_t *rgba16f, uint64_t first_pixel, uint64_t n_pixels);
/* ---- tonemapping operators and auto-exposure: what rend3-routine/src/tonemapping.rs:1-10 announces and does not have ("As of
 * right now there is no tonemapping applied as we don't have auto-exposure yet. Once we have auto-exposure, we can do proper
 * tonemapping, and will offer a variety of tonemapping operators").  Not in the reference; opt-in.  With nothing set every frame
 * is the reference's blit, fused into the resolve as before.  Arithmetic: DESIGN.md section 2 "Exposure and tonemapping
 * operators" (f32, one rounding per operation, table-driven 2^x, integer metering). */
#define R3N_TONEMAP_OP_BLIT 0u      /* no operator: exposure only (completes tonemapping.rs:1-10) */
#define R3N_TONEMAP_OP_REINHARD 1u  /* extended Reinhard per channel, white point (completes tonemapping.rs:1-10) */
#define R3N_TONEMAP_OP_ACES 2u      /* Narkowicz's rational ACES fit per channel (completes tonemapping.rs:1-10) */
#define R3N_EXPOSURE_MANUAL 0u      /* the exposure is exposure_ev (completes tonemapping.rs:1-10) */
#define R3N_EXPOSURE_AUTO 1u        /* metered from a luminance histogram of the HDR target (completes tonemapping.rs:1-10) */
typedef struct r3n_tonemap_opts {   /* 48 B */
    uint32_t op, exposure_mode;
    float exposure_ev;   /* MANUAL: the exposure in stops; AUTO: compensation added to the metered value */
    float white;         /* REINHARD: in (0, 65504] */
    float key_log2;      /* AUTO: log2 of the grey the mean luminance is brought to */
    float min_ev, max_ev;/* AUTO: clamp of the target; all three ev fields within [-32, 32] */
    float adapt;         /* AUTO: share of the distance to the target covered per frame, in (0, 1]; 1 = instant */
    uint32_t low_permille, high_permille; /* AUTO: ranks [low, high) of the sorted luminances are averaged; 0 <= low < high <= 1000 */
    uint32_t _pad[2];
} r3n_tonemap_opts;
/* Completes tonemapping.rs:1-10.  NULL, or {BLIT, MANUAL, exposure_ev = 0}: the reference's behaviour (default), r3n_tonemap
 * launches nothing after a resolve.  Otherwise r3n_tonemap runs [histogram, metering step,] operator over the HDR target behind
 * the resolve, whatever the resolve fused, every launch timed under R3N_STAGE_TONEMAP.  Every field is validated whatever the
 * mode (NaN anywhere, an unknown op or mode, white outside (0, 65504], an ev field outside [-32, 32], min_ev > max_ev, a
 * key_log2 that is not finite, adapt outside (0, 1], low >= high or high > 1000 -> R3N_ERR_INVALID_ARG, nothing changed).
 * Outside a frame only (R3N_ERR_STATE inside one).  Invalidates the adaptation state: the next metered frame adapts instantly.
 * Never waits for the GPU.  AUTO needs the whole target: r3n_tonemap returns R3N_ERR_UNSUPPORTED with nothing launched while
 * r3n_set_row_range leaves rows out (a rank that meters its own rows alone would expose differently); MANUAL works under any split. */
int r3n_tonemap_set(r3n_ctx *ctx, const r3n_tonemap_opts *opts);
typedef struct r3n_exposure_state {
    uint32_t histogram[256]; uint32_t excluded; uint32_t valid;
    float mean_log2, target_ev, current_ev, scale; uint32_t _pad[2];
} r3n_exposure_state;
/* Completes tonemapping.rs:1-10.  What the last r3n_tonemap that ran produced; waits for it.  MANUAL (or nothing set, or AUTO
 * before its first r3n_tonemap): an empty histogram, valid = 0, current_ev = target_ev = the exposure in use, its scale. */
int r3n_readback_exposure(r3n_ctx *ctx, r3n_exposure_state *out);
/* ---- bloom: a pyramid of the HDR target's highlights, composited in front of the operator.  Not in the reference (it hangs on
 * the same note, rend3-routine/src/tonemapping.rs:1-10); opt-in.  With nothing set every frame is what it is without this entry,
 * bit for bit and launch for launch.  Arithmetic: DESIGN.md section 2 "Bloom" (exposed units, soft-knee bright pass, 4x4 tent
 * down, 2x tent up with scatter, halves stored, f32 in a pinned order). */
#define R3N_BLOOM_MAX_LEVELS 16u     /* most levels of a bloom pyramid (extends tonemapping.rs:1-10) */
typedef struct r3n_bloom_opts {   /* 32 B */
    float intensity;      /* [0, 1024]; 0 = off */
    float threshold;      /* [0, 65504], exposed units: 1 = display white, under auto-exposure too */
    float knee;           /* [0, threshold]: the bright pass rises quadratically over [threshold - knee, threshold + knee] */
    float scatter;        /* [0, 1]: share of each coarser level added on the way up */
    uint32_t max_levels;  /* [1, 16] */
    uint32_t _pad[3];
} r3n_bloom_opts;
/* Extends tonemapping.rs:1-10.  NULL, or intensity == 0: off (default), r3n_tonemap launches exactly what it launches without
 * this entry.  Otherwise r3n_tonemap runs [histogram, metering step,] the bloom chain, then the operator with the composite, all
 * on one stream and timed under R3N_STAGE_TONEMAP; without r3n_tonemap_set options the operator is BLIT at scale 1.  Every field
 * is validated (a NaN anywhere or a field outside its range -> R3N_ERR_INVALID_ARG, nothing changed).  Outside a frame only
 * (R3N_ERR_STATE inside one).  Never waits for the GPU.  Independent of r3n_tonemap_set, in either order.  The HDR target is never
 * written.  Bloom needs neighbouring rows: r3n_tonemap returns R3N_ERR_UNSUPPORTED with nothing launched while r3n_set_row_range
 * leaves rows out. */
int r3n_bloom_set(r3n_ctx *ctx, const r3n_bloom_opts *opts);
/* Extends tonemapping.rs:1-10.  Test and diagnostic entry: level `level` of the up chain (a_level) as the last r3n_tonemap left
 * it, three halves per texel; waits for that call.  Under R3N_TUNE bloom_keep_down=1 the levels of the down chain are kept too:
 * `*levels + k` reads d_k.  rgb16f may be NULL (sizes only); otherwise capacity_texels >= width * height of the level.
 * R3N_ERR_STATE if the last r3n_tonemap ran no bloom, R3N_ERR_INVALID_ARG for a level that does not exist. */
int r3n_readback_bloom(r3n_ctx *ctx, uint32_t level, uint16_t *rgb16f, uint64_t capacity_texels,
                       uint32_t *width, uint32_t *height, uint32_t *levels);
/* Marks the end of the frame: swaps the temporal state (InputOutputBuffer::swap, culling/suballoc.rs:164-214). */
int r3n_frame_end(r3n_ctx *ctx);

/* ---- the whole frame in ONE call.  r3n_render_frame issues every node of BaseRenderGraph::add_to_graph
 * (rend3-routine/src/base.rs:129-185, executed by RenderGraph::execute, rend3/src/graph/graph.rs:265-518) in the reference's
 * order -- exactly the sequence of the per-node entry points above: r3n_frame_begin, r3n_shadow_viewport, r3n_skinning, per shadow
 * view r3n_uniform_bake / r3n_cull / r3n_forward(DEPTH, RESIDUAL, OPAQUE | CUTOUT), the viewport's r3n_uniform_bake,
 * r3n_forward(FORWARD, PREDICTED, ..), r3n_hi_z, r3n_cull, r3n_forward(FORWARD, RESIDUAL, ..), r3n_resolve_opaque, r3n_skybox, the
 * transparent r3n_forward, r3n_tonemap, r3n_frame_end.  The per-node entry points stay (a Rust integration calls them from its node closures);
 * this one is for hosts that do not need a graph between the nodes: one FFI crossing per frame instead of ~45.
 * `desc` carries what Renderer::evaluate_instructions + the node closures compute on the CPU in the reference: the FrameUniforms
 * (uniforms.rs:28-48), the viewport's PerCameraUniform header (culler.rs:485-502), one header + atlas viewport per shadow map
 * (directional.rs:99-157, base.rs:366-396), the light buffers, optionally this frame's skinning inputs. */
typedef struct r3n_shadow_view272 {
    r3n_camera_header240 header;   /* header.shadow_index == the view's index in the array */
    uint32_t x, y, size;           /* ShadowMap offset / size in the atlas (base.rs:369) */
    uint32_t _pad[5];
} r3n_shadow_view272;
/* multi-GPU hook (not in the reference): called on the calling thread at the points where ranks merge -- after the shadow
 * nodes, after pass 1 (before r3n_hi_z), after pass 2 (before r3n_resolve_opaque); the callee enqueues its collectives on
 * r3n_stream() (r3n_exchange_depth / r3n_exchange_buffers give the buffers), the shadow views' on the stream
 * r3n_exchange_shadow_stream returns.  Non-zero return aborts the frame (R3N_ERR_STATE). */
#define R3N_EXCHANGE_SHADOW 0u
#define R3N_EXCHANGE_PASS1 1u
#define R3N_EXCHANGE_PASS2 2u
typedef int (*r3n_exchange_fn)(void *user, uint32_t site);
#define R3N_FRAME_VIEWPORT_FIRST 1u  /* hand the GPU the viewport's bake + pass 1 before the shadow nodes (same results) */
#define R3N_FRAME_SHADOW_MASK 2u     /* shadow_view_mask is valid: bit v set = this rank renders view v, WHOLE (every object slot,
                                        whatever r3n_set_object_range says); the others are not rendered here (their atlas
                                        rectangles arrive through the exchange) */
typedef struct r3n_frame_desc {
    uint32_t struct_size;            /* sizeof(r3n_frame_desc) */
    uint32_t flags;                  /* R3N_FRAME_* */
    uint32_t width, height, samples; /* as r3n_frame_begin */
    uint32_t shadow_atlas_width, shadow_atlas_height;
    uint32_t n_shadow_views;
    float clear_color[4];
    const r3n_frame_uniforms496 *uniforms;
    const r3n_camera_header240 *viewport_header;
    const r3n_shadow_view272 *shadow_views;  /* n_shadow_views entries */
    uint64_t shadow_view_mask;
    /* light buffers as r3n_lights_write takes them; NULL directional_buffer = keep what the context has */
    const void *directional_buffer;
    uint64_t directional_bytes;
    const void *point_buffer;
    uint64_t point_bytes;
    /* skinning (base.rs:145) as r3n_skinning takes it; n_skeletons == 0 = no skinning node this frame */
    const r3n_skinning_input40 *skin_inputs;
    uint32_t n_skeletons, n_joint_matrices;
    const float *joint_matrices;
    r3n_exchange_fn exchange;        /* NULL = single GPU */
    void *exchange_user;
} r3n_frame_desc;
int r3n_render_frame(r3n_ctx *ctx, const r3n_frame_desc *desc);
/*      r3n_render_frame draws the opaque key of a shadow view in two phases: triangles the previous frame's
 *      tile minima of the view call hidden are set aside, tested against this frame's minima behind everything else, and drawn
 *      only if they can still change a texel.  The atlas is bit for bit the one-phase atlas.  The figures of the LAST frame for one
 *      shadow camera (waits for the frame): active = the view was drawn in two phases (a power-of-two view of at least 64 texels on
 *      a four-texel boundary, no communicators / exchange callback / row range / bands, R3N_TUNE shadow_occlusion not 0);
 *      predicted = phase 1 had a prediction (not on a context's first frame, nor after the view's size or anything but the
 *      translation of its view-projection changed, nor when it moved by a fraction of a texel); deferred = triangles set aside,
 *      dropped + survivors = deferred; capacity = records the deferred list holds (a triangle beyond it is drawn in phase 1). */
typedef struct r3n_shadow_occlusion_counters {
    uint32_t active, predicted, deferred, dropped, survivors, capacity;
} r3n_shadow_occlusion_counters;
int r3n_shadow_occlusion_stats(r3n_ctx *ctx, r3n_camera camera, r3n_shadow_occlusion_counters *out);

/* ---- multi-GPU support: object-range sharding (not in the reference).
 * Only objects with slot in [begin, end) are culled/drawn by this context; buffers stay replicated.  The ranges are the CALLER's
 * partition of the slots that exist when it is made: a slot beyond every rank's `end` (objects added after the object buffer grew) is
 * drawn by NO rank until the ranges are set again -- re-partition after world edits that add slots, or give the last rank
 * end = 0xFFFFFFFF. */
int r3n_set_object_range(r3n_ctx *ctx, uint32_t begin, uint32_t end);
/* The same sharding by OWNER BYTE instead of slot range: this context culls / draws the opaque and cutout objects whose
 * owners[slot] == rank (a spatial partition -- Morton order of the bounding-sphere centres -- gives every rank a compact region
 * of the world and of the screen; its slots are not contiguous).  n >= the object capacity (re-send after the object buffer
 * grows); owners == NULL returns to r3n_set_object_range.  Synchronises (world-edit rate). */
int r3n_set_object_owners(r3n_ctx *ctx, const uint8_t *owners, uint32_t n, uint32_t rank);
/* How the VIEWPORT camera is sharded over ranks (shadow views are sharded by view in both):
 *   R3N_SHARD_OBJECTS (default): a rank draws its objects (r3n_set_object_range / r3n_set_object_owners) over the whole target;
 *     ranks MAX-merge the depth plane after pass 1 and the keys after pass 2;
 *   R3N_SHARD_ROWS (sort-first): a rank culls and draws EVERY object, but rasterises only the rows [row_begin, row_end) of
 *     r3n_set_row_range -- its rows of the depth plane / keys are then final without a reduction: after pass 1 the ranks all-gather
 *     their rows of the depth plane (every rank culls against the whole Hi-Z pyramid and arrives at the unsharded visible sets),
 *     after pass 2 nothing is exchanged.  Culling is replicated, pixel work is divided, and the largest exchange (8 B per pixel of
 *     keys) disappears.  Do not combine with object ranges / owners. */
#define R3N_SHARD_OBJECTS 0u
#define R3N_SHARD_ROWS 1u
int r3n_set_shard_mode(r3n_ctx *ctx, uint32_t mode);
/* The exchanges of the sort-first split issued BY THE LIBRARY over RCCL, inside r3n_render_frame: no callback, no host-language
 * collective calls on the frame path (Python's torch.distributed calls cost 0.33 ms per frame, more than a rank's GPU work at
 * N = 8).  RCCL is bound at run time (the copy the process already holds -- PyTorch's -- else ROCm's librccl.so.1).
 *   r3n_comm_unique_id   one ncclUniqueId (128 B); rank 0 makes R3N_COMM_IDS of them and hands them to every rank through
 *                        whatever launched the ranks (torch.distributed broadcast, MPI, a file);
 *   r3n_comm_init        collective: three communicators -- main stream (depth bands), shadow lane (shadow views), resolve stream
 *                        (image rows) -- so that no exchange queues behind another stream's;  switches the context to
 *                        R3N_SHARD_ROWS; from then on r3n_render_frame owns the shadow views v with v mod world == rank, rasterises
 *                        the band of rows `rank` of r3n_host row ranges (rows split as evenly as possible, the first height mod world
 *                        bands one row taller), broadcasts the shadow rectangles on the shadow lane's stream, all-gathers the
 *                        depth bands in front of r3n_hi_z (keys under MSAA; in place when the bands are equal, else one grouped
 *                        broadcast per band) and the Rgba8 rows behind the resolve.  r3n_frame_desc.exchange must be NULL then.
 *   r3n_comm_set_split   R3N_SHARD_ROWS (what r3n_comm_init selects) or R3N_SHARD_OBJECTS: the object-range split of BASELINE.json's
 *                        north_star -- this rank culls + draws the viewport's objects of r3n_set_object_range / r3n_set_object_owners
 *                        over the WHOLE target; r3n_render_frame then issues a MAX all-reduce of the pass-1 depth plane (f32;
 *                        the u64 keys under MSAA) in front of r3n_hi_z and a MAX reduce-scatter of the u64 visibility keys onto
 *                        the row bands behind pass 2 (an all-reduce when the bands are ragged); shadow views, resolve bands and
 *                        the row gather as above.  Choose by workload: rows replicates the cull, objects moves 12 B per pixel.
 *   r3n_comm_destroy     collective; back to a single-rank context.
 * The three communicators run collectives concurrently on three streams; RCCL requires every rank to issue the collectives of one
 * communicator in the same order, so r3n_frame_desc.flags, samples, the target size and n_shadow_views MUST be identical on
 * every rank (tests/rccl_shim.cpp executes every collective synchronously and times out on an order mismatch). */
#define R3N_COMM_ID_BYTES 128
#define R3N_COMM_IDS 3
int r3n_comm_unique_id(uint8_t *id /* R3N_COMM_ID_BYTES */);
int r3n_comm_init(r3n_ctx *ctx, const uint8_t *ids /* R3N_COMM_IDS x R3N_COMM_ID_BYTES */, uint32_t rank, uint32_t world);
int r3n_comm_set_split(r3n_ctx *ctx, uint32_t mode /* R3N_SHARD_OBJECTS | R3N_SHARD_ROWS */);
int r3n_comm_destroy(r3n_ctx *ctx);
/* Device pointers + sizes of the exchange buffers, for RCCL (all-reduce MAX over ranks):
 * the 64-bit visibility/depth keys (width*height u64, as int64 non-negative) and the f32 shadow atlas. */
/* this camera's own object-slot range, overriding r3n_set_object_range for it (a shadow view owned whole by one rank draws
 * every object there and nothing elsewhere); begin == end == 0xFFFFFFFF returns the camera to the global range */
int r3n_set_camera_object_range(r3n_ctx *ctx, r3n_camera camera, uint32_t begin, uint32_t end);
/* the pass-1 exchange of single-sample targets: only DEPTH has to be global for the Hi-Z cull (33 MB at 4K instead of 66 MB of
 * keys).  Derives mip 0 of the Hi-Z pyramid (f32 depth plane) from the keys and returns its device address; after the callers'
 * element-wise MAX all-reduce of the plane on r3n_stream(), r3n_hi_z builds the pyramid from it. */
int r3n_exchange_depth(r3n_ctx *ctx, void **depth_f32, uint64_t *count);
int r3n_exchange_buffers(r3n_ctx *ctx, void **visibility_keys, uint64_t *visibility_count,
                         void **shadow_atlas, uint64_t *shadow_atlas_count);
/* The shadow atlas for the shadow-view exchange (a view's owner sends its atlas rectangle to the other ranks) WITHOUT ordering the
 * main stream behind the shadow views: *stream = a shadow lane's HIP stream, ordered behind every lane that drew a view this
 * frame (the main stream while R3N_SINGLE_STREAM=1).  Collectives enqueued there run beside the viewport's passes, which never
 * read the atlas; the resolve -- its only reader -- waits for that lane as it does for the views themselves. */
int r3n_exchange_shadow_stream(r3n_ctx *ctx, void **shadow_atlas, uint64_t *shadow_atlas_count, void **stream);
/* Device pointer of the tonemapped Rgba8 image (width*height*4 bytes) and the rows [row_begin,row_end) this
 * rank resolves/tonemaps when screen-space work is split after the exchange. */
int r3n_set_row_range(r3n_ctx *ctx, uint32_t row_begin, uint32_t row_end);
int r3n_output_buffer(r3n_ctx *ctx, void **rgba8, uint64_t *bytes);
/* The same buffer WITHOUT ordering the main stream behind the resolve, for work that only has to follow the resolve (the row
 * all-gather): *stream = the HIP stream this frame's resolve was enqueued on (its own stream while frames are in flight, else
 * the main stream).  Work enqueued there is announced with r3n_output_work_enqueued, so that whatever later waits for the resolve
 * (read-backs, the frame that reuses these targets) waits for that work too.  The next frame's culling and rasterisation then
 * overlap with the resolve AND the gather, as they do without an exchange. */
int r3n_output_buffer_async(r3n_ctx *ctx, void **rgba8, uint64_t *bytes, void **stream);
int r3n_output_work_enqueued(r3n_ctx *ctx);

/* ---- parity / debug taps (not in the reference; synchronise) */
/* L1 set: flags[i] = 1 iff object slot i survived the frustum test of `camera`'s last r3n_cull */
int r3n_readback_visible_objects(r3n_ctx *ctx, r3n_camera camera, uint8_t *flags, uint32_t capacity);
/* L2 set in canonical layout: bit for (object o, triangle t) at index tri_base[o] + t, where tri_base is the
 * exclusive scan of (enabled ? index_count/3 : 0) over object slots.  pass = execute_culling result
 * (cull.wgsl:264-324); residual = newly visible (cull.wgsl:366-371).  `n` = total triangle count. */
int r3n_readback_triangle_sets(r3n_ctx *ctx, r3n_camera camera, uint8_t *pass, uint8_t *residual, uint64_t n);
/* TEST AND DIAGNOSTIC ENTRY: the lists `camera`'s last r3n_cull appended, entry by entry as the device holds them.  The triangle
 * cull appends every passing triangle to the predicted list (list 0) and -- the viewport only -- every newly visible one to the
 * residual list (list 1); each list has one region per (material key k, sub-list q), and a region holds counts[k][q] entries of
 * the *subcap reserved for it.  `out` receives the regions' entries concatenated in (k, q) order, exactly as stored, never
 * re-sorted: sum(counts) entries.  out == NULL asks for counts and *subcap alone (R3N_OK).  Not culled yet -> R3N_ERR_STATE;
 * list 1 of a shadow camera (it has no residual list), a list number above 1 or a `capacity` (entries of `out`) below
 * sum(counts) -> R3N_ERR_INVALID_ARG.  Host-side only: copies, no launch. */
#define R3N_SUBQ 32
typedef struct r3n_tri_ref {
    uint32_t object;
    uint32_t triangle;
} r3n_tri_ref;
int r3n_readback_triangle_lists(r3n_ctx *ctx, r3n_camera camera, uint32_t list, r3n_tri_ref *out, uint64_t capacity,
                                uint32_t counts[3][R3N_SUBQ], uint32_t *subcap);
/* per-region IndirectCall as cull.wgsl leaves it: calls[0..3) predicted, calls[3..6) residual (by material key) */
int r3n_readback_draw_calls(r3n_ctx *ctx, r3n_camera camera, r3n_indirect_call calls[6]);
/* work-queue occupancy of the rasteriser: big_items[i] = number of >8x8 px work items the i-th r3n_forward call of
 * the last frame produced (performance diagnostics only) */
int r3n_readback_raster_stats(r3n_ctx *ctx, uint32_t big_items[64]);
/* what the transparent pass reads, whichever of r3n_blend_order_write / r3n_blend_sort wrote it: order[n] = blend objects back to
 * front, rank_base[n + 1] = exclusive scan of their triangle counts.  `capacity` = entries of `order` (and, plus one, of
 * `rank_base`); smaller than the set -> R3N_ERR_INVALID_ARG */
int r3n_readback_blend_order(r3n_ctx *ctx, uint32_t *order, uint32_t *rank_base, uint32_t capacity);
/* The camera's baked matrices, 32 floats per slot.  After r3n_render_frame only the slots inside the frustum this frame or last
 * frame are defined (see r3n_uniform_bake); after the per-node r3n_uniform_bake every enabled slot is. */
int r3n_readback_baked(r3n_ctx *ctx, r3n_camera camera, float *model_view_and_mvp, uint32_t capacity);
int r3n_readback_mesh(r3n_ctx *ctx, uint64_t byte_offset, void *dst, uint64_t bytes); /* e.g. skinned attribute runs */
/* The 128-byte object records [first_slot, first_slot + n) as the device holds them (ObjectManager's buffer, rend3/src/managers/
 * object.rs:344-364; after r3n_mesh_compact: with the relocated offsets, mesh.rs:197-211 being the reason a range ever moves here).
 * first_slot + n beyond the object capacity -> R3N_ERR_INVALID_ARG.  Waits for every frame in flight. */
int r3n_readback_objects(r3n_ctx *ctx, uint32_t first_slot, r3n_object128 *records, uint32_t n);
int r3n_readback_joint_matrices(r3n_ctx *ctx, uint32_t first_matrix, float *dst, uint32_t n_matrices); /* what the last r3n_skinning read */
/* The texture table as the device holds it (rend3/src/managers/texture.rs keeps one entry per handle): offset in pool words, width,
 * height, mips, format = the pool class (R3N_TEXTURE_RGBA8_UNORM / _SRGB, or 2 = four f32 per texel); removed slots have width =
 * height = 0 in THIS read-back.  *n_slots = table length; descs == NULL asks for the length alone (R3N_OK); a `capacity` below it
 * -> R3N_ERR_INVALID_ARG. */
int r3n_readback_texture_descs(r3n_ctx *ctx, r3n_texture_desc32 *descs, uint32_t capacity, uint32_t *n_slots);
int r3n_readback_texels(r3n_ctx *ctx, uint64_t first_texel, uint32_t *rgba8, uint64_t n_texels); /* the decoded RGBA8 texel pool (after
                                                                                         r3n_textures_write_encoded: texture i's levels back to back, textures
                                                                                         in array order, each starting on a 4-texel boundary) */
/* Diagnostic: bordered face `face` (0 .. 5: +X, -X, +Y, -Y, +Z, -Z) of level `level` of cube `cube` as the device holds it:
 * (n_level + 2)^2 texels, row-major, the four corner texels zero.  *pool_class (may be NULL) = 0 / 1: one RGBA8 word per texel
 * (Rgba8Unorm / Rgba8UnormSrgb), 2: four f32 words per texel.  `words` = the 32-bit words `dst` has room for.  A cube, level or
 * face that does not exist, or a `dst` shorter than the face -> R3N_ERR_INVALID_ARG. */
int r3n_readback_cube_face(r3n_ctx *ctx, uint32_t cube, uint32_t level, uint32_t face, void *dst, uint64_t words, uint32_t *pool_class);
int r3n_readback_visibility(r3n_ctx *ctx, uint64_t *keys);  /* width*height*samples, a pixel's samples contiguous */
int r3n_readback_depth(r3n_ctx *ctx, float *depth);         /* width*height, from the visibility keys (min over samples) */
int r3n_readback_hiz(r3n_ctx *ctx, float *pyramid, uint64_t count); /* all mips, mip0 first */
int r3n_readback_shadow_atlas(r3n_ctx *ctx, float *atlas);  /* atlas_w*atlas_h */
int r3n_readback_hdr(r3n_ctx *ctx, uint16_t *rgba16f);      /* width*height*4 half bits */
int r3n_readback_output(r3n_ctx *ctx, uint8_t *rgba8, float *rgba_f32); /* either may be NULL */

/* ---- timing taps for bench.py: HIP events recorded on the context's stream around every kernel launch of a
 * named stage.  r3n_stage_times returns accumulated milliseconds and launch counts since the last reset. */
#define R3N_STAGE_BAKE 0
#define R3N_STAGE_OBJECT_CULL 1
#define R3N_STAGE_TRIANGLE_CULL 2
#define R3N_STAGE_HIZ 3
#define R3N_STAGE_RASTER 4          /* viewport: per-triangle pass (small triangles + work-item emission) */
#define R3N_STAGE_SHADE 5
#define R3N_STAGE_TONEMAP 6
#define R3N_STAGE_CLEAR 7
#define R3N_STAGE_RASTER_BIG 8      /* viewport: wave-cooperative pass over the large-triangle work items */
#define R3N_STAGE_SHADOW_RASTER 9   /* shadow views: per-triangle pass */
#define R3N_STAGE_SHADOW_RASTER_BIG 10
#define R3N_STAGE_SKINNING 11
#define R3N_STAGE_VERTEX 12         /* resolve pre-pass: flag the visible triangles + one vertex stage per flagged triangle */
#define R3N_STAGE_POSE 13           /* animation poses evaluated in front of the skinning kernel */
#define R3N_STAGE_EXCHANGE_SHADOW 14 /* r3n_comm_init: shadow rectangles packed, broadcast, unpacked (shadow lane) */
#define R3N_STAGE_EXCHANGE_DEPTH 15  /* depth bands (keys under MSAA) gathered in front of Hi-Z (main stream) */
#define R3N_STAGE_EXCHANGE_ROWS 16   /* Rgba8 rows gathered behind the resolve (resolve's stream) */
#define R3N_STAGE_EXCHANGE_KEYS 17   /* object-range split: MAX reduce-scatter of the visibility keys onto the row bands (main stream) */
#define R3N_STAGE_RASTER_CUT 18      /* viewport, CUTOUT key: per-triangle pass (alpha test per fragment; the opaque key's launches stay under RASTER) */
#define R3N_STAGE_RASTER_BIG_CUT 19  /* viewport, CUTOUT key: work-item pass */
#define R3N_STAGE_SKYBOX 20          /* the skybox node (r3n_skybox) */
#define R3N_STAGE_BLEND_SORT 21      /* r3n_blend_sort: the transparent pass's draw order sorted on the device */
#define R3N_STAGE_MORPH 22           /* r3n_morph: morph targets blended into the instances' private runs */
#define R3N_STAGE_NORMALS 23         /* r3n_vertex_normals: normals of morphed meshes without NORMAL, recomputed */
#define R3N_STAGE_TANGENTS 24        /* r3n_vertex_tangents: tangents of morphed meshes without TANGENT, generated */
#define R3N_STAGE_COUNT 25
int r3n_timing_enable(r3n_ctx *ctx, int enable);
/* What a timed span holds besides its kernels -- two event packets and a launch's dispatch, measured around an empty kernel when
 * timing is first enabled (median of 32) -- and already taken off every span r3n_stage_times reports. */
int r3n_timing_overhead(r3n_ctx *ctx, double *ms_per_span);
/* Shadow views normally run on auxiliary streams concurrently with the viewport chain; per-kernel durations measured
 * while kernels of other streams are resident are inflated, so timing passes can serialise everything on the main
 * stream (enable = 0).  Only between frames. */
int r3n_set_multi_stream(r3n_ctx *ctx, int enable);
int r3n_stage_times(r3n_ctx *ctx, double ms[R3N_STAGE_COUNT], uint64_t launches[R3N_STAGE_COUNT], int reset);
/* Measured HBM streaming rate of this device, the denominator BASELINE.md section 5 asks for ("measured on the target
 * box, not taken from the datasheet"): a float4 grid-stride copy of `bytes` (>= 64 MiB, well past the 256 MiB Infinity
 * Cache when 1 GiB) repeated `repeats` times, HIP-event timed; *gb_per_s = (bytes read + bytes written) / best time.
 * Allocates and frees two scratch buffers; synchronises. */
int r3n_hbm_copy_rate(r3n_ctx *ctx, uint64_t bytes, uint32_t repeats, double *gb_per_s);
/* Self-test of the short correctly-rounded reciprocal / square root / reciprocal square root sequences the shading kernels use
 * (csrc/exact_math.h): all 2^32 f32 bit patterns on the device against the compiler's IEEE expansions.  hist[3][512]: patterns
 * on which the UNGUARDED sequences differ, by function (rcp, sqrt, rsqrt) and sign + biased exponent; guarded[3]: patterns on
 * which the guarded functions -- what the library evaluates -- differ (must be 0).  Needs no context; returns a hipError_t. */
int r3n_selftest_exact_math(int hip_device, unsigned long long *hist, unsigned long long *guarded);
/* exact_math::unorm8 (c / 255 without the division) against the division for all 256 inputs; *n_bad = how many differ (0). */
int r3n_selftest_unorm8(int hip_device, uint32_t *n_bad);

/* ---- host-side mirror of the reference's CPU math on the path (rend3_amd/csrc/host.cpp).
 * In a real integration these stay in Rust (rend3 core); they exist here so the standalone harness, the
 * bench and the parity tests can build the boundary inputs without the oracle.  Matrices are column-major f32[16]. */
/* glam Mat4 mul / inverse as used by camera.rs:64-73, uniforms.rs:41-43 */
void r3n_host_mat4_mul(const float *a, const float *b, float *out);
void r3n_host_mat4_inverse(const float *m, float *out);
/* glam look_at_{lh,rh} (shadow_camera.rs:12-14,28); rh != 0 selects the right-handed form */
void r3n_host_look_at(const float eye[3], const float center[3], const float up[3], int rh, float *out);
/* camera.rs:88-107: kind 0 = Orthographic{size[3]}, 1 = Perspective{vfov_deg = params[0], near = params[1]} */
void r3n_host_projection(int kind, const float *params, int rh, float aspect_ratio, float *out);
/* Frustum::from_matrix, rend3/src/util/frustum.rs:96-145: 5 planes x vec4 */
void r3n_host_frustum_from_matrix(const float *m, float *planes20);
/* Frustum::contains_sphere, rend3/src/util/frustum.rs:148-161: 1 when the sphere touches or is inside all 5 planes */
int r3n_host_frustum_contains_sphere(const float *planes20, const float center[3], float radius);
/* BoundingSphere::{from_mesh, apply_transform}, frustum.rs:15-56 */
void r3n_host_bounding_sphere_from_mesh(const float *positions, uint64_t vertex_count, float out_center[3],
                                        float *out_radius);
void r3n_host_bounding_sphere_apply_transform(const float center[3], float radius, const float *m,
                                              float out_center[3], float *out_radius);
/* ObjectManager::object_add_callback for `n` objects at once (rend3/src/managers/object.rs:236-300): fills the 128-byte
 * records (world bounding sphere = mesh sphere transformed, object.rs:268-269; enabled = 1).
 * mesh_desc[i] = {center.xyz, radius} as f32[4]; mesh_u32[i] = {first_index, index_count, attr_off[6]} as u32[8]. */
void r3n_host_build_object_records(uint32_t n, const float *transforms /* 16 n */, const float *mesh_desc /* 4 n */,
                                   const uint32_t *mesh_u32 /* 8 n */, const uint32_t *material_index /* n */,
                                   r3n_object128 *out_records);
/* Mesh::calculate_normals_for_buffers, rend3-types/src/lib.rs:662-704 */
void r3n_host_calculate_normals(const float *positions, uint64_t vertex_count, const uint32_t *indices,
                                uint64_t index_count, int left_handed, float *normals);
/* Mesh::calculate_tangents_for_buffers, rend3-types/src/lib.rs:784-837 (zeroed = true): the serial loop whose words
 * r3n_vertex_tangents reproduces (contract there).  uvs: vertex_count f32x2; tangents: vertex_count f32x3, written. */
void r3n_host_calculate_tangents(const float *positions, const float *normals, const float *uvs, uint64_t vertex_count,
                                 const uint32_t *indices, uint64_t index_count, float *tangents);
/* rows[0..V] then 3*floor(I/3) triangle numbers: row v = the triangles naming v, ascending, one entry per occurrence.
 * Returns 0, or nonzero if an index is >= vertex_count (nothing usable is written then). */
int r3n_host_vertex_adjacency(const uint32_t *indices, uint64_t index_count, uint64_t vertex_count, uint32_t *out);
/* shadow_camera, rend3/src/managers/directional/shadow_camera.rs:6-33: outputs the shadow view matrix and its
 * orthographic projection */
void r3n_host_shadow_camera(const float direction[3], float distance, uint32_t resolution,
                            const float camera_location[3], int rh, float *out_view, float *out_proj);
/* allocate_shadow_atlas, rend3/src/managers/directional/shadow_alloc.rs:59-136.  Returns the number of maps
 * written (0 when there is nothing to allocate); out_maps[i] = {offset_x, offset_y, size, handle}. */
uint32_t r3n_host_allocate_shadow_atlas(const uint32_t *handles, const uint16_t *resolutions, uint32_t n,
                                        uint32_t max_dimension, uint32_t out_dimensions[2],
                                        uint32_t *out_maps /* 4*n */);

/* Everything the CPU computes per frame on the path, in one call: CameraState::new (camera.rs:23-85) for the viewport,
 * DirectionalLightManager::evaluate (directional.rs:99-157: shadow atlas allocation, one shadow camera per light, the light
 * buffer), FrameUniforms::new (uniforms.rs:28-48) and the PerCameraUniform headers of the viewport and of every shadow view
 * (culler.rs:477-502).  `lights[i].resolution == 0` marks a free slot of the light manager (skipped; handles keep their index). */
typedef struct r3n_host_camera144 {
    float view[16];
    uint32_t projection_kind;      /* 0 Orthographic{size}, 1 Perspective{vfov, near}, 2 Raw(mat4) (camera.rs:88-107) */
    uint32_t handedness;           /* 0 left, 1 right */
    float aspect_ratio;            /* Option<f32>: <= 0 = None (1.0) */
    uint32_t _pad;
    float projection_params[16];   /* size.xyz | vfov degrees, near | the matrix */
} r3n_host_camera144;
typedef struct r3n_host_directional_light48 {
    float color[3];
    float intensity;
    float direction[3];
    float distance;
    uint32_t resolution;
    uint32_t _pad[3];
} r3n_host_directional_light48;
typedef struct r3n_host_frame {
    r3n_frame_uniforms496 uniforms;
    r3n_camera_header240 viewport_header;
    uint32_t shadow_atlas_width, shadow_atlas_height, n_shadow_views, _pad0;
    float camera_location[3];
    float _pad1;
    float view_proj[16];
    r3n_shadow_view272 shadow_views[R3N_MAX_SHADOW_VIEWS];
    uint32_t shadow_handles[R3N_MAX_SHADOW_VIEWS];  /* light handle of view i */
    uint64_t directional_bytes;                     /* 16 + 128 * n_shadow_views */
    uint8_t directional_buffer[8208];              /* 16 + 128 * R3N_MAX_SHADOW_VIEWS */
} r3n_host_frame;
/* returns 0, or -1 when more than R3N_MAX_SHADOW_VIEWS lights cast shadows */
int r3n_host_evaluate_frame(const r3n_host_camera144 *camera, const r3n_host_directional_light48 *lights, uint32_t n_lights,
                            uint32_t max_atlas_dimension, const float ambient[4], uint32_t width, uint32_t height, uint32_t samples,
                            uint32_t object_capacity, r3n_host_frame *out);

#ifdef __cplusplus
}
#endif
#endif /* R3N_H */
