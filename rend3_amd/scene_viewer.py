"""The reference's scene-viewer example as a harness over the C ABI: load a glTF / GLB file, instance it, add the flagged
directional light, place the camera -- the inputs the named BASELINE.json configs are quoted on (scifi-base.glb, Bistro, Emerald
Square: `examples/src/scene_viewer`).  Follows (reference file:line):

  SceneViewer::default / from_args        examples/src/scene_viewer/mod.rs:300-330, 336-431 (flags and their defaults)
  setup: the flagged light + load_gltf    :463-520  (light: colour 1, `--directional-light-intensity`, distance =
                                           `--shadow-distance`, resolution 2048)
  handle_redraw: camera, settings         :640-646 (view = euler XYZ(-pitch, -yaw, 0) * T(-location), Perspective{60, 0.1}),
                                           :678-681 (ambient = (a, a, a, 1), clear (0, 0, 0, 1))
  App::HANDEDNESS = Right                 :434
  the Bistro test                          :727-751 (flags + camera of BASELINE.json configs[2])
  load_skybox (add_skybox)                 :34-57 (six files right | left | top | bottom | front | back -> add_texture_cube,
                                           Rgba8UnormSrgb, one level), :675 (`skybox: Some(..)` in the frame's routines)

`build(renderer, host_module, material_record, settings)` works on anything with the Renderer's world-edit API -- the HIP
renderer and, in the tests / bench.py's cpu_baseline leg, the oracle -- so a real asset runs through exactly the parity and
measurement code the synthetic stand-ins do.  This module never imports the oracle.

Morph targets need no switch: a file whose primitives have targets gets a morph instance per (node, primitive) from
gltf.instance_scene, drawn with the file's default weights, and anim.pose_animation_frame plays its `weights` channels next to
the node and skin channels (the reference's loader stops at a TODO there; the HIP renderer blends the targets on the GPU).
--morph-normals recompute: primitives with targets and no NORMAL get their normals recomputed from the morphed positions on the
GPU (default base: the normals of the bind shape, under any weights).
--build-tangents: primitives with TEXCOORD_0 and no TANGENT get the tangents rend3's MeshBuilder generates (the reference always
does; here it is opt-in until the oracle follows).  --morph-tangents recompute: with it, morphed primitives get those tangents
regenerated from the morphed positions and normals on the GPU (default base: the tangents of the bind shape).
"""
import argparse
import os

import numpy as np

RIGHT = 1


def _vec3(s):
    v = [float(x) for x in s.split(",")]
    if len(v) != 3:
        raise argparse.ArgumentTypeError("expected x,y,z")
    return tuple(v)


def _camera(s):
    v = [float(x) for x in s.split(",")]
    if len(v) != 5:
        raise argparse.ArgumentTypeError("expected x,y,z,pitch,yaw")
    return tuple(v)


VECTOR_FLAGS = ("--directional-light", "--camera")


def normalize_argv(argv):
    """`--directional-light -1,-4,2` as the reference's parser (pico-args) accepts it: argparse would take the value for a flag
    because it starts with '-', so flag and value are joined with '=' first."""
    out, i = [], 0
    argv = list(argv)
    while i < len(argv):
        if argv[i] in VECTOR_FLAGS and i + 1 < len(argv):
            out.append(argv[i] + "=" + argv[i + 1])
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def add_arguments(ap):
    """The scene-viewer flags that reach the hot path (mod.rs:355-405); windowing / backend / control flags have no meaning here."""
    ap.add_argument("--msaa", type=int, choices=(1, 4), default=1, help="SampleCount (mod.rs:352: --msaa)")
    ap.add_argument("--normal-y-down", action="store_true", help="NormalTextureYDirection::Down (Bistro)")
    ap.add_argument("--directional-light", type=_vec3, default=None, metavar="X,Y,Z", help="add a directional light with this direction")
    ap.add_argument("--directional-light-intensity", type=float, default=1.0)
    ap.add_argument("--ambient", type=float, default=None, help="ambient light level (default 0.1)")
    ap.add_argument("--scale", type=float, default=1.0, help="GltfLoadSettings::scale")
    ap.add_argument("--shadow-distance", type=float, default=100.0, help="GltfLoadSettings::directional_light_shadow_distance")
    ap.add_argument("--shadow-resolution", type=int, default=2048, help="GltfLoadSettings::directional_light_resolution (lights of the file)")
    ap.add_argument("--gltf-disable-directional-lights", action="store_true", help="ignore KHR_lights_punctual lights of the file")
    ap.add_argument("--camera", type=_camera, default=None, metavar="X,Y,Z,PITCH,YAW",
                    help="camera location and angles (default: the default scene's, mod.rs:320-322)")
    ap.add_argument("--skybox", default=None, metavar="PATH",
                    help="the background cube (default: none): a directory holding right|left|top|bottom|front|back .jpg or .png, "
                         "or a .ktx2 / .dds cube map in any supported format with its mip chain (not in the reference, whose "
                         "example loads the six images), or a Radiance .hdr equirectangular panorama, turned into a cube on the GPU")
    ap.add_argument("--skybox-extent", type=int, default=None, metavar="N",
                    help="with a panorama: the extent of the cube's faces (default: half the panorama's height)")
    ap.add_argument("--skybox-equirect", default=None, metavar="FILE",
                    help="the background cube from a 2D .ktx2 / .dds file that holds an equirectangular panorama (its first level)")
    ap.add_argument("--ambient-from-skybox", type=float, default=None, metavar="SCALE",
                    help="ambient colour = SCALE x the mean colour of the panorama's cube (the box-filtered mean of its texels, not a "
                         "solid-angle integral) instead of --ambient")
    ap.add_argument("--lights-from-skybox", type=int, default=0, metavar="N",
                    help="read at most N (1..16) directional lights out of the skybox on the GPU (r3n_environment_lights) and add them, with "
                         "shadows; the ambient colour becomes the solid-angle mean of the sky the lights did not take, unless --ambient or "
                         "--ambient-from-skybox is given (light extraction, not image-based lighting; not in the reference)")
    ap.add_argument("--skybox-light-cone", type=float, default=6.0, metavar="DEG", help="with --lights-from-skybox: half-angle of a light's cone, in (0, 60]")
    ap.add_argument("--skybox-light-share", type=float, default=0.02, metavar="F",
                    help="with --lights-from-skybox: a cone with less than this share of the sky's energy ends the search, in [0, 1)")
    ap.add_argument("--skybox-light-scale", type=float, default=1.0, metavar="S", help="with --lights-from-skybox: scales the lights and their ambient")
    ap.add_argument("--blend-sort", choices=("host", "gpu"), default="host",
                    help="where the transparent pass's back-to-front order is sorted (not in the reference, whose CPU batcher sorts): "
                         "host = every frame on the CPU, gpu = r3n_blend_sort")
    ap.add_argument("--texture-compact", type=float, default=None, metavar="F",
                    help="with --texture-upload stream: compact the texel pool on the GPU (r3n_textures_compact) in front of a frame when "
                         "more than the fraction F in (0, 1] of it is holes; default: never")
    ap.add_argument("--texture-skip-mips", type=int, default=0, metavar="N",
                    help="with --texture-upload stream: replace every 2D texture of the file that has more than one level by its "
                         "levels from min(N, mips - 1) on, copied on the GPU (r3n_textures_from_texture), and remove the original; "
                         "default 0: keep every level")
    ap.add_argument("--texture-upload", choices=("whole", "stream"), default="whole",
                    help="how 2D textures reach the device: whole = the bindless array is re-sent when it changed, stream = single "
                         "entries are added and removed in place (r3n_textures_update), as the reference's TextureManager does")
    ap.add_argument("--mesh-upload", choices=("append", "stream"), default="append",
                    help="how mesh words reach the device: append = behind one cursor, nothing is given back; stream = pooled blocks "
                         "(r3n_mesh_blocks_add / _remove), as the reference's MeshManager sub-allocates and frees ranges")
    ap.add_argument("--mesh-compact", type=float, default=None, metavar="F",
                    help="with --mesh-upload stream: compact the mesh buffer on the GPU (r3n_mesh_compact) in front of a frame when more "
                         "than the fraction F in (0, 1] of it is holes; default: never")
    ap.add_argument("--morph-normals", choices=("base", "recompute"), default="base",
                    help="normals of morphed primitives without NORMAL: base = those of the bind shape under any weights, "
                         "recompute = recomputed from the morphed positions on the GPU (r3n_vertex_normals)")
    ap.add_argument("--build-tangents", action="store_true",
                    help="generate the tangents of primitives with TEXCOORD_0 and no TANGENT, as the reference's MeshBuilder does")
    ap.add_argument("--morph-tangents", choices=("base", "recompute"), default="base",
                    help="generated tangents of morphed primitives: base = those of the bind shape under any weights, "
                         "recompute = regenerated from the morphed positions and normals on the GPU (r3n_vertex_tangents)")
    ap.add_argument("--tonemap", choices=("blit", "reinhard", "aces"), default="blit",
                    help="tonemapping operator in front of the output transfer (r3n_tonemap_set; blit = none, as the reference)")
    ap.add_argument("--exposure", type=float, default=0.0, metavar="EV",
                    help="exposure in stops; with --auto-exposure: compensation added to the metered value")
    ap.add_argument("--auto-exposure", action="store_true",
                    help="meter the exposure on the GPU from a luminance histogram of the HDR target (the auto-exposure the reference's "
                         "tonemapping.rs:1-10 waits for)")
    ap.add_argument("--bloom", type=float, default=0.0, metavar="INTENSITY",
                    help="bloom in front of the tonemapping operator (r3n_bloom_set): the share of the blurred highlights added back; 0 = off")
    ap.add_argument("--bloom-threshold", type=float, default=1.0, metavar="T",
                    help="with --bloom: what is brighter than T after the exposure blooms (1 = display white)")
    ap.add_argument("--bloom-knee", type=float, default=0.5, metavar="K", help="with --bloom: half width of the soft knee around the threshold")
    ap.add_argument("--bloom-scatter", type=float, default=0.7, metavar="S", help="with --bloom: share of each coarser level added on the way up, in [0, 1]")
    ap.add_argument("--bloom-levels", type=int, default=8, metavar="N", help="with --bloom: most levels of the pyramid, 1..16")
    ap.add_argument("--skybox-blur", type=float, default=None, metavar="ROUGHNESS",
                    help="draw the skybox blurred: prefilter the environment on the GPU (r3n_environment_prefilter), bind the result and draw "
                         "its level ROUGHNESS * (levels - 1), ROUGHNESS in [0, 1] (not in the reference)")
    return ap


# SceneViewer::default(): camera of the default scene
DEFAULT_CAMERA = (-2.9936655, 2.189423, 5.308956, -0.08869916, 5.899576)
# examples/src/scene_viewer/mod.rs:727-751: the Bistro test's flags
BISTRO_FLAGS = ["--msaa", "4", "--normal-y-down", "--gltf-disable-directional-lights", "--directional-light", "1,-5,-1",
                "--directional-light-intensity", "15", "--camera", "-17.174278,3.715882,-4.631997,0.04430086,4.6065736"]


def settings_from(args):
    """argparse namespace (add_arguments) -> plain settings dict."""
    return dict(file=getattr(args, "scene", None) or getattr(args, "file", None), samples=args.msaa, normal_y_down=args.normal_y_down,
                directional_light=args.directional_light, directional_light_intensity=args.directional_light_intensity,
                ambient=0.1 if args.ambient is None else args.ambient, ambient_given=args.ambient is not None, scale=args.scale, shadow_distance=args.shadow_distance,
                shadow_resolution=args.shadow_resolution, enable_directional=not args.gltf_disable_directional_lights,
                camera=args.camera or DEFAULT_CAMERA, skybox=getattr(args, "skybox", None),
                skybox_extent=getattr(args, "skybox_extent", None), skybox_equirect=getattr(args, "skybox_equirect", None),
                ambient_from_skybox=getattr(args, "ambient_from_skybox", None),
                lights_from_skybox=getattr(args, "lights_from_skybox", 0), skybox_light_cone=getattr(args, "skybox_light_cone", 6.0),
                skybox_light_share=getattr(args, "skybox_light_share", 0.02), skybox_light_scale=getattr(args, "skybox_light_scale", 1.0),
                skybox_blur=getattr(args, "skybox_blur", None),
                blend_sort=getattr(args, "blend_sort", "host"), morph_normals=getattr(args, "morph_normals", "base"),
                build_tangents=getattr(args, "build_tangents", False), morph_tangents=getattr(args, "morph_tangents", "base"),
                texture_upload=getattr(args, "texture_upload", "whole"), texture_compact=getattr(args, "texture_compact", None),
                texture_skip_mips=getattr(args, "texture_skip_mips", 0),
                mesh_upload=getattr(args, "mesh_upload", "append"), mesh_compact=getattr(args, "mesh_compact", None),
                tonemap=getattr(args, "tonemap", "blit"), exposure=getattr(args, "exposure", 0.0),
                auto_exposure=getattr(args, "auto_exposure", False),
                bloom=getattr(args, "bloom", 0.0), bloom_threshold=getattr(args, "bloom_threshold", 1.0), bloom_knee=getattr(args, "bloom_knee", 0.5),
                bloom_scatter=getattr(args, "bloom_scatter", 0.7), bloom_levels=getattr(args, "bloom_levels", 8))


def default_settings(**over):
    s = settings_from(add_arguments(argparse.ArgumentParser()).parse_args([]))
    s.update(over)
    return s


def camera_view(hm, camera):
    """handle_redraw (mod.rs:640-641): view = Mat4::from_euler(XYZ, -pitch, -yaw, 0) * T(-location)."""
    x, y, z, pitch, yaw = (np.float32(v) for v in camera)
    return hm.mat4_mul(hm.from_euler_xyz(-pitch, -yaw, np.float32(0.0)), hm.translation((-x, -y, -z)))


SKYBOX_FACES = ("right", "left", "top", "bottom", "front", "back")  # cube layers +X, -X, +Y, -Y, +Z, -Z (mod.rs:38-45)


def load_skybox(directory):
    """The six face images of `directory` as uint8[6, N, N, 4] in layer order; every face square and of one size."""
    from PIL import Image
    faces = []
    for name in SKYBOX_FACES:
        path = next((os.path.join(directory, name + ext) for ext in (".jpg", ".png") if os.path.exists(os.path.join(directory, name + ext))), None)
        if path is None:
            raise FileNotFoundError(f"skybox: no {name}.jpg or {name}.png in {directory}")
        faces.append(np.ascontiguousarray(np.array(Image.open(path).convert("RGBA"), dtype=np.uint8)))
    n = faces[0].shape[0]
    if any(f.shape != (n, n, 4) for f in faces):
        raise ValueError("skybox: the six faces must be square and of one size")
    return np.stack(faces)


def load_skybox_file(path):
    """A .ktx2 / .dds cube map -> {"format", "width", "faces"} (containers.parse_ktx2_cube / parse_dds_cube), sRGB as the example's
    skybox is (Rgba8UnormSrgb)."""
    from . import containers
    with open(path, "rb") as f:
        data = f.read()
    cube = containers.parse_ktx2_cube(data, True) or containers.parse_dds_cube(data, True)
    if cube is None:
        raise ValueError(f"skybox: {path} is neither a KTX2 nor a DDS file")
    return cube


def load_panorama(path, container=False):
    """An equirectangular panorama -> (data, width, height, fmt) for Renderer.add_texture_cube_equirect: a Radiance .hdr file, or
    (container=True) the first level of a 2D .ktx2 / .dds file, linear (an HDR environment is not sRGB-encoded)."""
    from . import containers
    with open(path, "rb") as f:
        data = f.read()
    if not container:
        p = containers.parse_hdr(data)
        if p is None:
            raise ValueError(f"skybox: {path} is not a Radiance .hdr file")
        return p["rgbe"], p["width"], p["height"], "rgbe8"
    t = containers.parse_ktx2(data, False) or containers.parse_dds(data, False)
    if t is None:
        raise ValueError(f"skybox: {path} is neither a KTX2 nor a DDS file")
    return t["levels"][0], t["width"], t["height"], t["format"]


def add_skybox(r, path, extent=None, equirect=False):
    """binds the cube of --skybox PATH: a directory of six images, a cube-map file, or (a .hdr file, or equirect=True: --skybox-equirect)
    a panorama"""
    if equirect or (not os.path.isdir(path) and path.lower().endswith(".hdr")):
        if not hasattr(r, "add_texture_cube_equirect"):  # (a renderer that cannot build the cube fails here)
            raise ValueError("--skybox with a panorama: this renderer takes stored cube faces only")
        data, w, h, fmt = load_panorama(path, container=equirect)
        handle = r.add_texture_cube_equirect(data, w, h, fmt=fmt, face_extent=extent)
    elif os.path.isdir(path):
        handle = r.add_texture_cube(load_skybox(path), srgb=True)
    else:
        cube = load_skybox_file(path)
        handle = r.add_texture_cube_encoded(cube["format"], cube["width"], cube["faces"])
    r.set_background_texture(handle)
    return handle


PROJECTION = ("perspective", 60.0, 0.1)  # mod.rs:645
CLEAR = (0.0, 0.0, 0.0, 1.0)             # mod.rs:681


def build(r, hm, mk, settings):
    """setup + the first handle_redraw of the example on renderer `r` (right-handed): the flagged light, the file through
    rend3-gltf's load + instance path (rend3_amd/gltf.py), rend3-anim tables when the file has animations and the renderer
    poses on the GPU, the camera.  Returns dict(instance, animations, camera=(view, projection), ambient, clear, samples,
    objects, triangles)."""
    from . import gltf
    assert r.handedness == RIGHT, "scene_viewer is right-handed (App::HANDEDNESS, mod.rs:434)"
    if settings.get("skybox") and settings.get("skybox_equirect"):
        raise ValueError("--skybox and --skybox-equirect: one background")
    sky = None
    if settings.get("skybox"):  # load_skybox (mod.rs:34-57); a renderer without cube textures fails here, it does not skip the sky
        sky = add_skybox(r, settings["skybox"], extent=settings.get("skybox_extent"))
    elif settings.get("skybox_equirect"):
        sky = add_skybox(r, settings["skybox_equirect"], extent=settings.get("skybox_extent"), equirect=True)
    if settings.get("ambient_from_skybox") is not None and (sky is None or not hasattr(r, "environment_mean")):
        raise ValueError("--ambient-from-skybox needs a skybox on a renderer that can read its mean")
    blur = settings.get("skybox_blur")
    if blur is not None:
        if sky is None or not hasattr(r, "prefilter_environment"):
            raise ValueError("--skybox-blur needs a skybox on a renderer that can prefilter it")
        if not 0.0 <= float(blur) <= 1.0:
            raise ValueError("--skybox-blur: a roughness in [0, 1]")
    n_sky_lights = int(settings.get("lights_from_skybox", 0) or 0)
    if n_sky_lights:
        if not 1 <= n_sky_lights <= 16:
            raise ValueError("--lights-from-skybox: 1 .. 16 lights")
        if sky is None or not hasattr(r, "add_environment_lights"):
            raise ValueError("--lights-from-skybox needs a skybox on a renderer that can read lights out of it")
    if settings.get("tonemap", "blit") != "blit" or settings.get("exposure", 0.0) != 0.0 or settings.get("auto_exposure"):
        if not hasattr(r, "set_tonemapping"):  # (a renderer that only has the reference's blit fails here)
            raise ValueError("--tonemap / --exposure / --auto-exposure: this renderer has the blit alone")
        from .renderer import AutoExposure
        r.set_tonemapping(settings.get("tonemap", "blit"), exposure_ev=settings.get("exposure", 0.0),
                          auto_exposure=AutoExposure() if settings.get("auto_exposure") else None)
    if settings.get("bloom", 0.0) != 0.0:
        if not hasattr(r, "set_bloom"):  # (a renderer that only has the reference's blit fails here)
            raise ValueError("--bloom: this renderer has the blit alone")
        r.set_bloom(settings["bloom"], threshold=settings.get("bloom_threshold", 1.0), knee=settings.get("bloom_knee", 0.5),
                    scatter=settings.get("bloom_scatter", 0.7), max_levels=settings.get("bloom_levels", 8))
    if settings.get("blend_sort", "host") != "host":  # (a renderer that cannot sort on the device fails here)
        if not hasattr(r, "blend_sort"):
            raise ValueError("--blend-sort gpu: this renderer has no device sort")
        r.blend_sort = settings["blend_sort"]
    if settings.get("texture_upload", "whole") != "whole":  # (a renderer that cannot stream textures fails here)
        if not hasattr(r, "texture_upload"):
            raise ValueError("--texture-upload stream: this renderer re-sends the whole array")
        r.texture_upload = settings["texture_upload"]
    if settings.get("texture_compact") is not None:
        if settings.get("texture_upload", "whole") != "stream":
            raise ValueError("--texture-compact needs --texture-upload stream: the whole-array path lays its pool out densely")
        r.texture_compact = settings["texture_compact"]
    if settings.get("texture_skip_mips", 0):
        if settings["texture_skip_mips"] < 0:
            raise ValueError("--texture-skip-mips: a level count >= 0")
        if settings.get("texture_upload", "whole") != "stream":
            raise ValueError("--texture-skip-mips needs --texture-upload stream: the whole-array path keeps no resident pool to copy from")
    if settings.get("mesh_upload", "append") != "append":  # (a renderer without pooled mesh blocks fails here)
        if not hasattr(r, "mesh_upload"):
            raise ValueError("--mesh-upload stream: this renderer appends behind one cursor")
        r.mesh_upload = settings["mesh_upload"]
    if settings.get("mesh_compact") is not None:
        if settings.get("mesh_upload", "append") != "stream":
            raise ValueError("--mesh-compact needs --mesh-upload stream: the append path lays its buffer out densely")
        r.mesh_compact = settings["mesh_compact"]
    light = None
    if settings["directional_light"] is not None:  # setup (mod.rs:463-472)
        light = r.add_directional_light(color=(1.0, 1.0, 1.0), intensity=settings["directional_light_intensity"],
                                        direction=settings["directional_light"], distance=settings["shadow_distance"], resolution=2048)
    g = gltf.Gltf(settings["file"])
    # (passed only when asked for: a renderer whose add_mesh cannot recompute fails there, it does not fall back to base normals)
    recompute = dict(morph_normals="recompute") if settings.get("morph_normals", "base") == "recompute" else {}
    if settings.get("build_tangents", False):
        recompute["build_tangents"] = True
    if settings.get("morph_tangents", "base") == "recompute":
        recompute["morph_tangents"] = "recompute"
    if settings.get("texture_skip_mips", 0):
        recompute["texture_skip_mips"] = settings["texture_skip_mips"]
    inst = gltf.instance_scene(g, r, hm, mk, scale=settings["scale"], enable_directional=settings["enable_directional"],
                               directional_light_shadow_distance=settings["shadow_distance"],
                               directional_light_resolution=settings["shadow_resolution"], normal_y_down=settings["normal_y_down"],
                               **recompute)
    view = camera_view(hm, settings["camera"])
    r.set_camera_data(view, PROJECTION)
    a = settings["ambient"]
    ambient = (a, a, a, 1.0)
    if n_sky_lights:  # (behind the file's and the flagged lights: the call refuses more than 16 in all)
        _ids, rest = r.add_environment_lights(sky, max_lights=n_sky_lights, cone_degrees=settings.get("skybox_light_cone", 6.0),
                                              min_share=settings.get("skybox_light_share", 0.02), scale=settings.get("skybox_light_scale", 1.0),
                                              distance=settings["shadow_distance"], resolution=settings["shadow_resolution"])
        if not settings.get("ambient_given") and settings.get("ambient_from_skybox") is None:
            ambient = tuple(float(v) for v in rest[:3]) + (1.0,)
    if settings.get("ambient_from_skybox") is not None:
        mean = r.environment_mean(sky)
        ambient = tuple(float(settings["ambient_from_skybox"]) * float(v) for v in mean[:3]) + (1.0,)
    if blur is not None:  # last: the derived cube lives until the cube array is next re-sent
        blurred, _sh = r.prefilter_environment(sky)
        r.set_background_texture(blurred)
        r.set_skybox_level(float(blur) * (r.cubes[blurred].mips - 1))
    meshes = r.meshes
    tris = int(sum(meshes[m["mesh"]].index_count // 3 for m in r.object_meta.values() if m["enabled"]))
    return dict(instance=inst, gltf=g, light=light, camera=(view, PROJECTION), ambient=ambient, clear=CLEAR,
                samples=settings["samples"], objects=len(inst["objects"]), triangles=tris, file=os.path.basename(settings["file"]))
