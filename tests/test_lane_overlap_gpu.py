"""GPU: the shadow lanes run from frame to frame without joining the main stream (r3n.hip close_frame), the work-queue counters
and the resolve's triangle records exist once per frame slot, and the resolve's prepass runs on the main stream beside the
previous frame's resolve.

None of that may change a result.  Every case renders the same sequence of frames twice -- on a context with the default streams
(frames in flight, lanes running on) and on one created under R3N_PIPELINE=0 R3N_SINGLE_STREAM=1, where every kernel of every frame
runs in order on one stream -- with a moving camera and NO read-back for at least eight consecutive frames (a read-back joins every
stream, which is exactly what must not be needed), then reads back an odd frame and, after eight more, an even one: both frame
slots (slot = frame number & 1).  The two contexts run the same kernels on the same inputs, so everything is compared bit for bit:
visible objects, triangle sets, draw calls, the baked matrices of the visible slots, visibility keys, shadow atlas, HDR, both
tonemapped images, and the work items every r3n_forward queued (r3n_readback_raster_stats: it follows the frame slot).

Shapes: a 96 x 64 target, two or three 128^2 shadow views, 36 objects and a ground quad -- the ground and the nearer boxes draw
triangles far larger than 8 px in the target and in the shadow views, so the per-triangle pass AND the work-item rasteriser run on
the main stream and on both lanes (asserted from the queued work items).
"""
import math

import numpy as np
import pytest

import scenes
from oracle import host as oh

pytestmark = pytest.mark.gpu
f32 = np.float32
AMBIENT, CLEAR = (0.1, 0.1, 0.1, 1.0), (0.02, 0.03, 0.05, 1.0)
W, H, SHADOW = 96, 64, 128
BIGQ = 32  # layouts.h R3N_BIGQ
READ = (7, 16)  # an odd frame after eight frames without a read-back, an even one after nine more
HOOKS = ("R3N_PIPELINE", "R3N_SINGLE_STREAM", "R3N_FRAME_NODES", "R3N_ALWAYS_FORK", "R3N_BIG_CAPACITY")
SERIAL = {"R3N_PIPELINE": "0", "R3N_SINGLE_STREAM": "1"}


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def create(r3, monkeypatch, env, **kw):
    """A renderer created under `env` alone (r3n_create and Renderer.__init__ read the switches once)."""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    r = r3.Renderer(oh.LEFT, f32(W) / f32(H), **kw)
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    return r


def build(r, mk, lights=2):
    """36 random objects (a quarter of the materials cutout), a ground quad under them, `lights` shadow-casting lights."""
    st = {"objects": scenes.build_random_scene(r, oh, mk, 36, 0x1A9E, extent=(9.0, 3.0, 9.0), lights=lights, shadow_res=SHADOW,
                                               shadow_distance=30.0, with_cutout=True)}
    st["ground"] = r.add_object(scenes.plane_mesh(r), scenes.lit(r, mk, (0.4, 0.5, 0.3, 1.0)),
                                oh.mat4_mul(oh.translation((0.0, -3.5, 0.0)), oh.mat4_mul(oh.rotation_x(-math.pi / 2), oh.scale((14.0, 14.0, 14.0)))))
    st["cube"] = scenes.cube_mesh(r)
    st["mat"] = scenes.lit(r, mk, (0.8, 0.3, 0.2, 1.0))
    return st


def camera(r, f):
    r.set_camera_data(oh.look_at_lh((-11.0 + 0.7 * f, 3.0 + 0.2 * f, -12.0 + 0.5 * f), (0.0, -1.0, 0.0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def run(r, mk, step=None, lights=2):
    """The case's frames on `r`: {frame: (read-back, work items per r3n_forward call)} for the frames of READ."""
    st = build(r, mk, lights)
    out = {}
    for f in range(READ[-1] + 1):
        camera(r, f)
        size = step(r, mk, st, f) if step else None
        w, h = size or (W, H)
        got = r.render(w, h, ambient=AMBIENT, clear_color=CLEAR, readback=f in READ)
        if f in READ:
            out[f] = (got, r.raster_stats())
    r.sync()
    return out


def same_sets(a, b, tag):
    assert np.array_equal(a["visible"], b["visible"]), tag + " visible objects"
    assert np.array_equal(a["pass"], b["pass"]), tag + " pass set"
    assert np.array_equal(a["residual"], b["residual"]), tag + " residual set"
    assert np.array_equal(a["draw_calls"], b["draw_calls"]), tag + " draw calls"
    seen = a["visible"].astype(bool)  # (r3n_render_frame bakes the slots that pass the frustum test, not the whole buffer)
    assert np.array_equal(a["baked"].view(np.uint32)[seen], b["baked"].view(np.uint32)[seen]), tag + " baked matrices"


def same_frames(a, b, tag):
    """Bit for bit: sets, keys, atlas, HDR and the tonemapped images of two product frames."""
    assert a["capacity"] == b["capacity"], tag
    same_sets(a, b, tag)
    assert len(a["shadows"]) == len(b["shadows"]), tag + " shadow views"
    for k, (sa, sb) in enumerate(zip(a["shadows"], b["shadows"])):
        same_sets(sa, sb, tag + f" shadow view {k}")
    assert np.array_equal(a["vis"], b["vis"]), tag + f" visibility keys ({(a['vis'] != b['vis']).sum()} differ)"
    assert a["atlas_size"] == b["atlas_size"], tag
    assert np.array_equal(a["atlas"].view(np.uint32), b["atlas"].view(np.uint32)), tag + " shadow atlas"
    assert np.array_equal(a["hdr16"], b["hdr16"]), tag + f" HDR ({(a['hdr16'] != b['hdr16']).any(axis=2).sum()} px differ)"
    assert np.array_equal(a["rgba_f32"].view(np.uint32), b["rgba_f32"].view(np.uint32)), tag + " float image"
    assert np.array_equal(a["rgba8"], b["rgba8"]), tag + " 8-bit image"


def check(r3, monkeypatch, tag, step=None, lights=2, env=None, serial_env=None, views=None, **kw):
    env = env or {}
    p = create(r3, monkeypatch, env, **kw)
    q = create(r3, monkeypatch, {**(serial_env if serial_env is not None else env), **SERIAL}, **kw)
    try:
        got, ref = run(p, r3.material_record, step, lights), run(q, r3.material_record, step, lights)
    finally:
        p.close()
        q.close()
    assert sorted(got) == sorted(ref) == list(READ)
    for f in READ:
        (fa, sa), (fb, sb) = got[f], ref[f]
        same_frames(fa, fb, f"{tag} frame {f} (slot {f & 1})")
        # (on one stream every camera's calls count in the viewport's queue: the same numbers, in other places)
        assert sorted(sa[sa > 0].tolist()) == sorted(sb[sb > 0].tolist()), f"{tag} frame {f}: work items per call {sa.tolist()} != {sb.tolist()}"
        assert fa["vis"].any() and (fa["atlas"] != 0).any() and fa["rgba8"][..., :3].max() > 30, f"{tag} frame {f}: nothing drawn"
        n_views = len(fa["shadows"])
        assert n_views == (views[f] if views else lights), f"{tag} frame {f}: {n_views} shadow views"
        # the work-item rasteriser ran on the main stream and on every lane that drew a view ([0, 16): the viewport's calls, 12 per lane)
        assert sa[:16].max() > 0, f"{tag} frame {f}: no viewport work items {sa.tolist()}"
        for lane in range(min(n_views, 2)):
            assert sa[16 + 12 * lane:28 + 12 * lane].max() > 0, f"{tag} frame {f}: no work items on lane {lane} {sa.tolist()}"
    return got


# ------------------------------------------------------------------ a. steady motion
@pytest.mark.parametrize("lights", [2, 3])
def test_steady_motion(r3, monkeypatch, lights):
    """Two views: one per lane.  Three: lane 1 draws two views in series, as the bench scene's lanes do."""
    check(r3, monkeypatch, f"steady, {lights} views", lights=lights)


# ------------------------------------------------------------------ b. world edits between frames
def test_object_added_and_removed_between_frames(r3, monkeypatch):
    """r3n_objects_write (main stream) rewrites records, spheres and meta words the lanes' kernels of the previous frame read, and
    marks tri_base for its rebuild: both must come behind the lanes that r3n_frame_end no longer joins."""
    def step(r, mk, st, f):
        if f in (3, 10):
            st["extra"] = r.add_object(st["cube"], st["mat"], oh.mat4_mul(oh.translation((1.0 + 0.1 * f, 0.5, -2.0)), oh.scale((1.5, 1.5, 1.5))))
        if f in (5, 12):
            r.remove_object(st["objects"][f])
        if f in (6, 14):
            r.remove_object(st.pop("extra"))
        if f in (4, 9, 15):
            r.set_object_transform(st["objects"][20], oh.mat4_mul(oh.translation((0.5 * f - 4.0, 1.0, 1.0)), oh.scale((2.0, 2.0, 2.0))))
    check(r3, monkeypatch, "objects added / removed", step)


# ------------------------------------------------------------------ c. resolution change
def test_resolution_change(r3, monkeypatch):
    """Smaller (the targets keep their allocation), larger (every target of the slot is reallocated behind a full wait), and odd."""
    def step(r, mk, st, f):
        return (W, H) if f < 4 else (64, 40) if f < 10 else (117, 75) if f < 14 else (W, H)
    check(r3, monkeypatch, "resolution change", step)


# ------------------------------------------------------------------ d. a lane unused for a frame
def test_shadow_views_two_one_two(r3, monkeypatch):
    """The second light leaves for frames 4, 5 and 11 .. 13: its lane draws nothing then, and the resolve must neither wait for
    it for ever nor miss it when it is back."""
    def step(r, mk, st, f):
        if f in (4, 11):
            st["light"] = r.dir_lights.pop()
            r._lights_version += 1
        if f in (6, 14):
            r.dir_lights.append(st.pop("light"))
            r._lights_version += 1
    views = {f: 2 for f in READ}
    check(r3, monkeypatch, "views 2 -> 1 -> 2", step, views=views)
    # and read where only one view is drawn: the same case with the light away over both read-back frames' predecessors
    def step1(r, mk, st, f):
        if f in (6, 15):
            st["light"] = r.dir_lights.pop()
            r._lights_version += 1
        if f in (8,):
            r.dir_lights.append(st.pop("light"))
            r._lights_version += 1
    check(r3, monkeypatch, "views 2 -> 1 -> 2 -> 1", step1, views={7: 1, 16: 1})


# ------------------------------------------------------------------ e. the resolve alternates between the shade and the main stream
def test_blend_object_every_third_frame(r3, monkeypatch):
    """A translucent object exists in every third frame: that frame's resolve stays on the main stream (the transparent pass follows
    it there) and the frame is joined at its end; the frames between go to the shade stream and leave the lanes running."""
    def step(r, mk, st, f):
        if "blend_mat" not in st:
            st["blend_mat"] = r.add_material(mk(albedo=(0.9, 0.8, 0.2, 0.5), albedo_mode="value", roughness=0.5), scenes.BLEND)
        if f % 3 == 0:
            st["blend"] = r.add_object(st["cube"], st["blend_mat"], oh.mat4_mul(oh.translation((-2.0 + 0.2 * f, 0.0, -3.0)), oh.scale((2.0, 2.0, 0.2))))
        elif f % 3 == 1:
            r.remove_object(st.pop("blend"))
    check(r3, monkeypatch, "blend every third frame", step)


def test_leaving_and_reentering_the_pipelined_mode(r3, monkeypatch):
    """Stage timing on for frames 3 .. 5 (the resolve stays on the main stream under the taps) and one stream for frames 10 .. 12:
    the triangle records exist once per frame slot only while frames are pipelined, and the frames around each switch must read
    the set their own prepass wrote."""
    def step(r, mk, st, f):
        if f in (3, 6):
            r.timing_enable(f == 3)
        if f in (10, 13):
            r.set_multi_stream(f == 13)
    check(r3, monkeypatch, "timing taps / one stream for a few frames", step, serial_env={})


# ------------------------------------------------------------------ f. the work queues at their smallest
@pytest.mark.parametrize("how", ["config_floor", "create_hook"])
def test_smallest_work_queues(r3, monkeypatch, how):
    """r3n_config.max_big_items = 1 is raised to the ABI's floor (1 024 entries per sub-queue): the smallest queue a caller can ask
    for.  No sub-queue of these shapes fills at that size (a 128^2 view is 16 work items per triangle), so the case runs again at
    one entry per sub-queue (R3N_BIG_CAPACITY, r3n_create's hook): every call queues more than 32 x 1 items there, on the main
    stream and on both lanes, so the producers' queue-full path runs in consecutive frames on counters of alternating slots."""
    if how == "config_floor":
        check(r3, monkeypatch, "queues at the floor", max_big_items=1)
        return
    got = check(r3, monkeypatch, "queues of one entry", env={"R3N_BIG_CAPACITY": "1"})
    for f in READ:
        stats = got[f][1]
        assert stats[:16].max() > BIGQ and stats[16:28].max() > BIGQ and stats[28:40].max() > BIGQ, f"frame {f}: no queue overflowed {stats.tolist()}"


# ------------------------------------------------------------------ g. the per-node API; unconditional forks
@pytest.mark.parametrize("env", [{"R3N_FRAME_NODES": "1"}, {"R3N_ALWAYS_FORK": "1"}, {"R3N_FRAME_NODES": "1", "R3N_ALWAYS_FORK": "1"}],
                         ids=["frame_nodes", "always_fork", "both"])
def test_per_node_api_and_always_fork(r3, monkeypatch, env):
    """R3N_FRAME_NODES=1: one C call per node, headers uploaded at each r3n_uniform_bake (main stream, into the frame slot's block).
    R3N_ALWAYS_FORK=1: the lanes wait for the main stream at every fork -- a producer that forgot to bump main_epoch would show as a
    difference between this run and the steady one.  The serial context keeps R3N_FRAME_NODES (the per-node path bakes every slot)."""
    check(r3, monkeypatch, "+".join(sorted(env)), env=env, serial_env={k: v for k, v in env.items() if k == "R3N_FRAME_NODES"})
