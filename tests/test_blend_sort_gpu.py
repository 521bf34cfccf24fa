"""GPU: the transparent pass's draw order sorted on the device (r3n_blend_objects_write / r3n_blend_sort, rend3_amd/csrc/
blend_sort.hip) against the host order it replaces (host.blend_draw_order + the scan r3n_blend_order_write builds).

1. order and scan, exactly, through the raw ABI: both paths of the sort, sizes around the wave, the workgroup and the limit between
   the paths, ties, zero and infinite distances, a second camera without a second upload;
2. the mode rule and the argument errors;
3. the frames of test_transparent_pass_multi_frame with blend_sort="gpu": bit-identical to the oracle, and the blend set goes up
   only when the world changed;
4. a frame without a world edit makes one r3n_blend_sort call and no r3n_blend_order_write.
"""
import ctypes

import numpy as np
import pytest

import scenes
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from test_gpu_parity import compare_frames

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG = -1
SMALL = 4096  # blend_sort.h R3N_BLEND_SORT_SMALL: the largest set the one-workgroup path takes
N_MAX = 70_000  # more than one tile of the radix path, more than 16 bits of payload
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, SMALL, SMALL + 1, N_MAX]
CAMERAS = [(3.0, -2.0, 5.0), (4.0, -2.0, 5.0)]


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def lattice_locations(n):
    """Locations on the lattice CAMERAS[0] + k * 2^-10, k an integer vector, symmetric about that camera: object 2 j + 1 is the
    mirror image of object 2 j, so the two are at exactly the same distance (every prefix of even length ties completely); the
    first quarter of the pairs has whole-number k / 1024 in [-3, 3]^3, where many more share a distance.  The fine lattice gives
    distances with full mantissas: all four digit passes of the radix sort see varied digits.  Objects 4, 5: at the camera;
    6, 7: infinitely far.  Every sum is exact in f32."""
    rng = np.random.default_rng(0x50B7)
    pairs = (n + 1) // 2
    k = rng.integers(-20 * 1024, 20 * 1024 + 1, (pairs, 3))
    coarse = max(pairs // 4, min(pairs, 2))
    k[:coarse] = rng.integers(-3, 4, (coarse, 3)) * 1024
    off = (k.astype(np.float64) / 1024.0)
    loc = np.empty((2 * pairs, 3), dtype=np.float64)
    loc[0::2] = np.asarray(CAMERAS[0]) + off
    loc[1::2] = np.asarray(CAMERAS[0]) - off
    loc = loc[:n]
    assert np.array_equal(loc.astype(f32).astype(np.float64), loc), "the lattice is exact in f32"
    loc = loc.astype(f32)
    if n >= 8:
        loc[4] = loc[5] = CAMERAS[0]
        loc[6] = (3e20, 0.0, 0.0)
        loc[7] = (0.0, -3e20, 1e30)
    return loc


class World:
    """one context with N_MAX objects of 1..12 triangles at every third slot of a larger object buffer; a test uses a prefix"""

    def __init__(self, r3):
        from rend3_amd import _ffi
        self.ffi, self.host = _ffi, r3.host
        self.lib = _ffi.lib()
        self.ctx = self.lib.r3n_create(0, None)
        assert self.ctx
        self.capacity = 3 * N_MAX + 5
        self.slots = (3 * np.arange(N_MAX) + 1).astype(np.uint32)
        self.tris = (1 + (np.arange(N_MAX) * 7) % 12).astype(np.uint32)
        rec = np.zeros((N_MAX, 32), dtype=np.uint32)
        rec.view(f32)[:, [0, 5, 10, 15]] = 1.0
        rec[:, 21] = 3 * self.tris  # index_count (the order and the scan read nothing else of a mesh)
        rec[:, 29] = 1
        indices = np.arange(36, dtype=np.uint32) % 3
        assert self.lib.r3n_mesh_buffer_write(self.ctx, 0, _ffi.ptr(indices), indices.nbytes) == 0
        assert self.lib.r3n_objects_write(self.ctx, _ffi.ptr(self.slots), _ffi.ptr(rec), N_MAX, self.capacity) == 0
        self._ref = {}

    def close(self):
        self.lib.r3n_destroy(self.ctx)

    def set(self, n):
        """uploads the first n objects as the blend set"""
        slots, loc = np.ascontiguousarray(self.slots[:n]), np.ascontiguousarray(lattice_locations(n))
        return self.lib.r3n_blend_objects_write(self.ctx, self.ffi.ptr(slots) if n else None, self.ffi.ptr(loc) if n else None, n), loc

    def sort(self, camera):
        cam = np.asarray(camera, dtype=f32)
        return self.lib.r3n_blend_sort(self.ctx, self.ffi.ptr(cam))

    def readback(self, n):
        order, rank = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32), np.full(n + 1, 0xDEADBEEF, dtype=np.uint32)
        assert self.lib.r3n_readback_blend_order(self.ctx, self.ffi.ptr(order), self.ffi.ptr(rank), n) == 0
        return order[:n], rank

    def reference(self, n, camera, loc):
        """host.blend_draw_order of the first n objects and the scan r3n_blend_order_write builds of it; computed once per case"""
        key = (n, camera)
        if key not in self._ref:
            with np.errstate(over="ignore"):
                order = np.asarray(self.host.blend_draw_order(camera, self.slots[:n], loc), dtype=np.uint32)
            tris = self.tris[(order - 1) // 3] if n else np.zeros(0, dtype=np.uint32)
            self._ref[key] = (order, np.concatenate([[0], np.cumsum(tris)]).astype(np.uint32))
        return self._ref[key]


@pytest.fixture(scope="module")
def world(r3):
    w = World(r3)
    yield w
    w.close()


# ------------------------------------------------------------------ 1. order and scan are exact
@pytest.mark.parametrize("n", SIZES)
def test_order_and_scan_equal_the_host_order(world, n):
    code, loc = world.set(n)
    assert code == 0
    if n >= 2:  # a property of the input: at least a quarter of the objects share their distance with another one
        with np.errstate(over="ignore"):
            keys = np.array([int(world.host.blend_sort_key(CAMERAS[0], l)) for l in loc[:min(n, 5000)]])
        _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
        assert (counts[inverse] > 1).sum() * 4 >= len(keys)
    if n >= 8:
        assert keys[4] == keys[5] == 0x7FFFFFFF and keys[6] == keys[7] == 0x007FFFFF, "at the camera / infinitely far"
    for camera in CAMERAS:  # the second one without another upload
        assert world.sort(camera) == 0
        order, rank = world.readback(n)
        want_order, want_rank = world.reference(n, camera, loc)
        print(f"n {n} camera {camera}: order differs at {(order != want_order).sum()} of {n}, scan at {(rank != want_rank).sum()}")
        assert np.array_equal(order, want_order), f"n {n} camera {camera}: order"
        assert np.array_equal(rank, want_rank), f"n {n} camera {camera}: rank scan"


# ------------------------------------------------------------------ 2. mode switching and errors
def test_argument_errors(world):
    ffi, lib = world.ffi, world.lib
    n = 10
    assert world.set(n)[0] == 0 and world.sort(CAMERAS[0]) == 0
    before = world.readback(n)
    loc = np.zeros((4, 3), dtype=f32)
    for bad in ([1, 7, 4, 10], [1, 4, 4, 7], [7, 4, 1, 0]):  # not ascending, twice the same, descending
        slots = np.asarray(bad, dtype=np.uint32)
        assert lib.r3n_blend_objects_write(world.ctx, ffi.ptr(slots), ffi.ptr(loc), 4) == ERR_INVALID_ARG
    slots = np.asarray([1, 4, 7, world.capacity], dtype=np.uint32)
    assert lib.r3n_blend_objects_write(world.ctx, ffi.ptr(slots), ffi.ptr(loc), 4) == ERR_INVALID_ARG
    assert lib.r3n_blend_objects_write(world.ctx, None, None, 4) == ERR_INVALID_ARG
    # a refused call changes nothing
    assert world.sort(CAMERAS[0]) == 0
    after = world.readback(n)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # a read-back into too small a buffer
    order, rank = np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    assert lib.r3n_readback_blend_order(world.ctx, ffi.ptr(order), ffi.ptr(rank), n - 1) == ERR_INVALID_ARG


def test_sort_without_a_set_is_a_no_op(r3):
    from rend3_amd import _ffi
    lib = _ffi.lib()
    ctx = lib.r3n_create(0, None)
    cam = np.asarray(CAMERAS[0], dtype=f32)
    assert lib.r3n_blend_sort(ctx, _ffi.ptr(cam)) == 0
    order, rank = np.zeros(1, dtype=np.uint32), np.ones(1, dtype=np.uint32)
    assert lib.r3n_readback_blend_order(ctx, _ffi.ptr(order), _ffi.ptr(rank), 0) == 0 and rank[0] == 0
    assert lib.r3n_sync(ctx) == 0
    lib.r3n_destroy(ctx)


def test_the_last_upload_decides_the_mode(world):
    ffi, lib = world.ffi, world.lib
    n = 300
    code, loc = world.set(n)
    assert code == 0 and world.sort(CAMERAS[0]) == 0
    sorted_order, sorted_rank = world.reference(n, CAMERAS[0], loc)
    assert np.array_equal(world.readback(n)[0], sorted_order)
    # host order mode: some other order of fewer objects; r3n_blend_sort then leaves it alone
    given = np.ascontiguousarray(world.slots[:200][::-1])
    assert lib.r3n_blend_order_write(world.ctx, ffi.ptr(given), 200) == 0
    assert world.sort(CAMERAS[1]) == 0
    order, rank = world.readback(200)
    assert np.array_equal(order, given)
    assert np.array_equal(rank, np.concatenate([[0], np.cumsum(world.tris[:200][::-1])]))
    # and back
    assert world.set(n)[0] == 0 and world.sort(CAMERAS[0]) == 0
    order, rank = world.readback(n)
    assert np.array_equal(order, sorted_order) and np.array_equal(rank, sorted_rank)


def layer_world(r, mk, n):
    """n translucent triangles, each far larger than the view, 1 + 0.25 k units in front of a camera at the origin looking down +z"""
    m = r.add_mesh([(-40.0, -40.0, 0.0), (0.0, 40.0, 0.0), (40.0, -40.0, 0.0)], [0, 1, 2], normals=[(0.0, 0.0, -1.0)] * 3)
    for k in range(n):
        mat = r.add_material(mk(albedo=(0.9 - 0.2 * k, 0.2 + 0.3 * k, 0.5, 0.5), albedo_mode="value", roughness=0.5, unlit=True), scenes.BLEND)
        r.add_object(m, mat, oh.translation((0.0, 0.0, 1.0 + 0.25 * k)))
    r.set_camera_data(oh.look_at_lh((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def test_an_emptied_set_draws_no_translucent_triangle(r3):
    clear = (0.02, 0.03, 0.05, 1.0)
    empty = r3.Renderer(oh.LEFT, f32(1.0))
    layer_world(empty, r3.material_record, 0)
    bare = empty.render(64, 64, clear_color=clear)["hdr16"]
    empty.close()
    p = r3.Renderer(oh.LEFT, f32(1.0), blend_sort="gpu")
    layer_world(p, r3.material_record, 3)
    drawn = p.render(64, 64, clear_color=clear)["hdr16"]
    assert (drawn != bare).any(axis=-1).all(), "every pixel is covered by the translucent layers"
    assert p.lib.r3n_blend_objects_write(p.ctx, None, None, 0) == 0  # behind the mirror's back: it will not send the set again
    gone = p.render(64, 64, clear_color=clear)["hdr16"]
    assert np.array_equal(gone, bare)
    # host order mode for the same world brings them back, and the device order after it draws the same image
    p.blend_sort = "host"
    assert np.array_equal(p.render(64, 64, clear_color=clear)["hdr16"], drawn)
    p.blend_sort = "gpu"
    assert np.array_equal(p.render(64, 64, clear_color=clear)["hdr16"], drawn)
    p.close()


# ------------------------------------------------------------------ 3. frame parity, 4. no host dependence
class CountingLib:
    """the binding with every call counted, and the blend sets that went through it kept"""

    def __init__(self, lib):
        self._lib, self.calls, self.sets = lib, {}, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            if name == "r3n_blend_objects_write":
                n = args[3]
                grab = lambda p, dt, count: np.frombuffer(ctypes.string_at(p.value, 4 * count), dtype=dt).copy() if count else np.zeros(0, dt)  # noqa: E731
                self.sets.append((grab(args[1], np.uint32, n), grab(args[2], np.uint32, 3 * n).reshape(-1, 3)))
            return fn(*args)
        return call


@pytest.mark.parametrize("handedness,samples,textured", [(oh.LEFT, 1, False), (oh.RIGHT, 1, True), (oh.LEFT, 4, True)])
def test_transparent_pass_multi_frame_sorted_on_the_device(r3, handedness, samples, textured):
    """the scene, cameras and edit of test_gpu_parity.test_transparent_pass_multi_frame; the product sorts on the device"""
    aspect = f32(320) / f32(192)
    o, p = OracleRenderer(handedness, aspect), r3.Renderer(handedness, aspect, blend_sort="gpu")
    p.lib = spy = CountingLib(p.lib)
    for r, mk in ((o, omk), (p, r3.material_record)):
        scenes.build_random_scene(r, oh, mk, 120, 0xC0FFEE, handedness=handedness, lights=2, with_cutout=True)
    ho = scenes.add_blend_objects(o, oh, omk, 0xB1E2D, textured=textured)
    hp = scenes.add_blend_objects(p, oh, r3.material_record, 0xB1E2D, textured=textured)
    look = oh.look_at_lh if handedness == oh.LEFT else oh.look_at_rh
    zs = 1.0 if handedness == oh.LEFT else -1.0
    uploads = []
    for f in range(4):
        eye = (-2.0 + 1.5 * f, 1.0 + 0.3 * f, zs * (-3.0 + 0.5 * f))
        for r in (o, p):
            r.set_camera_data(look(eye, (0.5 * f, 0.5, zs * 8.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        if f == 2:
            for r, hs in ((o, ho), (p, hp)):
                r.set_object_transform(hs[1], oh.mat4_mul(oh.translation((0.5, 1.0, zs * 5.0)), oh.scale((2.0, 2.0, 0.2))))
        fo = o.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        fp = p.render(320, 192, samples=samples, ambient=(0.1, 0.1, 0.1, 1.0), clear_color=(0.02, 0.03, 0.05, 1.0))
        assert len(fo["blend_list"][0]) > 0
        compare_frames(fo, fp, f"transparent frame {f}, device order")
        uploads.append(len(spy.sets))
        # the order the pass read is the host's
        order, _rank = p.readback_blend_order()
        blend = sorted(hp)
        assert list(order) == r3.host.blend_draw_order(p.camera.location, blend, [p.object_meta[h]["location"] for h in blend])
    assert uploads == [1, 1, 2, 2], "the set goes up with the world and again when a blend object moved, never with the camera"
    (slots0, loc0), (slots2, loc2) = spy.sets
    assert np.array_equal(slots0, slots2) and list(slots0) == sorted(hp)
    moved = np.flatnonzero((loc0 != loc2).any(axis=1))
    assert list(slots2[moved]) == [hp[1]], "frame 2 re-sent one changed location: the moved object's"
    assert spy.calls["r3n_blend_sort"] == 4 and "r3n_blend_order_write" not in spy.calls
    assert p.stage_times()["blend_sort"][1] == 4
    p.close()


def test_a_frame_without_a_world_edit_only_sorts(r3):
    p = r3.Renderer(oh.LEFT, f32(1.0), blend_sort="gpu")
    layer_world(p, r3.material_record, 3)
    p.render(64, 64, readback=False)  # the world goes up
    p.lib = spy = CountingLib(p.lib)
    for eye in ((0.0, 0.0, 0.0), (0.5, 0.25, -1.0)):
        p.set_camera_data(oh.look_at_lh(eye, (0.0, 0.0, 1.0), (0, 1, 0)), ("perspective", 60.0, 0.1))
        before = dict(spy.calls)
        p.render(64, 64, readback=False)
        made = {k: v - before.get(k, 0) for k, v in spy.calls.items() if v != before.get(k, 0)}
        assert made.get("r3n_blend_sort") == 1, made
        assert "r3n_blend_order_write" not in made and "r3n_blend_objects_write" not in made and "r3n_objects_write" not in made, made
    p.close()
