"""CPU: the key the device sort of the transparent pass orders by (host.blend_sort_key, the mirror of blend_sort.hip's
blend_sort_key) against the order it replaces (host.blend_draw_order): sorting by (key, slot) IS that order, also where the
distance is zero, subnormal, infinite or shared by several objects."""
import numpy as np

from rend3_amd import _ffi, host

f32 = np.float32

# camera and the crafted locations around it (every sum below is exact in f32, so the distances are what the names say)
CAMERA = (3.0, -2.0, 5.0)
CRAFTED = [
    (3.0, -2.0, 5.0),                       # at the camera: dist = +0.0, key = -0.0
    (3.0, -2.0, 5.0),                       # ... twice
    (3.0 + 2.0 ** -20, -2.0, 5.0),          # dist = 2^-40
    (3e20, 0.0, 0.0),                       # dist overflows to +inf
    (0.0, -3e20, 1e30),                     # ... and ties with the other +inf
    (4.0, 0.0, 8.0), (2.0, -4.0, 2.0),      # mirrored about the camera: exactly equal distances (14)
    (1.0, -4.0, 4.0), (5.0, 0.0, 6.0), (2.0, 0.0, 3.0),  # the same distance (9) by three routes: d = (2,2,1), (-2,-2,-1), (1,-2,2)
]


def by_key(camera, slots, locations):
    keyed = sorted((int(host.blend_sort_key(camera, loc)), int(s)) for s, loc in zip(slots, locations))
    return [s for _k, s in keyed]


def test_key_order_is_the_draw_order_on_random_pairs():
    rng = np.random.default_rng(0xB1E2D)
    n = 10_000
    for camera in (CAMERA, tuple(rng.uniform(-50, 50, 3).astype(f32))):
        # a third of the locations on a coarse lattice about the camera (ties), the rest anywhere, over many magnitudes
        lattice = np.asarray(camera, dtype=f32) + rng.integers(-3, 4, (n // 3, 3)).astype(f32)
        free = (rng.standard_normal((n - n // 3, 3)) * 10.0 ** rng.uniform(-3, 6, (n - n // 3, 1))).astype(f32)
        locations = np.concatenate([lattice, free]).astype(f32)
        rng.shuffle(locations)
        slots = np.cumsum(rng.integers(1, 4, n))  # ascending, with gaps
        assert by_key(camera, slots, locations) == host.blend_draw_order(camera, slots, locations)


def test_key_order_is_the_draw_order_on_crafted_pairs():
    slots = [2 + 3 * i for i in range(len(CRAFTED))]
    with np.errstate(over="ignore"):
        order = host.blend_draw_order(CAMERA, slots, CRAFTED)
    assert by_key(CAMERA, slots, CRAFTED) == order
    # the +inf pair first (slot order), the pair at the camera last (slot order)
    assert order[:2] == [slots[3], slots[4]] and order[-2:] == [slots[0], slots[1]]
    assert order[-3] == slots[2]
    key = lambda i: int(host.blend_sort_key(CAMERA, CRAFTED[i]))  # noqa: E731
    assert key(0) == key(1) == 0x7FFFFFFF, "-0.0: the largest key there is"
    assert key(3) == key(4) == 0x007FFFFF, "-inf"
    assert key(5) == key(6) and key(7) == key(8) == key(9)
    # a subnormal distance^2: d = 2^-70, d * d = 2^-140
    tiny = (3.0, -2.0, 2.0 ** -70)
    cam0 = (3.0, -2.0, 0.0)
    assert 0x7FFFFFFF > int(host.blend_sort_key(cam0, tiny)) == 0x7FFFFFFF - (1 << 9)  # 2^-140 = subnormal 2^9 * 2^-149
    assert host.blend_draw_order(cam0, [5, 9], [cam0, tiny]) == [9, 5] == by_key(cam0, [5, 9], [cam0, tiny])


def test_key_is_monotone_in_minus_dist():
    """over the whole range of -dist -- every f32 from -inf to -0.0, sampled, neighbours included -- a smaller float gives a
    smaller key and equal floats give equal keys"""
    rng = np.random.default_rng(7)
    bits = np.unique(np.concatenate([rng.integers(0, 0x7F800001, 20_000, dtype=np.int64), np.arange(0, 2048), np.arange(0x7F800000 - 2048, 0x7F800001),
                                     np.arange(0x00800000 - 64, 0x00800000 + 64)])).astype(np.uint32)
    dist = bits.view(f32)  # ascending, +0.0 .. +inf
    assert np.all(np.diff(dist) > 0)
    origin = (0.0, 0.0, 0.0)
    # a location (sqrt-free) whose dist is exactly `dist`: not constructible in general, so the mapping is checked on its own
    keys = np.array([int(_map(-d)) for d in dist], dtype=np.int64)
    assert np.all(np.diff(keys) < 0), "dist ascending = -dist descending = key descending"
    # and the function composes the two: dist of (x, 0, 0) from the origin is x * x
    for x in (0.0, 1.0, 1.5, 3.0e-23, 2.0e19, 3.0e20):
        with np.errstate(over="ignore"):
            d = f32(x) * f32(x)
        assert int(host.blend_sort_key(origin, (x, 0.0, 0.0))) == int(_map(-d))
    assert int(host.blend_sort_key(origin, (3.0e20, 0.0, 0.0))) == 0x007FFFFF


def _map(v):
    b = np.array([v], dtype=f32).view(np.uint32)[0]
    return np.uint32(~b) if b & np.uint32(0x80000000) else np.uint32(b | np.uint32(0x80000000))


def test_new_symbols_are_declared():
    for name in ("r3n_blend_objects_write", "r3n_blend_sort", "r3n_readback_blend_order"):
        assert name in _ffi.SIGNATURES
    assert _ffi.STAGES[21] == "blend_sort" and len(_ffi.STAGES) == 22


def test_scene_viewer_switch():
    import argparse

    from rend3_amd import scene_viewer as sv
    ap = sv.add_arguments(argparse.ArgumentParser())
    assert sv.settings_from(ap.parse_args([]))["blend_sort"] == "host"
    assert sv.settings_from(ap.parse_args(["--blend-sort", "gpu"]))["blend_sort"] == "gpu"
