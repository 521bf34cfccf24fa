"""GPU: what the synchronous set-up entries of the cube and environment section leave behind for the cost tools -- the launch count
and the phase times of the LAST call (r3n_internal_{cube_source,envlight,ibl}_{launches,times}) -- and what they must not leave
behind: an event.  One small panorama goes through r3n_texture_cubes_write_sources, r3n_environment_lights and
r3n_environment_prefilter, with r3n_timing_enable off and on.  The launch counts are the ones tests/test_equirect_gpu.py,
tests/test_envlight_gpu.py and tests/test_ibl_gpu.py derive; the words the calls produce are theirs to check."""
import ctypes
import math

import numpy as np
import pytest

import envlight_reference as E
import equirect_reference as Q
from oracle import host as oh

pytestmark = pytest.mark.gpu
f32 = np.float32
ERR_INVALID_ARG = -1
W, H = 16, 8  # the panorama; its default cube: N = H // 2 = 4, levels 4, 2, 1 -- the smallest the prefilter takes two levels of
MAX_LIGHTS = 2
IBL_LAUNCHES = 6  # every call, whatever its shape (tests/test_ibl_gpu.py World.run)
PHASES = {"cube_source": 4, "envlight": 3, "ibl": 4}  # floats r3n_internal_<name>_times writes


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def panorama():
    rng = np.random.default_rng(W * 1000 + H)
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(120, 136, (H, W))  # RGBE exponents: radiance around 1
    return img


def events(r):
    out = (ctypes.c_uint64 * 4)()
    fn = r.lib.r3n_internal_live_resources  # an internal entry point: not in include/r3n.h, so it carries no signature
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64)]
    assert fn(out) == 0
    return int(out[2])  # (hip_owned::kEvents)


def cost(r, name):
    """(launches, times) of the last call as the exports give them; the export writes its floats and not one more"""
    fn = getattr(r.lib, f"r3n_internal_{name}_launches")
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_uint64
    launches = int(fn(r.ctx))
    fn = getattr(r.lib, f"r3n_internal_{name}_times")
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    ms = np.full(5, np.nan, dtype=f32)
    assert fn(r.ctx, ms.ctypes.data) == 0
    n = PHASES[name]
    assert np.isnan(ms[n:]).all(), (name, ms)
    assert fn(r.ctx, None) == ERR_INVALID_ARG and fn(None, ms.ctypes.data) == ERR_INVALID_ARG
    return launches, ms[:n].copy()


def check(r, name, launches, timed, before):
    got, ms = cost(r, name)
    print(f"{name}: timing {'on' if timed else 'off'}, launches {got}, ms {ms.tolist()}, events {before} -> {events(r)}")
    assert got == launches, name
    assert events(r) == before, f"{name}: the call's events are gone when it returns"
    if timed:
        assert np.isfinite(ms).all() and (ms >= 0).all(), (name, ms)
    else:
        assert ms.tobytes() == bytes(4 * PHASES[name]), (name, ms)
    return got, ms


def lights(r, cube, level):
    from rend3_amd import _ffi
    params = _ffi.EnvLightsParams(cube, level, MAX_LIGHTS, float(f32(math.cos(math.radians(6.0)))), 0.0)  # min_share 0: every light asked for runs
    out = _ffi.EnvLightsResult()
    return r.lib.r3n_environment_lights(r.ctx, ctypes.addressof(params), ctypes.addressof(out))


def prefilter(r, cube, level, levels):
    from rend3_amd import _ffi
    params = _ffi.EnvPrefilterParams(cube, level, levels)
    out = _ffi.EnvPrefilterResult()
    return r.lib.r3n_environment_prefilter(r.ctx, ctypes.addressof(params), ctypes.addressof(out))


@pytest.mark.parametrize("timed", [False, True], ids=["timing_off", "timing_on"])
def test_the_cost_of_the_last_call(r3, timed):
    p = r3.Renderer(oh.LEFT, f32(1.0))
    p.timing_enable(timed)
    cube = p.add_texture_cube_equirect(panorama(), W, H)
    n, mips = p._cube_extent_and_mips(cube)
    assert (n, mips) == (4, 3)
    plan = Q.plan([n], [mips], Q.TAIL_DEFAULT)
    assert plan["faces"] and plan["tail"], "a chain behind the faces: every phase of the upload has something in it"

    def same(a, b):
        return a[0] == b[0] and a[1].tobytes() == b[1].tobytes()

    # the upload (+ k_cube_assemble; RGBE needs no decode launch), then a refused one
    before = events(p)
    p._flush_cubes()
    kept = check(p, "cube_source", Q.plan_launches(plan) + 1, timed, before)
    assert p.lib.r3n_texture_cubes_write_sources(p.ctx, None, 1, None, 0) == ERR_INVALID_ARG
    assert same(cost(p, "cube_source"), kept) and events(p) == before

    # the lights of level 0, then a level past the cube's last
    before = events(p)
    assert lights(p, cube, 0) == 0, p.lib.r3n_last_error(p.ctx)
    kept = check(p, "envlight", 2 + (E.SHIFT_STEPS + 1) * MAX_LIGHTS, timed, before)
    assert lights(p, cube, mips) == ERR_INVALID_ARG
    assert same(cost(p, "envlight"), kept) and events(p) == before

    # two levels of the prefilter, then a level past the cube's last
    before = events(p)
    assert prefilter(p, cube, 0, 2) == 0, p.lib.r3n_last_error(p.ctx)
    kept = check(p, "ibl", IBL_LAUNCHES, timed, before)
    assert prefilter(p, cube, mips, 2) == ERR_INVALID_ARG
    assert same(cost(p, "ibl"), kept) and events(p) == before

    if timed:  # and with timing switched off again, a call overwrites the times it left with zeros
        p.timing_enable(False)
        before = events(p)
        assert lights(p, cube, 0) == 0, p.lib.r3n_last_error(p.ctx)
        check(p, "envlight", 2 + (E.SHIFT_STEPS + 1) * MAX_LIGHTS, False, before)
    p.close()
