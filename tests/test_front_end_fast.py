"""The identities the geometry front end's shortcuts rest on (kernels_cull.h execute_culling_clip, device_math.h mul_point_pk,
setup_triangle, tri_bounds), in numpy's IEEE f32 on the CPU: division by 1.0f and multiplication by 1.0f return
their other operand bit for bit -- both zeros, subnormals, the extremes, infinities -- and turn a NaN into a NaN; RN(1 / 1) is 1.
The GPU side is tests/test_front_end_fast_gpu.py."""
import os
import re

import numpy as np

f32, u32 = np.float32, np.uint32
ONE = f32(1.0)


def bit_patterns():
    """the corners of the format, every exponent with a few mantissas, and a seeded sample of all 2^32 patterns"""
    corners = [0x00000000, 0x80000000,              # +0, -0
               0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,   # subnormals: smallest, largest, the middle
               0x00800000, 0x80800000,              # smallest normals
               0x3F800000, 0xBF800000, 0x3F7FFFFF, 0x3F800001,               # +-1 and its neighbours
               0x7F7FFFFF, 0xFF7FFFFF,              # the extremes
               0x7F800000, 0xFF800000,              # infinities
               0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]               # NaNs: quiet, signalling, full payload
    exps = (np.arange(256, dtype=np.uint64)[:, None] << 23) | np.array([0, 1, 0x400000, 0x7FFFFF], dtype=np.uint64)[None, :]
    both_signs = np.concatenate([exps.reshape(-1), exps.reshape(-1) | 0x80000000])
    rng = np.random.default_rng(0xF0E)
    sample = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64)
    return np.concatenate([np.array(corners, dtype=np.uint64), both_signs, sample]).astype(u32)


BITS = bit_patterns()
X = BITS.view(f32)
NAN = np.isnan(X)


def same_bits_or_both_nan(got, want_bits):
    g = np.asarray(got, dtype=f32)
    return np.all(np.where(NAN, np.isnan(g), g.view(u32) == want_bits))


def test_the_sample_holds_the_corners():
    assert {0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000} <= set(BITS.tolist())
    assert NAN.sum() >= 4 and (~NAN).sum() > 1 << 19


def test_division_by_one_is_the_identity():
    with np.errstate(all="ignore"):
        q = X / ONE
    assert q.dtype == f32
    assert same_bits_or_both_nan(q, BITS), "x / 1.0f != x for some bit pattern"


def test_multiplication_by_one_is_the_identity():
    """setup_triangle's products by 1 / w = 1, and the contract's c3 * 1.0f that mul_point_pk does not form"""
    with np.errstate(all="ignore"):
        assert same_bits_or_both_nan(X * ONE, BITS) and same_bits_or_both_nan(ONE * X, BITS)


def test_reciprocal_of_one_is_one():
    assert (ONE / ONE).view(u32) == u32(0x3F800000)


def test_a_non_finite_coordinate_makes_w_a_nan():
    """w = ((0 * x + 0 * y) + 0 * z) + 1 under an affine matrix: 0 * inf is a NaN, and a NaN is not 1 -- the wave slot divides"""
    with np.errstate(all="ignore"):
        for bad in (f32(np.inf), f32(-np.inf), f32(np.nan)):
            w = ((f32(0.0) * bad + f32(0.0) * f32(0.5)) + f32(0.0) * f32(0.25)) + ONE
            assert np.isnan(w) and not (w == ONE)


def test_the_switch_and_the_three_forms_are_in_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    def read(*p):
        return open(os.path.join(root, *p)).read()
    hip, cull = read("rend3_amd", "csrc", "r3n.hip"), read("rend3_amd", "csrc", "kernels_cull.h")
    assert re.search(r'\{"front_end_fast", &t\.front_end_fast, 0, 1, 1\}', hip), "R3N_TUNE key front_end_fast, 0 or 1"
    assert re.search(r"uint32_t front_end_fast = 1;", hip), "on by default"
    for mode in ("R3N_CULL_PLAIN", "R3N_CULL_FAST_VIEW", "R3N_CULL_FAST_SHADOW"):
        assert re.search(r"k_triangle_cull<" + mode + ">", hip) and re.search(r"#define\s+" + mode + r"\s+\d", cull), mode
