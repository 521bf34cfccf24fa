"""Morph targets, CPU half: known answers of the numpy restatement of the contract (tests/morph_reference.py), the synthetic
fixture tests/golden/morph-plane.glb through the GLB reader and the scene instancer, and the weights channels of the animation
path.  The GPU half is tests/test_morph_gpu.py."""
import json
import os
import struct
import sys

import numpy as np
import pytest

import morph_reference as MR
from oracle import host as oh
from oracle.world import material_record as omk
from rend3_amd import anim, gltf

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "morph-plane.glb")


def _fixture_module():
    sys.path.insert(0, GOLDEN)
    try:
        import make_morph_fixture
    finally:
        sys.path.remove(GOLDEN)
    return make_morph_fixture


# ------------------------------------------------------------------ the reference's known answers
def test_one_hot_weight_is_base_plus_delta():
    rng = np.random.Generator(np.random.PCG64(1))
    base = rng.uniform(-2, 2, (17, 3)).astype(f32)
    deltas = rng.uniform(-1, 1, (3, 17, 3)).astype(f32)
    got = MR.blend(base, deltas, [0.0, 1.0, 0.0])
    assert np.array_equal(got.view(np.uint32), (base + deltas[1]).astype(f32).view(np.uint32))


def test_zero_weights_return_the_base_bit_for_bit():
    base = np.array([[-0.0, 1.5, -3.25], [0.0, -0.0, 7.0]], dtype=f32)
    deltas = np.ones((2, 2, 3), dtype=f32)
    for weights in ([0.0, 0.0], [-0.0, 0.0], [-0.0, -0.0]):
        got = MR.blend(base, deltas, np.array(weights, dtype=f32))
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    # the skip is what keeps -0.0: adding a +0.0 product would turn it into +0.0
    assert (f32(-0.0) + f32(0.0) * f32(1.0)).view(np.uint32) == 0 and base.view(np.uint32)[0, 0] == 0x80000000


def test_nan_weight_propagates():
    base = np.array([1.0, 2.0, 3.0], dtype=f32)
    deltas = np.zeros((2, 3), dtype=f32)  # even over all-zero deltas: NaN * 0 is NaN, and NaN is not skipped
    got = MR.blend(base, deltas, np.array([np.nan, 0.0], dtype=f32))
    assert np.isnan(got).all()


def test_summation_order_and_single_rounding_are_observable():
    base = np.array([1.0e8], dtype=f32)
    assert MR.blend(base, np.array([[1.0], [-1.0e8]], dtype=f32), [1.0, 1.0])[0] == 0.0   # (1e8 + 1) -> 1e8, then - 1e8
    assert MR.blend(base, np.array([[-1.0e8], [1.0]], dtype=f32), [1.0, 1.0])[0] == 1.0   # the same terms, swapped targets
    # the product rounds before the sum: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 -> 1 + 2^-11 (tie to even); a fused multiply-add
    # would leave 2^-24
    w = f32(1.0) + f32(2.0 ** -12)
    got = MR.blend(np.array([-(1.0 + 2.0 ** -11)], dtype=f32), np.array([[w]], dtype=f32), [w])
    assert got[0] == 0.0


def test_reach_and_radius():
    d = np.zeros((3, 4, 3), dtype=f32)
    d[0, 2] = (3.0, 4.0, 12.0)
    d[1, 1] = (0.0, -2.0, 0.0)
    rc = MR.reach(d)
    assert rc.dtype == f32 and list(rc) == [13.0, 2.0, 0.0]
    assert MR.radius(1.0, [0.5, -2.0, 9.0], rc) == f32(1.0 + 6.5 + 4.0)
    assert MR.radius(1.0, [0.0, -0.0, 0.0], rc) == f32(1.0)
    # in target order, one rounding per operation
    r = f32(f32(f32(0.1) + f32(f32(0.3) * f32(13.0))) + f32(f32(0.7) * f32(2.0)))
    assert MR.radius(0.1, [0.3, -0.7, 0.0], rc) == r


def test_product_bounds_follow_the_reference():
    from rend3_amd import renderer
    rng = np.random.Generator(np.random.PCG64(7))
    d = rng.uniform(-3, 3, (5, 33, 3)).astype(f32)
    rc = renderer.morph_reach(d, 5)
    assert rc.dtype == f32 and np.array_equal(rc, MR.reach(d))
    assert not renderer.morph_reach(None, 4).any()
    for w in ([0.5, -0.25, 0.0, 2.0, -0.0], [0.0] * 5, [-1.0, 1.0, -1.0, 1.0, 3.5]):
        got = renderer.morph_radius(f32(1.25), np.array(w, dtype=f32), rc)
        assert got == MR.radius(1.25, w, rc) and got.dtype == f32


# ------------------------------------------------------------------ the fixture through gltf.py
def test_fixture_is_what_its_generator_writes():
    assert open(FIXTURE, "rb").read() == _fixture_module().build()


def test_fixture_primitive_targets():
    a = _fixture_module().arrays()
    p = gltf.Gltf(FIXTURE).primitive(0, 0)
    assert len(p["positions"]) == 81 and p["tangents"].shape == (81, 3)
    t = p["targets"]
    assert t["positions"].shape == (3, 81, 3) and t["normals"].shape == (3, 81, 3) and t["tangents"].shape == (3, 81, 3)
    assert all(v.dtype == f32 for v in t.values())
    assert np.array_equal(t["positions"][0], a["t0_pos"]) and np.array_equal(t["normals"][0], a["t0_nrm"])
    # the sparse target: the listed vertices hold the stored values, every other vertex is zero
    dense = np.zeros((81, 3), dtype=f32)
    dense[a["t1_idx"]] = a["t1_val"]
    assert np.array_equal(t["positions"][1], dense) and np.count_nonzero(t["positions"][1].any(axis=1)) == 7
    # a target that lacks an attribute the others have contributes zeros
    assert not t["normals"][1].any() and not t["tangents"][0].any() and not t["tangents"][1].any()
    assert np.array_equal(t["positions"][2], a["t2_pos"]) and np.array_equal(t["normals"][2], a["t2_nrm"])
    assert np.array_equal(t["tangents"][2], a["t2_tan"])


class _Recorder:
    """The world-edit calls instance_scene makes, recorded."""
    handedness = 1

    def __init__(self):
        self.meshes, self.morphs, self.objects, self.skeletons = [], [], [], []

    def add_mesh(self, positions, indices=None, **kw):
        self.meshes.append(kw)
        return len(self.meshes) - 1

    def add_material(self, record, key=0):
        return 0

    def add_morph_instance(self, mesh, weights=None):
        self.morphs.append((mesh, None if weights is None else list(weights)))
        return len(self.morphs) - 1

    def add_object(self, mesh, material, transform, **kw):
        self.objects.append((mesh, kw))
        return len(self.objects) - 1


def test_fixture_instancing_and_weight_precedence():
    r = _Recorder()
    inst = gltf.instance_scene(gltf.Gltf(FIXTURE), r, oh, omk)
    assert len(r.meshes) == 1 and r.meshes[0]["morph_weights"] == [0.25, 0.0, 0.5]
    assert r.meshes[0]["morph_targets"]["positions"].shape == (3, 81, 3)
    # one morph instance per (node, primitive); node.weights win over mesh.weights
    assert r.morphs == [(0, [0.25, 0.0, 0.5]), (0, [0.0, 1.0, 0.25])]
    assert inst["nodes"][0]["morphs"] == [0] and inst["nodes"][1]["morphs"] == [1]
    assert r.objects == [(None, dict(morph=0)), (None, dict(morph=1))]


def test_file_without_targets_takes_the_old_calls():
    r = _Recorder()
    inst = gltf.instance_scene(gltf.Gltf(os.path.join(GOLDEN, "animation-cube.glb")), r, oh, omk)
    assert r.morphs == [] and all("morph_targets" not in kw for kw in r.meshes)
    assert all(kw == {} for _mesh, kw in r.objects) and all(n["morphs"] == [] for n in inst["nodes"])


def test_fixture_animation_channels_and_duration():
    a = _fixture_module().arrays()
    (an,) = gltf.load_animations(gltf.Gltf(FIXTURE))
    assert an["channels"] == {} and an["name"] == "weights"
    assert sorted(an["morph_channels"]) == [0, 1]
    times, values, interp = an["morph_channels"][1]
    assert interp == "LINEAR" and np.array_equal(times, a["lin_t"]) and np.array_equal(values, a["lin_w"]) and values.shape == (3, 3)
    times, values, interp = an["morph_channels"][0]
    assert interp == "STEP" and np.array_equal(times, a["step_t"]) and np.array_equal(values, a["step_w"])
    # a weights-only clip: the duration is its latest key, not 0
    assert an["duration"].dtype == f32 and an["duration"] == f32(1.25)


# ------------------------------------------------------------------ sampling
LIN = (np.array([0.0, 0.5, 1.25], dtype=f32), np.array([[0.0, 1.0, 0.25], [1.5, 0.0, -0.5], [0.0, 0.75, 1.0]], dtype=f32))


def _lerp(a, b, x):
    return np.array([f32(p + f32(f32(q - p) * f32(x))) for p, q in zip(a, b)], dtype=f32)


def test_sample_morph_weights_linear():
    ch = LIN + ("LINEAR",)
    s = anim.sample_morph_weights
    assert s(ch, f32(0.0)).dtype == f32
    assert np.array_equal(s(ch, f32(0.0)), LIN[1][0]) and np.array_equal(s(ch, f32(0.5)), LIN[1][1])          # at a key
    x = f32(f32(0.2) - f32(0.0)) / f32(f32(0.5) - f32(0.0))
    assert np.array_equal(s(ch, f32(0.2)), _lerp(LIN[1][0], LIN[1][1], x))                                    # between keys
    x = f32(f32(1.0) - f32(0.5)) / f32(f32(1.25) - f32(0.5))
    assert np.array_equal(s(ch, f32(1.0)), _lerp(LIN[1][1], LIN[1][2], x))
    assert np.array_equal(s(ch, f32(-1.0)), LIN[1][0])                                                       # before: x clamps to 0
    assert np.array_equal(s(ch, f32(1.25)), LIN[1][2]) and np.array_equal(s(ch, f32(9.0)), LIN[1][2])        # after: x clamps to 1


def test_sample_morph_weights_step():
    ch = LIN + ("STEP",)
    s = anim.sample_morph_weights
    assert np.array_equal(s(ch, f32(0.0)), LIN[1][0]) and np.array_equal(s(ch, f32(0.5)), LIN[1][1])          # at a key: that key
    assert np.array_equal(s(ch, f32(0.49)), LIN[1][0]) and np.array_equal(s(ch, f32(1.2)), LIN[1][1])        # between: the previous
    assert np.array_equal(s(ch, f32(-1.0)), LIN[1][0])                                                       # before the range
    assert np.array_equal(s(ch, f32(1.25)), LIN[1][2]) and np.array_equal(s(ch, f32(9.0)), LIN[1][2])        # from the last key on


def _with_interpolation(tmp_path, mode):
    data = open(FIXTURE, "rb").read()
    jlen = struct.unpack_from("<I", data, 12)[0]
    doc = json.loads(data[20:20 + jlen])
    doc["animations"][0]["samplers"][0]["interpolation"] = mode
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    body = struct.pack("<II", len(js), 0x4E4F534A) + js + data[20 + jlen:]
    path = tmp_path / "patched.glb"
    path.write_bytes(b"glTF" + struct.pack("<II", 2, 12 + len(body)) + body)
    return str(path)


def test_cubicspline_weights_are_refused(tmp_path):
    with pytest.raises(ValueError, match="weights"):
        gltf.load_animations(gltf.Gltf(_with_interpolation(tmp_path, "CUBICSPLINE")))
    with pytest.raises(ValueError, match="CUBICSPLINE"):
        anim.sample_morph_weights(LIN + ("CUBICSPLINE",), f32(0.1))
    # (the same file with a supported mode loads)
    assert gltf.load_animations(gltf.Gltf(_with_interpolation(tmp_path, "STEP")))[0]["morph_channels"][1][2] == "STEP"


class _Weights:
    handedness = 1

    def __init__(self):
        self.set = {}

    def set_morph_weights(self, handle, weights):
        self.set[handle] = np.array(weights, dtype=f32)

    def pose_skeletons(self, requests):
        assert requests == []


def test_pose_animation_frame_sets_the_weights():
    a = _fixture_module().arrays()
    g = gltf.Gltf(FIXTURE)
    inst = gltf.instance_scene(g, _Recorder(), oh, omk)

    class Data:
        animations, n_skins, skin_skeletons, clip_base = gltf.load_animations(g), 0, [], 0
    r = _Weights()
    anim.pose_animation_frame(r, inst, Data, 0, 0.5)
    assert np.array_equal(r.set[1], a["lin_w"][1]) and np.array_equal(r.set[0], a["step_w"][0])
    anim.pose_animation_frame(r, inst, Data, 0, 99.0)  # past the end: clamped to the duration, the last keys
    assert np.array_equal(r.set[1], a["lin_w"][2]) and np.array_equal(r.set[0], a["step_w"][1])


# ------------------------------------------------------------------ files without weights channels load as before
@pytest.mark.parametrize("name", ["animation-cube.glb", "animation-character.glb"])
def test_existing_animated_files_load_unchanged(name):
    g = gltf.Gltf(os.path.join(GOLDEN, name))
    got = gltf.load_animations(g)
    assert len(got) == len(g.json["animations"]) > 0
    for an, src in zip(got, g.json["animations"]):
        want, duration = {}, 0.0
        for ch in src["channels"]:  # the transform channels alone: what the loader returned before it read weights
            if "node" not in ch["target"] or ch["target"]["path"] == "weights":
                continue
            smp = src["samplers"][ch["sampler"]]
            times = g.accessor(smp["input"]).astype(f32).reshape(-1)
            want.setdefault(ch["target"]["node"], {})[ch["target"]["path"]] = (times, g.accessor(smp["output"]).astype(f32))
            duration = max(duration, float(times.max()))
        assert an["morph_channels"] == {}
        assert sorted(an["channels"]) == sorted(want)
        for node, paths in want.items():
            assert sorted(an["channels"][node]) == sorted(paths)
            for path, (times, values) in paths.items():
                assert np.array_equal(an["channels"][node][path][0], times) and np.array_equal(an["channels"][node][path][1], values)
        assert an["duration"] == f32(duration) and an["duration"].dtype == f32
