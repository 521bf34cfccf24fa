"""Recomputed normals, CPU half: the host-built vertex adjacency against its numpy restatement, the gather form of the contract
(tests/normals_reference.py) against the oracle's serial loop bit for bit, and the fixture tests/golden/morph-nonormal.glb through
the GLB reader and the scene instancer.  The GPU half is tests/test_normals_gpu.py."""
import os
import sys

import numpy as np
import pytest

import normals_reference as NR
from oracle import host as oh
from oracle.world import material_record as omk
from rend3_amd import anim, gltf

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "morph-nonormal.glb")
MESHES = NR.mesh_set()


def _words(a):
    return np.ascontiguousarray(a, dtype=f32).reshape(-1).view(np.uint32)


def _fixture_module():
    sys.path.insert(0, GOLDEN)
    try:
        import make_normals_fixture
    finally:
        sys.path.remove(GOLDEN)
    return make_normals_fixture


# ------------------------------------------------------------------ C1. the adjacency
@pytest.mark.parametrize("name,pos,idx", MESHES, ids=[m[0] for m in MESHES])
def test_host_adjacency_matches_the_restatement(name, pos, idx):
    from rend3_amd import host as ph
    got = ph.vertex_adjacency(idx, len(pos))
    want = NR.adjacency(idx, len(pos))
    assert got.dtype == np.uint32 and got.shape == want.shape == (len(pos) + 1 + 3 * (len(idx) // 3),)
    assert np.array_equal(got, want)
    rows, lst = got[: len(pos) + 1], got[len(pos) + 1:]
    assert rows[0] == 0 and rows[-1] == len(lst) and (np.diff(rows.astype(np.int64)) >= 0).all()
    for v in range(len(pos)):  # ascending inside every row; a repeated index gives a repeated entry
        row = lst[rows[v]: rows[v + 1]]
        assert (np.diff(row.astype(np.int64)) >= 0).all()
        assert len(row) == int((idx[: 3 * (len(idx) // 3)] == v).sum())


def test_host_adjacency_refuses_an_index_out_of_range():
    from rend3_amd import _ffi
    from rend3_amd import host as ph
    idx = np.array([0, 1, 2, 2, 1, 3], dtype=np.uint32)
    out = np.zeros(3 + 1 + 6, dtype=np.uint32)
    assert _ffi.lib().r3n_host_vertex_adjacency(_ffi.ptr(idx), len(idx), 3, _ffi.ptr(out)) != 0
    assert _ffi.lib().r3n_host_vertex_adjacency(_ffi.ptr(idx), len(idx), 4, _ffi.ptr(np.zeros(4 + 1 + 6, dtype=np.uint32))) == 0
    with pytest.raises(ValueError):
        ph.vertex_adjacency(idx, 3)
    # an out-of-range word in the ignored remainder of the index run is not an index
    assert ph.vertex_adjacency(np.array([0, 1, 2, 9], dtype=np.uint32), 3).tolist() == [0, 1, 2, 3, 0, 0, 0]


# ------------------------------------------------------------------ C2. gather == the serial loop; the order is observable
@pytest.mark.parametrize("left_handed", [True, False], ids=["lh", "rh"])
@pytest.mark.parametrize("name,pos,idx", MESHES, ids=[m[0] for m in MESHES])
def test_gather_equals_the_serial_loop(name, pos, idx, left_handed):
    want = oh.calculate_normals(pos, idx[: 3 * (len(idx) // 3)], left_handed)
    got = NR.gather(pos, idx, left_handed)
    assert np.array_equal(_words(got), _words(want)), f"{name}: {int((_words(got) != _words(want)).sum())} words differ"


def test_handedness_is_observable():
    _n, pos, idx = next(m for m in MESHES if m[0] == "grid 13x10")
    a, b = NR.gather(pos, idx, True), NR.gather(pos, idx, False)
    assert not np.array_equal(_words(a), _words(b)) and np.array_equal(a, -b)


@pytest.mark.parametrize("name,pos,idx", [m for m in MESHES if m[0].startswith("soup") and len(m[1]) >= 63],
                         ids=[m[0] for m in MESHES if m[0].startswith("soup") and len(m[1]) >= 63])
def test_summation_order_is_observable(name, pos, idx):
    """The same terms added in the reverse order give other words on the random soups: a kernel that summed in any order but the
    contract's would not pass the bit-exact tests on these inputs."""
    fwd, rev = NR.gather(pos, idx, True), NR.gather(pos, idx, True, reverse_rows=True)
    assert int((_words(fwd) != _words(rev)).sum()) >= 1


def test_unreferenced_and_degenerate_vertices_get_positive_zeros():
    pos, idx = NR.lone_vertex()
    assert _words(NR.gather(pos, idx)).tolist() == [0, 0, 0]
    _n, pos, idx = next(m for m in MESHES if m[0] == "soup 65")
    got = NR.gather(pos, idx)
    unreferenced = np.setdiff1d(np.arange(len(pos)), idx[:-1])
    assert len(unreferenced) and not _words(got[unreferenced]).any()
    # a triangle (i, i, j) has a zero face term: alone it leaves (+0, +0, +0), not a NaN
    assert _words(NR.gather(pos[:2], np.array([0, 0, 1], dtype=np.uint32))).tolist() == [0] * 6


# ------------------------------------------------------------------ C3. the fixture through gltf.py
def test_fixture_is_what_its_generator_writes():
    assert open(FIXTURE, "rb").read() == _fixture_module().build()
    assert os.path.getsize(FIXTURE) < 16 * 1024


def test_fixture_has_no_normals_and_position_only_targets():
    a = _fixture_module().arrays()
    p = gltf.Gltf(FIXTURE).primitive(0, 0)
    assert len(p["positions"]) == 81 and p.get("normals") is None and p.get("tangents") is None
    t = p["targets"]
    assert t["positions"].shape == (2, 81, 3) and t["normals"] is None and t["tangents"] is None
    assert np.array_equal(t["positions"][0], a["t0_pos"]) and np.array_equal(t["positions"][1], a["t1_pos"])


class _Recorder:
    """The world-edit calls instance_scene makes, recorded."""
    handedness = 1

    def __init__(self):
        self.meshes, self.morphs, self.objects = [], [], []

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


def test_loader_marks_the_primitive_only_when_asked():
    g = gltf.Gltf(FIXTURE)
    r = _Recorder()
    inst = gltf.instance_scene(g, r, oh, omk, morph_normals="recompute")
    assert len(r.meshes) == 1 and r.meshes[0]["morph_normals"] == "recompute" and r.meshes[0]["normals"] is None
    assert r.meshes[0]["morph_weights"] == [0.5, 0.25] and r.meshes[0]["morph_targets"]["positions"].shape == (2, 81, 3)
    assert r.morphs == [(0, [0.5, 0.25]), (0, [0.0, 1.0])]  # node.weights win over mesh.weights
    assert inst["nodes"][0]["morphs"] == [0] and inst["nodes"][1]["morphs"] == [1]
    assert r.objects == [(None, dict(morph=0)), (None, dict(morph=1))]
    # the default: the keyword is not passed at all (a renderer that does not know it takes the calls it always took)
    for kw in ({}, dict(morph_normals="base")):
        r = _Recorder()
        gltf.instance_scene(g, r, oh, omk, **kw)
        assert len(r.meshes) == 1 and "morph_normals" not in r.meshes[0] and "morph_targets" in r.meshes[0]
    with pytest.raises(ValueError):
        gltf.instance_scene(g, _Recorder(), oh, omk, morph_normals="sometimes")


@pytest.mark.parametrize("name", ["morph-plane.glb", "animation-cube.glb"])
def test_a_primitive_with_normals_or_without_targets_is_never_marked(name):
    r = _Recorder()
    gltf.instance_scene(gltf.Gltf(os.path.join(GOLDEN, name)), r, oh, omk, morph_normals="recompute")
    assert r.meshes and all("morph_normals" not in kw for kw in r.meshes)


def test_fixture_animation_drives_the_weights():
    a = _fixture_module().arrays()
    g = gltf.Gltf(FIXTURE)
    (an,) = gltf.load_animations(g)
    assert sorted(an["morph_channels"]) == [0, 1] and an["duration"] == f32(1.25)
    assert an["morph_channels"][1][2] == "LINEAR" and an["morph_channels"][0][2] == "STEP"
    inst = gltf.instance_scene(g, _Recorder(), oh, omk, morph_normals="recompute")

    class Data:
        animations, n_skins, skin_skeletons, clip_base = [an], 0, [], 0

    class Weights:
        handedness = 1
        set = {}

        def set_morph_weights(self, handle, weights):
            self.set[handle] = np.array(weights, dtype=f32)

        def pose_skeletons(self, requests):
            assert requests == []
    r = Weights()
    anim.pose_animation_frame(r, inst, Data, 0, 0.5)
    assert np.array_equal(r.set[1], a["lin_w"][1]) and np.array_equal(r.set[0], a["step_w"][0])


def test_scene_viewer_flag():
    import argparse
    from rend3_amd import scene_viewer as sv
    ap = sv.add_arguments(argparse.ArgumentParser())
    assert sv.settings_from(ap.parse_args([]))["morph_normals"] == "base" and sv.default_settings()["morph_normals"] == "base"
    assert sv.settings_from(ap.parse_args(["--morph-normals", "recompute"]))["morph_normals"] == "recompute"
    with pytest.raises(SystemExit):
        ap.parse_args(["--morph-normals", "flat"])


def test_stage_table_and_record_size():
    import ctypes
    from rend3_amd import _ffi
    assert _ffi.STAGE_NAMES[22:] == ["morph", "normals"] and len(_ffi.STAGES) == 22
    assert _ffi.SIGNATURES["r3n_vertex_normals"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32])
    assert hasattr(_ffi.lib(), "r3n_vertex_normals")
