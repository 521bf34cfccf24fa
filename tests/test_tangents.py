"""Generated tangents, CPU half: the two numpy restatements of the contract (tests/tangents_reference.py) against each other and the
library's host function against them, bit for bit; known answers derived by hand; the summation order is observable; the loader and
the viewer pass the options on.  Renderer.add_mesh needs a device, so its argument tests are in the GPU half,
tests/test_tangents_gpu.py."""
import os
import sys

import numpy as np
import pytest

import tangents_reference as TR
from oracle import host as oh
from oracle.world import material_record as omk
from rend3_amd import gltf

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "morph-notangent.glb")
MESHES = TR.mesh_set()
IDS = [m[0] for m in MESHES]
GRIDS = [m for m in MESHES if m[0].startswith("grid")]


def _words(a):
    return np.ascontiguousarray(a, dtype=f32).reshape(-1).view(np.uint32)


def _normal_cases(pos, idx, seed):
    """The two kinds of normals a tangent run is built over: the serial normals loop's and given unit vectors."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [("computed", oh.calculate_normals(pos, idx[: 3 * (len(idx) // 3)], True)), ("given", TR.unit_normals(rng, len(pos)))]


def _finite(a):
    return bool(np.isfinite(np.asarray(a)).all())


def _fixture_module():
    sys.path.insert(0, GOLDEN)
    try:
        import make_tangents_fixture
    finally:
        sys.path.remove(GOLDEN)
    return make_tangents_fixture


# ------------------------------------------------------------------ C1. serial == gather == the host function
def test_the_set():
    assert sorted({len(m[1]) for m in MESHES}) == [1, 3, 63, 64, 65, 130, 257] and len(MESHES) == 14
    for name, pos, idx, uv in MESHES:
        assert uv.shape == (len(pos), 2) and uv.dtype == f32
        if name.startswith("soup"):
            tri = idx[: 3 * (len(idx) // 3)].reshape(-1, 3)
            repeated = [t for t in range(len(tri)) if len(set(tri[t].tolist())) < 3]
            assert repeated == list(range(31, len(tri), 32)) and len(idx) % 3 == 1
            assert TR.zero_share(pos, idx, uv) <= 0.25


@pytest.mark.parametrize("name,pos,idx,uv", MESHES, ids=IDS)
def test_serial_equals_gather(name, pos, idx, uv):
    for kind, nrm in _normal_cases(pos, idx, 1):
        a, b = TR.serial(pos, nrm, uv, idx), TR.gather(pos, nrm, uv, idx)
        assert np.array_equal(_words(a), _words(b)), f"{name}, {kind} normals: {int((_words(a) != _words(b)).sum())} words differ"
        assert _finite(a)


@pytest.mark.parametrize("name,pos,idx,uv", MESHES, ids=IDS)
def test_host_function_equals_serial(name, pos, idx, uv):
    from rend3_amd import host as ph
    for kind, nrm in _normal_cases(pos, idx, 2):
        got, want = ph.calculate_tangents(pos, nrm, uv, idx), TR.serial(pos, nrm, uv, idx)
        assert got.dtype == f32 and got.shape == (len(pos), 3) and _finite(got)
        assert np.array_equal(_words(got), _words(want)), f"{name}, {kind} normals: {int((_words(got) != _words(want)).sum())} words differ"


def test_some_soup_vertices_are_poisoned_and_most_are_not():
    """The every-32nd triangle with a repeated index zeroes the vertices it names; the others keep unit tangents."""
    for name, pos, idx, uv in MESHES:
        if not name.startswith("soup") or len(pos) < 63:
            continue
        nrm = oh.calculate_normals(pos, idx[: 3 * (len(idx) // 3)], True)
        got = TR.serial(pos, nrm, uv, idx)
        tri = idx[: 3 * (len(idx) // 3)].reshape(-1, 3)
        named = np.unique(tri[31::32])
        assert len(named) and not _words(got[named]).any(), name
        length = np.linalg.norm(got.astype(np.float64), axis=1)
        assert ((np.abs(length - 1.0) < 1e-6) | (length == 0.0)).all() and (length > 0).sum() >= 0.75 * len(np.unique(tri))


# ------------------------------------------------------------------ C2. known answers
KAT_POS = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=f32)
KAT_NRM = np.array([(0, 0, 1)] * 3, dtype=f32)
KAT_IDX = np.array([0, 1, 2], dtype=np.uint32)


def _all_three(pos, nrm, uv, idx):
    from rend3_amd import host as ph
    return [TR.serial(pos, nrm, uv, idx), TR.gather(pos, nrm, uv, idx), ph.calculate_tangents(pos, nrm, uv, idx)]


def test_known_answer_r_multiplies_the_second_product_only():
    """e1 = (1,0,0), e2 = (0,1,0), a = (1,1), b = (0,2): r = 1 / (1*2 - 1*0) = 0.5; g = e1 * 2 - (e2 * 1) * 0.5 = (2, -0.5, 0), NOT
    (e1 * 2 - e2 * 1) * 0.5 = (1, -0.5, 0).  n.g = 0, so tangent = (2, -0.5, 0) / sqrt(4.25)."""
    uv = np.array([(0, 0), (1, 1), (0, 2)], dtype=f32)
    for got in _all_three(KAT_POS, KAT_NRM, uv, KAT_IDX):
        assert _words(got).reshape(3, 3).tolist() == [[1064852291, 3195558723, 0]] * 3
    assert np.array_equal(np.array([1064852291, 3195558723], dtype=np.uint32).view(f32), np.array([0.97014254, -0.24253564], dtype=f32))
    wrong = np.array([1.0, -0.5, 0.0]) / np.sqrt(1.25)
    assert abs(f32(0.97014254) - wrong[0]) > 0.05


def test_known_answer_degenerate_uv_gives_zero_tangents():
    """uv (0,0), (1,0), (2,0): a.x * b.y - a.y * b.x = 0, r = inf, the term is NaN and all three tangents are (+0, +0, +0)."""
    uv = np.array([(0, 0), (1, 0), (2, 0)], dtype=f32)
    for got in _all_three(KAT_POS, KAT_NRM, uv, KAT_IDX):
        assert _words(got).tolist() == [0] * 9


def test_a_repeated_index_zeroes_what_it_names_only():
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], dtype=f32)
    uv = np.array([(0, 0), (1, 0.25), (0.5, 1), (1.5, 1.25)], dtype=f32)
    nrm = np.array([(0, 0, 1)] * 4, dtype=f32)
    idx = np.array([0, 1, 2, 1, 1, 3, 9], dtype=np.uint32)  # (1, 1, 3) names 1 twice; the trailing word is no triangle
    for got in _all_three(pos, nrm, uv, idx):
        assert not _words(got[[1, 3]]).any() and _words(got[0]).any() and _words(got[2]).any() and _finite(got)


def test_unreferenced_vertices_get_positive_zeros():
    name, pos, idx, uv = MESHES[0]
    assert name == "lone vertex" and _words(TR.serial(pos, np.ones_like(pos), uv, idx)).tolist() == [0, 0, 0]
    _n, pos, idx, uv = next(m for m in MESHES if m[0] == "soup 65")
    got = TR.serial(pos, TR.unit_normals(np.random.Generator(np.random.PCG64(3)), len(pos)), uv, idx)
    unreferenced = np.setdiff1d(np.arange(len(pos)), idx[:-1])
    assert len(unreferenced) and not _words(got[unreferenced]).any()


# ------------------------------------------------------------------ C3. the order is observable
@pytest.mark.parametrize("name,pos,idx,uv", GRIDS, ids=[m[0] for m in GRIDS])
def test_summation_order_is_observable(name, pos, idx, uv):
    """The same terms added in the reverse order give other words on every grid: a kernel that summed in any order but the
    contract's would not pass the bit-exact tests."""
    nrm = oh.calculate_normals(pos, idx, True)
    fwd, rev = TR.serial(pos, nrm, uv, idx), TR.gather(pos, nrm, uv, idx, reverse_rows=True)
    changed = int((_words(fwd).reshape(-1, 3) != _words(rev).reshape(-1, 3)).any(axis=1).sum())
    print(f"{name}: {changed} of {len(pos)} vertices change with the triangle order reversed")
    assert changed >= 1 and _finite(rev)


# ------------------------------------------------------------------ C4. loader, viewer, tables
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

    def add_texture_2d(self, *a, **kw):
        return 0

    def add_morph_instance(self, mesh, weights=None):
        self.morphs.append((mesh, None if weights is None else list(weights)))
        return len(self.morphs) - 1

    def add_object(self, mesh, material, transform, **kw):
        self.objects.append((mesh, kw))
        return len(self.objects) - 1


def test_fixture_is_what_its_generator_writes():
    assert open(FIXTURE, "rb").read() == _fixture_module().build()
    assert os.path.getsize(FIXTURE) < 16 * 1024


def test_fixture_has_uv_a_normal_texture_and_no_tangents():
    g = gltf.Gltf(FIXTURE)
    p = g.primitive(0, 0)
    assert len(p["positions"]) == 81 and p.get("tangents") is None and p.get("normals") is None and p["uv0"].shape == (81, 2)
    t = p["targets"]
    assert t["positions"].shape == (2, 81, 3) and t["normals"] is None and t["tangents"] is None
    assert "normalTexture" in g.json["materials"][p["material"]]


def test_loader_passes_the_options_only_when_asked():
    g = gltf.Gltf(FIXTURE)
    r = _Recorder()
    gltf.instance_scene(g, r, oh, omk, build_tangents=True, morph_tangents="recompute", morph_normals="recompute")
    assert len(r.meshes) == 1 and r.meshes[0]["build_tangents"] is True and r.meshes[0]["morph_tangents"] == "recompute"
    assert r.meshes[0]["morph_normals"] == "recompute" and r.meshes[0]["tangents"] is None and r.meshes[0]["uv0"] is not None
    r = _Recorder()
    gltf.instance_scene(g, r, oh, omk, build_tangents=True)
    assert r.meshes[0]["build_tangents"] is True and "morph_tangents" not in r.meshes[0]
    # the default, and recompute without generated tangents: the keywords are not passed at all
    for kw in ({}, dict(build_tangents=False), dict(morph_tangents="recompute"), dict(morph_tangents="base")):
        r = _Recorder()
        gltf.instance_scene(g, r, oh, omk, **kw)
        assert len(r.meshes) == 1 and "build_tangents" not in r.meshes[0] and "morph_tangents" not in r.meshes[0]
    with pytest.raises(ValueError):
        gltf.instance_scene(g, _Recorder(), oh, omk, morph_tangents="sometimes")


@pytest.mark.parametrize("name", ["morph-plane.glb", "morph-nonormal.glb", "animation-cube.glb"])
def test_primitives_without_uv_or_with_tangents_are_never_marked(name):
    g = gltf.Gltf(os.path.join(GOLDEN, name))
    r = _Recorder()
    gltf.instance_scene(g, r, oh, omk, build_tangents=True, morph_tangents="recompute")
    assert r.meshes
    for kw in r.meshes:
        wants = kw.get("uv0") is not None and kw.get("tangents") is None
        assert ("build_tangents" in kw) == wants
        assert ("morph_tangents" in kw) == (wants and kw.get("morph_targets") is not None and kw["morph_targets"]["positions"] is not None
                                            and kw["morph_targets"]["tangents"] is None)


def test_scene_viewer_flags():
    import argparse
    from rend3_amd import scene_viewer as sv
    ap = sv.add_arguments(argparse.ArgumentParser())
    s = sv.settings_from(ap.parse_args([]))
    assert s["build_tangents"] is False and s["morph_tangents"] == "base" and sv.default_settings()["morph_tangents"] == "base"
    s = sv.settings_from(ap.parse_args(["--build-tangents", "--morph-tangents", "recompute"]))
    assert s["build_tangents"] is True and s["morph_tangents"] == "recompute"
    with pytest.raises(SystemExit):
        ap.parse_args(["--morph-tangents", "mikk"])


def test_stage_table_and_record_size():
    import ctypes
    from rend3_amd import _ffi
    assert _ffi.STAGE_TABLE[22:] == ["morph", "normals", "tangents"] and _ffi.STAGE_TABLE[:24] == _ffi.STAGE_NAMES
    sig = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32])
    assert _ffi.SIGNATURES["r3n_vertex_tangents"] == sig
    assert hasattr(_ffi.lib(), "r3n_vertex_tangents") and hasattr(_ffi.lib(), "r3n_host_calculate_tangents")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "r3n.h")).read()
    assert "#define R3N_STAGE_TANGENTS 24" in header and f"#define R3N_STAGE_COUNT {len(_ffi.STAGE_TABLE)}" in header
