"""Row S1 (GPU skinning) at its edges, GPU part: k_skinning and k_skinning_mfma on the worlds of tests/skinning_worlds.py --
uploaded word for word with r3n_mesh_buffer_write, skinned by r3n_skinning called directly, the WHOLE mesh buffer read back
(sentinels, inputs and INVALID outputs must be untouched) -- and the renderer's cache, rebuild, refusal and pose paths against
tests/skinning_reference.py applied to the product's own records.  NaN rule, NaN cap and float64 bounds: see
tests/test_skinning_edges.py."""
import numpy as np
import pytest

import skinning_reference as sr
import skinning_worlds as sw
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd.scenes import skinned_cylinder
from test_skinning_edges import FINITE, MFMA, WORLDS, assert_nan_cap, assert_same_words, check_f64_bounds, oracle_skin, reference

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def bare():
    """One renderer without a world: its context takes the raw worlds one after the other."""
    import torch
    assert torch.cuda.is_available()
    import rend3_amd as r3
    p = r3.Renderer()
    yield p
    p.close()


def _run_world(p, w, mode):
    import rend3_amd as r3
    words, records, mats = w.words.copy(), np.ascontiguousarray(w.records), np.ascontiguousarray(w.matrices)
    p._check(p.lib.r3n_mesh_buffer_write(p.ctx, 0, r3._ffi.ptr(words), words.nbytes), "r3n_mesh_buffer_write")
    p.set_skinning_mode(mode)
    try:
        p._check(p.lib.r3n_skinning(p.ctx, r3._ffi.ptr(records), len(records), r3._ffi.ptr(mats), len(mats)), "r3n_skinning")
    finally:
        p.set_skinning_mode(0)
    return p.readback_mesh_words(0, len(words))


@pytest.mark.parametrize("name", WORLDS)
def test_exact_kernel_equals_the_reference_on_every_world(bare, name):
    w = sw.worlds()[name]
    got = _run_world(bare, w, 0)
    assert_same_words(got, reference(name), f"{name}: k_skinning against skin(), whole buffer")
    assert_nan_cap(w, got, name)
    if w.finite:
        report = []
        check_f64_bounds(w, got, name, report)
        print(f"{name}: worst error / bound: position {report[0][1]:.3f}, normal and tangent {report[0][2]:.3f}")


@pytest.mark.parametrize("name", MFMA)
def test_mfma_kernel_equals_its_oracle_order(bare, name):
    w = sw.worlds()[name]
    got = _run_world(bare, w, 1)
    assert_same_words(got, oracle_skin(w, mfma_order=True), f"{name}: k_skinning_mfma against r3o_skinning_mfma_order, whole buffer")
    assert_nan_cap(w, got, name + " (matrix cores)")  # a joint slot without weight adds nothing, whatever its matrix holds
    if w.finite:
        assert np.isfinite(got.view(f32)).all()
        report = []
        check_f64_bounds(w, got, name + " (matrix cores)", report)
        print(f"{name}: worst error / bound: position {report[0][1]:.3f}, normal and tangent {report[0][2]:.3f}")


# ------------------------------------------------------------------ through the renderer
def _camera(r):
    r.set_camera_data(oh.look_at_lh((0, 1.2, -4), (0, 1, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def _cylinder(r, joints):
    pos, idx, nrm, tang, ji, jw = skinned_cylinder(joints)
    return r.add_mesh(pos, idx, normals=nrm, tangents=tang, joint_indices=ji, joint_weights=jw)


def _pose(joints, seed):
    return sw.random_matrices(np.random.Generator(np.random.PCG64(seed)), joints)


def _ident(n):
    return np.tile(oh.identity(), (n, 1))


def _extent(p):
    """Words of the mesh buffer up to the end of the last run any skinning record names."""
    records, _ = p.skinning_buffers()
    per = (3, 3, 3, 2, 4, 3, 3, 3)
    return max((int(r[k]) // 4 + per[k] * int(r[9])) for r in records for k in range(8) if int(r[k]) != sr.INVALID)


def _frame_equals_reference(p, what, size=(48, 32)):
    """One frame; the mesh buffer afterwards is skin() of the buffer before it over the renderer's own records, whose matrix
    bases are the running sums of the stored counts."""
    records, mats = p.skinning_buffers()
    live = [sk for sk in p.skeletons if sk is not None]
    stored = [len(sk["matrices"]) for sk in live]
    assert records[:, 8].tolist() == [int(b) for b in np.concatenate([[0], np.cumsum(stored)[:-1]])], what
    assert len(mats) == sum(stored), what
    n = _extent(p)
    before = p.readback_mesh_words(0, n)
    want = sr.skin(before, records, mats)
    p.render(*size, readback=False)
    assert_same_words(p.readback_mesh_words(0, n), want, what)
    assert np.array_equal(p.readback_joint_matrices(), mats), what


@pytest.mark.parametrize("upload", ["append", "stream"])
def test_record_set_changes_between_frames(upload):
    import rend3_amd as r3
    p = r3.Renderer(oh.LEFT, f32(1.5), mesh_upload=upload)
    m2, m5 = _cylinder(p, 2), _cylinder(p, 5)
    mat = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    a, b = p.add_skeleton(m2, _pose(2, 1)), p.add_skeleton(m5, _pose(5, 2))
    p.add_object(None, mat, oh.translation((-0.6, 0.0, 0.0)), skeleton=a)
    _camera(p)
    _frame_equals_reference(p, "frame 1: two skeletons of different meshes")
    p.set_skeleton_joint_matrices(a, _pose(2, 3))
    p.set_skeleton_joint_matrices(b, _pose(5, 4))
    cached = p._skin_inputs
    _frame_equals_reference(p, "frame 2: matrices only")
    assert p._skin_inputs is cached  # the records were not rebuilt
    c = p.add_skeleton(m2, _pose(2, 5))
    p.add_object(None, mat, oh.translation((0.6, 0.0, 0.0)), skeleton=c)
    _frame_equals_reference(p, "frame 3: a third skeleton")
    assert p.skinning_buffers()[0][:, 8].tolist() == [0, 2, 7]
    if upload == "stream":
        p.remove_skeleton(b)
        _frame_equals_reference(p, "frame 4: the middle skeleton removed")
        assert p.skinning_buffers()[0][:, 8].tolist() == [0, 2]
    p.close()


def _runs(r, sk):
    s = r.skeletons[sk]
    n = 3 * r.meshes[s["mesh"]].vertex_count
    if hasattr(r, "mesh_words"):
        return [r.mesh_words[o // 4:o // 4 + n].copy() for o in s["out_off"]]
    return [r.readback_mesh_words(o, n) for o in s["out_off"]]


def _pair(aspect=1.5):
    import rend3_amd as r3
    o, p = OracleRenderer(oh.LEFT, f32(aspect)), r3.Renderer(oh.LEFT, f32(aspect))
    return o, p, ((o, omk), (p, r3.material_record))


def test_extra_matrices_do_not_shift_the_next_skeleton():
    """set_skeleton_joint_matrices with two matrices too many on the first of two skeletons: they are dropped, and the second
    skeleton still skins with its own matrices at its own base."""
    from test_gpu_parity import compare_frames
    o, p, both = _pair()
    sks = []
    for r, mk in both:
        mesh = _cylinder(r, 2)
        mat = r.add_material(mk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
        sks.append([r.add_skeleton(mesh, _ident(2)), r.add_skeleton(mesh, _ident(2))])
        for i, sk in enumerate(sks[-1]):
            r.add_object(None, mat, oh.translation((-0.6 + 1.2 * i, 0.0, 0.0)), skeleton=sk)
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -1.0, 0.4), distance=10.0, resolution=128)
        _camera(r)
    compare_frames(o.render(96, 64), p.render(96, 64), "bind pose")  # the records are cached from here on
    long, second = _pose(4, 11), _pose(2, 12)
    for r, (first_sk, second_sk) in zip((o, p), sks):
        r.set_skeleton_joint_matrices(first_sk, long)
        r.set_skeleton_joint_matrices(second_sk, second)
    fo, fp = o.render(96, 64), p.render(96, 64)
    for i in range(2):
        for x, y in zip(_runs(o, sks[0][i]), _runs(p, sks[1][i])):
            assert np.array_equal(x, y), f"skinned run of skeleton {i} differs from the oracle's"
    got = p.readback_joint_matrices()
    assert got.shape == (4, 16) and np.array_equal(got[:2], long[:2]) and np.array_equal(got[2:], second)
    assert p.skinning_buffers()[0][:, 8].tolist() == [0, 2]
    compare_frames(fo, fp, "after the long list")
    p.close()


class _NoCalls:
    """Stands in for the library while a call must be refused on the host: any C call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called by an edit that had to be refused first")


def _refused(p, match, fn, *args, **kw):
    lib, p.lib = p.lib, _NoCalls()
    try:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    finally:
        p.lib = lib


def _state(p):
    return (p.mesh_cursor, len(p.meshes), len(p.skeletons), p.mesh_stats()["blocks_live"],
            [None if sk is None else sk["matrices"].tobytes() for sk in p.skeletons], dict(p._pose_state))


@pytest.mark.parametrize("upload", ["append", "stream"])
def test_refusals_change_nothing_and_the_next_frame_equals_the_oracle(upload):
    import rend3_amd as r3
    import rend3_amd.anim as pa
    from test_anim import random_rig_case
    from test_gpu_parity import compare_frames
    o = OracleRenderer(oh.LEFT, f32(1.5))
    p = r3.Renderer(oh.LEFT, f32(1.5), mesh_upload=upload)
    sks = []
    for r, mk in ((o, omk), (p, r3.material_record)):
        mesh = _cylinder(r, 5)
        mat = r.add_material(mk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
        sk = r.add_skeleton(mesh, _pose(5, 21))
        r.add_object(None, mat, oh.identity(), skeleton=sk)
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -1.0, 0.4), distance=10.0, resolution=128)
        _camera(r)
        sks.append(sk)
    mesh, sk = 0, sks[1]
    inst, anim = random_rig_case(np.random.default_rng(0xB0A), 7)  # a rig of seven joints: two more than the skeleton stores
    inst["nodes"][0]["skin"], inst["nodes"][0]["skeletons"] = 0, []
    pa.AnimationData.from_gltf_scene(p, [anim], inst)
    before = _state(p)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=f32)
    _refused(p, "MissingAttributesJointWeights", p.add_mesh, tri, np.array([0, 1, 2], dtype=np.uint32), joint_indices=np.zeros((3, 4), dtype=np.uint16))
    _refused(p, r"NotEnoughJoints.* 5 joints.* 4 joint matrices", p.add_skeleton, mesh, _ident(4))
    _refused(p, r"NotEnoughJoints.* 5 joints.* 3 joint matrices", p.add_skeletons_bulk, mesh, [_ident(5), _ident(3), _ident(5)])
    _refused(p, r"stores 5 joint matrices.* 4 joint matrices", p.set_skeleton_joint_matrices, sk, _ident(4))
    _refused(p, r"7 joints.* stores only 5", p.pose_skeletons, [(0, 0.5, sk)])
    _refused(p, "does not exist", p.pose_skeletons, [(0, 0.5, len(p.skeletons))])
    assert _state(p) == before
    with pytest.raises(ValueError, match="NotEnoughJoints"):
        o.add_skeleton(0, _ident(4))
    with pytest.raises(ValueError, match="stores 5 joint matrices"):
        o.set_skeleton_joint_matrices(sks[0], _ident(4))
    fo, fp = o.render(96, 64), p.render(96, 64)
    for x, y in zip(_runs(o, sks[0]), _runs(p, sk)):
        assert np.array_equal(x, y)
    compare_frames(fo, fp, "the frame after the refusals")
    p.close()


def test_mfma_mode_refuses_rigs_of_more_than_four_matrices():
    """R3N_SKIN_MFMA takes a skeleton's joint count from the distance to the next matrix base: a 5-joint rig among legal ones is
    refused, and so is a 2-joint mesh whose skeleton was given 6 matrices -- the stored count is the given one, not the
    mesh's."""
    import rend3_amd as r3
    for second_joints, second_matrices in ((5, 5), (2, 6)):
        p = r3.Renderer(oh.LEFT, f32(1.5))
        m2, other = _cylinder(p, 2), _cylinder(p, second_joints)
        mat = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value"), 0)
        a = p.add_skeleton(m2, _pose(2, 31))
        p.add_skeleton(other, _pose(second_matrices, 32))
        p.add_skeleton(m2, _pose(2, 33))
        p.add_object(None, mat, oh.identity(), skeleton=a)
        _camera(p)
        p.set_skinning_mode(1)
        with pytest.raises(r3._ffi.R3nError, match="four joints"):
            p.render(48, 32, readback=False)
        p.close()


def test_a_pose_writes_its_own_skeleton_only():
    """Two skeletons; the first is posed by a clip whose rig has exactly the joints it stores.  The pose lands at its base and
    the second skeleton's matrices behind it are the ones it was given."""
    import rend3_amd as r3
    import rend3_amd.anim as pa
    import oracle.anim as oa
    from test_anim import random_rig_case
    inst, anim = random_rig_case(np.random.default_rng(0xB0B), 5)
    p = r3.Renderer(oh.LEFT, f32(1.5))
    mesh = _cylinder(p, 3)
    mat = p.add_material(r3.material_record(albedo=(1, 1, 1, 1)), 0)
    own = _pose(3, 41)
    first, second = p.add_skeleton(mesh, _ident(5)), p.add_skeleton(mesh, own)
    inst["nodes"][0]["skin"], inst["nodes"][0]["skeletons"] = 0, [first]
    data = pa.AnimationData.from_gltf_scene(p, [anim], inst)
    assert data.skin_skeletons == [[first]]
    with pytest.raises(ValueError, match=r"5 joints.* stores only 3"):
        p.pose_skeletons([(0, 0.3, first), (0, 0.3, second)])
    assert p._pose_state == {}  # the legal request of a refused call is not taken either
    p.pose_skeletons([(0, 0.3, first)])
    p.add_object(None, mat, oh.identity(), skeleton=first)
    p.add_object(None, mat, oh.translation((1.0, 0.0, 0.0)), skeleton=second)
    _camera(p)
    p.render(48, 32, readback=False)
    got = p.readback_joint_matrices()
    want = oa.pose_skin(anim, inst["skins"][0], inst["nodes"], inst["topological_order"], oa.clamp_time(anim, 0.3))
    assert got.shape == (8, 16)
    assert np.array_equal(got[:5].view(np.uint32), np.asarray(want, dtype=f32).reshape(5, 16).view(np.uint32))
    assert np.array_equal(got[5:], own)
    # and the second skeleton's skinned runs are skin() of its own matrices
    records, _mats = p.skinning_buffers()
    n = _extent(p)
    words = p.readback_mesh_words(0, n)
    assert_same_words(words, sr.skin(words, records, got), "skinned runs under the posed matrices")
    p.close()
