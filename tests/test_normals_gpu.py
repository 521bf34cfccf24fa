"""Recomputed normals on the GPU (r3n_vertex_normals, csrc/normals.hip).  The reference is oracle.host.calculate_normals -- the
restatement of the reference's serial loop -- applied to positions blended by tests/morph_reference.py; never the library's own
host function, never the kernel.  Everything is compared as u32 words; there is no tolerance.  Whole frames are compared with the
oracle, whose mesh words are overwritten before every frame with the reference-morphed positions AND the reference-recomputed
normals (the _OracleMorph pattern of tests/test_morph_gpu.py)."""
import argparse
import os

import numpy as np
import pytest

import morph_reference as MR
import normals_reference as NR
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd.scenes import Pcg32, skinned_cylinder

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 0xFFFFFFFF
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph-nonormal.glb")
R3N_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def _compare(fo, fp, tag):
    from test_gpu_parity import compare_frames
    compare_frames(fo, fp, tag)


def _words(a):
    return np.ascontiguousarray(a, dtype=f32).reshape(-1).view(np.uint32)


def _whole(idx):
    return idx[: 3 * (len(idx) // 3)]  # (the oracle's restatement reshapes to triangles; the remainder is no triangle)


def _reference(pos, targets, weights, idx, left_handed):
    """(morphed positions, their normals by the serial loop)"""
    morphed = MR.blend(pos, targets, weights)
    return morphed, oh.calculate_normals(morphed, _whole(idx), left_handed)


def _targets(rng, n_targets, pos, scale=0.2):
    """Position deltas of the positions' own magnitude per vertex (the soups span binades), so that every weight moves every normal."""
    mag = np.maximum(np.abs(pos).max(axis=1, keepdims=True), f32(2.0 ** -8))
    return (rng.uniform(-scale, scale, (n_targets,) + pos.shape) * mag).astype(f32)


# ------------------------------------------------------------------ G1 + G2. the runs, bit for bit, one launch
@pytest.fixture(scope="module")
def world(r3):
    """Every mesh of the set in both handednesses with two instances each (one with all-zero weights), a plain mesh behind the last
    run, ONE flush: the buffer before and after, the launch counts, the reference per instance."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x4E31))
    cases = []
    for name, pos, idx in NR.mesh_set():
        for hand in (oh.LEFT, oh.RIGHT):
            targets = _targets(rng, 2, pos)
            mesh = p.add_mesh(pos, idx, mesh_handedness=hand, morph_targets=dict(positions=targets, normals=None, tangents=None),
                              morph_normals="recompute")
            weights = [rng.uniform(-1.0, 1.5, 2).astype(f32), np.zeros(2, dtype=f32)]
            for h, w in zip(p.add_morph_instances_bulk(mesh, weights), weights):
                cases.append(dict(name=name, handle=h, mesh=mesh, pos=pos, idx=idx, targets=targets, weights=w, left=hand == oh.LEFT))
    canary = p.add_mesh(np.ones((4, 3), dtype=f32), np.array([0, 1, 2], dtype=np.uint32), normals=np.ones((4, 3), dtype=f32))
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    p._flush_morphs()
    times = p.stage_times()
    after = p.readback_mesh_words(0, p.mesh_cursor)
    for c in cases:
        c["ref_pos"], c["ref_nrm"] = _reference(c["pos"], c["targets"], c["weights"], c["idx"], c["left"])
    yield dict(p=p, cases=cases, before=before, after=after, times=times, canary=canary)
    p.close()


def test_runs_bit_exact_one_launch(world):
    """G1: ONE `normals` launch (and one `morph` launch) for all 56 instances; every instance's normal run equals the serial loop
    over the reference-morphed positions; no other word of the mesh buffer changed."""
    p, cases, before, after = world["p"], world["cases"], world["before"], world["after"]
    assert world["times"]["normals"][1] == 1 and world["times"]["morph"][1] == 1
    assert len(cases) == 56 and {len(c["pos"]) for c in cases} == {1, 3, 63, 64, 65, 130, 257}
    want = before.copy()
    differing_meshes = 0
    for c in cases:
        m, out = p.meshes[c["mesh"]], p.morphs[c["handle"]]["out_off"]
        assert out[0] != INVALID and out[1] != INVALID and out[2] == INVALID and out[1] % 16 == 0 and m.adjacency_off % 16 == 0
        n = 3 * len(c["pos"])
        for off, ref in ((out[0], c["ref_pos"]), (out[1], c["ref_nrm"])):
            assert not want[off // 4: off // 4 + n].any()  # (runs do not overlap: still zero-filled)
            want[off // 4: off // 4 + n] = _words(ref)
        got = after[out[1] // 4: out[1] // 4 + n]
        bad = int((got != _words(c["ref_nrm"])).sum())
        assert bad == 0, f"{c['name']} {'lh' if c['left'] else 'rh'} weights {c['weights']}: {bad} of {n} normal words differ"
        if c["weights"].any():
            differing_meshes += int(not np.array_equal(got, before[m.attr_off[1] // 4: m.attr_off[1] // 4 + n]))
    assert differing_meshes >= 20, "the morphed normals hardly differ from the base shape's: the test shows nothing"
    assert np.array_equal(after, want), "a word outside the output runs changed"


def test_zero_weights_give_the_mesh_normals(world):
    """G2: with all-zero weights the recomputed run is the run add_mesh computed for the base shape, bit for bit."""
    p, after = world["p"], world["after"]
    seen = 0
    for c in world["cases"]:
        if c["weights"].any():
            continue
        m, out = p.meshes[c["mesh"]], p.morphs[c["handle"]]["out_off"]
        n = 3 * len(c["pos"])
        assert np.array_equal(after[out[1] // 4: out[1] // 4 + n], after[m.attr_off[1] // 4: m.attr_off[1] // 4 + n]), c["name"]
        assert np.array_equal(after[m.attr_off[1] // 4: m.attr_off[1] // 4 + n], _words(oh.calculate_normals(c["pos"], _whole(c["idx"]), c["left"])))
        seen += 1
    assert seen == 28


# ------------------------------------------------------------------ G3. nothing when nothing changes
def test_no_launch_without_a_change(r3):
    rng = np.random.Generator(np.random.PCG64(0x4E33))
    p = r3.Renderer(oh.LEFT, f32(1.5))
    pos, idx = _facing_grid(rng)
    targets = _targets(rng, 2, pos)
    mesh = p.add_mesh(pos, idx, morph_targets=dict(positions=targets, normals=None, tangents=None), morph_normals="recompute")
    mat = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    insts = p.add_morph_instances_bulk(mesh, [[0.5, 0.0], [0.25, 1.0], None])
    for i, x in zip(insts, (-1.5, 0.0, 1.5)):
        p.add_object(None, mat, oh.translation((x, 1.0, 0.0)), morph=i)
    _light_and_camera(p)
    p.stage_times()
    p.render(96, 64)
    t = p.stage_times()
    assert t["morph"][1] == 1 and t["normals"][1] == 1  # the three new instances, one call each
    f1 = p.render(96, 64)
    t = p.stage_times()
    assert t["morph"][1] == 0 and t["normals"][1] == 0, "a frame without a weight change launched"
    before = p.readback_mesh_words(0, p.mesh_cursor)
    w = np.array([-0.5, 0.75], dtype=f32)
    p.set_morph_weights(insts[1], w)
    p._flush_morphs()
    t = p.stage_times()
    assert t["morph"][1] == 1 and t["normals"][1] == 1
    after = p.readback_mesh_words(0, p.mesh_cursor)
    want = before.copy()
    ref_pos, ref_nrm = _reference(pos, targets, w, idx, True)
    out = p.morphs[insts[1]]["out_off"]
    want[out[0] // 4: out[0] // 4 + ref_pos.size] = _words(ref_pos)
    want[out[1] // 4: out[1] // 4 + ref_nrm.size] = _words(ref_nrm)
    assert not np.array_equal(before, want) and np.array_equal(after, want), "the launch rewrote more than the changed instance's runs"
    f2 = p.render(96, 64)
    assert p.stage_times()["normals"][1] == 0 and not np.array_equal(f1["hdr16"], f2["hdr16"])
    p.close()


# ------------------------------------------------------------------ G4. rendered
def _light_and_camera(r):
    r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -1.0, 0.4), distance=10.0, resolution=256)
    r.set_camera_data(oh.look_at_lh((0, 1.2, -4), (0, 1, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))


class _OracleRecompute:
    """One morphed mesh WITHOUT normals on the oracle's side: add_mesh of the base shape (the oracle computes the base normals);
    apply() overwrites the position run with the reference's blend, the normal run with the serial loop over those positions, sets
    the mesh radius to radius' and refreshes the objects."""

    def __init__(self, o, pos, idx, targets, hand, **mesh_kw):
        self.o, self.pos, self.idx, self.targets, self.left = o, pos, idx, targets, hand == oh.LEFT
        self.mesh = o.add_mesh(pos, idx, normals=None, mesh_handedness=hand, **mesh_kw)
        self.radius = o.meshes[self.mesh].radius
        self.reach = MR.reach(targets)
        self.objects = []

    def apply(self, weights, recompute=True):
        m = self.o.meshes[self.mesh]
        morphed, normals = _reference(self.pos, self.targets, weights, self.idx, self.left)
        self.o.mesh_words[m.attr_off[0] // 4: m.attr_off[0] // 4 + morphed.size] = _words(morphed)
        if recompute:
            self.o.mesh_words[m.attr_off[1] // 4: m.attr_off[1] // 4 + normals.size] = _words(normals)
        m.radius = MR.radius(self.radius, weights, self.reach)
        for h in self.objects:
            self.o.set_object_transform(h, self.o.object_meta[h]["transform"])


def _facing_grid(rng):
    """A 13 x 10 grid facing the camera of _light_and_camera (wound so that its left-handed normals point to -z)."""
    pos, idx = NR.grid(rng, 13, 10)
    return pos, np.ascontiguousarray(idx.reshape(-1, 3)[:, ::-1]).reshape(-1)


def _pose(joints, seed):
    import scenes
    rng = Pcg32(seed)
    return np.array([oh.mat4_mul(oh.translation((rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2))),
                                 scenes.random_rotation(rng, oh)) for _ in range(joints)], dtype=f32)


def _rendered_pair(r3, recompute):
    """A grid bound directly to its morph instance and a skinned cylinder (added WITHOUT normals) bound through a skeleton, over a
    floor, one directional light with a 256^2 shadow view."""
    rng = np.random.Generator(np.random.PCG64(0x4E34))
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    mat_o = o.add_material(omk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    mat_p = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    kw = dict(morph_normals="recompute") if recompute else {}
    gpos, gidx = _facing_grid(rng)
    gt = _targets(rng, 2, gpos, scale=0.35)
    cpos, cidx, _nrm, _tang, ji, jw = skinned_cylinder(7)
    ct = rng.uniform(-0.12, 0.12, (3,) + cpos.shape).astype(f32)
    gm = p.add_mesh(gpos, gidx, morph_targets=dict(positions=gt, normals=None, tangents=None), **kw)
    cm = p.add_mesh(cpos, cidx, joint_indices=ji, joint_weights=jw, morph_targets=dict(positions=ct, normals=None, tangents=None), **kw)
    gi, ci = p.add_morph_instance(gm), p.add_morph_instance(cm)
    ident = np.tile(oh.identity(), (7, 1))
    sk_p = p.add_skeleton(cm, ident, morph=ci)
    xg, xc = oh.translation((-1.0, 1.2, 0.0)), oh.translation((1.0, 0.0, 0.0))
    p.add_object(None, mat_p, xg, morph=gi)
    p.add_object(None, mat_p, xc, skeleton=sk_p)
    og = _OracleRecompute(o, gpos, gidx, gt, oh.LEFT)
    oc = _OracleRecompute(o, cpos, cidx, ct, oh.LEFT, joint_indices=ji, joint_weights=jw)
    sk_o = o.add_skeleton(oc.mesh, ident)
    og.objects.append(o.add_object(og.mesh, mat_o, xg))
    oc.objects.append(o.add_object(None, mat_o, xc, skeleton=sk_o))
    for r in (o, p):
        floor = r.add_mesh([(-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4)], [0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2], normals=[(0, 1, 0)] * 4)
        r.add_object(floor, mat_o if r is o else mat_p, oh.identity())
        _light_and_camera(r)
    return dict(o=o, p=p, rng=rng, insts=(gi, ci), oracle=(og, oc), skeletons=(sk_p, sk_o), meshes=(gm, cm))


def _rendered_frame(s, f, samples, recompute=True):
    o, p, rng = s["o"], s["p"], s["rng"]
    for hp, om in zip(s["insts"], s["oracle"]):
        w = rng.uniform(-1.0, 1.6, om.targets.shape[0]).astype(f32)
        p.set_morph_weights(hp, w)
        om.apply(w, recompute)
        assert p.morph_radius(hp) == o.meshes[om.mesh].radius
    pose = _pose(7, 70 + f)
    p.set_skeleton_joint_matrices(s["skeletons"][0], pose)
    o.set_skeleton_joint_matrices(s["skeletons"][1], pose)
    kw = dict(samples=samples, ambient=(0.1, 0.1, 0.1, 1))
    return o.render(192, 128, **kw), p.render(192, 128, **kw)


def test_rendered_frames_match_the_oracle(r3):
    """G4: three frames, 192 x 128, weights and pose changing every frame, then one frame at samples = 4: sets, keys, atlas and HDR
    bit-identical to the oracle drawing reference-morphed positions with reference-recomputed normals; the skeleton skins from the
    instance's recomputed normal run."""
    s = _rendered_pair(r3, True)
    p = s["p"]
    sk_in, _m = p.skinning_buffers()
    assert list(sk_in[0, :3]) == p.morphs[s["insts"][1]]["out_off"] and sk_in[0, 1] != INVALID and sk_in[0, 2] == INVALID
    p.stage_times()
    frames = []
    for f, samples in enumerate((1, 1, 1, 4)):
        fo, fp = _rendered_frame(s, f, samples)
        assert p.stage_times()["normals"][1] == 1
        _compare(fo, fp, f"recomputed normals, frame {f}, samples {samples}")
        assert fo["pass"].sum() > 100 and (fo["atlas"] != 0).any()
        frames.append(fp)
        n = 3 * p.meshes[s["meshes"][1]].vertex_count  # the skinned normal run: the oracle's skinning of the recomputed normals
        want = s["o"].mesh_words[s["o"].skeletons[s["skeletons"][1]]["out_off"][1] // 4:][:n]
        assert np.array_equal(p.readback_mesh_words(p.skeletons[s["skeletons"][0]]["out_off"][1], n), want), f"frame {f}: skinned normals"
    assert not np.array_equal(frames[0]["hdr16"], frames[1]["hdr16"])
    p.close()


# ------------------------------------------------------------------ G5. errors
def test_argument_errors(r3):
    """Every validation rule of r3n_vertex_normals answers R3N_ERR_INVALID_ARG on the host with nothing launched and no word
    changed; a good call on the same context still succeeds; add_mesh refuses morph_normals="recompute" where it makes no sense."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x4E35))
    pos, idx = NR.grid(rng, 8, 8)
    pos = np.concatenate([pos, rng.uniform(-1, 1, (1, 3)).astype(f32)])  # V = 65
    targets = _targets(rng, 2, pos)
    mt = dict(positions=targets, normals=None, tangents=None)
    mesh = p.add_mesh(pos, idx, morph_targets=mt, morph_normals="recompute")
    w = np.array([0.5, -1.0], dtype=f32)
    inst = p.add_morph_instance(mesh, w)
    m, out = p.meshes[mesh], p.morphs[inst]["out_off"]
    names = ["position", "normal", "index", "index_count", "adjacency", "vertex_count", "left_handed", "pad"]
    good = np.array([out[0], out[1], 4 * m.first_index, m.index_count, m.adjacency_off, m.vertex_count, 1, 0], dtype=np.uint32)

    def call(rec):
        rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 8)
        return p.lib.r3n_vertex_normals(p.ctx, r3._ffi.ptr(rec), len(rec))

    def edit(**fields):
        rec = good.copy()
        for k, val in fields.items():
            rec[names.index(k)] = val
        return rec

    adjacency_words = m.vertex_count + 1 + m.index_count
    bad = {
        "position run outside the mesh buffer": edit(position=0xFFFFFF00),
        "normal run outside the mesh buffer": edit(normal=0xFFFFFF00),
        "index run outside the mesh buffer": edit(index=0xFFFFFF00),
        "index count past the mesh buffer": edit(index_count=0x7FFFFFFF),
        "adjacency run outside the mesh buffer": edit(adjacency=0xFFFFFF00),
        "position run not 4-byte aligned": edit(position=int(good[0]) + 2),
        "normal run not 4-byte aligned": edit(normal=int(good[1]) + 1),
        "index run not 4-byte aligned": edit(index=int(good[2]) + 3),
        "adjacency run not 4-byte aligned": edit(adjacency=int(good[4]) + 2),
        "no vertices": edit(vertex_count=0),
        "normal run overlaps the positions": edit(normal=int(good[0])),
        "normal run overlaps the positions' tail": edit(normal=int(good[0]) + 12 * (m.vertex_count - 1)),
        "normal run overlaps the indices": edit(normal=int(good[2]) + 4 * (m.index_count - 1)),
        "normal run overlaps the adjacency": edit(normal=int(good[4]) + 4 * (adjacency_words - 1)),
        "left_handed is 2": edit(left_handed=2),
    }
    p._flush_morphs()  # the instance's first evaluation, so that the rejected calls below leave a known state behind
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    for what, rec in bad.items():
        assert call(rec) == R3N_ERR_INVALID_ARG, what
        assert p.lib.r3n_last_error(p.ctx).decode().startswith("normals:"), what
        assert call(np.stack([good, rec])) == R3N_ERR_INVALID_ARG, what  # a bad record behind a good one rejects the whole call
    assert p.lib.r3n_vertex_normals(p.ctx, None, 1) == R3N_ERR_INVALID_ARG  # as r3n_morph answers NULL inputs
    assert p.stage_times()["normals"][1] == 0 and np.array_equal(p.readback_mesh_words(0, p.mesh_cursor), before)
    assert p.lib.r3n_vertex_normals(p.ctx, None, 0) == 0 and call(np.zeros((0, 8), dtype=np.uint32)) == 0  # no instances: R3N_OK
    assert p.stage_times()["normals"][1] == 0
    # a good call still works: the other handedness into the same run
    assert call(edit(left_handed=0)) == 0
    assert p.stage_times()["normals"][1] == 1
    _pos, ref = _reference(pos, targets, w, idx, False)
    assert np.array_equal(p.readback_mesh_words(out[1], ref.size), _words(ref))
    # add_mesh
    with pytest.raises(ValueError):
        p.add_mesh(pos, idx, normals=np.ones_like(pos), morph_targets=mt, morph_normals="recompute")  # explicit normals
    with pytest.raises(ValueError):
        p.add_mesh(pos, idx, morph_normals="recompute")                                               # no targets
    with pytest.raises(ValueError):
        p.add_mesh(pos, idx, morph_targets=dict(positions=targets, normals=targets, tangents=None), morph_normals="recompute")  # normal deltas
    with pytest.raises(ValueError):
        p.add_mesh(pos, idx, normals=None, morph_targets=dict(positions=None, normals=targets, tangents=None), morph_normals="recompute")
    with pytest.raises(ValueError):
        p.add_mesh(pos, idx, morph_targets=mt, morph_normals="always")
    cursor = p.mesh_cursor
    with pytest.raises(ValueError):  # an index past the vertices cannot be given an adjacency row
        p.add_mesh(pos, np.array([0, 1, 65], dtype=np.uint32), morph_targets=mt, morph_normals="recompute")
    assert p.mesh_cursor == cursor
    p.close()


# ------------------------------------------------------------------ G6. the default is unchanged
def test_default_keeps_the_base_normals(r3):
    """The same scene without the option: no private normal run, no `normals` launch, frames equal to the oracle drawing the
    reference-morphed positions with the BASE shape's normals."""
    s = _rendered_pair(r3, False)
    p = s["p"]
    for h, mesh in zip(s["insts"], s["meshes"]):
        assert p.morphs[h]["out_off"][1] == INVALID and p.morphs[h]["out_off"][0] != INVALID and p.meshes[mesh].adjacency_off == INVALID
    p.stage_times()
    for f in range(2):
        fo, fp = _rendered_frame(s, f, 1, recompute=False)
        t = p.stage_times()
        assert t["normals"][1] == 0 and t["morph"][1] == 1
        _compare(fo, fp, f"base normals, frame {f}")
        assert fo["pass"].sum() > 100
    p.close()


# ------------------------------------------------------------------ G7. the fixture through the scene-viewer harness
def test_fixture_through_the_scene_viewer(r3):
    """morph-nonormal.glb through scene_viewer.build with --morph-normals recompute, its `weights` animation at two times: product ==
    oracle over reference-morphed positions and reference-recomputed normals."""
    from rend3_amd import anim, gltf
    from rend3_amd import scene_viewer as sv
    ap = sv.add_arguments(argparse.ArgumentParser())
    ap.add_argument("file")
    settings = sv.settings_from(ap.parse_args(sv.normalize_argv([FIXTURE, "--morph-normals", "recompute", "--camera", "0,0.3,4,0,0"])))
    o, p = OracleRenderer(oh.RIGHT, f32(1.5)), r3.Renderer(oh.RIGHT, f32(1.5))
    info = sv.build(p, r3.host, r3.material_record, settings)
    inst, g = info["instance"], info["gltf"]
    assert len(inst["objects"]) == 2 and all(p.meshes[m].adjacency_off != INVALID for m in {p.morphs[h]["mesh"] for h in (0, 1)})
    assert all(p.morphs[n["morphs"][0]]["out_off"][1] != INVALID for n in inst["nodes"])
    prim = g.primitive(0, 0)
    rec, key = gltf.material_from_gltf(g, prim["material"], omk, o)
    mat = o.add_material(rec, key)
    nodes = []
    for ni in range(2):
        om = _OracleRecompute(o, prim["positions"], prim["indices"], prim["targets"]["positions"], oh.RIGHT)
        om.objects.append(o.add_object(om.mesh, mat, inst["node_transforms"][ni]))
        nodes.append(om)
    for r in (o, p):
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -0.4, -1.0), distance=10.0, resolution=256)
    o.set_camera_data(sv.camera_view(oh, settings["camera"]), sv.PROJECTION)
    animations = gltf.load_animations(g)
    data = anim.AnimationData.from_gltf_scene(p, animations, inst)
    frames = []
    p.stage_times()
    for t in (0.3, 1.0):
        anim.pose_animation_frame(p, inst, data, 0, t)
        for ni, om in enumerate(nodes):  # the oracle's side samples the channels itself
            om.apply(anim.sample_morph_weights(animations[0]["morph_channels"][ni], f32(t)))
        kw = dict(samples=info["samples"], ambient=info["ambient"], clear_color=info["clear"])
        fo, fp = o.render(192, 128, **kw), p.render(192, 128, **kw)
        assert p.stage_times()["normals"][1] == 1
        _compare(fo, fp, f"fixture, recomputed normals, t = {t}")
        assert fo["pass"].sum() > 100
        frames.append(fp)
    assert not np.array_equal(frames[0]["hdr16"], frames[1]["hdr16"])
    p.close()
