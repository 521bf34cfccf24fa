"""Morph targets on the GPU (r3n_morph, csrc/morph.hip) against the numpy restatement of the contract (tests/morph_reference.py):
the blended runs bit for bit, and whole frames against the oracle rendering geometry that was morphed by the reference.  The
oracle has no morph stage (neither has the project it restates): its mesh words are overwritten with the reference-morphed
attributes and its mesh radius with the contract's radius' before every frame."""
import os

import numpy as np
import pytest

import morph_reference as MR
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd.scenes import Pcg32, skinned_cylinder

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 0xFFFFFFFF
KEYS = ("positions", "normals", "tangents")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph-plane.glb")


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def _compare(fo, fp, tag):
    from test_gpu_parity import compare_frames
    compare_frames(fo, fp, tag)


def _deltas(rng, n_targets, n_vertices, keys, scale=0.15):
    return {k: (rng.uniform(-scale, scale, (n_targets, n_vertices, 3)).astype(f32) if k in keys else None) for k in KEYS}


class _OracleMorph:
    """One morphed mesh on the oracle's side: add_mesh of the base shape; apply() overwrites the morphed attribute runs with the
    reference's blend of `weights`, sets the mesh radius to radius' and refreshes the objects through set_object_transform."""

    def __init__(self, o, base, targets, **mesh_kw):
        self.o, self.base, self.targets = o, base, targets
        self.mesh = o.add_mesh(base["positions"], base["indices"], normals=base["normals"], tangents=base.get("tangents"), **mesh_kw)
        self.radius = o.meshes[self.mesh].radius
        self.reach = MR.reach(targets["positions"]) if targets["positions"] is not None else None
        self.objects = []

    def apply(self, weights):
        m = self.o.meshes[self.mesh]
        for a, k in enumerate(KEYS):
            if self.targets[k] is not None:
                out = MR.blend(np.asarray(self.base[k], dtype=f32).reshape(-1, 3), self.targets[k], weights)
                self.o.mesh_words[m.attr_off[a] // 4: m.attr_off[a] // 4 + out.size] = out.reshape(-1).view(np.uint32)
        if self.reach is not None:
            m.radius = MR.radius(self.radius, weights, self.reach)
        for h in self.objects:
            self.o.set_object_transform(h, self.o.object_meta[h]["transform"])


# ------------------------------------------------------------------ 1. the runs, bit for bit
POOL = np.array([0.0, -0.0, -0.75, 1.5, 0.3, 2.25, -1.0, 0.0, 1.0], dtype=f32)


def test_runs_bit_exact_one_call_many_instances(r3):
    """Eighteen meshes -- V in {1, 63, 64, 65, 130, 257} x T in {1, 3, 9}, deltas on P, P+N or P+N+T -- with two instances each,
    evaluated by ONE r3n_morph call: every output run equals the reference as u32 words and no other word of the mesh buffer
    changed (in particular the words in front of and behind every output run)."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x4D30))
    subsets = [KEYS[:1], KEYS[:2], KEYS[:3]]
    cases, k = [], 0
    for v in (1, 63, 64, 65, 130, 257):
        for t in (1, 3, 9):
            keys = subsets[(k + k // 3) % 3]
            k += 1
            base = {key: rng.uniform(-2.0, 2.0, (v, 3)).astype(f32) for key in KEYS}
            base["positions"][0, 0] = -0.0  # a -0.0 word of a base run survives a copy
            targets = _deltas(rng, t, v, keys)
            mesh = p.add_mesh(base["positions"], np.zeros(3, dtype=np.uint32), normals=base["normals"], tangents=base["tangents"],
                              morph_targets=targets)
            assert np.array_equal(p.meshes[mesh].reach, MR.reach(targets["positions"]))
            weights = [rng.choice(POOL, t).astype(f32), rng.choice(POOL, t).astype(f32)]
            if t == 1:
                weights = [np.array([1.5], dtype=f32), np.array([-0.0], dtype=f32)]
            if t == 9:
                weights[0] = np.array([0.0, -0.75, -0.0, 1.5, 0.0, 2.25, 0.3, -1.0, 1.0], dtype=f32)  # zeros, negatives, > 1, -0.0: 6 terms
            for h, w in zip(p.add_morph_instances_bulk(mesh, weights), weights):
                cases.append((h, mesh, base, targets, keys, w))
    p.add_mesh(np.zeros((4, 3), dtype=f32), np.zeros(3, dtype=np.uint32), normals=np.zeros((4, 3), dtype=f32))  # words behind the last run
    subset_by_t = {(len(c[5]), c[4]) for c in cases}
    assert len({s for _t, s in subset_by_t}) == 3 and len(subset_by_t) > 3
    offsets = [p.meshes[c[1]].attr_off[a] for c in cases for a in range(len(c[4]))]
    assert any(off % 16 != 0 for off in offsets), "no base run that is 4- but not 16-byte aligned"
    assert all(off % 16 == 0 for c in cases for off in p.morphs[c[0]]["out_off"] if off != INVALID)
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    p._flush_morphs()
    assert p.stage_times()["morph"][1] == 1, "one launch for all instances of the call"
    after = p.readback_mesh_words(0, p.mesh_cursor)
    want = before.copy()
    for h, mesh, base, targets, keys, w in cases:
        out_off = p.morphs[h]["out_off"]
        for a, key in enumerate(KEYS):
            if key not in keys:
                assert out_off[a] == INVALID  # an attribute without deltas is not copied
                continue
            ref = MR.blend(base[key], targets[key], w).reshape(-1).view(np.uint32)
            assert not want[out_off[a] // 4: out_off[a] // 4 + ref.size].any()  # (runs do not overlap: still zero-filled)
            want[out_off[a] // 4: out_off[a] // 4 + ref.size] = ref
            got = after[out_off[a] // 4: out_off[a] // 4 + ref.size]
            assert np.array_equal(got, ref), f"V={len(base[key])} T={len(w)} {key}: {int((got != ref).sum())} of {ref.size} words differ"
    assert np.array_equal(after, want), "a word outside the output runs changed"
    # all-zero weights: the base, bit for bit, -0.0 included
    h, mesh, base, _t, _k, w = next(c for c in cases if len(c[5]) == 1 and not c[5].any())
    got = p.readback_mesh_words(p.morphs[h]["out_off"][0], base["positions"].size)
    assert np.array_equal(got, base["positions"].reshape(-1).view(np.uint32)) and got[0] == 0x80000000
    p.close()


# ------------------------------------------------------------------ 2. rendered
def _cylinder_base():
    pos, idx, nrm, tang, ji, jw = skinned_cylinder(7)
    return dict(positions=pos, indices=idx, normals=nrm, tangents=tang), ji, jw


def _light_and_camera(r):
    r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -1.0, 0.4), distance=10.0, resolution=256)
    r.set_camera_data(oh.look_at_lh((0, 1.2, -4), (0, 1, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def test_rendered_frames_match_the_oracle(r3):
    """Three frames, 192 x 128, one directional light with a 256^2 shadow view, two morph instances of one mesh (P+N+T deltas) and
    one of another (P only), weights changing every frame: sets, keys, atlas and HDR bit-identical to the oracle."""
    base, _ji, _jw = _cylinder_base()
    rng = np.random.Generator(np.random.PCG64(0x4D31))
    n = len(base["positions"])
    targets = [_deltas(rng, 3, n, KEYS), _deltas(rng, 2, n, KEYS[:1], scale=0.3)]
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    mat_o = o.add_material(omk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    mat_p = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    layout = [(0, -1.2), (0, 0.0), (1, 1.2)]  # (target set, x)
    meshes_p = [p.add_mesh(base["positions"], base["indices"], normals=base["normals"], tangents=base["tangents"], morph_targets=t)
                for t in targets]
    inst_p, inst_o = [], []
    for which, x in layout:
        inst_p.append(p.add_morph_instance(meshes_p[which]))
        p.add_object(None, mat_p, oh.translation((x, 0.0, 0.0)), morph=inst_p[-1])
        om = _OracleMorph(o, base, targets[which])
        om.objects.append(o.add_object(om.mesh, mat_o, oh.translation((x, 0.0, 0.0))))
        inst_o.append(om)
    for r in (o, p):  # a floor under them, to catch the shadows
        floor = r.add_mesh([(-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4)], [0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2], normals=[(0, 1, 0)] * 4)
        r.add_object(floor, mat_o if r is o else mat_p, oh.identity())
        _light_and_camera(r)
    for f in range(3):
        for i, (which, _x) in enumerate(layout):
            w = rng.uniform(-1.0, 1.6, targets[which]["positions"].shape[0]).astype(f32)
            if (f + i) % 3 == 0:
                w[0] = 0.0
            p.set_morph_weights(inst_p[i], w)
            inst_o[i].apply(w)
            assert p.morph_radius(inst_p[i]) == o.meshes[inst_o[i].mesh].radius
        fo, fp = o.render(192, 128, ambient=(0.1, 0.1, 0.1, 1)), p.render(192, 128, ambient=(0.1, 0.1, 0.1, 1))
        _compare(fo, fp, f"morphed frame {f}")
        assert fo["pass"].sum() > 0 and (fo["atlas"] != 0).any()
    p.close()


# ------------------------------------------------------------------ 3. morph, then skin
def _pose(joints, seed):
    import scenes
    rng = Pcg32(seed)
    return np.array([oh.mat4_mul(oh.translation((rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2))),
                                 scenes.random_rotation(rng, oh)) for _ in range(joints)], dtype=f32)


def test_morph_then_skin(r3):
    """skinned_cylinder with seeded deltas, 7 joints, two skeleton instances with their own weights and poses: the skinned runs are
    bit-identical to the oracle's skinning of the reference-morphed base, and the frames compare equal."""
    base, ji, jw = _cylinder_base()
    rng = np.random.Generator(np.random.PCG64(0x4D32))
    targets = _deltas(rng, 3, len(base["positions"]), KEYS)
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    mat_o = o.add_material(omk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    mat_p = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    mesh_p = p.add_mesh(base["positions"], base["indices"], normals=base["normals"], tangents=base["tangents"], joint_indices=ji,
                        joint_weights=jw, morph_targets=targets)
    ident = np.tile(oh.identity(), (7, 1))
    rigs = []
    for i, x in enumerate((-0.8, 0.8)):
        mi = p.add_morph_instance(mesh_p)
        sk_p = p.add_skeleton(mesh_p, ident, morph=mi)
        p.add_object(None, mat_p, oh.translation((x, 0.0, 0.0)), skeleton=sk_p)
        om = _OracleMorph(o, base, targets, joint_indices=ji, joint_weights=jw)
        sk_o = o.add_skeleton(om.mesh, ident)
        om.objects.append(o.add_object(None, mat_o, oh.translation((x, 0.0, 0.0)), skeleton=sk_o))
        rigs.append((mi, sk_p, om, sk_o))
    sk_in, _m = p.skinning_buffers()
    for i, (mi, _sk, _om, _so) in enumerate(rigs):  # the skeleton skins from the morph instance's outputs
        assert list(sk_in[i, :3]) == p.morphs[mi]["out_off"]
    for r in (o, p):
        _light_and_camera(r)
    n = 3 * len(base["positions"])
    for f in range(2):
        for i, (mi, sk_p, om, sk_o) in enumerate(rigs):
            w = rng.uniform(-0.8, 1.4, 3).astype(f32)
            pose = _pose(7, 50 * f + i)
            p.set_morph_weights(mi, w)
            p.set_skeleton_joint_matrices(sk_p, pose)
            om.apply(w)
            o.set_skeleton_joint_matrices(sk_o, pose)
        fo, fp = o.render(192, 128, ambient=(0.1, 0.1, 0.1, 1)), p.render(192, 128, ambient=(0.1, 0.1, 0.1, 1))
        for i, (_mi, sk_p, _om, sk_o) in enumerate(rigs):
            for a in range(3):
                want = o.mesh_words[o.skeletons[sk_o]["out_off"][a] // 4:][:n]
                got = p.readback_mesh_words(p.skeletons[sk_p]["out_off"][a], n)
                assert np.array_equal(got, want), f"frame {f} skeleton {i} {KEYS[a]}: skinned run differs"
        _compare(fo, fp, f"morph + skin frame {f}")
        assert fo["pass"].sum() > 0
    p.close()


# ------------------------------------------------------------------ 4. bounds
def test_bounds_follow_the_weights(r3):
    """A quad wholly outside the frustum whose one target moves it to the centre: drawn at weight 1 (the sphere grew by |w| reach),
    culled at weight 0 -- in the product and in the oracle given the contract's radius'."""
    base = dict(positions=np.array([(49.5, -0.5, 0.0), (50.5, -0.5, 0.0), (50.5, 0.5, 0.0), (49.5, 0.5, 0.0)], dtype=f32),
                indices=np.array([0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2], dtype=np.uint32), normals=np.array([(0.0, 0.0, -1.0)] * 4, dtype=f32))
    targets = dict(positions=np.tile(np.array([-50.0, 0.0, 0.0], dtype=f32), (1, 4, 1)), normals=None, tangents=None)
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    mesh = p.add_mesh(base["positions"], base["indices"], normals=base["normals"], morph_targets=targets)
    assert list(p.meshes[mesh].reach) == [50.0]
    inst = p.add_morph_instance(mesh)
    hp = p.add_object(None, p.add_material(r3.material_record(albedo=(0.9, 0.2, 0.2, 1.0), albedo_mode="value", unlit=True), 0), oh.identity(), morph=inst)
    om = _OracleMorph(o, base, targets)
    ho = o.add_object(om.mesh, o.add_material(omk(albedo=(0.9, 0.2, 0.2, 1.0), albedo_mode="value", unlit=True), 0), oh.identity())
    om.objects.append(ho)
    assert hp == ho
    for r in (o, p):
        r.set_camera_data(oh.look_at_lh((0, 0, -4), (0, 0, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    for f, (w, drawn) in enumerate([(1.0, True), (0.0, False), (1.0, True)]):
        p.set_morph_weights(inst, [w])
        om.apply(np.array([w], dtype=f32))
        fo, fp = o.render(192, 128), p.render(192, 128)
        _compare(fo, fp, f"bounds frame {f} weight {w}")
        assert bool(fp["visible"][hp]) == drawn and bool(fo["visible"][ho]) == drawn
        assert (fp["pass"].sum() > 0) == drawn and ((fp["vis"] != 0).sum() > 50) == drawn
    p.close()


# ------------------------------------------------------------------ 5. nothing when nothing changes
def test_no_launch_without_a_change(r3):
    base, _ji, _jw = _cylinder_base()
    rng = np.random.Generator(np.random.PCG64(0x4D33))
    p = r3.Renderer(oh.LEFT, f32(1.5))
    mesh = p.add_mesh(base["positions"], base["indices"], normals=base["normals"], tangents=base["tangents"],
                      morph_targets=_deltas(rng, 2, len(base["positions"]), KEYS[:2]))
    mat = p.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5), 0)
    insts = p.add_morph_instances_bulk(mesh, [[0.5, 0.0], None])
    for i, x in zip(insts, (-0.7, 0.7)):
        p.add_object(None, mat, oh.translation((x, 0.0, 0.0)), morph=i)
    _light_and_camera(p)
    p.stage_times()
    p.render(192, 128)
    assert p.stage_times()["morph"][1] == 1  # both new instances, one call
    p.set_morph_weights(insts[1], [0.25, -0.5])
    f1 = p.render(192, 128)
    assert p.stage_times()["morph"][1] == 1  # the changed instance alone
    f2 = p.render(192, 128)
    assert p.stage_times()["morph"][1] == 0, "a frame without a weight change launched the morph kernel"
    for k in ("vis", "hdr16", "rgba8", "atlas"):
        assert np.array_equal(f1[k], f2[k]), k
    p.close()
    # a renderer without morph instances never calls it
    q = r3.Renderer(oh.LEFT, f32(1.5))
    q.add_object(q.add_mesh(base["positions"], base["indices"], normals=base["normals"]),
                 q.add_material(r3.material_record(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value"), 0), oh.identity())
    _light_and_camera(q)
    for _ in range(2):
        q.render(96, 64)
        assert q.stage_times()["morph"][1] == 0
    q.close()


# ------------------------------------------------------------------ 6. the fixture, animated
def _fixture_pair(r3, make_product):
    """(oracle, product, per-node oracle meshes, instance, animation data): morph-plane.glb instanced by the product's loader;
    on the oracle's side one base mesh per node, to be morphed by the reference."""
    from rend3_amd import anim, gltf
    g = gltf.Gltf(FIXTURE)
    o, p = OracleRenderer(oh.RIGHT, f32(1.5)), make_product()
    inst = gltf.instance_scene(g, p, r3.host, r3.material_record)
    assert len(inst["objects"]) == 2 and inst["nodes"][0]["morphs"] and inst["nodes"][1]["morphs"]
    prim = g.primitive(0, 0)
    rec, key = gltf.material_from_gltf(g, prim["material"], omk, o)
    mat = o.add_material(rec, key)
    nodes = []
    for ni in range(2):
        om = _OracleMorph(o, prim, prim["targets"])
        om.objects.append(o.add_object(om.mesh, mat, inst["node_transforms"][ni]))
        nodes.append(om)
    for r in (o, p):
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -0.4, -1.0), distance=10.0, resolution=256)
        r.set_camera_data(oh.look_at_rh((0.0, 0.3, 4.0), (0, 0, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))
    animations = gltf.load_animations(g)
    return o, p, nodes, inst, anim.AnimationData.from_gltf_scene(p, animations, inst), animations


def _fixture_frame(o, p, nodes, inst, data, animations, t):
    from rend3_amd import anim
    anim.pose_animation_frame(p, inst, data, 0, t)
    tc = min(max(f32(t), f32(0.0)), animations[0]["duration"])
    for ni, om in enumerate(nodes):  # the oracle's side samples the channels itself
        om.apply(anim.sample_morph_weights(animations[0]["morph_channels"][ni], tc))
    kw = dict(ambient=(0.1, 0.1, 0.1, 1), clear_color=(0.02, 0.03, 0.05, 1.0))
    return o.render(192, 128, **kw), p.render(192, 128, **kw)


def test_fixture_animated(r3, monkeypatch):
    """morph-plane.glb through instance_scene and pose_animation_frame at three times, one past the end: product == oracle over the
    reference-morphed geometry.  Then once more on a renderer created under R3N_FRAME_NODES=1 (the per-node graph path, with the
    Morph node in front of Skinning; the switch is read when the renderer is created, as in test_runtime_switches): same bytes."""
    made = _fixture_pair(r3, lambda: r3.Renderer(oh.RIGHT, f32(1.5)))
    o, p, nodes = made[0], made[1], made[2]
    # before any animation: the file's own weights, node over mesh
    assert list(p.morphs[made[3]["nodes"][0]["morphs"][0]]["weights"]) == [0.25, 0.0, 0.5]
    assert list(p.morphs[made[3]["nodes"][1]["morphs"][0]]["weights"]) == [0.0, 1.0, 0.25]
    frames = {}
    for t in (0.0, 0.6, 5.0):
        fo, fp = _fixture_frame(*made, t)
        _compare(fo, fp, f"fixture t = {t}")
        assert fo["pass"].sum() > 100
        frames[t] = fp
    assert not np.array_equal(frames[0.0]["vis"], frames[0.6]["vis"])
    p.close()
    monkeypatch.setenv("R3N_FRAME_NODES", "1")
    made = _fixture_pair(r3, lambda: r3.Renderer(oh.RIGHT, f32(1.5)))
    assert made[1].frame_nodes
    for t in (0.0, 0.6):
        fo, fp = _fixture_frame(*made, t)
        _compare(fo, fp, f"fixture, node by node, t = {t}")
        for k in ("vis", "hdr16", "rgba8", "atlas"):
            assert np.array_equal(fp[k], frames[t][k]), k
    made[1].close()


# ------------------------------------------------------------------ 7. errors
def test_argument_errors(r3):
    """Every validation rule of r3n_morph answers R3N_ERR_INVALID_ARG on the host (nothing is launched: the launch count stays 0),
    and a good call on the same context still succeeds."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x4D34))
    v = 65
    base = {key: rng.uniform(-1, 1, (v, 3)).astype(f32) for key in KEYS}
    targets = _deltas(rng, 3, v, KEYS[:2])
    mesh = p.add_mesh(base["positions"], np.zeros(3, dtype=np.uint32), normals=base["normals"], tangents=base["tangents"], morph_targets=targets)
    inst = p.add_morph_instance(mesh, [0.5, -1.0, 2.0])
    m, out = p.meshes[mesh], p.morphs[inst]["out_off"]
    good = np.array([m.attr_off[0], m.attr_off[1], INVALID, m.delta_off[0], m.delta_off[1], INVALID, out[0], out[1], INVALID, 0, 3, v], dtype=np.uint32)
    weights = np.array([0.5, -1.0, 2.0], dtype=f32)

    def call(rec, w=weights):
        rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 12)
        return p.lib.r3n_morph(p.ctx, r3._ffi.ptr(rec), len(rec), r3._ffi.ptr(w), len(w))

    def edit(**fields):
        names = ["bp", "bn", "bt", "dp", "dn", "dt", "up", "un", "ut", "weight_base", "n_targets", "vertex_count"]
        rec = good.copy()
        for k, val in fields.items():
            rec[names.index(k)] = val
        return rec

    bad = {
        "output run outside the mesh buffer": edit(up=0xFFFFFF00),
        "delta run outside the mesh buffer": edit(dn=0xFFFFFF00),
        "base run not 4-byte aligned": edit(bp=int(good[0]) + 2),
        "output run not 4-byte aligned": edit(un=int(good[7]) + 1),
        "delta without its base": edit(bp=INVALID),
        "delta without its output": edit(un=INVALID),
        "base without a delta": edit(bt=m.attr_off[2]),
        "output without a delta": edit(ut=int(good[6])),
        "weights past the array": edit(weight_base=1),
        "no targets": edit(n_targets=0),
        "too many targets": edit(n_targets=r3._ffi.MAX_MORPH_TARGETS + 1),
        "output overlaps its base": edit(up=int(good[0])),
        "output overlaps its deltas": edit(un=int(good[4]) + 12 * v),
        "nothing morphed": edit(bp=INVALID, bn=INVALID, dp=INVALID, dn=INVALID, up=INVALID, un=INVALID),
    }
    p._flush_morphs()  # the instance's first evaluation, so that the rejected calls below leave a known state behind
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    for what, rec in bad.items():
        assert call(rec) == -1, what  # R3N_ERR_INVALID_ARG
        assert p.lib.r3n_last_error(p.ctx).decode().startswith("morph:"), what
        # a bad record behind a good one rejects the whole call
        assert call(np.stack([good, rec])) == -1, what
    big = np.zeros(r3._ffi.MAX_MORPH_TARGETS + 1, dtype=f32)
    assert call(edit(n_targets=r3._ffi.MAX_MORPH_TARGETS + 1), big) == -1
    assert p.lib.r3n_morph(p.ctx, r3._ffi.ptr(good), 1, None, 3) == -1 and p.lib.r3n_morph(p.ctx, None, 1, r3._ffi.ptr(weights), 3) == -1
    assert p.stage_times()["morph"][1] == 0 and np.array_equal(p.readback_mesh_words(0, p.mesh_cursor), before)
    assert p.lib.r3n_morph(p.ctx, None, 0, None, 0) == 0  # no instances: R3N_OK, nothing launched
    assert p.stage_times()["morph"][1] == 0
    # and a good call still works
    w2 = np.array([-0.25, 0.0, 1.0], dtype=f32)
    assert call(good, w2) == 0
    assert p.stage_times()["morph"][1] == 1
    for a in range(2):
        ref = MR.blend(base[KEYS[a]], targets[KEYS[a]], w2).reshape(-1).view(np.uint32)
        assert np.array_equal(p.readback_mesh_words(out[a], ref.size), ref)
    p.close()
