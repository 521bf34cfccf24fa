"""Generated tangents on the GPU (r3n_vertex_tangents, csrc/tangents.hip) and through Renderer.add_mesh(build_tangents=,
morph_tangents=).  The reference everywhere is tangents_reference.serial -- the line-by-line restatement of the reference's loop --
over positions blended by tests/morph_reference.py and normals from oracle.host.calculate_normals of those positions (or the mesh's
own where they are not recomputed); never the library's own host function, never the kernel.  Everything is compared as u32 words;
there is no tolerance.  Whole frames are compared with the oracle, whose mesh words are overwritten before every frame with the
reference's positions, normals AND tangents (the _OracleMorph pattern of tests/test_morph_gpu.py, extended by the tangent run)."""
import os

import numpy as np
import pytest

import morph_reference as MR
import normals_reference as NR
import tangents_reference as TR
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd.scenes import Pcg32, skinned_cylinder

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 0xFFFFFFFF
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph-notangent.glb")
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
    return idx[: 3 * (len(idx) // 3)]  # (the oracle's normals restatement reshapes to triangles; the remainder is no triangle)


def _reference(pos, targets, weights, idx, uv, left=True, given=None):
    """(morphed positions, their normals -- the serial loop's, or `given` -- and the serial tangents over both)"""
    morphed = MR.blend(pos, targets, weights)
    normals = oh.calculate_normals(morphed, _whole(idx), left) if given is None else given
    return morphed, normals, TR.serial(morphed, normals, uv, idx)


def _targets(rng, n_targets, pos, scale=0.2):
    """Position deltas of the positions' own magnitude per vertex (the soups span binades), so that every weight moves every tangent."""
    mag = np.maximum(np.abs(pos).max(axis=1, keepdims=True), f32(2.0 ** -8))
    return (rng.uniform(-scale, scale, (n_targets,) + pos.shape) * mag).astype(f32)


def _mt(targets):
    return dict(positions=targets, normals=None, tangents=None)


def _run(words, off, n):
    return words[off // 4: off // 4 + n]


# ------------------------------------------------------------------ G1 + G2. the runs, bit for bit, one launch
@pytest.fixture(scope="module")
def world(r3):
    """Every mesh of the set twice -- normals recomputed, normals given -- with two instances each (one with all-zero weights), a
    plain mesh behind the last run, ONE flush: the buffer before and after, the launch counts, the reference per instance."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x5431))
    cases = []
    for name, pos, idx, uv in TR.mesh_set():
        for given in (None, TR.unit_normals(rng, len(pos))):
            targets = _targets(rng, 2, pos)
            kw = dict(morph_normals="recompute") if given is None else dict(normals=given)
            mesh = p.add_mesh(pos, idx, uv0=uv, morph_targets=_mt(targets), build_tangents=True, morph_tangents="recompute", **kw)
            weights = [rng.uniform(-1.0, 1.5, 2).astype(f32), np.zeros(2, dtype=f32)]
            for h, w in zip(p.add_morph_instances_bulk(mesh, weights), weights):
                cases.append(dict(name=name, handle=h, mesh=mesh, pos=pos, idx=idx, uv=uv, targets=targets, weights=w, given=given))
    canary = p.add_mesh(np.ones((4, 3), dtype=f32), np.array([0, 1, 2], dtype=np.uint32), normals=np.ones((4, 3), dtype=f32))
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    p._flush_morphs()
    times = p.stage_times()
    after = p.readback_mesh_words(0, p.mesh_cursor)
    for c in cases:
        c["ref_pos"], c["ref_nrm"], c["ref_tan"] = _reference(c["pos"], c["targets"], c["weights"], c["idx"], c["uv"], given=c["given"])
    yield dict(p=p, cases=cases, before=before, after=after, times=times, canary=canary)
    p.close()


def test_runs_bit_exact_one_launch(world):
    """G1: ONE `morph`, ONE `normals` and ONE `tangents` launch for all 56 instances; every private tangent run equals the serial
    loop over the reference's positions and normals; no other word of the mesh buffer changed."""
    p, cases, before, after = world["p"], world["cases"], world["before"], world["after"]
    assert world["times"]["morph"][1] == 1 and world["times"]["normals"][1] == 1 and world["times"]["tangents"][1] == 1
    assert len(cases) == 56 and {len(c["pos"]) for c in cases} == {1, 3, 63, 64, 65, 130, 257}
    want = before.copy()
    moving, differing, adjacencies = 0, 0, set()
    for c in cases:
        m, out = p.meshes[c["mesh"]], p.morphs[c["handle"]]["out_off"]
        assert out[0] != INVALID and out[2] != INVALID and out[2] % 16 == 0 and m.adjacency_off % 16 == 0
        assert (out[1] != INVALID) == (c["given"] is None)
        adjacencies.add(m.adjacency_off)
        n = 3 * len(c["pos"])
        runs = [(out[0], c["ref_pos"]), (out[2], c["ref_tan"])] + ([(out[1], c["ref_nrm"])] if c["given"] is None else [])
        for off, ref in runs:
            assert not _run(want, off, n).any()  # (runs do not overlap: still zero-filled)
            want[off // 4: off // 4 + n] = _words(ref)
        got = _run(after, out[2], n)
        bad = int((got != _words(c["ref_tan"])).sum())
        kind = "normals recomputed" if c["given"] is None else "normals given"
        assert bad == 0, f"{c['name']}, {kind}, weights {c['weights']}: {bad} of {n} tangent words differ"
        assert np.isfinite(got.view(f32)).all()
        if c["weights"].any():
            moving += 1
            differing += int(not np.array_equal(got, _run(before, m.attr_off[2], n)))
    assert len(adjacencies) == 28  # one adjacency per mesh, shared by the normals and the tangents kernel
    print(f"{differing} of {moving} instances with non-zero weights have tangents other than the bind shape's")
    assert moving == 28 and differing >= moving // 2, "the morphed tangents hardly differ from the base shape's: the test shows nothing"
    assert np.array_equal(after, want), "a word outside the output runs changed"


def test_zero_weights_give_the_mesh_tangents(world):
    """G2: with all-zero weights the private run is the run add_mesh built on the host for the base shape, which is serial()."""
    p, after = world["p"], world["after"]
    seen = 0
    for c in world["cases"]:
        if c["weights"].any():
            continue
        m, out = p.meshes[c["mesh"]], p.morphs[c["handle"]]["out_off"]
        n = 3 * len(c["pos"])
        assert m.attr_off[2] != INVALID
        assert np.array_equal(_run(after, out[2], n), _run(after, m.attr_off[2], n)), c["name"]
        normals = oh.calculate_normals(c["pos"], _whole(c["idx"]), True) if c["given"] is None else c["given"]
        assert np.array_equal(_run(after, m.attr_off[2], n), _words(TR.serial(c["pos"], normals, c["uv"], c["idx"]))), c["name"]
        seen += 1
    assert seen == 28


# ------------------------------------------------------------------ scenes
def _light_and_camera(r):
    r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -1.0, 0.4), distance=10.0, resolution=256)
    r.set_camera_data(oh.look_at_lh((0, 1.2, -4), (0, 1, 0), (0, 1, 0)), ("perspective", 60.0, 0.1))


def _facing_grid(rng, n=9):
    """An n x n grid facing the camera of _light_and_camera (wound so that its left-handed normals point to -z), with a sheared,
    noisy uv0: no triangle's uv footprint is degenerate."""
    pos, idx = NR.grid(rng, n, n)
    uv = np.stack([0.5 + 0.45 * pos[:, 0] + 0.1 * pos[:, 1], 0.5 - 0.4 * pos[:, 1]], axis=1) + rng.uniform(-0.01, 0.01, (len(pos), 2))
    return pos, np.ascontiguousarray(idx.reshape(-1, 3)[:, ::-1]).reshape(-1), uv.astype(f32)


def _normal_map(rng):
    """8 x 8 RGBA8 tangent-space normals, tilted up to ~40 degrees: not flat, so that a pixel's shading depends on its tangent."""
    xy = rng.integers(-76, 77, (8, 8, 2))
    z = np.floor(np.sqrt(127.0 * 127.0 - (xy * xy).sum(axis=2))).astype(np.int64)
    return np.stack([128 + xy[..., 0], 128 + xy[..., 1], 128 + z, np.full((8, 8), 255)], axis=2).astype(np.uint8)


def _normal_mapped_material(r, mk, texels):
    tex = r.add_texture_2d(texels, srgb=False)
    return r.add_material(mk(albedo=(0.8, 0.6, 0.4, 1.0), albedo_mode="value", roughness=0.5, normal_texture=tex, normal_mode="tricomponent"), 0)


class _OracleTangents:
    """One morphed mesh without normals and tangents of its own on the oracle's side: add_mesh of the base shape with tangents=
    serial() (the oracle computes the base normals itself); apply() overwrites the position run with the reference's blend, the
    normal run with the serial normals loop over those positions and the tangent run with serial() over both, sets the mesh radius
    to radius' and refreshes the objects.  recompute_normals=False keeps the base shape's normals (and builds the tangents over
    them); recompute_tangents=False keeps the bind shape's tangents."""

    def __init__(self, o, pos, idx, uv, targets, hand=oh.LEFT, recompute_normals=True, **mesh_kw):
        self.o, self.pos, self.idx, self.uv, self.targets, self.left = o, pos, idx, uv, targets, hand == oh.LEFT
        self.recompute_normals = recompute_normals
        self.base_normals = oh.calculate_normals(pos, _whole(idx), self.left)
        self.mesh = o.add_mesh(pos, idx, normals=None, tangents=TR.serial(pos, self.base_normals, uv, idx), uv0=uv,
                               mesh_handedness=hand, **mesh_kw)
        self.radius = o.meshes[self.mesh].radius
        self.reach = MR.reach(targets)
        self.objects = []

    def apply(self, weights, recompute_tangents=True):
        m = self.o.meshes[self.mesh]
        morphed, normals, tangents = _reference(self.pos, self.targets, weights, self.idx, self.uv, self.left,
                                                given=None if self.recompute_normals else self.base_normals)
        runs = [(0, morphed)] + ([(1, normals)] if self.recompute_normals else []) + ([(2, tangents)] if recompute_tangents else [])
        for a, ref in runs:
            self.o.mesh_words[m.attr_off[a] // 4: m.attr_off[a] // 4 + ref.size] = _words(ref)
        m.radius = MR.radius(self.radius, weights, self.reach)
        for h in self.objects:
            self.o.set_object_transform(h, self.o.object_meta[h]["transform"])
        return morphed, normals, tangents


# ------------------------------------------------------------------ G3. nothing when nothing changes
def test_no_launch_without_a_change(r3):
    rng = np.random.Generator(np.random.PCG64(0x5433))
    p = r3.Renderer(oh.LEFT, f32(1.5))
    pos, idx, uv = _facing_grid(rng)
    targets = _targets(rng, 2, pos)
    mesh = p.add_mesh(pos, idx, uv0=uv, morph_targets=_mt(targets), morph_normals="recompute", build_tangents=True, morph_tangents="recompute")
    mat = _normal_mapped_material(p, r3.material_record, _normal_map(rng))
    insts = p.add_morph_instances_bulk(mesh, [[0.5, 0.0], [0.25, 1.0], None])
    for i, x in zip(insts, (-1.5, 0.0, 1.5)):
        p.add_object(None, mat, oh.translation((x, 1.0, 0.0)), morph=i)
    _light_and_camera(p)
    p.stage_times()
    p.render(96, 64)
    t = p.stage_times()
    assert (t["morph"][1], t["normals"][1], t["tangents"][1]) == (1, 1, 1)  # the three new instances, one call each
    f1 = p.render(96, 64)
    t = p.stage_times()
    assert (t["morph"][1], t["normals"][1], t["tangents"][1]) == (0, 0, 0), "a frame without a weight change launched"
    before = p.readback_mesh_words(0, p.mesh_cursor)
    w = np.array([-0.5, 0.75], dtype=f32)
    p.set_morph_weights(insts[1], w)
    p._flush_morphs()
    t = p.stage_times()
    assert (t["morph"][1], t["normals"][1], t["tangents"][1]) == (1, 1, 1)
    after = p.readback_mesh_words(0, p.mesh_cursor)
    want = before.copy()
    out = p.morphs[insts[1]]["out_off"]
    for off, ref in zip(out, _reference(pos, targets, w, idx, uv)):
        want[off // 4: off // 4 + ref.size] = _words(ref)
    assert not np.array_equal(before, want) and np.array_equal(after, want), "the launch rewrote more than the changed instance's runs"
    f2 = p.render(96, 64)
    assert p.stage_times()["tangents"][1] == 0 and not np.array_equal(f1["hdr16"], f2["hdr16"])
    p.close()


# ------------------------------------------------------------------ G4. rendered
def _frames_scene(r3, morph_tangents):
    """Three instances of a normal-mapped 9 x 9 grid with different weights and one static build_tangents=True object, one
    directional light."""
    rng = np.random.Generator(np.random.PCG64(0x5434))
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    texels = _normal_map(rng)
    mat_o, mat_p = _normal_mapped_material(o, omk, texels), _normal_mapped_material(p, r3.material_record, texels)
    pos, idx, uv = _facing_grid(rng)
    targets = _targets(rng, 2, pos, scale=0.35)
    mesh = p.add_mesh(pos, idx, uv0=uv, morph_targets=_mt(targets), morph_normals="recompute", build_tangents=True,
                      morph_tangents=morph_tangents)
    insts = p.add_morph_instances_bulk(mesh, [None, None, None])
    oracle = []
    for i, x in zip(insts, (-2.1, 0.0, 2.1)):
        xf = oh.translation((x, 1.9, 0.0))
        p.add_object(None, mat_p, xf, morph=i)
        om = _OracleTangents(o, pos, idx, uv, targets)
        om.objects.append(o.add_object(om.mesh, mat_o, xf))
        oracle.append(om)
    spos, sidx, suv = _facing_grid(rng)
    xf = oh.translation((0.0, -0.2, 0.0))
    static = p.add_mesh(spos, sidx, uv0=suv, build_tangents=True)
    p.add_object(static, mat_p, xf)
    o.add_object(o.add_mesh(spos, sidx, uv0=suv, tangents=TR.serial(spos, oh.calculate_normals(spos, sidx, True), suv, sidx)), mat_o, xf)
    for r in (o, p):
        _light_and_camera(r)
    return dict(o=o, p=p, insts=insts, oracle=oracle, static=static, static_ref=(spos, sidx, suv))


def _frames_weights(f):
    rng = np.random.Generator(np.random.PCG64(0x5440 + f))
    return [rng.uniform(-1.0, 1.6, 2).astype(f32) for _ in range(3)]


def test_rendered_frames_match_the_oracle(r3):
    """G4: three 96 x 64 frames with changing weights, bit-identical to the oracle drawing the reference's positions, normals and
    tangents; the static object's tangent run is serial(); the last frame differs from the same frame with morph_tangents="base"."""
    s = _frames_scene(r3, "recompute")
    o, p = s["o"], s["p"]
    spos, sidx, suv = s["static_ref"]
    m = p.meshes[s["static"]]
    assert m.attr_off[2] != INVALID and m.adjacency_off == INVALID
    assert np.array_equal(p.readback_mesh_words(m.attr_off[2], spos.size), _words(TR.serial(spos, oh.calculate_normals(spos, sidx, True), suv, sidx)))
    p.stage_times()
    kw = dict(samples=1, ambient=(0.1, 0.1, 0.1, 1))
    frames = []
    for f in range(3):
        for hp, om, w in zip(s["insts"], s["oracle"], _frames_weights(f)):
            p.set_morph_weights(hp, w)
            om.apply(w)
        fo, fp = o.render(96, 64, **kw), p.render(96, 64, **kw)
        assert p.stage_times()["tangents"][1] == 1
        _compare(fo, fp, f"recomputed tangents, frame {f}")
        assert fo["pass"].sum() > 100
        frames.append(fp)
    assert not np.array_equal(frames[0]["hdr16"], frames[1]["hdr16"])
    p.close()
    # the same last frame with the bind shape's tangents: the normal map looked at the tangent
    b = _frames_scene(r3, "base")
    for hp, om, w in zip(b["insts"], b["oracle"], _frames_weights(2)):
        b["p"].set_morph_weights(hp, w)
        om.apply(w, recompute_tangents=False)
        assert b["p"].morphs[hp]["out_off"][2] == INVALID
    b["p"].stage_times()
    fo, fb = b["o"].render(96, 64, **kw), b["p"].render(96, 64, **kw)
    assert b["p"].stage_times()["tangents"][1] == 0
    _compare(fo, fb, "base tangents")
    assert not np.array_equal(fb["hdr16"], frames[2]["hdr16"]), "the frame does not depend on the tangents"
    b["p"].close()


# ------------------------------------------------------------------ G5. through a skeleton
def _pose(joints, seed):
    import scenes
    rng = Pcg32(seed)
    return np.array([oh.mat4_mul(oh.translation((rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2))),
                                 scenes.random_rotation(rng, oh)) for _ in range(joints)], dtype=f32)


def test_skeleton_skins_the_recomputed_tangents(r3):
    """G5: a skinned cylinder with uv0, added without normals and tangents, bound through a skeleton to a recomputing morph
    instance: the skeleton's base runs are the instance's private runs, the skinned tangent run is the oracle's skinning of the
    reference tangents, and the frames match."""
    rng = np.random.Generator(np.random.PCG64(0x5435))
    o, p = OracleRenderer(oh.LEFT, f32(1.5)), r3.Renderer(oh.LEFT, f32(1.5))
    texels = _normal_map(rng)
    mat_o, mat_p = _normal_mapped_material(o, omk, texels), _normal_mapped_material(p, r3.material_record, texels)
    cpos, cidx, _nrm, _tang, ji, jw = skinned_cylinder(7)
    cuv = rng.uniform(0.0, 1.0, (len(cpos), 2)).astype(f32)
    ct = rng.uniform(-0.12, 0.12, (3,) + cpos.shape).astype(f32)
    cm = p.add_mesh(cpos, cidx, uv0=cuv, joint_indices=ji, joint_weights=jw, morph_targets=_mt(ct), morph_normals="recompute",
                    build_tangents=True, morph_tangents="recompute")
    ci = p.add_morph_instance(cm)
    ident = np.tile(oh.identity(), (7, 1))
    sk_p = p.add_skeleton(cm, ident, morph=ci)
    xc = oh.translation((0.0, 0.0, 0.0))
    p.add_object(None, mat_p, xc, skeleton=sk_p)
    oc = _OracleTangents(o, cpos, cidx, cuv, ct, joint_indices=ji, joint_weights=jw)
    sk_o = o.add_skeleton(oc.mesh, ident)
    oc.objects.append(o.add_object(None, mat_o, xc, skeleton=sk_o))
    for r in (o, p):
        _light_and_camera(r)
    sk_in, _m = p.skinning_buffers()
    assert list(sk_in[0, :3]) == p.morphs[ci]["out_off"] and INVALID not in list(sk_in[0, :3]) and sk_in[0, 7] != INVALID
    p.stage_times()
    n = 3 * len(cpos)
    for f in range(2):
        w = rng.uniform(-1.0, 1.6, 3).astype(f32)
        p.set_morph_weights(ci, w)
        _pos, _nrm, ref_tan = oc.apply(w)
        pose = _pose(7, 90 + f)
        p.set_skeleton_joint_matrices(sk_p, pose)
        o.set_skeleton_joint_matrices(sk_o, pose)
        kw = dict(samples=1, ambient=(0.1, 0.1, 0.1, 1))
        fo, fp = o.render(96, 64, **kw), p.render(96, 64, **kw)
        assert p.stage_times()["tangents"][1] == 1
        assert np.array_equal(p.readback_mesh_words(p.morphs[ci]["out_off"][2], n), _words(ref_tan)), f"frame {f}: the instance's tangents"
        want = o.mesh_words[o.skeletons[sk_o]["out_off"][2] // 4:][:n]
        assert want.any() and np.array_equal(p.readback_mesh_words(p.skeletons[sk_p]["out_off"][2], n), want), f"frame {f}: skinned tangents"
        _compare(fo, fp, f"skinned recomputed tangents, frame {f}")
        assert fo["pass"].sum() > 50
    p.close()


# ------------------------------------------------------------------ G6. errors
def test_argument_errors(r3):
    """Every validation rule of r3n_vertex_tangents answers R3N_ERR_INVALID_ARG on the host with nothing launched and no word
    changed; no instances is R3N_OK; a good call on the same context still succeeds."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x5436))
    pos, idx = NR.grid(rng, 8, 8)
    pos = np.concatenate([pos, rng.uniform(-1, 1, (1, 3)).astype(f32)])  # V = 65
    uv = rng.uniform(-2.0, 2.0, (65, 2)).astype(f32)
    targets = _targets(rng, 2, pos)
    mesh = p.add_mesh(pos, idx, uv0=uv, morph_targets=_mt(targets), morph_normals="recompute", build_tangents=True, morph_tangents="recompute")
    w = np.array([0.5, -1.0], dtype=f32)
    inst = p.add_morph_instance(mesh, w)
    m, out = p.meshes[mesh], p.morphs[inst]["out_off"]
    names = ["position", "normal", "uv", "tangent", "index", "index_count", "adjacency", "vertex_count"]
    good = np.array([out[0], out[1], m.attr_off[3], out[2], 4 * m.first_index, m.index_count, m.adjacency_off, m.vertex_count], dtype=np.uint32)

    def call(rec):
        rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 8)
        return p.lib.r3n_vertex_tangents(p.ctx, r3._ffi.ptr(rec), len(rec))

    def edit(**fields):
        rec = good.copy()
        for k, val in fields.items():
            rec[names.index(k)] = val
        return rec

    adjacency_words = m.vertex_count + 1 + m.index_count
    bad = {f"{k} run outside the mesh buffer": edit(**{k: 0xFFFFFF00}) for k in ("position", "normal", "uv", "tangent", "index", "adjacency")}
    bad.update({f"{k} run not 4-byte aligned": edit(**{k: int(good[names.index(k)]) + 1 + i % 3})
                for i, k in enumerate(("position", "normal", "uv", "tangent", "index", "adjacency"))})
    bad.update({
        "index count past the mesh buffer": edit(index_count=0x7FFFFFFF),
        "no vertices": edit(vertex_count=0),
        "tangent run is the position run": edit(tangent=int(good[0])),
        "tangent run overlaps the positions' tail": edit(tangent=int(good[0]) + 12 * (m.vertex_count - 1)),
        "tangent run is the normal run": edit(tangent=int(good[1])),
        "tangent run overlaps the normals' tail": edit(tangent=int(good[1]) + 12 * (m.vertex_count - 1)),
        "tangent run overlaps the uvs' tail": edit(tangent=int(good[2]) + 8 * m.vertex_count - 4),
        "tangent run overlaps the indices' tail": edit(tangent=int(good[4]) + 4 * (m.index_count - 1)),
        "tangent run overlaps the adjacency's tail": edit(tangent=int(good[6]) + 4 * (adjacency_words - 1)),
    })
    assert len(bad) == 21
    p._flush_morphs()  # the instance's first evaluation, so that the rejected calls below leave a known state behind
    before = p.readback_mesh_words(0, p.mesh_cursor)
    p.stage_times()
    for what, rec in bad.items():
        assert call(rec) == R3N_ERR_INVALID_ARG, what
        assert p.lib.r3n_last_error(p.ctx).decode().startswith("tangents:"), what
        assert call(np.stack([good, rec])) == R3N_ERR_INVALID_ARG, what  # a bad record behind a good one rejects the whole call
    assert p.lib.r3n_vertex_tangents(p.ctx, None, 1) == R3N_ERR_INVALID_ARG
    assert p.stage_times()["tangents"][1] == 0 and np.array_equal(p.readback_mesh_words(0, p.mesh_cursor), before)
    assert p.lib.r3n_vertex_tangents(p.ctx, None, 0) == 0 and call(np.zeros((0, 8), dtype=np.uint32)) == 0  # no instances: R3N_OK
    assert p.stage_times()["tangents"][1] == 0
    # a good call still works: the tangents over the MESH's normal run (the bind shape's normals) into the same run
    assert call(edit(normal=m.attr_off[1])) == 0
    assert p.stage_times()["tangents"][1] == 1
    morphed = MR.blend(pos, targets, w)
    ref = TR.serial(morphed, oh.calculate_normals(pos, idx, True), uv, idx)
    assert np.array_equal(p.readback_mesh_words(out[2], ref.size), _words(ref))
    p.close()


def test_add_mesh_arguments(r3):
    """Every ValueError of add_mesh(morph_tangents=); build_tangents=True with tangents given or without uv0 creates nothing; the
    default leaves attribute 2 absent."""
    p = r3.Renderer(oh.LEFT)
    rng = np.random.Generator(np.random.PCG64(0x5437))
    pos, idx = NR.grid(rng, 8, 8)
    uv = rng.uniform(-2.0, 2.0, (64, 2)).astype(f32)
    targets = _targets(rng, 2, pos)
    mt = _mt(targets)
    own = TR.unit_normals(rng, 64)
    ok = dict(uv0=uv, morph_targets=mt, build_tangents=True, morph_tangents="recompute")
    refused = {
        "tangents are not generated": dict(ok, build_tangents=False),
        "build_tangents left at its default": {k: v for k, v in ok.items() if k != "build_tangents"},
        "tangents of its own": dict(ok, tangents=own),
        "no uv0": dict(ok, uv0=None),
        "no targets": dict(ok, morph_targets=None),
        "no position deltas": dict(ok, normals=own, morph_targets=dict(positions=None, normals=targets, tangents=None)),
        "tangent deltas": dict(ok, morph_targets=dict(positions=targets, normals=None, tangents=targets)),
        "an unknown mode": dict(ok, morph_tangents="always"),
    }
    cursor = p.mesh_cursor
    for what, kw in refused.items():
        with pytest.raises(ValueError, match="morph_tangents"):
            p.add_mesh(pos, idx, **kw)
        assert p.mesh_cursor == cursor, what
    with pytest.raises(ValueError):  # an index past the vertices cannot be given an adjacency row
        p.add_mesh(pos, np.array([0, 1, 64], dtype=np.uint32), **ok)
    assert p.mesh_cursor == cursor
    # the flag does nothing with tangents given (they are kept) or without uv0 (no run)
    given = p.meshes[p.add_mesh(pos, idx, uv0=uv, tangents=own, build_tangents=True)]
    assert np.array_equal(p.readback_mesh_words(given.attr_off[2], own.size), _words(own))
    assert p.meshes[p.add_mesh(pos, idx, build_tangents=True)].attr_off[2] == INVALID
    # the default: no tangent run, with or without targets; no private tangent run either
    assert p.meshes[p.add_mesh(pos, idx, uv0=uv)].attr_off[2] == INVALID
    plain = p.add_mesh(pos, idx, uv0=uv, morph_targets=mt)
    assert p.meshes[plain].attr_off[2] == INVALID and p.meshes[plain].adjacency_off == INVALID
    assert p.morphs[p.add_morph_instance(plain)]["out_off"][1:] == [INVALID, INVALID]
    # opted in: the run is serial() over the normals add_mesh computed; "base" keeps it for every instance
    built = p.add_mesh(pos, idx, uv0=uv, morph_targets=mt, build_tangents=True)
    m = p.meshes[built]
    assert np.array_equal(p.readback_mesh_words(m.attr_off[2], pos.size), _words(TR.serial(pos, oh.calculate_normals(pos, idx, True), uv, idx)))
    assert m.adjacency_off == INVALID and p.morphs[p.add_morph_instance(built)]["out_off"][2] == INVALID
    p.stage_times()
    p._flush_morphs()
    t = p.stage_times()
    assert t["morph"][1] == 1 and t["tangents"][1] == 0 and t["normals"][1] == 0
    p.close()


# ------------------------------------------------------------------ G7. the fixture through the loader
def test_fixture_through_the_loader(r3):
    """morph-notangent.glb through gltf.instance_scene(build_tangents=True, morph_tangents="recompute"): the normals stay the bind
    shape's (morph_normals is not asked for), the tangent runs equal serial() over the morphed positions and those normals, and the
    frame equals the oracle's."""
    from rend3_amd import gltf
    o, p = OracleRenderer(oh.RIGHT, f32(1.5)), r3.Renderer(oh.RIGHT, f32(1.5))
    g = gltf.Gltf(FIXTURE)
    inst = gltf.instance_scene(g, p, r3.host, r3.material_record, build_tangents=True, morph_tangents="recompute")
    assert len(inst["objects"]) == 2 and [n["morphs"] for n in inst["nodes"]] == [[0], [1]]
    prim = g.primitive(0, 0)
    pos, idx, uv, targets = prim["positions"], prim["indices"], prim["uv0"], prim["targets"]["positions"]
    rec, key = gltf.material_from_gltf(g, prim["material"], omk, o)
    mat = o.add_material(rec, key)
    weights = [np.array([0.5, 0.25], dtype=f32), np.array([0.0, 1.0], dtype=f32)]  # mesh.weights, node 1's own
    nodes = []
    for ni in range(2):
        om = _OracleTangents(o, pos, idx, uv, targets, hand=oh.RIGHT, recompute_normals=False)
        om.objects.append(o.add_object(om.mesh, mat, inst["node_transforms"][ni]))
        nodes.append(om)
    for r in (o, p):
        r.add_directional_light(color=(1, 1, 1), intensity=3.0, direction=(0.3, -0.4, -1.0), distance=10.0, resolution=256)
        r.set_camera_data(oh.translation((0.0, -0.3, -4.0)), ("perspective", 60.0, 0.1))
    refs = [om.apply(w) for om, w in zip(nodes, weights)]
    p.stage_times()
    kw = dict(samples=1, ambient=(0.1, 0.1, 0.1, 1))
    fo, fp = o.render(96, 64, **kw), p.render(96, 64, **kw)
    t = p.stage_times()
    assert (t["morph"][1], t["normals"][1], t["tangents"][1]) == (1, 0, 1)
    for h, (ref_pos, _nrm, ref_tan) in zip((0, 1), refs):
        out = p.morphs[h]["out_off"]
        assert out[1] == INVALID and out[2] != INVALID
        assert np.array_equal(p.readback_mesh_words(out[0], ref_pos.size), _words(ref_pos))
        assert np.array_equal(p.readback_mesh_words(out[2], ref_tan.size), _words(ref_tan)), f"node {h}: tangent run"
        assert ref_tan.any(axis=1).all()
    _compare(fo, fp, "fixture, recomputed tangents")
    assert fo["pass"].sum() > 100
    p.close()
