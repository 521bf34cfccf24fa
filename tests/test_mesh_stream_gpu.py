"""Pooled mesh blocks on the GPU: r3n_mesh_blocks_add / r3n_mesh_blocks_remove / r3n_mesh_compact and Renderer(mesh_upload="stream").

  * the relocation kernel (csrc/mesh_reloc.hip) against the numpy restatement tests/mesh_reloc_reference.py, all 32 words of every
    record, for tables on both sides of the constant where its lookup changes form;
  * the buffer's words across a seeded add / remove / add / compact sequence, with the offsets the allocator of the check program
    (tests/mesh_reloc_check.cpp, its `pool` mode) predicts;
  * frames of a small world with a skinned and a morphed (recomputed normals and tangents) object across removals and a compaction,
    against a fresh "append" renderer holding the surviving world and against the oracle;
  * the waits (r3n_mesh_stats), the absence of any r3n_objects_write across a compaction, and the refusals.

Frames are 64 x 64, meshes have 3 to ~300 vertices."""
import ctypes

import numpy as np
import pytest

import mesh_reloc_reference as MR
import tangents_reference as TR
from oracle import host as oh
from oracle.world import OracleRenderer
from oracle.world import material_record as omk
from rend3_amd.scenes import skinned_cylinder
from test_mesh_stream import pool_ops
from test_tangents_gpu import _facing_grid, _light_and_camera, _mt, _normal_map, _normal_mapped_material, _OracleTangents, _pose, _targets

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 0xFFFFFFFF
OK, INVALID_ARG, STATE = 0, -1, -4


@pytest.fixture(scope="module")
def r3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import rend3_amd
    return rend3_amd


def align4(v):
    return (v + 3) & ~3


def raw_remove(p, offsets):
    """r3n_mesh_blocks_remove on anything with .lib and .ctx; returns the code"""
    offs = np.array(offsets, dtype=np.uint64)
    return p.lib.r3n_mesh_blocks_remove(p.ctx, offs.ctypes.data_as(ctypes.c_void_p), len(offs))


class Raw:
    """A context of the C ABI alone: its object capacity starts at 0, so the relocation kernel can be run over exactly 1, 63, ...
    slots (a Renderer's object buffer starts at 16 slots, FreelistDerivedBuffer::STARTING_SIZE, and cannot shrink)."""

    def __init__(self):
        from rend3_amd import _ffi
        self.ffi, self.lib = _ffi, _ffi.lib()
        self.ctx = self.lib.r3n_create(0, None)
        assert self.ctx, self.lib.r3n_create_error()

    def close(self):
        self.lib.r3n_destroy(self.ctx)

    def ok(self, code):
        assert code == 0, (code, self.lib.r3n_last_error(self.ctx))

    def add_zero_blocks(self, words):
        recs = (self.ffi.MeshBlock24 * len(words))()
        for r, w in zip(recs, words):
            r.words, r.flags = w, self.ffi.MESH_BLOCK_ZERO
        out = np.zeros(len(words), dtype=np.uint64)
        self.ok(self.lib.r3n_mesh_blocks_add(self.ctx, recs, len(words), None, 0, self.ffi.ptr(out)))
        return [int(b) for b in out]

    def write_objects(self, recs, capacity):
        slots = np.arange(len(recs), dtype=np.uint32)
        self.ok(self.lib.r3n_objects_write(self.ctx, self.ffi.ptr(slots), self.ffi.ptr(np.ascontiguousarray(recs)), len(recs), capacity))

    def objects(self, n):
        out = np.zeros((n, 32), dtype=np.uint32)
        self.ok(self.lib.r3n_readback_objects(self.ctx, 0, self.ffi.ptr(out), n))
        return out

    def compact(self):
        st = self.stats()
        moves = (self.ffi.MeshMove24 * max(st["blocks_live"], 1))()
        out = self.ffi.MeshCompactResult()
        self.ok(self.lib.r3n_mesh_compact(self.ctx, None, ctypes.byref(out), moves, max(st["blocks_live"], 1)))
        res = {name: int(getattr(out, name)) for name, _ in self.ffi.MeshCompactResult._fields_}
        res["moves"] = np.array([(m.old_byte_offset, m.new_byte_offset, m.padded_words) for m in moves[:res["blocks_moved"]]],
                                dtype=np.uint64).reshape(-1, 3)
        return res

    def stats(self):
        out = self.ffi.MeshCounters()
        self.ok(self.lib.r3n_mesh_stats(self.ctx, ctypes.byref(out), 0))
        return {name: int(getattr(out, name)) for name, _ in self.ffi.MeshCounters._fields_}


# ------------------------------------------------------------------ 1. the relocation kernel
SIZES = (1, 3, 4, 5, 8)


def layout(n_moving):
    """Blocks in address order as (words, kept): a 16-word block that stays, then n_moving kept blocks of 1, 3, 4, 5, 8 words in turn
    with a block to remove in front of the first and behind every third: n_moving moves whose shifts grow along the buffer."""
    items = [(16, True), (4, False)]
    for i in range(n_moving):
        items.append((SIZES[i % len(SIZES)], True))
        if i % 3 == 2:
            items.append((4 * (1 + i % 2), False))
    return items


def starts_of(items):
    out, cur = [], 0
    for words, _ in items:
        out.append(align4(cur))
        cur = out[-1] + words
    return out


def expected_table(items):
    """rows (src, end, shift) in words of the compaction of `items` without a budget"""
    rows, cur = [], 0
    for (words, kept), start in zip(items, starts_of(items)):
        if not kept:
            continue
        dst = align4(cur)
        if dst != start:
            rows.append((start, start + align4(words), start - dst))
        cur = dst + words
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


def synthetic_records(items, n_slots, seed):
    """n_slots records whose seven address fields come from the edge list: the first word of a block, its last word, its last
    padding word, one past the padding, one before its start, INVALID, a word of the block below the first move, a word of a
    removed block, and -- in every third record -- fields in three different moved blocks.  Byte fields carry low bits.  Even slots
    are enabled, odd ones disabled; every other word is random (index_count and material_index small: r3n_objects_write reads them)."""
    rng = np.random.default_rng(seed)
    starts = starts_of(items)
    kept = [(s, w) for (w, k), s in zip(items, starts) if k][1:]  # the moving blocks
    gone = [(s, w) for (w, k), s in zip(items, starts) if not k]
    recs = rng.integers(0, 2 ** 32, (n_slots, 32), dtype=np.uint64).astype(np.uint32)
    recs[:, 21] = 3 * rng.integers(0, 50, n_slots)
    recs[:, 22] = rng.integers(0, 3, n_slots)
    recs[:, 29] = (np.arange(n_slots) + 1) % 2
    for slot in range(n_slots):
        s, w = kept[int(rng.integers(0, len(kept)))]
        pad = align4(w)
        edge = [s, s + w - 1, s + pad - 1, s + pad, s - 1, INVALID, int(rng.integers(0, 16)), gone[int(rng.integers(0, len(gone)))][0] + int(rng.integers(0, 4))]
        if slot % 3 == 2:  # three different blocks (as many as there are)
            edge += [kept[int(rng.integers(0, len(kept)))][0] + 0, kept[len(kept) // 2][0], kept[-1][0] + kept[-1][1] - 1, kept[0][0]] * 2
        pick = [edge[int(k)] for k in rng.permutation(len(edge))[:7]] if slot >= 2 else (edge[:7] if slot == 0 else edge[1:8])
        recs[slot, 20] = pick[0]
        for a in range(6):
            word = pick[1 + a]
            recs[slot, 23 + a] = INVALID if word == INVALID else (word << 2) | int(rng.integers(0, 4))
    return recs


LDS = 256  # mesh_reloc::LDS_TABLE_ENTRIES; test_threshold_constant pins it against the header


def test_threshold_constant():
    from test_mesh_stream import ROOT
    import os
    import re
    text = open(os.path.join(ROOT, "rend3_amd", "csrc", "mesh_reloc.h")).read()
    assert int(re.search(r"LDS_TABLE_ENTRIES\s*=\s*(\d+)u", text).group(1)) == LDS


@pytest.mark.parametrize("n_moves", [1, 2, 64, 65, 1000, LDS - 1, LDS, LDS + 1])
def test_relocation_kernel_word_for_word(r3, n_moves):
    """For an object buffer of exactly 1, 63, 64, 65, 257 and 1 025 slots in turn: the layout is built (and rebuilt at the same
    offsets), synthetic records go up with one r3n_objects_write, r3n_mesh_compact, r3n_readback_objects -- all 32 words of every
    record equal the numpy restatement applied to what was written, so nothing but the seven fields is touched, enabled slot or
    not.  The table is computed here from the layout, not taken from the call; the call's moves must agree with it.  (Through the
    C ABI: see Raw.  Renderer.write_object_records + compact_meshes over 1 025 slots follow at the end.)"""
    p = Raw()
    items = layout(n_moves)
    table = expected_table(items)
    assert len(table) == n_moves
    live = []
    for n_slots in (1, 63, 64, 65, 257, 1025):
        if live:
            assert raw_remove(p, live) == OK  # everything goes; the same sizes then take the same places
        blocks = p.add_zero_blocks([w for w, _ in items])
        assert blocks == [4 * s for s in starts_of(items)], "first fit at the lowest address: the layout of ascending appends"
        assert raw_remove(p, [b for b, (_, kept) in zip(blocks, items) if not kept]) == OK
        recs = synthetic_records(items, n_slots, 0x3E50 + n_slots)
        p.write_objects(recs, n_slots)
        assert np.array_equal(p.objects(n_slots), recs)
        res = p.compact()
        assert res["blocks_moved"] == n_moves and res["full_syncs"] == 1 and res["free_ranges_after"] == 0
        assert np.array_equal(MR.table_from_moves(res["moves"]), table), "the moves the call reports"
        got = p.objects(n_slots)
        want = MR.relocate_records(recs, table)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{n_slots} slots, {n_moves} moves: {len(bad)} words differ, first (slot, word) {bad[:4].tolist()}"
        assert (want != recs).any(axis=1).sum() >= min(n_slots, 2) - 1  # the records did change
        live = [4 * s for s in starts_of([(w, True) for w, kept in items if kept])]
        assert p.stats()["blocks_live"] == len(live)
    p.close()
    # the same through the renderer: write_object_records over a pooled buffer, compact_meshes, readback_objects
    r = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream")
    blocks = r._add_mesh_blocks([w for w, _ in items])
    assert raw_remove(r, [b for b, (_, kept) in zip(blocks, items) if not kept]) == OK
    recs = synthetic_records(items, 1025, 0x3E4F)
    r.write_object_records(np.arange(1025), recs, 1025)
    writes = r.object_writes
    res = r.compact_meshes()
    assert r.object_writes == writes and res["blocks_moved"] == n_moves
    assert np.array_equal(r.readback_objects(0, 1025), MR.relocate_records(recs, table))
    r.close()


# ------------------------------------------------------------------ 2. the buffer's words
def test_buffer_contents_and_offsets_across_add_remove_compact(r3):
    """A seeded sequence over blocks of 1, 3, 4, 5, 1 020, 1 024 and 1 028 words, uploaded and zero-filled: removals, adds that
    reuse the freed words, a compaction with stage_words = 256 over a 4-word hole in front of long blocks (staged passes), a
    compaction whose max_words stops mid-way, and one that finishes.  Every offset and every move equals what the check
    program's Pool and planner give for the same calls; at the end (and after every compaction) r3n_readback_mesh of every live
    block equals what was uploaded, zero-filled blocks read back as zeros."""
    rng = np.random.default_rng(0x3E51)
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream")
    script = [("A", 4, False), ("A", 1028, False), ("A", 1024, False), ("A", 1, False), ("A", 3, True), ("A", 1020, False), ("A", 5, False),
              ("A", 1024, True), ("R", 0), ("R", 3), ("C", 0, 256),          # a 4-word hole in front of 1 028 + 1 024 words: staged
              ("R", 2), ("A", 1020, True), ("A", 4, False),                  # the 1 024-word hole takes 1 020 zero-filled words, then 4
              ("R", 1), ("R", 5), ("A", 1028, False), ("A", 1024, False),    # parked words: taken with a wait, or fresh ones behind the mark
              ("R", 4), ("R", 7), ("A", 5, True), ("A", 3, False), ("A", 1, True),
              ("R", 8), ("C", 1040, 256), ("C", 0, 0)]
    ops, data, offset, got = [], [], [], []  # per added block: its words (None: zero-filled), its byte offset (None: removed)

    def check_contents(tag):
        for k, off in enumerate(offset):
            if off is None:
                continue
            want = np.zeros(data[k], dtype=np.uint32) if isinstance(data[k], int) else data[k]
            assert np.array_equal(p.readback_mesh_words(off, len(want)), want), f"{tag}: block {k} at byte {off}"

    for step in script:
        before = p.mesh_stats()
        if step[0] == "A":
            words = rng.integers(0, 2 ** 32, step[1], dtype=np.uint64).astype(np.uint32)
            off = p._add_mesh_blocks([step[1] if step[2] else words])[0]
            data.append(step[1] if step[2] else words)
            offset.append(off)
            after = p.mesh_stats()
            grew = after["growths"] != before["growths"]  # (a growth waits too: whether words were merged in does not show then)
            got.append(("A", off // 4, None if grew else after["full_waits"] - before["full_waits"]))
            ops.append(f"A{step[1]}")
            if after["growths"] != before["growths"]:  # the device block grew behind a full wait: parked words are holes now
                got.append(("S", after["pool_words"]))
                ops.append("S")
        elif step[0] == "R":
            assert raw_remove(p, [offset[step[1]]]) == OK
            got.append(("R", offset[step[1]] // 4))
            offset[step[1]] = None
            ops.append(f"R{step[1]}")
        else:
            res = p.compact_meshes(max_words=step[1], stage_words=step[2])
            got.append(("C", res["blocks_moved"], res["passes"], res["kernel_launches"] - (1 if res["blocks_moved"] else 0), res["pool_words_after"]))
            for old, new, padded in res["moves"].tolist():
                got.append(("M", old // 4, new // 4, padded))
                k = offset.index(old)
                offset[k] = new
            ops.append(f"C{step[1]}:{step[2]}")
            assert res["full_syncs"] == (1 if res["blocks_moved"] else 0)
            check_contents(f"after {ops[-1]}")
    want = pool_ops(ops, sanitize=False)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w or (g[0] == "A" and g[2] is None and g[:2] == w[:2]), f"the device {g}, the check program {w}"
    compactions = [row for row in got if row[0] == "C"]
    assert compactions[0][1] >= 5 and compactions[0][2] < compactions[0][3], "the first compaction went through scratch"
    assert 0 < compactions[1][1] and compactions[2][1] > 0, "the budget stopped mid-way; the last call finished"
    st = p.mesh_stats()
    assert st["free_ranges"] == 0 and st["pool_words"] == max(o // 4 + (d if isinstance(d, int) else len(d)) for o, d in zip(offset, data) if o is not None)
    check_contents("at the end")
    # an in-place edit inside a live block stays legal; outside one it is refused
    k = next(i for i, (o, d) in enumerate(zip(offset, data)) if o is not None and not isinstance(d, int) and len(d) >= 1020)
    patch = np.arange(8, dtype=np.uint32)
    assert p.lib.r3n_mesh_buffer_write(p.ctx, offset[k] + 16, patch.ctypes.data_as(ctypes.c_void_p), 32) == OK
    data[k][4:12] = patch
    assert p.lib.r3n_mesh_buffer_write(p.ctx, 4 * st["pool_words"] + 64, patch.ctypes.data_as(ctypes.c_void_p), 32) == STATE
    check_contents("after the in-place edit")
    p.close()


# ------------------------------------------------------------------ 3. frames
KW = dict(samples=1, ambient=(0.1, 0.1, 0.1, 1))
PLACES = dict(s0=(-1.2, 2.3, 0.0), s1=(1.2, 2.3, 0.0), morph=(-1.2, 0.1, 0.0), cyl=(1.2, -0.9, 0.0))
DOOMED_PLACES = [(0.0, 1.0, -1.0), (-0.5, 0.5, -1.5), (0.5, 1.5, -1.2), (0.0, 0.0, -0.8), (0.3, 0.8, -1.1)]


def _world_data():
    rng = np.random.Generator(np.random.PCG64(0x3E52))
    d = dict(texels=_normal_map(rng))
    d["grids"] = [_facing_grid(rng, 5) for _ in range(5)]  # s0, s1 and three doomed ones
    d["morph"] = _facing_grid(rng, 9)
    d["targets"] = _targets(rng, 2, d["morph"][0], scale=0.35)
    cpos, cidx, cnrm, ctan, ji, jw = skinned_cylinder(5)
    d["cyl"] = (cpos, cidx, cnrm, ctan, ji, jw, rng.uniform(0.0, 1.0, (len(cpos), 2)).astype(f32))
    return d


def _cyl_mesh(r, d):
    cpos, cidx, cnrm, ctan, ji, jw, cuv = d["cyl"]
    return r.add_mesh(cpos, cidx, normals=cnrm, tangents=ctan, uv0=cuv, joint_indices=ji, joint_weights=jw)


def _product_world(r3, d, mode):
    """mode "stream": the whole world -- three doomed static meshes, a doomed skeleton and a doomed morph instance are added IN
    FRONT of what survives, so that every surviving block moves at the compaction; "append": the surviving world alone.  The
    survivors' objects come first, so both renderers give them the same handles."""
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload=mode)
    mat = _normal_mapped_material(p, r3.material_record, d["texels"])
    full = mode == "stream"
    w = dict(p=p, doomed_meshes=[], doomed_objects=[])
    g = d["grids"]

    def grid_mesh(k):
        pos, idx, uv = g[k]
        return p.add_mesh(pos, idx, uv0=uv, build_tangents=True)
    if full:
        w["doomed_meshes"].append(grid_mesh(2))
    s0 = grid_mesh(0)
    if full:
        w["doomed_meshes"].append(grid_mesh(3))
    s1 = grid_mesh(1)
    cyl = _cyl_mesh(p, d)
    if full:
        w["doomed_meshes"].append(grid_mesh(4))
    mpos, midx, muv = d["morph"]
    mm = p.add_mesh(mpos, midx, uv0=muv, morph_targets=_mt(d["targets"]), morph_normals="recompute", build_tangents=True, morph_tangents="recompute")
    ident = np.tile(oh.identity(), (5, 1))
    if full:
        w["doomed_inst"], w["inst"] = p.add_morph_instances_bulk(mm, [None, None])
        w["doomed_sk"], w["sk"] = p.add_skeletons_bulk(cyl, [ident, ident])
    else:
        w["inst"], w["sk"] = p.add_morph_instance(mm), p.add_skeleton(cyl, ident)
    w["objects"] = [p.add_object(s0, mat, oh.translation(PLACES["s0"])), p.add_object(s1, mat, oh.translation(PLACES["s1"])),
                    p.add_object(None, mat, oh.translation(PLACES["cyl"]), skeleton=w["sk"]),
                    p.add_object(None, mat, oh.translation(PLACES["morph"]), morph=w["inst"])]
    if full:
        for mesh, at in zip(w["doomed_meshes"], DOOMED_PLACES):
            w["doomed_objects"].append(p.add_object(mesh, mat, oh.translation(at)))
        w["doomed_objects"].append(p.add_object(None, mat, oh.translation(DOOMED_PLACES[3]), skeleton=w["doomed_sk"]))
        w["doomed_objects"].append(p.add_object(None, mat, oh.translation(DOOMED_PLACES[4]), morph=w["doomed_inst"]))
    _light_and_camera(p)
    w.update(meshes=dict(s0=s0, s1=s1, cyl=cyl, morph=mm))
    return w


def _oracle_world(d):
    o = OracleRenderer(oh.LEFT, f32(1.0))
    mat = _normal_mapped_material(o, omk, d["texels"])
    objects = []
    for k, place in ((0, "s0"), (1, "s1")):
        pos, idx, uv = d["grids"][k]
        mesh = o.add_mesh(pos, idx, uv0=uv, tangents=TR.serial(pos, oh.calculate_normals(pos, idx, True), uv, idx))
        objects.append((mesh, place))
    cyl = _cyl_mesh(o, d)
    mpos, midx, muv = d["morph"]
    om = _OracleTangents(o, mpos, midx, muv, d["targets"])
    sk = o.add_skeleton(cyl, np.tile(oh.identity(), (5, 1)))
    for mesh, place in objects:
        o.add_object(mesh, mat, oh.translation(PLACES[place]))
    o.add_object(None, mat, oh.translation(PLACES["cyl"]), skeleton=sk)
    om.objects.append(o.add_object(om.mesh, mat, oh.translation(PLACES["morph"])))
    _light_and_camera(o)
    return dict(o=o, om=om, sk=sk)


def _same_frame(a, b, tag):
    """visibility keys and the HDR buffer bit for bit; the framebuffer within the parity tests' tolerances"""
    assert np.array_equal(a["vis"], b["vis"]), tag + f": visibility keys ({(a['vis'] != b['vis']).sum()} px differ)"
    hd = (a["hdr16"] != b["hdr16"]).any(axis=2).sum()
    assert hd == 0, tag + f": HDR f16 differs in {hd} px"
    assert np.abs(a["rgba_f32"] - b["rgba_f32"]).max() <= 1e-3, tag + ": framebuffer > 1e-3"
    assert np.abs(a["rgba8"].astype(int) - b["rgba8"].astype(int)).max() <= 1, tag + ": rgba8 > 1 LSB"


def test_frames_across_removals_and_a_compaction(r3):
    """The stream renderer draws the whole world, retires the doomed half (objects, then their meshes, skeleton and morph
    instance), and is compared with a fresh append renderer and the oracle, both holding the surviving world: before the
    compaction, in the frame right after it (nothing re-evaluated: the moved runs and the patched records alone), and two frames
    later with new joint matrices and morph weights (the fixed-up skinning, morph, normals and tangents inputs write the moved
    runs).  No r3n_objects_write is issued across the compaction, and _object_record(h) of every live handle equals the record
    the device holds."""
    d = _world_data()
    s, q, ow = _product_world(r3, d, "stream"), _product_world(r3, d, "append"), _oracle_world(d)
    p, a, o = s["p"], q["p"], ow["o"]
    assert s["objects"] == q["objects"] == [0, 1, 2, 3]

    def pose_all(seed, weights):
        pose = _pose(5, seed)
        w = np.asarray(weights, dtype=f32)
        for r, sk, inst in ((p, s["sk"], s["inst"]), (a, q["sk"], q["inst"])):
            r.set_skeleton_joint_matrices(sk, pose)
            r.set_morph_weights(inst, w)
        o.set_skeleton_joint_matrices(ow["sk"], pose)
        ow["om"].apply(w)

    def three(tag):
        fp, fa, fo = p.render(64, 64, **KW), a.render(64, 64, **KW), o.render(64, 64, **KW)
        _same_frame(fa, fp, tag + ", stream against append")
        _same_frame(fo, fp, tag + ", stream against the oracle")
        return fp

    pose_all(70, [0.6, -0.4])
    p.set_skeleton_joint_matrices(s["doomed_sk"], _pose(5, 71))
    p.set_morph_weights(s["doomed_inst"], np.array([1.0, 1.0], dtype=f32))
    whole = p.render(64, 64, **KW)
    with pytest.raises(ValueError):
        p.remove_mesh(s["doomed_meshes"][0])  # an enabled object names it
    with pytest.raises(ValueError):
        p.remove_skeleton(s["doomed_sk"])
    with pytest.raises(ValueError):
        p.remove_morph_instance(s["doomed_inst"])
    with pytest.raises(ValueError):
        p.remove_mesh(s["meshes"]["cyl"])  # no object names the mesh itself, but two skeletons do
    for h in s["doomed_objects"]:
        p.remove_object(h)
    p.render(64, 64, readback=False, **KW)
    for m in s["doomed_meshes"]:
        p.remove_mesh(m)
    p.remove_skeleton(s["doomed_sk"])
    p.remove_morph_instance(s["doomed_inst"])
    with pytest.raises(ValueError):
        p.remove_mesh(s["doomed_meshes"][0])  # handles are not reused, a removed one stays removed
    st = p.mesh_stats()
    assert st["blocks_live"] == 6 and st["remove_calls"] == 5
    before = three("before the compaction")
    assert (before["vis"] != whole["vis"]).any(), "the doomed objects were in view"
    assert (before["hdr16"] != 0).any(axis=2).sum() > 200, "the survivors are in view"
    # ---- the compaction
    old = dict(sk=list(p.skeletons[s["sk"]]["out_off"]), inst=list(p.morphs[s["inst"]]["out_off"]),
               meshes={k: p.meshes[m].attr_off[0] for k, m in s["meshes"].items()})
    writes = p.object_writes
    res = p.compact_meshes()
    assert p.object_writes == writes, "compact_meshes re-sent object records"
    assert res["blocks_moved"] == 6 and res["full_syncs"] == 1 and res["free_ranges_after"] == 0
    assert all(a2 < b2 for a2, b2 in zip(p.skeletons[s["sk"]]["out_off"], old["sk"]) if b2 != INVALID)
    assert all(a2 < b2 for a2, b2 in zip(p.morphs[s["inst"]]["out_off"], old["inst"]) if b2 != INVALID)
    assert all(p.meshes[m].attr_off[0] < old["meshes"][k] for k, m in s["meshes"].items())
    for mesh in (p.meshes[m] for m in s["meshes"].values()):  # the alignments a slide by whole blocks keeps
        assert all(off % 16 == 0 for off in mesh.delta_off if off != INVALID) and (mesh.adjacency_off == INVALID or mesh.adjacency_off % 16 == 0)
    assert all(off % 16 == 0 for off in p.morphs[s["inst"]]["out_off"] if off != INVALID)
    device = p.readback_objects()
    for h in s["objects"]:
        assert np.array_equal(p._object_record(h), device[h]), f"handle {h}: the mirror and the device's patched record"
    assert not p.dirty_objects and p.object_writes == writes
    after = three("right after the compaction")
    assert np.array_equal(after["hdr16"], before["hdr16"])
    three("one frame later")
    pose_all(72, [-0.7, 1.2])
    changed = three("two frames later, new joint matrices and morph weights")
    assert (changed["hdr16"] != after["hdr16"]).any(), "the new pose and weights show"
    assert p.object_writes > writes  # (the morphed object's bounding sphere went up through the dirty path, as always)
    # freed words are reused: the next mesh lands below the old mark
    pos, idx, uv = d["grids"][2]
    again = p.add_mesh(pos, idx, uv0=uv, build_tangents=True)
    assert p.meshes[again].block == 4 * align4(res["pool_words_after"]) and p.mesh_stats()["pool_words"] < st["pool_words"]
    p.close()
    a.close()


def test_mesh_compact_fraction(r3):
    """Renderer(mesh_compact=f): evaluate_instructions compacts when the holes exceed the fraction f of the mark, and not before."""
    rng = np.random.Generator(np.random.PCG64(0x3E53))
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream", mesh_compact=0.5)
    meshes = [p.add_mesh(*_facing_grid(rng, 5)[:2]) for _ in range(4)]
    mat = p.add_material(r3.material_record(albedo=(0.5, 0.5, 0.5, 1.0), albedo_mode="value"), 0)
    p.add_object(meshes[3], mat, oh.translation((0.0, 1.0, 0.0)))
    _light_and_camera(p)
    p.render(64, 64, readback=False, **KW)
    p.remove_mesh(meshes[0])
    p.render(64, 64, readback=False, **KW)
    assert p.mesh_stats()["compact_calls"] == 0  # a quarter is holes
    p.remove_mesh(meshes[1])
    p.remove_mesh(meshes[2])
    f1 = p.render(64, 64, **KW)
    st = p.mesh_stats()
    assert st["compact_calls"] == 1 and st["free_ranges"] == 0 and p.meshes[meshes[3]].block == 0
    f2 = p.render(64, 64, **KW)
    assert np.array_equal(f1["hdr16"], f2["hdr16"]) and (f1["hdr16"] != 0).any() and p.mesh_stats()["compact_calls"] == 1
    p.close()


# ------------------------------------------------------------------ 4. the waits
def test_no_stall_for_fresh_words_one_wait_for_parked_ones(r3):
    rng = np.random.Generator(np.random.PCG64(0x3E54))
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream")
    """With a frame in flight: a mesh added behind the high-water mark leaves full_waits of r3n_mesh_stats unchanged; one added
    into the words a removal freed since the last full wait raises it by exactly one.  (No hole is left in the buffer, so the
    second add has nowhere else to go; the device block doubles at the second add_mesh, which leaves room behind the mark.)"""
    p.add_mesh(*_facing_grid(rng, 17)[:2])  # 289 vertices, stays live
    small = p.add_mesh(*_facing_grid(rng, 5)[:2])
    mat = p.add_material(r3.material_record(albedo=(0.5, 0.5, 0.5, 1.0), albedo_mode="value"), 0)
    p.add_object(small, mat, oh.translation((0.0, 1.0, 0.0)))
    _light_and_camera(p)
    for _ in range(2):
        p.render(64, 64, readback=False, **KW)
    p.sync()
    pos, idx, _uv = _facing_grid(rng, 5)
    assert p.mesh_stats()["free_ranges"] == 0
    # ---- a frame in flight, fresh words
    p.render(64, 64, readback=False, **KW)
    s0 = p.mesh_stats()
    fresh = p.add_mesh(pos, idx)
    s1 = p.mesh_stats()
    assert s1["add_calls"] == s0["add_calls"] + 1 and s1["growths"] == s0["growths"]
    assert s1["full_waits"] == s0["full_waits"], "adding a mesh into fresh words waited for the frames in flight"
    assert p.meshes[fresh].block == 4 * align4(s0["pool_words"]), "behind the mark"
    # ---- a frame in flight, words freed since the last full wait
    p.render(64, 64, readback=False, **KW)
    where = p.meshes[fresh].block
    p.remove_mesh(fresh)
    s2 = p.mesh_stats()
    assert s2["full_waits"] == s1["full_waits"]  # a removal never waits
    again = p.add_mesh(pos, idx)
    s3 = p.mesh_stats()
    assert p.meshes[again].block == where, "the parked words were not reused"
    assert s3["full_waits"] == s2["full_waits"] + 1 and s3["growths"] == s2["growths"]
    p.add_object(again, mat, oh.translation((1.0, 1.0, 0.0)))
    out = p.render(64, 64, **KW)
    assert (out["hdr16"] != 0).any()
    p.close()


# ------------------------------------------------------------------ 5. the refusals
def _state(p):
    st = p.mesh_stats()
    words = p.readback_mesh_words(0, st["pool_words"]) if st["pool_words"] else np.zeros(0, dtype=np.uint32)
    return st, words


def _unchanged(p, state, tag):
    st, words = _state(p)
    assert st == state[0], tag + ": the pool or the counters changed"
    assert np.array_equal(words, state[1]), tag + ": the buffer changed"


def test_refusals_change_nothing(r3):
    rng = np.random.Generator(np.random.PCG64(0x3E55))
    p = r3.Renderer(oh.LEFT, f32(1.0), mesh_upload="stream")
    m0 = p.add_mesh(*_facing_grid(rng, 5)[:2])
    m1 = p.add_mesh(*_facing_grid(rng, 5)[:2])
    m2 = p.add_mesh(*_facing_grid(rng, 5)[:2])
    mat = p.add_material(r3.material_record(albedo=(0.5, 0.5, 0.5, 1.0), albedo_mode="value"), 0)
    p.add_object(m1, mat, oh.translation((0.0, 1.0, 0.0)))
    _light_and_camera(p)
    p.render(64, 64, readback=False, **KW)
    p.remove_mesh(m0)  # a hole in front: a compaction has something to do
    s0 = _state(p)
    # removing a mesh that an enabled object names
    with pytest.raises(ValueError):
        p.remove_mesh(m1)
    _unchanged(p, s0, "remove_mesh of a mesh in use")
    # something that is not a block start; a block named twice; a removed block
    for offs in ([p.meshes[m1].block + 16], [p.meshes[m2].block, p.meshes[m2].block], [0], [p.meshes[m1].block + 4]):
        assert raw_remove(p, offs) == INVALID_ARG and p.lib.r3n_last_error(p.ctx), offs
        _unchanged(p, s0, f"r3n_mesh_blocks_remove {offs}")
    # a too-small moves_capacity
    from rend3_amd import _ffi
    opts, out, moves = _ffi.MeshCompactOpts(), _ffi.MeshCompactResult(), (_ffi.MeshMove24 * 2)()
    assert p.lib.r3n_mesh_compact(p.ctx, ctypes.byref(opts), ctypes.byref(out), moves, 1) == INVALID_ARG
    assert b"moves_capacity" in p.lib.r3n_last_error(p.ctx)
    _unchanged(p, s0, "a too-small moves_capacity")
    opts.stage_words = 100
    assert p.lib.r3n_mesh_compact(p.ctx, ctypes.byref(opts), ctypes.byref(out), moves, 2) == INVALID_ARG
    _unchanged(p, s0, "stage_words 100")
    opts.stage_words = 0
    # bad add records: nothing is allocated
    rec, off_out, payload = (_ffi.MeshBlock24 * 2)(), np.zeros(2, dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    rec[0].words, rec[0].flags = 4, _ffi.MESH_BLOCK_ZERO
    for words, flags, payload_offset in ((0, 1, 0), (4, 2, 0), (16, 0, 0), (4, 0, 2), (4, 0, 32)):
        rec[1].words, rec[1].flags, rec[1].payload_offset = words, flags, payload_offset
        assert p.lib.r3n_mesh_blocks_add(p.ctx, rec, 2, _ffi.ptr(payload), payload.nbytes, _ffi.ptr(off_out)) == INVALID_ARG, (words, flags, payload_offset)
        _unchanged(p, s0, "a bad block record")
    rec[1].words, rec[1].flags = (1 << 30) + 4, 1
    assert p.lib.r3n_mesh_blocks_add(p.ctx, rec, 2, _ffi.ptr(payload), payload.nbytes, _ffi.ptr(off_out)) == -6  # R3N_ERR_CAPACITY
    _unchanged(p, s0, "a block past 2^32 bytes")
    # pooled calls inside a frame
    fu, clear = np.zeros(496, dtype=np.uint8), np.zeros(4, dtype=f32)
    assert p.lib.r3n_frame_begin(p.ctx, _ffi.ptr(fu), 16, 16, 1, _ffi.ptr(clear), 32, 32) == OK
    rec[1].words, rec[1].flags = 4, 1
    assert p.lib.r3n_mesh_blocks_add(p.ctx, rec, 2, _ffi.ptr(payload), payload.nbytes, _ffi.ptr(off_out)) == STATE
    assert b"inside a frame" in p.lib.r3n_last_error(p.ctx)
    assert raw_remove(p, [p.meshes[m2].block]) == STATE
    assert p.lib.r3n_mesh_compact(p.ctx, ctypes.byref(opts), ctypes.byref(out), moves, 2) == STATE
    assert p.lib.r3n_frame_end(p.ctx) == OK
    _unchanged(p, s0, "inside a frame")
    # the context still works
    res = p.compact_meshes()
    assert res["blocks_moved"] == 2 and p.meshes[m1].block == 0
    p.close()
    # r3n_mesh_blocks_add after an appending r3n_mesh_buffer_write
    q = r3.Renderer(oh.LEFT, f32(1.0))
    q.add_mesh(*_facing_grid(rng, 5)[:2])
    for call in (lambda: q.remove_mesh(0), q.compact_meshes):
        with pytest.raises(ValueError):
            call()
    s1 = q.mesh_stats()
    words = q.readback_mesh_words(0, q.mesh_cursor)
    assert q.lib.r3n_mesh_blocks_add(q.ctx, rec, 2, _ffi.ptr(payload), payload.nbytes, _ffi.ptr(off_out)) == STATE
    assert b"r3n_mesh_buffer_write" in q.lib.r3n_last_error(q.ctx)
    assert q.mesh_stats() == s1 and s1["blocks_live"] == 0 and s1["add_calls"] == 0 and np.array_equal(q.readback_mesh_words(0, q.mesh_cursor), words)
    q.close()
