"""The planner of the cube uploads (rend3_amd/csrc/cube_plan.h: what r3n_texture_cubes_write, r3n_texture_cubes_write_encoded and
r3n_texture_cubes_write_sources decide before their first HIP call) on the CPU, through tests/cube_plan_check.cpp -- a stand-alone
program built plain and with the address and undefined-behaviour sanitizers and run as a child process.  The refusals are the rows
of tests/cube_refusals.py, the list the GPU tests send to the entries themselves."""
import os
import subprocess

import pytest

import cube_refusals as R
import host_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SRC = os.path.join(HERE, "cube_plan_check.cpp")
HEADERS = [os.path.join(ROOT, "rend3_amd", "csrc", h) for h in ("cube_plan.h", "cube_faces.h", "equirect.h", "equirect_rule.h", "texture_jobs.h",
                                                                 "vertex_block.h")]
HEADERS.append(os.path.join(ROOT, "include", "r3n.h"))


def program(sanitize):
    """Path of the built check program (built once, when its sources are newer); sanitize=False: a plain build under its own name."""
    return host_check.program(SRC, HEADERS, sanitize=sanitize)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_plans_hold_their_invariants(sanitize):
    """Inside the program: stored RGBA8 cubes of N = 1, 2, 3, 5 (full chains and one level), four one-level cubes in one array, a
    BC6H cube, an RGBE and a BC6H panorama, a 130 x 65 panorama with equirect_tail 0 and 64, all of them in one array under four
    tails, the empty array.  Per array: bordered faces inside their cube and disjoint, levels and cubes on 4 words, decode jobs
    inside the payload and the dense words, every dense face written in front of the assemble, chain records fed by the level
    above, wave maps that give the wave counts back, scratch offsets ascending on 256 bytes, and the same plan from the descs of
    the encoded and the plain adapter."""
    res = subprocess.run([program(sanitize)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # a sanitizer report goes there
    lines = dict(line.split(" ", 1) for line in res.stdout.splitlines())
    assert set(lines) == {"arrays", "records", "jobs", "resampled", "failures"}, res.stdout
    assert lines["failures"] == "0"
    assert int(lines["arrays"]) == 4 * 2 + 1 + 1 + 2 + 2 + 4 + 1
    chains = 1 + 2 + 2 + 3  # levels of N = 1, 2, 3, 5
    singles = 6 * (chains + 4) + 6 * 4 + 6 * 4 + 6 * 3 + 6 * 3 + 2 * 6 * 3  # arrays of one kind: faces of every level
    mixed = 6 * (chains + 4 + 3 + 3 + 3 + 2)
    assert int(lines["records"]) == singles + 4 * mixed
    assert int(lines["jobs"]) > 0 and int(lines["resampled"]) > 0


def refusal(entry, cubes, payload_bytes, sanitize):
    args = [entry, str(payload_bytes), "64", str(len(cubes))]
    for cube in cubes:
        args += [str(int(v)) for v in cube]
    res = subprocess.run([program(sanitize), "refuse"] + args, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stdout + res.stderr
    code, _, message = res.stdout.strip().partition(" ")
    return int(code), message


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_refusals_are_the_entries_own(sanitize):
    """every row of the list the GPU tests send to the two entries, by code and by message; the rows that break two rules at once
    state the check that comes first"""
    assert len(R.ENCODED) >= 13 + 4 and len(R.SOURCES) >= 19 + 3
    for row in R.ENCODED:
        # (KIND FORMAT WIDTH HEIGHT EXTENT MIPS OFFSET STORED; a desc has no kind and no face extent of its own)
        cubes = [(0, d[4], d[1], d[2], d[1], d[3], d[0], d[5]) for d in R.encoded_cubes(row)]
        assert refusal("encoded", cubes, row[2], sanitize) == (row[3], row[4]), row[0]
    for row in R.SOURCES:
        cubes = [s + (0,) for s in R.source_cubes(row)]
        assert refusal("sources", cubes, row[2], sanitize) == (row[3], row[4]), row[0]
    # and what they accept: stored_mips == mips is the same as 0; the defaults of either list
    assert refusal("encoded", [(0, 0, 4, 4, 4, 3, 0, 3)], 4096, sanitize) == (0, "accepted")
    assert refusal("encoded", [(0, 0, 4, 4, 4, 1, 0, 0)], 4096, sanitize) == (0, "accepted")
    assert refusal("sources", [(1, R.RGBE8, 8, 4, 4, 1, 0, 0)], 4096, sanitize) == (0, "accepted")
    assert refusal("sources", [], 0, sanitize) == (0, "accepted")


def test_the_entries_are_adapters_over_one_plan():
    """r3n.hip holds no cube planning, no cube geometry and no second scratch layout; the build knows the header"""
    src = open(os.path.join(ROOT, "rend3_amd", "csrc", "r3n.hip")).read()
    for gone in ("cube_face_point", "cube_nearest_texel", "dense_at =", "asm_at =", "cube_faces::Record{", "equirect::FaceRec", "equirect::ChainRec"):
        assert gone not in src, gone
    assert src.count("cube_plan::plan(") == 1 and src.count("write_cube_plan(") == 2  # its definition and ONE call
    from rend3_amd import build
    assert "cube_plan.h" in build.UNITS["r3n.hip"]
    hdr = open(os.path.join(ROOT, "include", "r3n.h")).read()
    plain = hdr[hdr.index("/*      The cube textures"):hdr.index("int r3n_texture_cubes_write(")]
    assert "R3N_ERR_CAPACITY" in plain and "k_cube_assemble" in plain
