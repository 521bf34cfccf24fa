"""Who owns the context's GPU resources, read from the source without a GPU: r3n.hip holds every device block, pinned block, event
and stream in an owning type of csrc/hip_owned.h (or a DeviceSpan view), so it never calls the HIP allocation / creation /
destruction entry points itself and carries no free lists; and the build table names every header a unit reaches, so an edit to
any of them rebuilds the unit (tests/test_resources_gpu.py holds the ledger of live resources to its baseline on the device)."""
import os
import re

from rend3_amd import build

CSRC = build.CSRC
RAW_CALLS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreate", "hipEventDestroy(", "hipStreamCreate",
             "hipStreamDestroy(")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_r3n_hip_calls_no_raw_resource_entry_point():
    host = _read("r3n.hip")
    assert [c for c in RAW_CALLS if c in host] == []
    owned = _read("hip_owned.h")
    assert [c for c in RAW_CALLS if c.rstrip("(") not in owned] == []  # ... because hip_owned.h is where they are used
    assert "__global__" not in owned and "__device__" not in owned  # host-only


def test_the_free_lists_are_gone():
    host = _read("r3n.hip")
    assert "free_cam" not in host
    assert re.search(r"\bDevBuf\b", host) is None
    assert '#include "hip_owned.h"' in host


def test_build_table_names_the_new_header_and_the_arithmetic_contract():
    assert "hip_owned.h" in build.UNITS["r3n.hip"]
    assert "exact_math.h" in build.COMMON


def _reached(path, seen):
    """every file the quoted #include lines reach from `path`, transitively"""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if target not in seen:
            seen.add(target)
            _reached(target, seen)
    return seen


def test_every_reached_header_is_a_dependency_of_its_unit():
    for unit in build.UNITS:
        deps = {os.path.normpath(d) for d in build._deps(unit)}
        missing = sorted(os.path.relpath(p, CSRC) for p in _reached(os.path.join(CSRC, unit), set()) - deps)
        assert missing == [], (unit, missing)
