"""Host logic (CPU, no GPU) of the mesh updates (include/cutrace_update.h): the level schedule and the per-slot refit arithmetic of
cutrace_amd/csrc/mesh_refit.h, the shared triangle records of tri_record.h, and mesh_updated with the guard behind it
(scene_flatten.cpp, guard.cpp) — run through scripts/mesh_update_check.cpp, which states what it checks.  Plus the argument
checks of the two entry points that need neither a handle nor a device."""
import ctypes as C
import os
import re

import pytest

from cutrace_amd import _lib
from tests.checkers import CSRC, check_report, declared



@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/mesh_update_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "mesh_update_check")


def _trees(report):
    trees = {}
    for line in report:
        m = re.match(r"tree (.+?)\s+triangles\s+(\d+) nodes\s+(\d+) levels\s+(\d+) identity_value_diff (\d+) identity_byte_diff (\d+)$", line)
        if m:
            trees[m.group(1)] = dict(zip(("triangles", "nodes", "levels", "value_diff", "byte_diff"), (int(x) for x in m.groups()[1:])))
    return trees


def test_level_schedule_and_refit_arithmetic(report):
    """Every tree the issue names went through the schedule and the refit checks (the program fails on the first that does not
    hold); here: they were all there, and their shapes are what the sizes promise."""
    trees = _trees(report)
    for n in (1, 4, 5, 64, 65, 1000, 20000):
        assert trees[f"random {n}"]["triangles"] == n
    for name in ("coincident points", "flat in x", "with zero coordinates", "geometric cluster"):
        assert name in trees
    for n in (1, 4):                                            # one leaf: one node, one level
        assert (trees[f"random {n}"]["nodes"], trees[f"random {n}"]["levels"]) == (1, 1)
    assert trees["random 5"]["nodes"] == 1 and trees["random 5"]["levels"] == 1     # two leaves under one root
    assert trees["random 65"]["levels"] >= 2 and trees["random 20000"]["levels"] >= 5
    depth = int(re.search(r"#define\s+BVH4_MAX_DEPTH\s+(\d+)", open(os.path.join(CSRC, "bvh.h")).read()).group(1))
    assert all(t["levels"] <= depth + 1 for t in trees.values())


def test_identity_refit_reproduces_the_builders_boxes(report):
    """As values always; byte for byte on every set here, the one with zero coordinates of either sign included (DESIGN.md §18
    says why only the sign of a zero could differ).  tests/test_gpu_mesh_update.py's identity case relies on this."""
    trees = _trees(report)
    assert trees and all(t["value_diff"] == 0 for t in trees.values())
    assert all(t["byte_diff"] == 0 for name, t in trees.items() if name != "with zero coordinates")
    print("identity refit, box words that differ in a sign of zero:", trees["with zero coordinates"]["byte_diff"])


def test_shared_records_and_the_update_on_the_host(report):
    assert "records tri_record.h against flatten_scene: 0 differ" in report
    updates = {m.group(1).strip(): (int(m.group(2)), int(m.group(3)))
               for m in (re.match(r"update (.+?)\s+guarded\s+(\d+) linear (\d)$", line) for line in report) if m}
    assert updates["moved"] == (0, 0)
    assert updates["3 in the eye's plane"] == (3, 0)                       # guard records
    assert updates["70 in the eye's plane"] == (0, 1)                      # more than the 64 slots: the linear fallback
    assert updates["70 again: linear payload after refit"] == (0, 1)
    assert updates["none in the plane"] == (0, 0)                          # back to culling
    assert "reflective mesh moved" in updates


def test_update_entry_points_are_declared_and_check_their_arguments_without_a_device():
    names = declared("cutrace_update.h")
    assert set(names) == set(_lib.UPDATE_SYMBOLS) == {"ctr_scene_update_mesh", "ctr_scene_mesh_box"}
    L = _lib.hip_lib()
    assert not set(names) & (set(_lib.HIP_SYMBOLS) | set(_lib.HOST_SYMBOLS))  # cutrace_amd.h and cutrace_host.h are unchanged
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_update.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n    # the prototype is applied
    assert not any(n in symbols for symbols in _lib.HIP_PROTOS.values() for n in names)   # no symbol in two tables
    assert L.ctr_abi_version() == 3
    tri = (_lib.Triangle * 1)()
    lo, hi = _lib.Vec3(), _lib.Vec3()
    assert L.ctr_scene_update_mesh(None, 0, C.cast(tri, C.c_void_p), 1, None) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_mesh_box(None, 0, C.byref(lo), C.byref(hi)) == 1 and b"null argument" in L.ctr_last_error()
