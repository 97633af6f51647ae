"""Host logic (CPU, no GPU) of the mesh replaces (include/cutrace_replace.h): mesh_replaced with the update's steps and
the guard behind it (scene_flatten.cpp, guard.cpp) against flatten_scene of the replaced description — through
scripts/mesh_replace_check.cpp, which states what it compares.  Plus the declaration of the one entry point and the argument checks
that need neither a handle nor a device."""
import ctypes as C
import os
import re

import pytest

from cutrace_amd import _lib
from tests.checkers import ROOT, check_report, declared



@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/mesh_replace_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "mesh_replace_check")


def _replaces(report):
    """name -> (count, tri_cap, tris_moved, nodes_moved, guarded, linear)"""
    out = {}
    for line in report:
        m = re.match(r"replace (.+?)\s+count\s+(\d+) tri_cap\s+(\d+) tris_moved (\d) nodes_moved (\d) guarded\s+(\d+) linear (\d)$", line)
        if m:
            out[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    return out


def test_the_triangle_range_stays_while_the_count_fits_and_doubles_when_it_does_not(report):
    """cases 1, 2, 7: every step compared with flatten_scene of the replaced description by the program (it fails on the first
    difference); here the range rules: in place at or below tri_cap, max(n, 2 * tri_cap) records at the end of the array above it"""
    r = _replaces(report)
    assert r["65 -> 5"][:4] == (5, 65, 0, 0)                               # shrink in place: the room stays what it was
    assert [r[f"-> {n}"][:3] for n in (66, 67, 130, 131)] == [(66, 130, 1), (67, 130, 0), (130, 130, 0), (131, 260, 1)]
    assert r["1 -> 1"][:4] == (1, 1, 0, 0)
    assert r["1 -> 1000"][:4] == (1000, 1000, 1, 1)                        # max(n, 2 * tri_cap) = n


def test_the_node_range_moves_on_its_own(report):
    """case 3: the same triangles under the host's builder with leaves of one triangle: more nodes than the range holds, and the
    triangle range stays; a later tree of the usual size fits the doubled room"""
    r = _replaces(report)
    assert r["65 -> 65, leaf size 1"][:4] == (65, 65, 0, 1)
    assert r["65 -> 70 after the node move"][:4] == (70, 130, 1, 0)


def test_a_stand_alone_triangle_and_the_other_mesh_are_not_disturbed(report):
    """case 4: mesh, stand-alone triangle, mesh, sphere; the program compares the triangle's record, the second mesh's ranges and its
    MeshGuard with what they were before, byte for byte"""
    r = _replaces(report)
    assert r["mixed: first mesh 40 -> 90"][:4] == (90, 90, 1, 1)
    assert r["mixed: second mesh 30 -> 7"][:4] == (7, 30, 0, 0)
    assert r["mixed: first mesh 90 -> 150"][:3] == (150, 180, 1)
    assert r["mixed: first mesh 150 -> 170"][:3] == (170, 180, 0)


def test_guard_states_follow_the_new_triangles(report):
    """case 5: guard records, the linear fallback, a linear mesh replaced into another linear state, back to culling, each at another
    count; case 6: a reflecting mesh is mirrors to the guard at 12 triangles and not at 20; case 8: rebuilds and updates afterwards"""
    r = _replaces(report)
    assert r["3 in the eye's plane, of 40"][4:] == (3, 0) and r["3 in the eye's plane, of 40"][0] == 40
    assert r["70 in the eye's plane, of 200"][4:] == (0, 1) and r["70 in the eye's plane, of 200"][0] == 200
    assert r["70 again, of 150, leaf size 2"][4:] == (0, 1) and r["70 again, of 150, leaf size 2"][0] == 150
    assert r["none in the plane, of 90"][4:] == (0, 0) and r["none in the plane, of 90"][0] == 90
    origins = {int(m.group(1)): int(m.group(2)) for m in (re.match(r"mirror mesh of (\d+): origins (\d+)$", line) for line in report) if m}
    assert origins[20] == 1 and origins[12] > 1, origins                   # CTR_MIRROR_MESH_TRIS = 16 lies between
    assert r["reflecting mesh -> 20"][:3] == (20, 24, 1) and r["reflecting mesh -> 12"][:3] == (12, 24, 0)
    assert "rebuild after replaces: moved 0" in report and "update after replaces: holds" in report


def test_replace_entry_point_is_declared_and_checks_its_arguments_without_a_device():
    names = declared("cutrace_replace.h")
    assert set(names) == set(_lib.REPLACE_SYMBOLS) == {"ctr_scene_replace_mesh"}
    L = _lib.hip_lib()
    later = {h: set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_replace.h"}
    assert not any(set(names) & t for t in later.values())                # in no other table
    assert not any(n in symbols for symbols in _lib.HIP_PROTOS.values() for n in names)
    assert not set(names) & set(_lib.HOST_SYMBOLS)
    assert set(declared("cutrace_rebuild.h")) == {"ctr_scene_rebuild_mesh"}                       # the neighbours' lists are as they were
    assert set(declared("cutrace_update.h")) == {"ctr_scene_update_mesh", "ctr_scene_mesh_box"}
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_replace.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert L.ctr_abi_version() == 3
    assert C.sizeof(_lib.ReplaceInfo) == 32
    assert re.search(r"#define\s+CTR_REPLACE_HOST\s+1u", open(os.path.join(ROOT, "include", "cutrace_replace.h")).read()) and _lib.REPLACE_HOST == 1
    tri = (_lib.Triangle * 1)()
    info = _lib.ReplaceInfo()
    assert L.ctr_scene_replace_mesh(None, 0, C.cast(tri, C.c_void_p), 1, 0, C.byref(info), None) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_replace_mesh(None, 0, C.cast(tri, C.c_void_p), 1, 0, None, None) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_replace_mesh(None, 0, None, 1, 0, None, None) == 1 and b"null argument" in L.ctr_last_error()
    for flags in (2, 3, 0x80000000):
        assert L.ctr_scene_replace_mesh(None, 0, C.cast(tri, C.c_void_p), 1, flags, None, None) == 1 and b"unknown flag bits" in L.ctr_last_error()
