"""Host logic (CPU, no GPU) of the mesh rebuilds (include/cutrace_rebuild.h): the linear-BVH text of
cutrace_amd/csrc/lbvh.h run on the host, the acceptance check in front of every device-built tree, and mesh_rebuilt with the
update's steps and the guard behind it (scene_flatten.cpp, guard.cpp) — through scripts/mesh_rebuild_check.cpp, which states what
it checks.  Plus the declaration of the one entry point and the argument checks that need neither a handle nor a device."""
import ctypes as C
import os
import re

import pytest

from cutrace_amd import _lib
from tests.checkers import CSRC, ROOT, check_report, declared



@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/mesh_rebuild_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "mesh_rebuild_check")


def _max_levels():
    return int(re.search(r"#define\s+BVH4_MAX_DEPTH\s+(\d+)", open(os.path.join(CSRC, "bvh.h")).read()).group(1)) + 1


def _trees(report):
    trees = {}
    for line in report:
        m = re.match(r"lbvh (.+?)\s+triangles\s+(\d+) nodes\s+(\d+) levels\s+(\d+) host_nodes\s+(\d+) host_levels\s+(\d+)$", line)
        if m:
            trees[m.group(1)] = dict(zip(("triangles", "nodes", "levels", "host_nodes", "host_levels"), (int(x) for x in m.groups()[1:])))
    return trees


def test_the_builders_text_gives_trees_the_kernels_may_walk(report):
    """Every set the issue names went through the builder's text and the checks behind it (every triangle in one leaf of
    1 .. BVH_LEAF, child after parent, level_schedule, boxes that hold what lies below: the program fails on the first that
    does not hold); here: they were all there, and their shapes are what the sizes promise."""
    trees = _trees(report)
    for n in (1, 2, 4, 5, 64, 65, 1000, 20000):
        assert trees[f"random {n}"]["triangles"] == n
    for name in ("70 identical triangles", "flat in x", "centroids on a line", "geometric cluster"):
        assert name in trees
    for n in (1, 2, 4):                                         # one leaf: one node, one level
        assert (trees[f"random {n}"]["nodes"], trees[f"random {n}"]["levels"]) == (1, 1)
    assert trees["random 65"]["levels"] >= 2 and trees["random 20000"]["levels"] >= 5
    assert trees["70 identical triangles"]["levels"] <= 4       # equal keys split by position: balanced, not a chain of 70
    assert all(t["levels"] <= _max_levels() for t in trees.values())
    # the set tests/test_gpu_mesh_rebuild.py rebuilds for its stack test: deeper than the tree the handle was created with
    assert trees["geometric cluster of 200"]["levels"] > trees["geometric cluster of 200"]["host_levels"]
    for name, t in trees.items():
        print(f"{name}: {t}")


def test_the_morton_staircase_is_refused(report):
    """63 keys with a highest bit of their own each: one peels off per split.  The collapsed tree needs more levels than the
    walk's stack holds, and the acceptance check says no — the call then builds on the host (tests/test_gpu_mesh_rebuild.py)."""
    m = [re.match(r"staircase triangles (\d+) levels (\d+) accepted (\d)$", line) for line in report]
    (m,) = [x for x in m if x]
    tris, levels, accepted = (int(x) for x in m.groups())
    print("staircase levels:", levels)
    assert tris == 63
    assert levels > _max_levels()
    assert accepted == 0
    assert "broken trees refused" in report


def test_mesh_rebuilt_on_the_host(report):
    assert "install in place: moved 0" in report                # bvh4_build's own tree: byte for byte the fresh scene (same_flat)
    m = [re.match(r"install leaf size 1: moved (\d) nodes (\d+) range (\d+)$", line) for line in report]
    (m,) = [x for x in m if x]
    moved, nodes, room = (int(x) for x in m.groups())
    assert moved == 1 and nodes > room
    rebuilds = {m.group(1).strip(): (int(m.group(2)), int(m.group(3)))
                for m in (re.match(r"rebuild (.+?)\s+guarded\s+(\d+) linear (\d) nodes\s+\d+$", line) for line in report) if m}
    for name in ("one mesh, LBVH tree", "two meshes, leaf size 1: moved", "two meshes, back to leaf size 4: in place"):
        assert rebuilds[name] == (0, 0)
    assert rebuilds["moved"] == (0, 0)
    assert rebuilds["3 in the eye's plane"] == (3, 0)                      # guard records
    assert rebuilds["70 in the eye's plane"] == (0, 1)                     # more than the 64 slots: the linear fallback
    assert rebuilds["70 again: linear payload after refit"] == (0, 1)
    assert rebuilds["none in the plane"] == (0, 0)                         # back to culling
    assert "reflective mesh rebuilt" in rebuilds and "reflective mesh rebuilt: the other mesh" in rebuilds


def test_rebuild_entry_point_is_declared_and_checks_its_arguments_without_a_device():
    names = declared("cutrace_rebuild.h")
    assert set(names) == set(_lib.REBUILD_SYMBOLS) == {"ctr_scene_rebuild_mesh"}
    L = _lib.hip_lib()
    later = {h: set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_rebuild.h"}
    assert not any(set(names) & t for t in later.values())                # in no other table
    assert not any(n in symbols for symbols in _lib.HIP_PROTOS.values() for n in names)
    assert not set(names) & set(_lib.HOST_SYMBOLS)
    assert set(declared("cutrace_update.h")) == {"ctr_scene_update_mesh", "ctr_scene_mesh_box"}   # the neighbours' lists are as they were
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_rebuild.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert L.ctr_abi_version() == 3
    assert C.sizeof(_lib.RebuildInfo) == 32
    assert re.search(r"#define\s+CTR_REBUILD_HOST\s+1u", open(os.path.join(ROOT, "include", "cutrace_rebuild.h")).read()) and _lib.REBUILD_HOST == 1
    tri = (_lib.Triangle * 1)()
    info = _lib.RebuildInfo()
    assert L.ctr_scene_rebuild_mesh(None, 0, C.cast(tri, C.c_void_p), 1, 0, C.byref(info), None) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_rebuild_mesh(None, 0, C.cast(tri, C.c_void_p), 1, 0, None, None) == 1 and b"null argument" in L.ctr_last_error()
    for flags in (2, 3, 0x80000000):
        assert L.ctr_scene_rebuild_mesh(None, 0, C.cast(tri, C.c_void_p), 1, flags, None, None) == 1 and b"unknown flag bits" in L.ctr_last_error()
