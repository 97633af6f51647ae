"""Host logic (CPU, no GPU) of a live object count (include/cutrace_topology.h): object_added, mesh_added with the update's
steps and mesh_joined behind it, object_removed (scene_flatten.cpp) and the guard against flatten_scene of the edited description —
through scripts/topology_check.cpp, which states what it compares and fails on the first difference.  Here: the rows it ran, and the
range rules its lines show."""
import re

import pytest

from tests.checkers import check_report


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/topology_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "topology_check")


def _rows(report):
    """name -> dict(objects, meshes, planes, axis, tris_live, tris_total, nodes4_live, nodes4_total, tris_reused, nodes_reused, guarded)"""
    keys = ("objects", "meshes", "planes", "axis", "tris_live", "tris_total", "nodes4_live", "nodes4_total", "tris_reused", "nodes_reused", "guarded")
    out = {}
    for line in report:
        m = re.match(r"topology (.+?)\s+objects\s+(\d+) meshes (\d+) planes (\d+) axis (\d+) tris (\d+)/(\d+) nodes4 (\d+)/(\d+) reused (\d) (\d) guarded (\d+)$", line)
        if m:
            out[m.group(1)] = dict(zip(keys, (int(x) for x in m.groups()[1:])))
    return out


def test_each_type_leaves_and_joins_the_nine_object_room(report):
    r = _rows(report)
    for what in ("the sphere", "the triangle", "a wall", "the small mesh", "the big mesh"):
        assert r[f"room: remove {what}"]["objects"] == 8, what
    assert r["room: remove the small mesh"]["meshes"] == 1 and r["room: remove the big mesh"]["meshes"] == 1
    assert r["room: remove the big mesh"]["tris_live"] == 1 + 12 + 64         # the stand-alone triangle, the small mesh and its spare records
    assert r["room: remove all five in a row"] == dict(r["room: remove all five in a row"], objects=4, meshes=0, tris_live=0, nodes4_live=0)
    for what in ("a sphere", "a plane", "a triangle", "a mesh of 12", "a mesh of 70"):
        assert r[f"room: add {what}"]["objects"] == 10, what
    assert r["room: add a triangle"]["tris_total"] == r["room: add a sphere"]["tris_total"] + 1
    assert r["room: add a mesh of 12"]["tris_total"] == r["room: add a sphere"]["tris_total"] + 12 + 64 and r["room: add a mesh of 12"]["meshes"] == 3
    assert r["room: add all five in a row"]["objects"] == 14 and r["room: add all five in a row"]["meshes"] == 4


def test_the_top_level_tree_follows_the_mesh_count(report):
    r = _rows(report)
    assert [r[f"meshes {k}"]["meshes"] for k in ("1 -> 2", "2 -> 1", "1 -> 0", "0 -> 1")] == [2, 1, 0, 1]
    assert r["meshes 1 -> 0"]["tris_live"] == 0 and r["meshes 1 -> 0"]["nodes4_live"] == 0
    assert (r["meshes 0 -> 1"]["tris_reused"], r["meshes 0 -> 1"]["nodes_reused"]) == (1, 1)
    assert r["meshes 0 -> 1"]["tris_total"] == r["meshes 1 -> 2"]["tris_total"]
    assert r["six meshes: remove the third"]["meshes"] == 5 and r["six meshes: add one back"]["meshes"] == 6


def test_planes_repack_between_triples_and_pairs(report):
    r = _rows(report)
    assert (r["planes 5 -> 4"]["planes"], r["planes 5 -> 4"]["axis"]) == (3, 3)
    assert (r["planes 4 -> 2: general pairs"]["planes"], r["planes 4 -> 2: general pairs"]["axis"]) == (1, 0)
    assert (r["planes 2 -> 5: triples again"]["planes"], r["planes 2 -> 5: triples again"]["axis"]) == (3, 3)
    assert (r["planes 5 -> 6: a general one beside the triple"]["planes"], r["planes 5 -> 6: a general one beside the triple"]["axis"]) == (4, 3)


def test_an_emptied_scene_takes_objects_again(report):
    r = _rows(report)
    e = r["remove everything"]
    assert (e["objects"], e["meshes"], e["planes"], e["tris_live"], e["nodes4_live"]) == (0, 0, 0, 0, 0) and e["tris_total"] > 0
    assert r["empty: add a triangle"]["tris_reused"] == 1 and r["empty: add a triangle"]["tris_live"] == 1
    full = r["empty: add a sphere, a plane, a mesh of 12"]
    assert (full["objects"], full["meshes"], full["tris_reused"], full["nodes_reused"]) == (4, 1, 1, 1) and full["tris_total"] == e["tris_total"]
    assert full["tris_live"] == 1 + 70 + 64                                   # the lowest-addressed range that fits is the big mesh's, taken whole
    assert r["remove an empty mesh"]["objects"] == 2


def test_a_steady_spawn_and_despawn_stops_growing_the_arrays(report):
    r = _rows(report)
    rounds = [r[f"steady state: round {k}"] for k in range(8)]
    assert [(x["tris_reused"], x["nodes_reused"]) for x in rounds] == [(0, 0)] + [(1, 1)] * 7
    assert len({(x["tris_total"], x["nodes4_total"]) for x in rounds}) == 1
    assert len({(x["tris_live"], x["nodes4_live"]) for x in rounds}) == 1
    grown = r["a mesh of 71 after one of 70: appended"]
    assert (grown["tris_reused"], grown["tris_total"]) == (0, rounds[0]["tris_total"] + 71 + 64)
    whole = r["a mesh of 30 into the range of 70: whole"]
    assert whole["tris_reused"] == 1 and whole["tris_total"] == grown["tris_total"] and whole["tris_live"] == grown["tris_live"] + 70 + 64


def test_the_guard_follows_a_mirror_that_comes_and_goes(report):
    r = _rows(report)
    assert r["mirror wall: add a mesh with 5 in z = 0.5"]["guarded"] == 5 and r["mirror wall: remove the wall"]["guarded"] == 0
    assert "refusals: hold" in report
