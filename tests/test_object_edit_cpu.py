"""Host logic (CPU, no GPU) of the object edits (include/cutrace_objects.h): check_objects / objects_edited / object_of of
scene_flatten.cpp with the guard behind them, run through scripts/object_edit_check.cpp, which states what it checks: every edit
of its rows applied to ONE flat scene against flatten_scene of the edited description, byte for byte."""
import re

import pytest

from tests.checkers import ROOT, check_report

A, B, C_ = "a: planes, spheres, triangles", "b: box room", "c: two meshes"
ROWS = [A, B, B + " (merged)", C_, C_ + " (merged)"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/object_edit_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "object_edit_check", cwd=ROOT)


def _edits(report):
    """scene -> step -> the plane packing and guard counts of the edited scene (which equalled the freshly flattened one, or the program failed)"""
    edits = {}
    for line in report:
        m = re.match(r"edit (.+?) \| (.+?) \| planes (\d+) axis (\d+) guarded (\d+) linear (\d+) mirrors (\d+)$", line)
        if m:
            edits.setdefault(m.group(1), {})[m.group(2)] = dict(zip(("planes", "axis", "guarded", "linear", "mirrors"), (int(x) for x in m.groups()[2:])))
    return edits


def _rejects(report):
    rejects = {}
    for line in report:
        m = re.match(r"reject (.+?) \| (.+?) \| untouched$", line)
        if m:
            rejects.setdefault(m.group(1), set()).add(m.group(2))
    return rejects


def test_every_scene_went_through_the_row_of_edits(report):
    edits = _edits(report)
    assert set(edits) == set(ROWS)
    for row in ROWS:
        steps = set(edits[row])
        assert {"nothing changed", "everything transparent", "everything as it was", "materials 0 and 1 swapped on every object",
                "a point light in z = 0.5", "every plane takes the new material", "the first lights again"} <= steps, row
        assert any(re.match(r"sphere #\d+ radius 0$", s) for s in steps) and any(re.match(r"sphere #\d+ moved$", s) for s in steps), row
        for what in ("tilted off its axis", "back on its axis", "point beyond 1e37", "normal with -0.0 components", "zero normal"):
            assert any(re.match(rf"plane #\d+ {re.escape(what)}$", s) for s in steps), (row, what)
    for row in (A, B, B + " (merged)"):
        assert any(re.match(r"triangle #\d+ three points moved$", s) for s in edits[row]), row
    # every object type through opaque -> transparent -> opaque and not reflecting -> reflecting -> back
    for row, types in ((A, (0, 2, 3)), (B, (0, 1, 2, 3)), (C_, (1, 2, 3))):
        for t in types:
            for what in ("transparent", "opaque", "reflecting", "its own material again"):
                assert any(re.match(rf"object #\d+ \(type {t}\) {what}$", s) for s in edits[row]), (row, t, what)
    # ... and once more after the 70-triangle mesh was updated, where the refitted box has to survive (the program checks it)
    for row in (B, B + " (merged)"):
        assert "after mesh_updated" in edits[row]
        assert {"updated: " + s for s in edits[row] if not s.startswith("updated: ") and s != "after mesh_updated"
                and re.match(r"(nothing|sphere|triangle|plane|object|all but|the planes|every plane normal|everything|the (wall|mirror))", s)} <= set(edits[row]), row


def test_the_planes_are_packed_again_at_every_edit(report):
    """a plane that becomes or stops being axis-aligned changes which records exist and how many; fewer than three axis-aligned
    planes turn the whole array into general pairs"""
    room = _edits(report)[B]
    pack = lambda what: (room[what]["planes"], room[what]["axis"])
    assert pack("nothing changed") == (3, 3)                                     # five walls: one triple
    assert pack("plane #0 tilted off its axis") == (4, 3) and pack("plane #0 back on its axis") == (3, 3)
    assert pack("plane #0 point beyond 1e37") == (4, 3)                          # still axis-aligned, but out of the fast path's range
    assert pack("plane #0 normal with -0.0 components") == (3, 3)                # -0 counts as zero
    assert pack("plane #0 zero normal") == (4, 3)
    assert pack("all but two planes tilted") == (3, 0)                           # two axis-aligned ones left: five planes in general pairs
    assert pack("the planes back on their axes") == (3, 3)
    assert pack("every plane normal to y") == (9, 9)                             # three triples: more records than the scene was created with
    assert pack("every plane normal to y but the last, which is general") == (7, 6)
    assert pack("every plane general") == (3, 0) and pack("from general pairs to every plane normal to y but the last") == (7, 6)
    assert pack("the planes as they were") == (3, 3)
    no_mesh = _edits(report)[A]
    assert (no_mesh["nothing changed"]["planes"], no_mesh["nothing changed"]["axis"]) == (4, 3)
    assert (no_mesh["plane #0 tilted off its axis"]["planes"], no_mesh["plane #0 tilted off its axis"]["axis"]) == (2, 0)   # 3 -> 2 axis-aligned planes
    # four planes: all on one axis 6 records, three on it beside a general one 7 — the most four planes can need, from the fewest
    packs = {what: (no_mesh[what]["planes"], no_mesh[what]["axis"]) for what in no_mesh}
    assert packs["every plane normal to y"] == (6, 6) and packs["every plane normal to y but the last, which is general"] == (7, 6)
    assert packs["every plane general"] == (2, 0) and packs["from general pairs to every plane normal to y but the last"] == (7, 6)


def test_the_room_for_the_plane_records_is_the_worst_packing(report):
    """plane_records_at_most against flatten_scene over every spread of 1 .. 9 planes: a * 3 / 2 rounded up is NOT it for an even count"""
    bounds = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in (re.match(r"bound (\d+) planes \| worst packing (\d+) records \| at most (\d+)$", l) for l in report) if m}
    assert bounds == {1: (1, 1), 2: (1, 1), 3: (6, 6), 4: (7, 7), 5: (9, 9), 6: (10, 10), 7: (12, 12), 8: (13, 13), 9: (15, 15)}


def test_the_guard_follows_a_moving_mirror_and_reassigned_materials(report):
    edits = _edits(report)
    for row in (B, B + " (merged)"):
        for tag in ("", "updated: "):
            steps = edits[row]
            base = steps[tag + "nothing changed"]
            assert base["guarded"] == 0 and base["mirrors"] == 12                # the 12-triangle mesh reflects: each triangle a mirror
            assert steps[tag + "the wall reflects"]["mirrors"] == 13 and steps[tag + "the wall reflects"]["guarded"] == 0
            assert steps[tag + "the mirror moved: the eye's image in z = 0.5"]["guarded"] == 5
            assert steps[tag + "the mirror moved back"]["guarded"] == 0
            assert steps[tag + "the wall reflects no more"]["mirrors"] == 12
            # the 12-triangle mesh (object #6) losing and regaining its reflecting material; the 70-triangle one (#2) is too large to be a mirror
            assert steps[tag + "object #6 (type 1) opaque"]["mirrors"] == 0 and steps[tag + "object #6 (type 1) its own material again"]["mirrors"] == 12
            assert steps[tag + "object #2 (type 1) reflecting"]["mirrors"] == 12
            assert steps[tag + "object #7 (type 0) reflecting"]["mirrors"] == 13   # a stand-alone triangle
            assert steps[tag + "object #4 (type 3) reflecting"]["mirrors"] == 12   # a sphere is not flat
    assert edits[A]["object #0 (type 2) reflecting"]["mirrors"] == 1 and edits[A]["object #0 (type 2) its own material again"]["mirrors"] == 0


def test_every_rejection_leaves_the_flat_scene_untouched(report):
    rejects = _rejects(report)
    common = {"null objects", "one object fewer", "one object more", "a type above the last", "another type",
              "a material index one past the last", "a material index beyond 32 bits"}
    assert set(rejects) == set(ROWS)
    assert rejects[A] == common
    for row in ROWS[1:]:
        assert rejects[row] == common | {"a mesh with one triangle more", "a mesh with no triangle"}, row
