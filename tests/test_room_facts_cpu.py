"""The room facts of a launch (cutrace_amd/csrc/scene_flatten.cpp room_facts, fill_room_facts; DESIGN.md "Shadow casts from inside a
plane room") on the CPU, through scripts/room_facts_check.cpp, which states what it checks: a search for counter-examples of the
lemma in float (10^6 origins here; its default from the command line is 2 * 10^7), the two mutations under which the search
must find some, and the facts of the project's own scenes — where they must be set and where every word must be zero."""
import json
import os
import re

import pytest

import cutrace_amd as ca
from tests.checkers import FLATTEN_SOURCES, HOST_FLAGS, ROOT, check_output, check_program, write_scene

N = 1000000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return check_program(tmp_path_factory, "room_facts_check", HOST_FLAGS, FLATTEN_SOURCES)


def search(checker, *args):
    line = check_output(checker, [str(N), *args]).strip().splitlines()[-1]
    assert line.startswith("checked "), line
    words = line.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1) if re.fullmatch(r"\d+", words[i + 1])}
    print(line)
    return got


def test_the_search_finds_no_occluding_plane(checker):
    got = search(checker)
    assert got["origins"] >= N and got["safe_pairs"] > N // 4 and got["violations"] == 0, got
    # every case of the lemma that can occur is among the plane tests (c': a numerator above zero with a ray that runs away
    # from the wall needs a light behind that wall, and such a light has no bit)
    assert min(got["a"], got["b"], got["c"], got["d"]) > 1000, got


def test_an_eighth_of_the_margin_still_finds_none(checker):
    """the factor K of case b carries eight times what the search can break"""
    assert search(checker, "--k-div", "8")["violations"] == 0


def test_the_mutations_are_found(checker):
    """a tolerance eight times too wide, and a margin cut to where the roundings of t0 and light_dist reach it: K / 64 (K / 8 has
    to be safe, the test above; 2 * 10^7 origins find their first two counter-examples at K / 16)"""
    assert search(checker, "--delta-mul", "8")["violations"] > 0
    assert search(checker, "--k-div", "64")["violations"] > 0


# ---- the facts of whole scenes ----
def facts(checker, tmp_path, s, switch=False):
    path = str(tmp_path / "scene.bin")
    write_scene(path, s)
    env = dict(os.environ)
    env.pop("CUTRACE_NO_WALL_SKIP", None)
    if switch:
        env["CUTRACE_NO_WALL_SKIP"] = "1"
    out = check_output(checker, ["scene", path], env=env)
    assert out.startswith("facts "), out[-2000:]
    w = out.split()
    return dict(c=[float(x) for x in w[2:5]], r=float(w[6]), delta=float(w[8]), lights=int(w[10], 16), box_holds=int(w[12]),
                n_axis_recs=int(w[14]), plane_recs=int(w[16]), all_opaque=int(w[18]))


def all_zero(f):
    return f["c"] == [0.0, 0.0, 0.0] and f["r"] == 0.0 and f["delta"] == 0.0 and f["lights"] == 0


def load(name):
    s = ca.HostScene.load(os.path.join(ROOT, "scene", name))
    assert s.ok
    return s


def test_bunny_json(checker, tmp_path):
    f = facts(checker, tmp_path, load("bunny.json"))
    assert f["lights"] == 0xF and f["delta"] >= 2e-6 and f["box_holds"] == 1 and f["r"] > 0.0, f
    assert all_zero(facts(checker, tmp_path, load("bunny.json"), switch=True))


def test_scenes_without_facts(checker, tmp_path):
    f = facts(checker, tmp_path, load("mirror.json"))
    if f["plane_recs"] != 3 or f["n_axis_recs"] != 3:   # an oblique plane, or more than one triple
        assert all_zero(f), f
    f = facts(checker, tmp_path, load("sphere_plane.json"))
    assert f["all_opaque"] == 0 and all_zero(f), f


WALLS = [([-1, 0, 0], [1, 0, 0]), ([0, 0, -1], [0, 0, 1]), ([0, 1, 0], [0, -1, 0]), ([1, 0, 0], [-1, 0, 0]), ([0, -1, 0], [0, 1, 0])]


def room(lights, extra=()):
    objs = [{"type": "plane", "point": p, "normal": n, "material": 0} for p, n in WALLS] + list(extra)
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40}]
    cam = {"eye": [0, 0, 2.8], "up": [0, 1, 0], "look": [0.0, 0.0, -1.0], "near_plane": 0.1, "far_plane": 100.0, "width": 16, "height": 16, "ambient": 0.1}
    s = ca.HostScene.parse(json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs}))
    assert s.ok
    return s


def point(x, y, z):
    return {"type": "point", "point": [x, y, z], "color": [0.5, 0.5, 0.5]}


def test_rooms(checker, tmp_path):
    inside = [point(0.5, 0.8, 1.5), point(-0.6, 0.7, 1.0)]
    f = facts(checker, tmp_path, room(inside))
    assert f["lights"] == 0b11 and f["delta"] > 0 and f["box_holds"] == 1, f
    # a light outside a wall: only its bit is clear
    f = facts(checker, tmp_path, room(inside + [point(-1.001, 0.2, 0.5)]))
    assert f["lights"] == 0b011 and f["box_holds"] == 1, f
    # suns never qualify; a scene of suns has no facts
    sun = {"type": "sun", "direction": [0.3, -0.8, 0.5], "color": [0.5, 0.5, 0.5]}
    assert facts(checker, tmp_path, room([sun] + inside))["lights"] == 0b110
    assert all_zero(facts(checker, tmp_path, room([sun])))
    # an oblique plane: the triple no longer holds every plane
    f = facts(checker, tmp_path, room(inside, extra=[{"type": "plane", "point": [0, -0.9, 0], "normal": [0.1, 1, 0], "material": 0}]))
    assert all_zero(f), f
    # the switch
    assert all_zero(facts(checker, tmp_path, room(inside), switch=True))
