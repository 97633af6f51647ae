"""What the tests of a live object count (tests/test_gpu_topology.py; include/cutrace_topology.h) add to tests/live.py: the edited
description of a scene whose objects were removed and appended, and the handle created from it."""
import json

import numpy as np

from cutrace_amd import scenes
from tests.live import LIGHTS, MATERIALS, camera
from tests.util import parse

W, H = 48, 27
f32 = np.float32

WALLS = [{"type": "plane", "point": [-5, 0, 0], "normal": [1, 0, 0], "material": 1}, {"type": "plane", "point": [5, 0, 0], "normal": [-1, 0, 0], "material": 1},
         {"type": "plane", "point": [0, -3, 0], "normal": [0, 1, 0], "material": 1}, {"type": "plane", "point": [0, 8, 0], "normal": [0, -1, 0], "material": 1},
         {"type": "plane", "point": [0, 0, -6], "normal": [0, 0, 1], "material": 1}]
NEW_SPHERE = {"type": "sphere", "center": [1.5, -2.0, 4.0], "radius": 0.5, "material": 2}
NEW_WALL = {"type": "plane", "point": [0, 0, 9], "normal": [0, 0, -1], "material": 3}
NEW_TRIANGLE = {"type": "triangle", "p1": [2, -1, 5], "p2": [3, -0.5, 5.5], "p3": [2.5, 1, 5], "material": 1}


def without(sc, i):
    """a copy of the description with object `i` deleted"""
    out = json.loads(json.dumps(sc))
    del out["objects"][i]
    return out


def appended(sc, obj):
    """a copy of the description with `obj` as its last object"""
    out = json.loads(json.dumps(sc))
    out["objects"].append(obj)
    return out


def mesh_object(tmp_path, name, tris, material):
    """the description's entry of a mesh of `tris`, written where the loader finds it"""
    path = str(tmp_path / f"{name}.stl")
    scenes.write_stl(path, tris)
    return {"type": "mesh", "file": path, "material": material}


def add_described(ds, obj):
    """`obj`, an analytic object as a description names it, through DeviceScene.add_object"""
    fields = {k: v for k, v in obj.items() if k not in ("type", "material")}
    return ds.add_object(obj["type"], material=obj["material"], **fields)


def fresh_handle(ca, sc):
    """(the handle created from the description, its parsed scene)"""
    hs = parse(ca, sc)
    return ca.DeviceScene(hs), hs


def one_mesh_room(tmp_path, name, tris):
    """one mesh in a room of five axis-aligned walls, every material opaque: the one-mesh launch shape, and room facts"""
    return {"camera": camera([0.3, 0.2, -0.5], [0.0, 0.1, 1.0], W, H), "lights": LIGHTS, "materials": [MATERIALS[0], MATERIALS[1]],
            "objects": [mesh_object(tmp_path, name, tris, 0)] + WALLS}
