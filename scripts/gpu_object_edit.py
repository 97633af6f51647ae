"""Object edits (include/cutrace_objects.h) measured on the bunny room plus one sphere, with the 1000-triangle mesh of
scene/bunny.json and with the 64 000-triangle bunny, 20 repetitions after warm-up, medians with their spread (min .. max) ->
profiles/object_edit/edit.txt (or --out DIR).  One GPU process; run it under a time limit of its own.

  (a) set_objects moving the sphere, and set_objects moving one reflecting wall (the eyes' images move with it: the guard plans
      anew), each against destroy + create of the edited description, same process: the path the parent commit offers
  (b) the first frame after an edit against the steady frame (the tile cost history is kept)
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.gpu_scene_edit import REPS, WARM, stat  # noqa: E402

SPHERE = {"type": "sphere", "material": 1, "center": [0.5, -0.6, 0.5], "radius": 0.25}
WALL = 2   # the wall z = -1 of scene/bunny.json: reflect 0.1, so a mirror of the guard


def room_with_sphere(d, name, base_json, changes=None):
    """base_json with the sphere appended (and {object index: {field: value}} applied); returns the path and the sphere's index"""
    sc = json.load(open(base_json))
    for o in sc["objects"]:
        if o["type"] == "mesh":
            o["file"] = o["file"] if os.path.isabs(o["file"]) else os.path.join(ROOT, o["file"])
    sc["objects"].append(dict(SPHERE))
    for i, kw in (changes or {}).items():
        sc["objects"][i].update(kw)
    path = os.path.join(d, name + ".json")
    json.dump(sc, open(path, "w"))
    return path, len(sc["objects"]) - 1


def time_edits(ds, obj, edit):
    """set_objects with object `obj` changed by edit(record, k) at every k; every other record as the handle has it"""
    objs = [ds.get_object(i) for i in range(ds.object_count())]
    ts = []
    for k in range(WARM + REPS):
        edit(objs[obj], k)
        t0 = time.perf_counter()
        ds.set_objects(objs)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts[WARM:]


def time_create(ca, paths):
    hosts = [ca.HostScene.load(p) for p in paths]
    ts = []
    ds = ca.DeviceScene(hosts[0])
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        ds.close()
        ds = ca.DeviceScene(hosts[(k + 1) % 2])
        ts.append((time.perf_counter() - t0) * 1e3)
    ds.close()
    return ts[WARM:]


def main(out_dir):
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    d = tempfile.mkdtemp()
    bases = (("bunny room + sphere, 1000 triangles", os.path.join(ROOT, "scene", "bunny.json")),
             ("bunny room + sphere, 64 000 triangles", scenes.make_dense_bunny(d, 3)))

    def move_sphere(o, k):
        o.v0 = ca.Vec3(0.5 + 0.01 * (k % 7), -0.6, 0.5 - 0.013 * (k % 5))

    def move_wall(o, k):
        o.v0 = ca.Vec3(0.0, 0.0, -1.0 - 0.01 * (k % 7))
    say("object edits on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    for name, base in bases:
        path, sphere = room_with_sphere(d, "room_%d" % len(name), base)
        ds = ca.DeviceScene(ca.HostScene.load(path))
        ds.render(pinned=True)
        t_sphere, t_wall = time_edits(ds, sphere, move_sphere), time_edits(ds, WALL, move_wall)
        ds.close()
        moved = {"sphere": [room_with_sphere(d, "sphere%d_%d" % (k, len(name)), base, {sphere: dict(center=[0.5 + 0.01 * (k + 1), -0.6, 0.5])})[0] for k in range(2)],
                 "wall": [room_with_sphere(d, "wall%d_%d" % (k, len(name)), base, {WALL: dict(point=[0, 0, -1.0 - 0.01 * (k + 1)])})[0] for k in range(2)]}
        say()
        say("(a) %s" % name)
        say("    set_objects, the sphere moved             %s" % stat(t_sphere))
        say("    destroy + create, the sphere moved        %s" % stat(time_create(ca, moved["sphere"])))
        say("    set_objects, a reflecting wall moved      %s" % stat(t_wall))
        say("    destroy + create, a reflecting wall moved %s" % stat(time_create(ca, moved["wall"])))
    say()
    say("(b) 1920x1080 frame, kernel time: the first frame after an edit against the steady frames before it")
    for name, base in bases:
        path, sphere = room_with_sphere(d, "frame_%d" % len(name), base)
        ds = ca.DeviceScene(ca.HostScene.load(path))
        ds.set_size(1920, 1080)
        steady = [ds.render(pinned=True)["kernel_ms"] for _ in range(WARM + REPS)][WARM:]
        for what, obj, edit in (("the sphere moved", sphere, move_sphere), ("a reflecting wall moved", WALL, move_wall)):
            objs = [ds.get_object(i) for i in range(ds.object_count())]
            first = []
            for k in range(REPS):
                edit(objs[obj], k)
                ds.set_objects(objs)
                first.append(ds.render(pinned=True)["kernel_ms"])
                ds.render(pinned=True)
            say("    %-38s steady %s   first after set_objects, %-24s %s" % (name, stat(steady), what, stat(first)))
        ds.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "edit.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "object_edit"))
