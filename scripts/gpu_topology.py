"""A live object count (include/cutrace_topology.h) measured in the rooms of scripts/gpu_mesh_update.py: scene/bunny.json and its
64 000-triangle version, 20 repetitions after warm-up, medians with their spread (min .. max) -> profiles/topology/topology.txt (or
--out DIR).  The baseline of every row is destroy + create of the edited description, timed in the same process.

  (a) add_object of a sphere, then remove_object of it, alternated on one handle
  (b) add_mesh of a second mesh of the room's own size from a device tensor, per builder: into a fresh range (a handle created per
      repetition, its creation not timed) and into a reused one (one handle, the mesh removed in between), and remove_object of it
  (c) the first 1920x1080 frame at bounces 5 after each edit, wall time, against the steady frame of the same handle
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_mesh_update import REPS, WARM, cases, mesh_of, rotated, stat  # noqa: E402
from gpu_mesh_rebuild import median  # noqa: E402

SPHERE = {"type": "sphere", "center": [0.1, 0.3, 0.2], "radius": 0.05, "material": 0}


def main(out_dir):
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return (time.perf_counter() - t0) * 1e3, out

    def create_times(host_a, host_b):
        """destroy + create of host_b's description, on a handle that alternates between the two"""
        ds = ca.DeviceScene(host_a)
        ts = []
        for k in range(2 * (WARM + REPS)):
            t0 = time.perf_counter()
            ds.close()
            ds = ca.DeviceScene(host_b if k % 2 == 0 else host_a)
            if k >= 2 * WARM and k % 2 == 0:
                ts.append((time.perf_counter() - t0) * 1e3)
        ds.close()
        return ts

    def first_frame(ds, edit, undo):
        """wall time of the first frame after `edit` and of the frame after that one, per repetition"""
        first, steady = [], []
        for k in range(WARM + REPS):
            edit()
            a = timed(lambda: ds.render(bounces=5, pinned=True))[0]
            b = timed(lambda: ds.render(bounces=5, pinned=True))[0]
            undo()
            if k >= WARM:
                first.append(a)
                steady.append(b)
        return first, steady

    d = tempfile.mkdtemp()
    say("a live object count on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    for name, path in cases(d):
        obj, base = mesh_of(path)
        sc = json.load(open(path))
        for o in sc["objects"]:
            if o["type"] == "mesh" and not os.path.isabs(o["file"]):
                o["file"] = os.path.join(ROOT, o["file"])
        n_obj, n = len(sc["objects"]), len(base)
        mat = sc["objects"][obj]["material"]
        second = rotated(base, 25.0) + np.float32([0.15, 0.0, 0.1])
        stl = os.path.join(d, "second_%d.stl" % n)
        scenes.write_stl(stl, second)

        def host(extra, tag):
            p = os.path.join(d, "%s_%d.json" % (tag, n))
            json.dump(dict(sc, objects=sc["objects"] + extra), open(p, "w"))
            return ca.HostScene.load(p)
        plain, with_sphere, with_mesh = host([], "plain"), host([SPHERE], "sphere"), host([{"type": "mesh", "file": stl, "material": mat}], "mesh")
        second_dev = torch.from_numpy(second).cuda()
        say()
        say("== %s" % name)

        # (a)
        ds = ca.DeviceScene(plain)
        ds.render(pinned=True)
        t_add, t_rm = [], []
        for k in range(WARM + REPS):
            a = timed(lambda: ds.add_object("sphere", material=0, center=SPHERE["center"], radius=SPHERE["radius"]))[0]
            b = timed(lambda: ds.remove_object(n_obj))[0]
            if k >= WARM:
                t_add.append(a)
                t_rm.append(b)
        t_create, t_back = create_times(plain, with_sphere), create_times(with_sphere, plain)
        say("(a) add_object (a sphere)            %s   destroy + create %s   %.0fx" % (stat(t_add), stat(t_create), median(t_create) / median(t_add)))
        say("    remove_object (the sphere)       %s   destroy + create %s   %.0fx" % (stat(t_rm), stat(t_back), median(t_back) / median(t_rm)))
        ds.set_size(1920, 1080)
        first, steady = first_frame(ds, lambda: ds.add_object("sphere", material=0, center=SPHERE["center"], radius=SPHERE["radius"]), lambda: ds.remove_object(n_obj))
        say("(c) first 1080p frame after add_object %s   the next frame %s" % (stat(first), stat(steady)))
        ds.close()

        # (b)
        t_create, t_back = create_times(plain, with_mesh), create_times(with_mesh, plain)
        for builder in ("device", "host"):
            fresh, info = [], None
            for k in range(WARM + REPS):
                h = ca.DeviceScene(plain)
                h.render(pinned=True)
                t, info = timed(lambda: h.add_mesh(second_dev, material=mat, builder=builder))
                h.close()
                if k >= WARM:
                    fresh.append(t)
            say("(b) add_mesh of %d, %-6s builder, fresh range    %s   destroy + create %s   %.1fx   %s" %
                (n, builder, stat(fresh), stat(t_create), median(t_create) / median(fresh), info))
            ds = ca.DeviceScene(plain)
            ds.render(pinned=True)
            ds.add_mesh(second_dev, material=mat, builder=builder)
            ds.remove_object(n_obj)
            reused, removed = [], []
            for k in range(WARM + REPS):
                a, info = timed(lambda: ds.add_mesh(second_dev, material=mat, builder=builder))
                b = timed(lambda: ds.remove_object(n_obj))[0]
                if k >= WARM:
                    reused.append(a)
                    removed.append(b)
            say("    add_mesh of %d, %-6s builder, reused range   %s   destroy + create %s   %.1fx   %s" %
                (n, builder, stat(reused), stat(t_create), median(t_create) / median(reused), info))
            say("    remove_object (that mesh)                      %s   destroy + create %s   %.0fx" % (stat(removed), stat(t_back), median(t_back) / median(removed)))
            ds.set_size(1920, 1080)
            first, steady = first_frame(ds, lambda: ds.add_mesh(second_dev, material=mat, builder=builder), lambda: ds.remove_object(n_obj))
            say("(c) first 1080p frame after add_mesh, %-6s builder  %s   the next frame %s" % (builder, stat(first), stat(steady)))
            ds.add_mesh(second_dev, material=mat, builder=builder)
            first, steady = first_frame(ds, lambda: ds.remove_object(n_obj), lambda: ds.add_mesh(second_dev, material=mat, builder=builder))
            say("    first 1080p frame after remove_object            %s   the next frame %s" % (stat(first), stat(steady)))
            fresh_h = ca.DeviceScene(with_mesh)
            fresh_h.set_size(1920, 1080)
            same = np.array_equal(ds.render(bounces=5)["depth"].view(np.uint32), fresh_h.render(bounces=5)["depth"].view(np.uint32))
            say("    depth of the edited handle bitwise equal to a fresh handle's: %s" % same)
            fresh_h.close()
            ds.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "topology.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "topology"))
