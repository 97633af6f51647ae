"""Mesh replaces (include/cutrace_replace.h) measured in the rooms of scripts/gpu_mesh_rebuild.py: scene/bunny.json and its 64 000-triangle
version, the mesh resized to the counts below, 20 repetitions after warm-up, medians with their spread (min .. max)
-> profiles/mesh_replace/replace.txt (or --out DIR).

  (a) replace_mesh from a device tensor, per builder: 64 000 -> 48 000 (in place), 48 000 -> 96 000 (both ranges move: a handle created
      at 48 000 for every repetition, its creation not timed), 1000 -> 1500 (moves, likewise) and 1500 -> 1000 -> 1500 on a handle that
      has moved already (in place); against destroy + create with the triangles the replace installs, same process
  (b) replace_mesh at an UNCHANGED count against rebuild_mesh, alternated on one handle: the same steps, so the replace should sit inside
      the rebuild's spread
  (c) the 1920x1080 frame at bounces 5, kernel time, on the replaced handles against a handle created with the same triangles
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_mesh_update import REPS, WARM, cases, mesh_of, rotated, scene_json, stat  # noqa: E402
from gpu_mesh_rebuild import median  # noqa: E402


def resized(base, n):
    """`n` triangles of the mesh `base`: its first n, or all of them and copies of the first ones shrunk a little about the mesh's
    centre (a shell just inside the surface), rotated by 10 degrees like the sets of the other two scripts"""
    p = base.reshape(-1, 3).astype(np.float64)
    c = 0.5 * (p.min(0) + p.max(0))
    out = [base[:n]]
    k = 1
    while sum(len(x) for x in out) < n:
        part = base[:n - sum(len(x) for x in out)]
        out.append(((part.astype(np.float64) - c) * (1.0 - 0.01 * k) + c).astype(np.float32))
        k += 1
    return rotated(np.concatenate(out), 10.0)


def main(out_dir):
    import torch
    import cutrace_amd as ca
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    d = tempfile.mkdtemp()
    say("mesh replaces on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    (_, small_path), (_, dense_path) = cases(d)
    tris, hosts, dev, objs = {}, {}, {}, {}   # by triangle count: the set, its description, the set on the device, the mesh's object index
    for path, counts in ((dense_path, (64000, 48000, 96000)), (small_path, (1000, 1500))):
        obj, base = mesh_of(path)
        for n in counts:
            tris[n] = resized(base, n)
            hosts[n] = ca.HostScene.load(scene_json(d, "n%d" % n, path, tris[n]))
            dev[n] = torch.from_numpy(tris[n]).cuda()
            objs[n] = obj

    def create_times(n_from, n_to):
        ds = ca.DeviceScene(hosts[n_from])
        ts = []
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.close()
            ds = ca.DeviceScene(hosts[n_to if k % 2 == 0 else n_from])
            if k >= WARM and k % 2 == 0:
                ts.append((time.perf_counter() - t0) * 1e3)
        ds.close()
        return ts

    # (a)
    handles = {}
    for n_from, n_to, fresh_each in ((64000, 48000, False), (48000, 96000, True), (1000, 1500, True), (1500, 1000, False)):
        say()
        say("(a) %d -> %d, device tensor%s" % (n_from, n_to, ": a handle created at %d per repetition" % n_from if fresh_each else ": one handle, back to %d in between" % n_from))
        t_create = create_times(n_from, n_to) + create_times(n_from, n_to)
        for builder in ("device", "host"):
            ts, info = [], None
            ds = None
            if not fresh_each:
                ds = ca.DeviceScene(hosts[n_from])
                if n_from == 1500:
                    ds.close()
                    ds = ca.DeviceScene(hosts[1000])              # (a handle that has moved already: created at 1000, room for 2000)
                    ds.replace_mesh(objs[1000], dev[1500], builder=builder)
                ds.render(pinned=True)
            for k in range(WARM + REPS):
                if fresh_each:
                    ds = ca.DeviceScene(hosts[n_from])
                    ds.render(pinned=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = ds.replace_mesh(objs[n_to], dev[n_to], builder=builder)
                t1 = time.perf_counter()
                if k >= WARM:
                    ts.append((t1 - t0) * 1e3)
                if fresh_each and k < WARM + REPS - 1:
                    ds.close()
                elif not fresh_each and k < WARM + REPS - 1:
                    ds.replace_mesh(objs[n_from], dev[n_from], builder=builder)
            say("    replace_mesh, %-6s builder %s   %s" % (builder, stat(ts), info))
            handles[(n_to, builder, n_from)] = ds
            if builder == "device":
                t_dev = ts
        say("    destroy + create at %-6d     %s" % (n_to, stat(t_create)))
        say("    create / replace (device)      %.1fx" % (median(t_create) / median(t_dev)))

    # (b)
    say()
    say("(b) replace_mesh at an unchanged count against rebuild_mesh, alternated on one handle, device tensor")
    for n in (64000, 1000):
        ds = ca.DeviceScene(hosts[n])
        ds.render(pinned=True)
        other = torch.from_numpy(rotated(tris[n], -10.0)).cuda()
        for builder in ("device", "host"):
            t = {"replace": [], "rebuild": []}
            for k in range(WARM + REPS):
                t0 = time.perf_counter()
                ds.replace_mesh(objs[n], other if k % 2 else dev[n], builder=builder)
                t1 = time.perf_counter()
                ds.rebuild_mesh(objs[n], dev[n] if k % 2 else other, builder=builder)
                t2 = time.perf_counter()
                if k >= WARM:
                    t["replace"].append((t1 - t0) * 1e3)
                    t["rebuild"].append((t2 - t1) * 1e3)
            inside = min(t["rebuild"]) <= median(t["replace"]) <= max(t["rebuild"])
            say("    %6d triangles, %-6s builder   replace %s   rebuild %s   replace's median inside the rebuild's spread: %s" %
                (n, builder, stat(t["replace"]), stat(t["rebuild"]), inside))
        ds.close()

    # (c)
    say()
    say("(c) 1920x1080 frame at bounces 5, kernel time, replaced handle against a handle created with the same triangles")
    for (n_to, builder, n_from), h in handles.items():
        fresh = ca.DeviceScene(hosts[n_to])
        ms, depth = {}, {}
        for label, x in (("replaced", h), ("fresh", fresh)):
            x.set_size(1920, 1080)
            ms[label] = [x.render(bounces=5, pinned=True)["kernel_ms"] for _ in range(WARM + REPS)][WARM:]
            depth[label] = x.render(bounces=5, pinned=True)["depth"].view(np.uint32).copy()
        say("    %6d -> %-6d %-6s builder   replaced %s   fresh %s   ratio %.3f   depth bitwise equal: %s" %
            (n_from, n_to, builder, stat(ms["replaced"]), stat(ms["fresh"]), median(ms["replaced"]) / median(ms["fresh"]), np.array_equal(depth["replaced"], depth["fresh"])))
        h.close()
        fresh.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "replace.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_replace"))
