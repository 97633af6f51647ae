"""Mesh updates (include/cutrace_update.h) measured on scene/bunny.json's mesh (1000 triangles) and on the 64 000-triangle bunny,
20 repetitions after warm-up, medians with their spread (min .. max) -> profiles/mesh_update/update.txt (or --out DIR).

  (a) update_mesh from a device tensor and from a host array against destroy + create of the same description, same process
  (b) the split of the update's time (CUTRACE_DEBUG_UPDATE=1, a child process: the phases are printed by the library)
  (c) the 1920x1080 frame on the updated handle against a fresh handle, after a rigid rotation by 30 degrees and after a twist
      of 90 degrees along the mesh's long axis: the price of a refitted tree against a rebuilt one
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 20, 3


def stat(xs):
    xs = sorted(xs)
    return "%8.3f ms (%.3f .. %.3f)" % (xs[len(xs) // 2], xs[0], xs[-1])


def rotated(t, deg, twist=False):
    """about the mesh's centre: a rigid rotation about y by `deg`, or a twist about the long axis growing from 0 to `deg`"""
    p = t.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    c = 0.5 * (lo + hi)
    q = p - c
    ax = int(np.argmax(hi - lo)) if twist else 1
    u, v = [a for a in range(3) if a != ax]
    ang = np.radians(deg) * ((q[:, ax] - (lo - c)[ax]) / (hi - lo)[ax] if twist else 1.0)
    out = q.copy()
    out[:, u] = q[:, u] * np.cos(ang) - q[:, v] * np.sin(ang)
    out[:, v] = q[:, u] * np.sin(ang) + q[:, v] * np.cos(ang)
    return (out + c).astype(np.float32).reshape(t.shape)


def scene_json(d, name, base_json, tris):
    from cutrace_amd import scenes
    sc = json.load(open(base_json))
    stl = os.path.join(d, name + ".stl")
    scenes.write_stl(stl, tris)
    for o in sc["objects"]:
        if o["type"] == "mesh":
            o["file"] = stl
    path = os.path.join(d, name + ".json")
    json.dump(sc, open(path, "w"))
    return path


def mesh_of(sc_json):
    from cutrace_amd import scenes
    sc = json.load(open(sc_json))
    obj = next(i for i, o in enumerate(sc["objects"]) if o["type"] == "mesh")
    f = sc["objects"][obj]["file"]
    return obj, scenes.read_stl(f if os.path.isabs(f) else os.path.join(ROOT, f))


def cases(d):
    from cutrace_amd import scenes
    return (("bunny.json, 1000 triangles", os.path.join(ROOT, "scene", "bunny.json")), ("dense bunny, 64 000 triangles", scenes.make_dense_bunny(d, 3)))


def child_split():
    import torch
    import cutrace_amd as ca
    d = tempfile.mkdtemp()
    for name, path in cases(d):
        obj, base = mesh_of(path)
        ds = ca.DeviceScene(ca.HostScene.load(path))
        sets = [torch.from_numpy(rotated(base, a)).cuda() for a in (10.0, -10.0)]
        for k in range(WARM + REPS):
            if k == WARM:
                print("== split", name, flush=True)
                sys.stderr.flush()
            ds.update_mesh(obj, sets[k % 2])
        sys.stderr.flush()
        ds.close()


def main(out_dir):
    import torch
    import cutrace_amd as ca
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    d = tempfile.mkdtemp()
    say("mesh updates on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    for name, path in cases(d):
        obj, base = mesh_of(path)
        sets = [rotated(base, a) for a in (10.0, -10.0)]
        hosts = [ca.HostScene.load(scene_json(d, "set%d_%d" % (k, len(base)), path, t)) for k, t in enumerate(sets)]
        dev_sets = [torch.from_numpy(t).cuda() for t in sets]
        ds = ca.DeviceScene(hosts[0])
        ds.render(pinned=True)
        t_dev, t_host, t_create = [], [], []
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.update_mesh(obj, dev_sets[k % 2])
            t1 = time.perf_counter()
            ds.update_mesh(obj, sets[(k + 1) % 2])
            t2 = time.perf_counter()
            if k >= WARM:
                t_dev.append((t1 - t0) * 1e3)
                t_host.append((t2 - t1) * 1e3)
        ds.close()
        ds = ca.DeviceScene(hosts[0])
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.close()
            ds = ca.DeviceScene(hosts[(k + 1) % 2])
            if k >= WARM:
                t_create.append((time.perf_counter() - t0) * 1e3)
        ds.close()
        say()
        say("(a) %s" % name)
        say("    update_mesh, device tensor   %s" % stat(t_dev))
        say("    update_mesh, host array      %s" % stat(t_host))
        say("    destroy + create             %s" % stat(t_create))
        say("    create / update (device)     %.1fx" % (sorted(t_create)[REPS // 2] / sorted(t_dev)[REPS // 2]))
    # (b)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "split"], env=dict(os.environ, CUTRACE_DEBUG_UPDATE="1"), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout
    phases, case = {}, None
    for line in out.splitlines():
        if line.startswith("== split"):
            case = line[9:]
        m = re.match(r"cutrace_amd update_mesh: (.+?)\s+([0-9.]+) ms$", line)
        if m and case:
            phases.setdefault(case, {}).setdefault(m.group(1), []).append(float(m.group(2)))
    say()
    say("(b) the split of update_mesh from a device tensor (the kernels waited for separately)")
    for case, ph in phases.items():
        say("    %s" % case)
        for what, xs in ph.items():
            say("      %-26s %s" % (what, stat(xs[-REPS:])))
    # (c)
    say()
    say("(c) 1920x1080 frame, kernel time: handle updated from the original mesh against a handle created from the moved mesh")
    for name, path in cases(d):
        obj, base = mesh_of(path)
        for what, tris in (("rigid rotation by 30 degrees", rotated(base, 30.0)), ("twist of 90 degrees along the long axis", rotated(base, 90.0, twist=True))):
            upd = ca.DeviceScene(ca.HostScene.load(path))
            upd.update_mesh(obj, tris)
            fresh = ca.DeviceScene(ca.HostScene.load(scene_json(d, "c_%d_%d" % (len(base), len(what)), path, tris)))
            ms = {}
            for label, h in (("updated", upd), ("fresh", fresh)):
                h.set_size(1920, 1080)
                ms[label] = [h.render(pinned=True)["kernel_ms"] for _ in range(WARM + REPS)][WARM:]
            same = np.array_equal(upd.render(pinned=True)["depth"].view(np.uint32), fresh.render(pinned=True)["depth"].view(np.uint32))
            say("    %-30s %-40s updated %s   fresh %s   ratio %.3f   depth bitwise equal: %s" %
                (name, what, stat(ms["updated"]), stat(ms["fresh"]), sorted(ms["updated"])[REPS // 2] / sorted(ms["fresh"])[REPS // 2], same))
            upd.close()
            fresh.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "update.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "split":
        child_split()
    else:
        main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_update"))
