"""Mesh rebuilds (include/cutrace_rebuild.h) measured on scene/bunny.json's mesh (1000 triangles) and on the 64 000-triangle bunny
(the rooms of scripts/gpu_mesh_update.py), 20 repetitions after warm-up, medians with their spread (min .. max)
-> profiles/mesh_rebuild/rebuild.txt (or --out DIR).

  (a) the calls, from a device tensor: rebuild_mesh with the device builder, with the host builder, update_mesh, and destroy + create of
      the same description, same process
  (b) the split of the two rebuilds' time (CUTRACE_DEBUG_UPDATE=1, a child process: the stages are printed by the library)
  (c) the 1920x1080 frame at bounces 5, kernel time, on a fresh handle, the refit-only handle, the device-rebuilt and the host-rebuilt
      handle: after a rigid rotation by 30 degrees, a twist of 90 degrees along the long axis, and a fold that passes the mesh
      through itself
"""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_mesh_update import REPS, WARM, cases, mesh_of, rotated, scene_json, stat  # noqa: E402


def folded(t):
    """the half of the mesh beyond its centre, along its long axis, mirrored back through the other half"""
    p = t.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    ax = int(np.argmax(hi - lo))
    c = 0.5 * (lo[ax] + hi[ax])
    out = p.copy()
    out[:, ax] = c - np.abs(p[:, ax] - c) + 0.25 * (hi[ax] - lo[ax])
    return out.astype(np.float32).reshape(t.shape)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def child_split():
    import torch
    import cutrace_amd as ca
    d = tempfile.mkdtemp()
    for name, path in cases(d):
        obj, base = mesh_of(path)
        ds = ca.DeviceScene(ca.HostScene.load(path))
        sets = [torch.from_numpy(rotated(base, a)).cuda() for a in (10.0, -10.0)]
        for builder in ("device", "host"):
            for k in range(WARM + REPS):
                if k in (0, WARM):
                    print("== split %s builder, %s" % (builder, name) if k else "== warm-up", flush=True)
                    sys.stderr.flush()
                ds.rebuild_mesh(obj, sets[k % 2], builder=builder)
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
    say("mesh rebuilds on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    for name, path in cases(d):
        obj, base = mesh_of(path)
        sets = [rotated(base, a) for a in (10.0, -10.0)]
        hosts = [ca.HostScene.load(scene_json(d, "set%d_%d" % (k, len(base)), path, t)) for k, t in enumerate(sets)]
        dev_sets = [torch.from_numpy(t).cuda() for t in sets]
        ds = ca.DeviceScene(hosts[0])
        ds.render(pinned=True)
        t = {"dev": [], "host": [], "upd": [], "create": []}
        infos = {}
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            infos["dev"] = ds.rebuild_mesh(obj, dev_sets[k % 2], builder="device")
            t1 = time.perf_counter()
            infos["host"] = ds.rebuild_mesh(obj, dev_sets[(k + 1) % 2], builder="host")
            t2 = time.perf_counter()
            ds.update_mesh(obj, dev_sets[k % 2])
            t3 = time.perf_counter()
            if k >= WARM:
                t["dev"].append((t1 - t0) * 1e3)
                t["host"].append((t2 - t1) * 1e3)
                t["upd"].append((t3 - t2) * 1e3)
        ds.close()
        ds = ca.DeviceScene(hosts[0])
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.close()
            ds = ca.DeviceScene(hosts[(k + 1) % 2])
            if k >= WARM:
                t["create"].append((time.perf_counter() - t0) * 1e3)
        ds.close()
        say()
        say("(a) %s, device tensor" % name)
        say("    rebuild_mesh, device builder %s   %s" % (stat(t["dev"]), infos["dev"]))
        say("    rebuild_mesh, host builder   %s   %s" % (stat(t["host"]), infos["host"]))
        say("    update_mesh                  %s" % stat(t["upd"]))
        say("    destroy + create             %s" % stat(t["create"]))
        say("    create / rebuild (device)    %.1fx      host rebuild / device rebuild %.1fx      device rebuild / update %.1fx" %
            (median(t["create"]) / median(t["dev"]), median(t["host"]) / median(t["dev"]), median(t["dev"]) / median(t["upd"])))
    # (b)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "split"], env=dict(os.environ, CUTRACE_DEBUG_UPDATE="1"), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout
    phases, case = {}, None
    for line in out.splitlines():
        if line.startswith("== "):
            case = line[9:] if line.startswith("== split") else None
        m = re.match(r"cutrace_amd rebuild_mesh: (.+?)\s+([0-9.]+) ms$", line)
        if m and case:
            phases.setdefault(case, {}).setdefault(m.group(1), []).append(float(m.group(2)))
    say()
    say("(b) the split of rebuild_mesh from a device tensor (every stage's kernels waited for separately)")
    for case, ph in phases.items():
        say("    %s" % case)
        for what, xs in ph.items():
            say("      %-26s %s" % (what, stat(xs[-REPS:])))
    # (c)
    say()
    say("(c) 1920x1080 frame at bounces 5, kernel time; every handle but `fresh` was created from the original mesh")
    for name, path in cases(d):
        obj, base = mesh_of(path)
        for what, tris in (("rigid rotation by 30 degrees", rotated(base, 30.0)), ("twist of 90 degrees along the long axis", rotated(base, 90.0, twist=True)),
                           ("fold through itself", folded(base))):
            handles = {"fresh": ca.DeviceScene(ca.HostScene.load(scene_json(d, "c_%d_%d" % (len(base), len(what)), path, tris)))}
            for label in ("refit only", "device rebuilt", "host rebuilt"):
                handles[label] = ca.DeviceScene(ca.HostScene.load(path))
            handles["refit only"].update_mesh(obj, tris)
            info = handles["device rebuilt"].rebuild_mesh(obj, tris, builder="device")
            handles["host rebuilt"].rebuild_mesh(obj, tris, builder="host")
            ms, depth = {}, {}
            for label, h in handles.items():
                h.set_size(1920, 1080)
                ms[label] = [h.render(bounces=5, pinned=True)["kernel_ms"] for _ in range(WARM + REPS)][WARM:]
                depth[label] = h.render(bounces=5, pinned=True)["depth"].view(np.uint32).copy()
            same = all(np.array_equal(depth[k], depth["fresh"]) for k in depth)
            say("    %s, %s   (device builder: %s)" % (name, what, info))
            for label in handles:
                say("      %-16s %s   / fresh %.3f" % (label, stat(ms[label]), median(ms[label]) / median(ms["fresh"])))
            say("      depth bitwise equal on all four: %s" % same)
            for h in handles.values():
                h.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "rebuild.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "split":
        child_split()
    else:
        main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_rebuild"))
