"""Light edits and the guard's plane scan (include/cutrace_edit.h) measured on scene/bunny.json (1000 triangles) and on the
64 000-triangle bunny, 20 repetitions after warm-up, medians with their spread (min .. max) -> profiles/scene_edit/edit.txt (or
--out DIR).  One GPU process at a time; run every step under a time limit of its own.

  (a) set_lights, one point light moving, with the scan on the device and on the host (CUTRACE_GUARD_SCAN), against destroy +
      create of the edited description, same process
  (b) update_mesh from a device tensor with its stage split (CUTRACE_DEBUG_UPDATE=1, a child process each): this build with
      the scan on the device and on the host, and — with --parent-lib PATH, the parent commit's libcutrace_amd.so built in the
      same session — the parent, scripts/gpu_mesh_update.py's method
  (c) the crossover of the two scans: set_lights over mesh size at the bunny room's probe count; the device path is entitled to
      a size only where its median beats the host's by more than the two min .. max spreads together
  (d) the first frame after an edit against the steady frame (the tile cost history is kept)
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
from scripts.gpu_mesh_update import mesh_of, rotated, scene_json  # noqa: E402

REPS, WARM = 20, 3


def med(xs):
    return sorted(xs)[len(xs) // 2]


def stat(xs):
    return "%8.3f ms (%.3f .. %.3f)" % (med(xs), min(xs), max(xs))


def moved_lights(ca, host, k):
    """the scene's lights with light 0 (a point light) a little elsewhere at every k"""
    d = host.desc.contents
    out = []
    for i in range(int(d.n_lights)):
        l = ca.Light()
        l.type, l.v, l.color = d.lights[i].type, ca.Vec3(*d.lights[i].v.tup()), ca.Vec3(*d.lights[i].color.tup())
        out.append(l)
    out[0].v = ca.Vec3(out[0].v.x + 0.01 * (k % 7), out[0].v.y, out[0].v.z - 0.013 * (k % 5))
    return out


def time_set_lights(ca, ds, host, scan):
    os.environ["CUTRACE_GUARD_SCAN"] = scan
    ts = []
    for k in range(WARM + REPS):
        lights = moved_lights(ca, host, k)
        t0 = time.perf_counter()
        ds.set_lights(lights)
        ts.append((time.perf_counter() - t0) * 1e3)
    del os.environ["CUTRACE_GUARD_SCAN"]
    return ts[WARM:]


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
    # the whole call without the stamps' extra wait: a second pass with the variable unset
    os.environ.pop("CUTRACE_DEBUG_UPDATE", None)
    for name, path in cases(d):
        obj, base = mesh_of(path)
        ds = ca.DeviceScene(ca.HostScene.load(path))
        sets = [torch.from_numpy(rotated(base, a)).cuda() for a in (10.0, -10.0)]
        total = []
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.update_mesh(obj, sets[k % 2])
            total.append((time.perf_counter() - t0) * 1e3)
        print("== total %s | %s" % (name, stat(total[WARM:])), flush=True)
        ds.close()


def main(out_dir, parent_lib):
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    d = tempfile.mkdtemp()
    say("light edits and the guard's plane scan on %s, %d repetitions after %d warm-up, median (min .. max)" % (torch.cuda.get_device_name(0), REPS, WARM))
    # (a)
    for name, path in cases(d):
        host = ca.HostScene.load(path)
        ds = ca.DeviceScene(host)
        ds.render(pinned=True)
        t = {scan: time_set_lights(ca, ds, host, scan) for scan in ("device", "host", "device", "host")}
        ds.close()
        sc = json.load(open(path))
        hosts = []
        for k in range(2):
            sc["lights"][0]["point"][0] += 0.01
            p = os.path.join(d, "moved%d_%d.json" % (k, len(name)))
            json.dump(sc, open(p, "w"))
            hosts.append(ca.HostScene.load(p))
        t_create = []
        ds = ca.DeviceScene(hosts[0])
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ds.close()
            ds = ca.DeviceScene(hosts[(k + 1) % 2])
            t_create.append((time.perf_counter() - t0) * 1e3)
        ds.close()
        say()
        say("(a) %s: one point light moved" % name)
        say("    set_lights, scan on the device  %s" % stat(t["device"]))
        say("    set_lights, scan on the host    %s" % stat(t["host"]))
        say("    destroy + create                %s" % stat(t_create[WARM:]))
    # (b)
    say()
    say("(b) update_mesh from a device tensor: the whole call, and its split with the kernels waited for separately (CUTRACE_DEBUG_UPDATE=1)")
    builds = [("this build, scan on the device", dict(CUTRACE_GUARD_SCAN="device")), ("this build, scan on the host", dict(CUTRACE_GUARD_SCAN="host")),
              ("this build, the default choice", {})]
    if parent_lib:
        builds.append(("the parent commit", dict(CUTRACE_AMD_LIB=os.path.abspath(parent_lib))))
    for label, env in builds:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "split"], env=dict(os.environ, CUTRACE_DEBUG_UPDATE="1", **env), cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout
        phases, totals, case = {}, {}, None
        for line in out.splitlines():
            if line.startswith("== split"):
                case = line[9:]
            m = re.match(r"== total (.+?) \| (.+)$", line)
            if m:
                totals[m.group(1)] = m.group(2)
            m = re.match(r"cutrace_amd update_mesh: (.+?)\s+([0-9.]+) ms$", line)
            if m and case:
                phases.setdefault(case, {}).setdefault(m.group(1), []).append(float(m.group(2)))
        say("    %s" % label)
        for case, ph in phases.items():
            say("      %-32s whole call %s" % (case, totals.get(case, "?")))
            for what, xs in ph.items():
                say("        %-26s %s" % (what, stat(xs[-REPS:])))
    # (c)
    say()
    bunny = scenes.read_stl(os.path.join(ROOT, "scene", "bunny.stl"))
    say("(c) set_lights over mesh size, the bunny room (30 probes: the eye, its 25 images in the five reflecting walls, 4 point lights)")
    say("    %9s  %-34s %-34s %s" % ("triangles", "scan on the device", "scan on the host", "device entitled"))
    first_entitled, last_not = None, 0
    for n in (64, 125, 250, 500, 1000, 2000, 4000, 8000, 16000, 64000):
        tris = bunny[:n] if n <= len(bunny) else scenes.subdivide(bunny, 1 if n <= 4000 else 2 if n <= 16000 else 3)[:n]
        host = ca.HostScene.load(scene_json(d, "sweep_%d" % n, os.path.join(ROOT, "scene", "bunny.json"), tris))
        ds = ca.DeviceScene(host)
        t = {}
        for scan in ("device", "host", "device", "host"):   # (twice each, interleaved; the second pass counts)
            t[scan] = time_set_lights(ca, ds, host, scan)
        ds.close()
        entitled = med(t["host"]) - med(t["device"]) > (max(t["host"]) - min(t["host"])) + (max(t["device"]) - min(t["device"]))
        if entitled and first_entitled is None:
            first_entitled = n
        if not entitled:
            first_entitled, last_not = None, n
        say("    %9d  %-34s %-34s %s" % (n, stat(t["device"]), stat(t["host"]), "yes" if entitled else "no"))
    say("    the device path beats the host path by more than both spreads from %s triangles x 30 probes on (not at %d)" % (first_entitled, last_not))
    # (d)
    say()
    say("(d) 1920x1080 frame, kernel time: the first frame after a light edit against the steady frames before it")
    for name, path in cases(d):
        host = ca.HostScene.load(path)
        ds = ca.DeviceScene(host)
        ds.set_size(1920, 1080)
        steady = [ds.render(pinned=True)["kernel_ms"] for _ in range(WARM + REPS)][WARM:]
        first = []
        for k in range(REPS):
            ds.set_lights(moved_lights(ca, host, k))
            first.append(ds.render(pinned=True)["kernel_ms"])
            ds.render(pinned=True)
        say("    %-30s steady %s   first after set_lights %s" % (name, stat(steady), stat(first)))
        ds.close()
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "edit.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "split":
        child_split()
    else:
        arg = lambda k, default: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else default
        main(arg("--out", os.path.join(ROOT, "profiles", "scene_edit")), arg("--parent-lib", None))
