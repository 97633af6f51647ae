"""Host time per call of the ray queries and the mesh update, two builds of libcutrace_amd.so alternated on one MI355X.

  python scripts/gpu_query_ab.py parent=build_variants/parent/libcutrace_amd.so new=cutrace_amd/libcutrace_amd.so
         [--rounds 5 --calls 200] [--bench] [--out profiles/query_path/host_ab.txt]

Per round and library a fresh process (CUTRACE_AMD_LIB selects the library, the Python package is this tree's): wall time of
--calls consecutive calls through the C-ABI, divided by their number, after 20 warm-up calls — ctr_cast_rays, ctr_shade_rays
and ctr_shade_points at 64 rays on scene/triangle.json (queued on the stream, no wait inside the timed loop) and
ctr_scene_update_mesh of scene/bunny.json's mesh from a host array.  A library is accepted when each of its medians over the
rounds lies inside the first library's min .. max.  --bench: `bench.py --gpus 1 --steps 20 --warmup 3` alternated likewise,
reported under the same rule."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = ("ctr_cast_rays", "ctr_shade_rays", "ctr_shade_points", "ctr_scene_update_mesh")


def child(calls):
    import numpy as np
    import torch
    import cutrace_amd as ca
    from cutrace_amd import _lib
    import gpu_mesh_update
    L = _lib.hip_lib()
    s = ca.HostScene.load(os.path.join(ROOT, "scene", "triangle.json"))
    ds = ca.DeviceScene(s)
    n = 64
    o = torch.tensor([[0.0, 0.0, -5.0]], device="cuda").repeat(n, 1).contiguous()
    d = torch.tensor([[0.0, 0.0, 1.0]], device="cuda").repeat(n, 1).contiguous()
    out3, out1 = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rq = _lib.RayQuery(n_rays=n, min_t=1e-3, d_origin=o.data_ptr(), d_dir=d.data_ptr(), d_t=out1.data_ptr())
    sq = _lib.ShadeQuery(n_rays=n, bounces=5, min_t=1e-3, ambient=0.01, d_origin=o.data_ptr(), d_dir=d.data_ptr(), d_color=out3.data_ptr())
    pq = _lib.PointQuery(n_points=n, ambient=0.01, d_point=o.data_ptr(), d_normal=d.data_ptr(), d_view=d.data_ptr(), d_color=out3.data_ptr())
    bunny = os.path.join(ROOT, "scene", "bunny.json")
    obj, tris = gpu_mesh_update.mesh_of(bunny)
    tris = np.ascontiguousarray(tris, np.float32)
    dsb = ca.DeviceScene(ca.HostScene.load(bunny))
    fns = {"ctr_cast_rays": lambda: L.ctr_cast_rays(ds._h, C.byref(rq), stream),
           "ctr_shade_rays": lambda: L.ctr_shade_rays(ds._h, C.byref(sq), stream),
           "ctr_shade_points": lambda: L.ctr_shade_points(ds._h, C.byref(pq), stream),
           "ctr_scene_update_mesh": lambda: L.ctr_scene_update_mesh(dsb._h, obj, C.c_void_p(tris.ctypes.data), len(tris), stream)}
    res = {}
    for name in CALLS:
        fn = fns[name]
        assert sum(fn() for _ in range(20)) == 0, name
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bad = 0
        for _ in range(calls):
            bad |= fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        assert bad == 0, name
        res[name] = (t1 - t0) / calls * 1e6
    print("RESULT " + json.dumps(res))


def main():
    argv = sys.argv[1:]
    opt = {k: int(argv[argv.index(k) + 1]) if k in argv else v for k, v in (("--rounds", 5), ("--calls", 200))}
    if "--child" in argv:
        return child(opt["--calls"])
    libs = [a.split("=", 1) for a in argv if "=" in a]
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def run(cmd, lib):
        env = dict(os.environ, CUTRACE_AMD_LIB=os.path.join(ROOT, lib))
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        if r.returncode:
            sys.exit(f"{lib}: {' '.join(cmd)} failed ({r.returncode})\n{r.stderr[-2000:]}")  # (nothing more is started)
        return r.stdout

    def verdict(res, key, unit, fmt):
        ref = [x[key] for x in res[libs[0][0]]]
        for name, _ in libs:
            v = [x[key] for x in res[name]]
            say(f"  {name:8s} median {statistics.median(v):{fmt}} {unit} (min {min(v):{fmt}}, max {max(v):{fmt}})")
        for name, _ in libs[1:]:
            m = statistics.median(x[key] for x in res[name])
            say(f"  {name}'s median {m:{fmt}} lies {'inside' if min(ref) <= m <= max(ref) else 'OUTSIDE'} {libs[0][0]}'s min .. max "
                f"({min(ref):{fmt}} .. {max(ref):{fmt}})")

    say(f"host time per call in microseconds, {opt['--calls']} calls per round after 20 warm-up calls, {opt['--rounds']} rounds, a fresh "
        f"process per round and library,")
    say("the libraries alternating (scripts/gpu_query_ab.py): the three queries at 64 rays on scene/triangle.json, the update on")
    say("scene/bunny.json's mesh (1000 triangles, host array)")
    say()
    res = {name: [] for name, _ in libs}
    for r in range(opt["--rounds"]):
        for name, lib in libs:
            outp = run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(opt["--calls"])], lib)
            res[name].append(json.loads(next(l for l in outp.splitlines() if l.startswith("RESULT "))[7:]))
            say(f"{name:8s} {r + 1}  " + "  ".join(f"{k} {res[name][-1][k]:9.2f}" for k in CALLS))
    for k in CALLS:
        say()
        say(k)
        verdict(res, k, "us", "9.2f")
    if "--bench" in argv:
        say()
        say("`python bench.py --gpus 1 --steps 20 --warmup 3` (bunny.json, 1920x1080, bounces 5), fresh processes alternating likewise")
        say()
        bres = {name: [] for name, _ in libs}
        for r in range(opt["--rounds"]):
            for name, lib in libs:
                outp = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], lib)
                b = json.loads([l for l in outp.splitlines() if l.startswith("{")][-1])
                bres[name].append({"ms_per_step": b["ms_per_step"]})
                say(f"{name:8s} {r + 1}  ms_per_step {b['ms_per_step']:.5f}")
        say()
        verdict(bres, "ms_per_step", "ms", ".5f")
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
