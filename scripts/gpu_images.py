"""Display frames (include/cutrace_images.h) on one MI355X: what quantising on the GPU costs and what it saves.

bunny.json at 1920x1080, bounces 5.  Three measurements, written to <out>/images.txt and <out>/images.json:
  (a) the quantise kernel alone on a rendered frame that stays on the device: device events around a replayed batch of
      launches, all three planes, max depth read from the counter block, in two fresh child processes.  Bytes moved per
      launch: 28 read + 9 written per pixel.  (`--kernel-only` is one such process, JSON on stdout; alternating such
      processes between two kernels is how profiles/images/widened_ab.txt was made while both kernels existed.)
  (b) ctr_render_images into pageable and into page-locked destinations against what the parent commit offers for the
      same bytes: ctr_render into the same kind of memory, then the three host quantisers — on one thread, and on three
      threads as the CLI runs them.  Host clock around synchronous calls, the sides alternated call by call.
  (c) the CLI's wall time (process start to exit, JPEG encoding included) with and without CUTRACE_GPU_IMAGES=1, alternated.

  python scripts/gpu_images.py --out profiles/images [--reps 30 --warmup 5 --cli-reps 15]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def fmt(m):
    return f"{m['median']:8.3f} ms  (min {m['min']:.3f}, max {m['max']:.3f}, n {m['n']})"


def kernel_only(a):
    """(a), one process: JSON on stdout"""
    import torch
    import cutrace_amd as ca
    dev = torch.device("cuda", 0)
    s = ca.HostScene.load("scene/bunny.json")
    s.set_size(W, H)
    ds = ca.DeviceScene(s)
    depth, color, normal = torch.empty(H, W, device=dev), torch.empty(H, W, 3, device=dev), torch.empty(H, W, 3, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), d_counters=counters.data_ptr(), stream=stream.cuda_stream,
                     bounces=a.bounces)
    out = {k: torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for k in ("depth", "color", "normal")}
    batch = 1000   # (a timed window of about 14 ms)

    def launches():
        for _ in range(batch):
            ds.quantise(depth=depth, color=color, normal=normal, counters=counters, out=out)

    # (a launch from Python costs more host time than the kernel runs: the batch is captured once, as one linear chain,
    #  and replayed, so that the events bracket kernels and not the interpreter)
    side = torch.cuda.Stream(dev)
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        launches()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launches()
    for _ in range(a.warmup):
        g.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.replay()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    del g
    print(json.dumps({"kernel_ms": ms, "checksum": int(sum(int(v.sum()) for v in out.values()))}))
    ds.close()


def child(extra_env, args):
    env = dict(os.environ, **extra_env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise RuntimeError(f"child failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "images"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cli-reps", type=int, default=15)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    os.chdir(ROOT)
    if a.kernel_only:
        kernel_only(a)
        return
    import numpy as np
    import torch
    import cutrace_amd as ca
    from cutrace_amd import _lib, build
    assert torch.cuda.is_available(), "gpu_images.py needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    res = {"size": [W, H], "bounces": a.bounces, "scene": "scene/bunny.json"}
    lines = [f"display frames: bunny.json {W}x{H}, bounces {a.bounces}; {torch.cuda.get_device_name(0)}", ""]

    # ---- (a) the kernel alone, in fresh processes ----
    env_base = dict(os.environ)
    args = ["--kernel-only", "--reps", str(a.reps), "--warmup", str(a.warmup), "--bounces", str(a.bounces)]
    ka, sums = [], set()
    for _ in range(2):
        r = child({}, args)
        ka += r["kernel_ms"]
        sums.add(r["checksum"])
    assert len(sums) == 1, f"two processes, two results: {sums}"
    px = W * H
    m = res["kernel"] = med(ka)
    lines.append("(a) quantise kernel alone, three planes, device events over a replayed batch of 1000 launches (two processes)")
    lines.append(f"    {'frame_images_kernel':22s} {fmt(m)}   {37 * px / (m['median'] * 1e-3) / 1e12:.2f} TB/s of the 37 bytes per pixel it must move")
    lines.append("    (the frame was written just before and is read again launch after launch: it need not come from HBM)")
    lines.append("")

    # ---- (b) the host forms ----
    s = ca.HostScene.load("scene/bunny.json")
    s.set_size(W, H)
    ds = ca.DeviceScene(s)
    Lh = _lib.host_lib()

    def quantise_host(r, out, threads):
        jobs = [lambda: Lh.ctr_quantise_depth(r["depth"].ctypes.data, px, C.c_float(r["max_depth"]), out["depth"].ctypes.data),
                lambda: Lh.ctr_quantise_normal(r["normal"].ctypes.data, px, out["normal"].ctypes.data),
                lambda: Lh.ctr_quantise_color(r["color"].ctypes.data, px, out["color"].ctypes.data)]
        if threads == 1:
            for j in jobs:
                j()
            return
        th = [threading.Thread(target=j) for j in jobs[:2]]   # (the CLI: two threads beside the calling one)
        for t in th:
            t.start()
        jobs[2]()
        for t in th:
            t.join()

    Lg = _lib.hip_lib()
    rows = ca.make_rows(H, None)

    def render_images(dst):
        stats = _lib.RenderStats()
        st = Lg.ctr_render_images(ds._h, C.c_float(1e-3), a.bounces, 1, C.byref(rows), dst["depth"].ctypes.data, dst["color"].ctypes.data,
                                  dst["normal"].ctypes.data, C.byref(stats))
        assert st == 0, Lg.ctr_last_error()
        return dst

    hb = {}
    for pinned in (False, True):
        kind = "page-locked" if pinned else "pageable"
        out = {k: np.empty((H, W, 3), np.uint8) for k in ("depth", "color", "normal")}
        # destinations allocated once, outside the timed calls, on every side
        keep = {k: torch.empty(H, W, 3, dtype=torch.uint8) for k in out}
        if pinned:
            keep = {k: v.pin_memory() for k, v in keep.items()}
        dst = {k: v.numpy() for k, v in keep.items()}
        into = None if pinned else ds.render(bounces=a.bounces)   # (pinned: the handle's own page-locked frame block)
        t = {f"render_images ({kind})": [], f"render + host quantisers, 1 thread ({kind})": [],
             f"render + host quantisers, 3 threads ({kind})": [], f"render alone ({kind})": []}
        check = None
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            img = render_images(dst)
            t1 = time.perf_counter()
            r = ds.render(bounces=a.bounces, pinned=pinned, into=into)
            t2 = time.perf_counter()
            quantise_host(r, out, 1)
            t3 = time.perf_counter()
            r = ds.render(bounces=a.bounces, pinned=pinned, into=into)
            t4 = time.perf_counter()
            quantise_host(r, out, 3)
            t5 = time.perf_counter()
            if check is None:
                check = all(np.array_equal(img[k], out[k]) for k in out)
            if it >= a.warmup:
                t[f"render_images ({kind})"].append(1e3 * (t1 - t0))
                t[f"render + host quantisers, 1 thread ({kind})"].append(1e3 * (t3 - t1))
                t[f"render + host quantisers, 3 threads ({kind})"].append(1e3 * (t5 - t3))
                t[f"render alone ({kind})"].append(1e3 * (t4 - t3))
        assert check, "render_images and the host path disagree"
        hb.update({k: med(v) for k, v in t.items()})
    res["host_forms"] = hb
    lines.append("(b) one frame as three byte planes in host memory, host clock around synchronous calls, sides alternated call by call")
    lines.append("    (render_images: this change; render + host quantisers: what the parent commit offers for the same bytes;")
    lines.append("     every destination is allocated once, outside the timed calls)")
    for k, m in hb.items():
        lines.append(f"    {k:58s} {fmt(m)}")
    lines.append("    same bytes on both sides")
    lines.append("")
    ds.close()

    # ---- (c) the CLI ----
    exe = build.build_cli()
    cli = {"default": [], "CUTRACE_GPU_IMAGES=1": []}
    env = dict(env_base, CUTRACE_WIDTH=str(W), CUTRACE_HEIGHT=str(H), CUTRACE_BOUNCES=str(a.bounces))
    for k in ("CUTRACE_SAMPLES", "CUTRACE_DEVICES", "CUTRACE_DEVICE_LIST", "CUTRACE_GPU_IMAGES"):
        env.pop(k, None)
    files = {}
    with tempfile.TemporaryDirectory() as td:
        os.symlink(os.path.join(ROOT, "scene"), os.path.join(td, "scene"))
        for it in range(1 + a.cli_reps):
            for tag, extra in (("default", {}), ("CUTRACE_GPU_IMAGES=1", {"CUTRACE_GPU_IMAGES": "1"})):
                t0 = time.perf_counter()
                p = subprocess.run([exe, "scene/bunny.json"], cwd=td, env=dict(env, **extra), capture_output=True, text=True, timeout=300)
                dt = 1e3 * (time.perf_counter() - t0)
                if p.returncode:
                    raise RuntimeError(f"cutrace failed ({p.returncode}): {p.stderr[-2000:]}")
                files[tag] = [open(os.path.join(td, n), "rb").read() for n in ("frame.jpg", "depth_map.jpg", "normal_map.jpg")]
                if it:   # (the first pair warms the file cache)
                    cli[tag].append(dt)
    assert files["default"] == files["CUTRACE_GPU_IMAGES=1"], "the CLI's files differ"
    res["cli_wall_ms"] = {k: med(v) for k, v in cli.items()}
    lines.append("(c) cutrace scene/bunny.json, wall time of the whole process (start, scene load, upload, render, JPEG encoding), alternated")
    for k, m in res["cli_wall_ms"].items():
        lines.append(f"    {k:22s} {fmt(m)}")
    lines.append("    the three files are byte-identical")
    with open(os.path.join(a.out, "images.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, "images.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
