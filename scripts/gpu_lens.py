"""Lens render (ctr_render_device_lens) on one MI355X against the calls it stands beside.

Per scene (bunny.json and its 64 000-triangle version, 1920x1080, bounces 5), in ONE process, the two sides of each pair
alternated call by call after both are warm; every call is timed with device events on the stream it runs on:
  (a) the lens render of the camera's own rays (lenses.pinhole)  vs  ctr_render_device of the same frame
      — the same pixels bit for bit; the lens render reads 24 bytes per pixel more
  (b) a 180 degree fisheye through render_lens                    vs  ctr_shade_rays of its unmasked rays in image order
  (c) lenses.thin_lens at samples = 4, reduced in the kernel      vs  ctr_shade_rays of all 16 w h samples + a torch mean
`--plain-only`: only ctr_render_device, as JSON on stdout — what a driver alternates between this tree's library and another
build's (CUTRACE_AMD_LIB) to see whether the plain render moved.
Writes <out>/lens.json and <out>/lens.txt.  `--resources` (no GPU needed): the compiler's resource report of every
render_kernel instantiation into <out>/resources.txt, in the format of scripts/gpu_aa.py.

  python scripts/gpu_lens.py --out profiles/lens [--reps 30 --warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--scenes", default="bunny,bunny_dense64k")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        import gpu_aa
        gpu_aa.KV_NAMES = gpu_aa.KV_NAMES + ((4096, "RAYS"),)
        gpu_aa.resources(a.out)
        return
    import numpy as np
    import torch
    import cutrace_amd as ca
    from cutrace_amd import _lib, lenses, scenes
    assert torch.cuda.is_available(), "gpu_lens.py needs a GPU"
    dev = torch.device("cuda", 0)
    W, H, B = 1920, 1080, a.bounces
    stream = torch.cuda.current_stream(dev)

    def med(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def pair(fa, fb, reps=a.reps):
        """fa, fb alternated: (times of fa, times of fb) in ms"""
        for _ in range(a.warmup):
            fa()
            fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(fa))
            tb.append(timed(fb))
        return med(ta), med(tb)

    tmp = tempfile.mkdtemp(prefix="lens_scenes_")
    paths = {"bunny": lambda: os.path.join(ROOT, "scene", "bunny.json"),
             "bunny_dense64k": lambda: scenes.make_dense_bunny(tmp, rounds=3, width=W, height=H)}
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "bounces": B, "width": W, "height": H,
              "scenes": {}}
    for name in a.scenes.split(","):
        s = ca.HostScene.load(paths[name]())
        assert s.ok
        s.set_size(W, H)
        ds = ca.DeviceScene(s)
        cam = s.desc.contents.cam
        depth = torch.empty((H, W), device=dev)
        color = torch.empty((H, W, 3), device=dev)
        normal = torch.empty((H, W, 3), device=dev)
        L = _lib.hip_lib()

        def plain():
            ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=stream.cuda_stream, bounces=B)

        if a.plain_only:
            for _ in range(a.warmup):
                plain()
            torch.cuda.synchronize()
            result["scenes"][name] = {"plain_ms": med([timed(plain) for _ in range(a.reps)])}
            ds.close()
            continue

        def lens_call(o, d, samples=1):
            q = _lib.Lens(o.shape[0], samples, ds._ambient, o.data_ptr(), d.data_ptr())

            def run():
                st = L.ctr_render_device_lens(ds._h, C.c_float(1e-3), B, C.byref(q), None, depth.data_ptr(), color.data_ptr(),
                                              normal.data_ptr(), None, C.c_void_p(stream.cuda_stream))
                assert st == 0, L.ctr_last_error()
            return run

        def up(x):
            return torch.from_numpy(np.ascontiguousarray(x.reshape(-1, 3))).to(dev)

        rec = {}
        # (a) the camera's rays
        o, d = (up(x) for x in lenses.pinhole(cam, W, H))
        plain()
        torch.cuda.synchronize()
        want = color.clone()
        run = lens_call(o, d)
        run()
        torch.cuda.synchronize()
        rec["a_same_bits_as_plain"] = bool(torch.equal(want.view(torch.int32), color.view(torch.int32)))
        rec["a_lens_pinhole_ms"], rec["a_plain_ms"] = pair(run, plain)
        rec["a_plain_again_ms"], rec["a_plain_again2_ms"] = pair(plain, plain)  # the plain call's own run-to-run spread
        print(name, "a", json.dumps(rec), flush=True)
        # (b) a fisheye
        fo, fd = lenses.fisheye(cam, W, H, 180.0)
        keep = ~lenses.is_masked(fo, fd).reshape(-1)
        o, d = up(fo), up(fd)
        ko, kd = o[torch.from_numpy(keep).to(dev)].contiguous(), d[torch.from_numpy(keep).to(dev)].contiguous()
        rec["b_unmasked_rays"] = int(keep.sum())
        rec["b_lens_fisheye_ms"], rec["b_shade_rays_ms"] = pair(lens_call(o, d), lambda: ds.shade_rays(ko, kd, bounces=B))
        print(name, "b", json.dumps({k: v for k, v in rec.items() if k.startswith("b_")}), flush=True)
        del o, d, ko, kd
        # (c) a thin lens, 4 x 4 samples per pixel
        ss = 4
        to, td = lenses.thin_lens(cam, W, H, ss, 0.05, 4.0, seed=1)
        o, d = up(to), up(td)
        del to, td

        def shade_and_mean():
            c = ds.shade_rays(o, d, bounces=B)["color"]
            return c.view(H, ss, W, ss, 3).mean((1, 3))

        rec["c_lens_thin_s4_ms"], rec["c_shade_rays_plus_mean_ms"] = pair(lens_call(o, d, ss), shade_and_mean, reps=max(a.reps // 3, 5))
        print(name, "c", json.dumps({k: v for k, v in rec.items() if k.startswith("c_")}), flush=True)
        del o, d
        result["scenes"][name] = rec
        ds.close()
    if a.plain_only:
        print("PLAIN_ONLY " + json.dumps(result["scenes"]), flush=True)
        return
    with open(os.path.join(a.out, "lens.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"lens render on {result['device']}: {W}x{H}, bounces {B}; device-event times in ms, median [min, max] of {a.reps} calls "
             f"((c): {max(a.reps // 3, 5)}) after {a.warmup} warm-up calls, the two sides of a pair alternated call by call", ""]
    for name, rec in result["scenes"].items():
        lines.append(name)
        for k, v in rec.items():
            lines.append(f"    {k:28s} " + (f"{v['median']:9.3f} [{v['min']:.3f}, {v['max']:.3f}]" if isinstance(v, dict) else str(v)))
    lines += ["", "a: lenses.pinhole through ctr_render_device_lens against ctr_render_device (same pixels, a_same_bits_as_plain); a_plain_again*:",
              "the plain call against itself, its run-to-run spread.  b: a 180 degree fisheye (rim masked) against ctr_shade_rays of the",
              "unmasked rays in image order.  c: lenses.thin_lens, 4 x 4 samples per pixel reduced in the kernel, against ctr_shade_rays of",
              "all samples plus torch's mean over each block."]
    with open(os.path.join(a.out, "lens.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
