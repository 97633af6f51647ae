"""Supersampled render (ctr_render_aa) on one MI355X, against what it replaces: the plain render of the s*w x s*h frame
plus a box filter on the host.

Per scene (bunny.json and its 64 000-triangle version, 1920x1080 output, bounces 5) and s in {2, 4}, in ONE process, the
two alternated call by call after both shapes are warm (--reps timed calls each):
  (aa)   ctr_render_aa at w x h into a page-locked block: kernel_ms and the whole host call
  (big)  ctr_scene_set_size(s*w, s*h), ctr_render into a page-locked block (the kernel delivers the frame itself), then the
         box filter of the colour in numpy: kernel_ms, the host call, and call + filter
and, on the dense scene, the AA kernel with and without the 6-waves-per-SIMD build (CTR_VAR_NO_OCC6).
Writes <out>/aa.json and <out>/aa.txt.  `--resources` (no GPU needed): the compiler's resource report of every
render_kernel instantiation into <out>/resources.txt (`--csrc DIR`: of another tree's cutrace_amd/csrc, to diff against).

  python scripts/gpu_aa.py --out profiles/aa [--reps 20 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)

KV_NAMES = ((1, "PREFILTER"), (2, "ANYHIT"), (4, "COUNT"), (8, "BVH"), (16, "STATS"), (32, "FASTPOW"), (64, "OCC6"),
            (128, "HOSTOUT"), (256, "UV"), (512, "MERGE"), (1024, "IGNTR"), (2048, "SS"))


def resources(out, csrc=None, name="resources.txt"):
    gpu_common.write_report(out, name, gpu_common.resource_report(
        "render_kernel.hip", "render_kernel", KV_NAMES, "plain",
        "\n(LDS Size is the static part: the recursion stack is dynamic, frames x frame_dwords x 64 lanes x 4 bytes per wave,\n"
        " plus 1280 bytes under OCC6; frames = bounces, frame_dwords = 4, or 10 when a material both reflects and transmits)\n",
        csrc=csrc, by_number=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--csrc", default=None)
    ap.add_argument("--name", default="resources.txt")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        resources(a.out, a.csrc, a.name)
        return
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    from tests import aa_ref
    assert torch.cuda.is_available(), "gpu_aa.py needs a GPU"
    W, H = 1920, 1080

    def med(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    dense_dir = os.path.join(a.out, "_scenes")
    cases = [("bunny", os.path.join(ROOT, "scene", "bunny.json"), False),
             ("bunny_dense64k", scenes.make_dense_bunny(dense_dir, rounds=3, width=W, height=H), True)]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "bounces": a.bounces,
              "width": W, "height": H, "scenes": {}}
    for name, path, dense in cases:
        s = ca.HostScene.load(path)
        assert s.ok
        s.set_size(W, H)
        ds = ca.DeviceScene(s)
        rec = {}
        for ss in (2, 4):
            ds.set_size(ss * W, ss * H)
            ds.render(bounces=a.bounces, pinned=True)  # the handle's page-locked block, sized for the larger frame once

            def run_aa():
                ds.set_size(W, H)
                t0 = time.perf_counter()
                r = ds.render(bounces=a.bounces, pinned=True, samples=ss)
                return r["kernel_ms"], (time.perf_counter() - t0) * 1e3, 0.0

            def run_big(box_filter=True):
                ds.set_size(ss * W, ss * H)
                t0 = time.perf_counter()
                r = ds.render(bounces=a.bounces, pinned=True)
                t1 = time.perf_counter()
                if box_filter:
                    aa_ref.reduce_color(r["color"], ss)
                return r["kernel_ms"], (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

            def alone(fn):
                for _ in range(a.warmup):
                    fn()
                return med([fn()[0] for _ in range(a.reps)])

            for _ in range(a.warmup):
                run_aa()
                run_big()
            ta, tb = [], []
            for _ in range(a.reps):
                ta.append(run_aa())
                tb.append(run_big())
            r = {"aa_kernel_ms": med([t[0] for t in ta]), "aa_call_ms": med([t[1] for t in ta]),
                 "big_kernel_ms": med([t[0] for t in tb]), "big_call_ms": med([t[1] for t in tb]),
                 "big_filter_ms": med([t[2] for t in tb]), "big_call_plus_filter_ms": med([t[1] + t[2] for t in tb])}
            # alternated on one handle the two shapes relearn their tile order every call (cutrace_aa.h); the same kernels,
            # each shape repeated on its own
            r["aa_kernel_alone_ms"] = alone(run_aa)
            if dense:
                ds.set_variant(ca.VAR_NO_OCC6)
                r["aa_kernel_alone_no_occ6_ms"] = alone(run_aa)
                ds.set_variant(0)
            r["big_kernel_alone_ms"] = alone(lambda: run_big(False))
            ds.set_variant(ca.VAR_NO_DIRECT)  # the big frame through device buffers and one DMA, as the AA frame leaves
            r["big_kernel_alone_no_direct_ms"] = alone(lambda: run_big(False))
            ds.set_variant(0)
            ds.set_size(W, H)
            rec[f"s{ss}"] = r
            print(name, ss, json.dumps(r), flush=True)
        result["scenes"][name] = rec
        ds.close()
    with open(os.path.join(a.out, "aa.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"supersampled render on {result['device']}: {W}x{H} output, bounces {a.bounces}; median [min, max] in ms of {a.reps} calls "
             f"after {a.warmup} warm-up calls", ""]

    def fmt(m):
        return f"{m['median']:8.3f} [{m['min']:.3f}, {m['max']:.3f}]"

    for name, rec in result["scenes"].items():
        for key, r in rec.items():
            lines.append(f"{name} {key}")
            for k, v in r.items():
                lines.append(f"    {k:28s} {fmt(v)}")
    lines += ["", "aa_*: ctr_render_aa into a page-locked block.  big_*: ctr_render of the s*w x s*h frame into a page-locked block",
              "(kernel-delivered) and the numpy box filter of its colour (tests/aa_ref.py).  aa / big calls alternate on one handle, so",
              "both relearn their tile order each call; *_alone: each shape repeated on its own (its order learned), kernel_ms;",
              "no_occ6: under CTR_VAR_NO_OCC6; no_direct: under CTR_VAR_NO_DIRECT (device buffers + DMA, the kernel build without delivery)."]
    with open(os.path.join(a.out, "aa.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
