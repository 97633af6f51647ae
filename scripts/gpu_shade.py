"""Kernel time of radiance queries (ctr_shade_rays) on one MI355X, against the render of the same frame.

Per scene (bunny.json and its 64 000-triangle version, 1920x1080, bounces 5), HIP-event time of one launch, median of
--reps after --warmup launches:
  (a) the camera's rays in image order (DeviceScene.shade_rays, colour only)
  (b) the same rays, randomly permuted
  (c) ctr_render_device of the same frame: the same rays, walked wave-uniformly by the render kernel
Writes <out>/shade.json and <out>/shade.txt.  `--resources` (no GPU needed): the compiler's resource report of every
radiance-query kernel instantiation into <out>/shade_resources.txt.

  python scripts/gpu_shade.py --out profiles/rays [--reps 25 --warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)


def resources(out):
    gpu_common.write_report(out, "shade_resources.txt", gpu_common.resource_report(
        "ray_shade.hip", "ray_shade_kernel", ((1, "LINEAR"), (2, "EXACT_POW")), "default",
        "\n(LDS Size is the static part: the walk stack and the recursion frames are dynamic, (stack_slots + frames x "
        "frame_dwords) x 64 lanes x 4 bytes\n per workgroup; LINEAR has no walk stack; frames = bounces, "
        "frame_dwords = 4, or 10 when a material both reflects and transmits)\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        resources(a.out)
        return
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    from tests import ray_ref
    assert torch.cuda.is_available(), "gpu_shade.py needs a GPU"
    dev = torch.device("cuda", 0)

    def timed(fn):
        return gpu_common.timed(fn, a.reps, a.warmup)

    dense_dir = os.path.join(a.out, "_scenes")
    cases = [("bunny", os.path.join(ROOT, "scene", "bunny.json")),
             ("bunny_dense64k", scenes.make_dense_bunny(dense_dir, rounds=3, width=1920, height=1080))]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "bounces": a.bounces, "scenes": {}}
    for name, path in cases:
        s = ca.HostScene.load(path)
        assert s.ok
        s.set_size(1920, 1080)
        rs = ray_ref.RefScene(s)
        ds = ca.DeviceScene(s)
        o_np, d_np = ray_ref.camera_rays(rs.cam)
        o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
        n = o.shape[0]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
        op, dp = o[perm].contiguous(), d[perm].contiguous()
        ta = timed(lambda: ds.shade_rays(o, d, bounces=a.bounces))
        tb = timed(lambda: ds.shade_rays(op, dp, bounces=a.bounces))
        ca_, cb = ds.shade_rays(o, d, bounces=a.bounces)["color"], ds.shade_rays(op, dp, bounces=a.bounces)["color"]
        same = torch.equal(ca_[perm].view(torch.int32), cb.view(torch.int32))  # the two orders answer alike, ray for ray
        depth = torch.empty(n, device=dev)
        color = torch.empty(n * 3, device=dev)
        normal = torch.empty(n * 3, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        tc = timed(lambda: ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=stream, fudge=1e-3,
                                            bounces=a.bounces))
        torch.cuda.synchronize()
        diff = float((ca_.reshape(-1) - color).abs().max())
        rec = {"rays": n, "a_image_order_ms": ta[0], "b_permuted_ms": tb[0], "c_render_ms": tc[0],
               "a_over_render": ta[0] / tc[0], "b_over_render": tb[0] / tc[0],
               "a_mrays_s": n / ta[0] / 1e3, "b_mrays_s": n / tb[0] / 1e3,
               "min_max_ms": {"a": ta[1:], "b": tb[1:], "c": tc[1:]},
               "permuted_same_bits": bool(same), "a_color_max_abs_diff_to_render": diff}
        result["scenes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        ds.close()
    with open(os.path.join(a.out, "shade.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"radiance queries on {result['device']}: HIP-event kernel time, median of {a.reps} after {a.warmup} warm-up launches, "
             f"bounces {a.bounces}", ""]
    lines.append(f"{'scene':16s} {'rays':>9s} {'(a) ms':>8s} {'Mrays/s':>8s} {'(b) ms':>8s} {'Mrays/s':>8s} {'(c) ms':>8s} {'(a)/(c)':>8s} {'(b)/(c)':>8s}")
    for name, r in result["scenes"].items():
        lines.append(f"{name:16s} {r['rays']:9d} {r['a_image_order_ms']:8.3f} {r['a_mrays_s']:8.1f} {r['b_permuted_ms']:8.3f} "
                     f"{r['b_mrays_s']:8.1f} {r['c_render_ms']:8.3f} {r['a_over_render']:8.2f} {r['b_over_render']:8.2f}")
    lines += ["", "(a) shade_rays of the camera's rays in image order, colour only; (b) the same rays permuted;",
              "(c) ctr_render_device of the same frame (the render kernel's wave-uniform walk).  Rays are the caller's rays:",
              "each is a whole ray_color activation tree (shadow rays and bounces are not counted)."]
    with open(os.path.join(a.out, "shade.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
