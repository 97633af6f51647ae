"""Kernel time of ray queries (ctr_cast_rays) on one MI355X, against the render of the same frame.

Per scene (bunny.json and its 64 000-triangle version, 1920x1080), HIP-event time of one launch, median of --reps after
--warmup launches:
  (a) the camera's primary rays in image order (DeviceScene.cast_rays, every output)
  (b) the same rays, randomly permuted
  (c) one random hemisphere shadow ray per primary hit, max_t 0.5 (DeviceScene.shadow: an ambient-occlusion pattern)
  (d) ctr_render_device(bounces=0) of the same frame: the same primary rays plus up to one shadow ray per light and hit
Writes <out>/rays.json and <out>/rays.txt.  `--resources` (no GPU needed): the compiler's resource report of every
ray-query kernel instantiation into <out>/resources.txt.

  python scripts/gpu_rays.py --out profiles/rays [--reps 25 --warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)


def resources(out):
    gpu_common.write_report(out, "resources.txt", gpu_common.resource_report(
        "ray_query.hip", "ray_query_kernel", ((1, "LINEAR"), (2, "SHADOW"), (4, "ANYHIT")), "nearest",
        "\n(LDS Size is the static part: the stack is dynamic, stack_slots x 128 lanes x 4 bytes per workgroup)\n"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        resources(a.out)
        return
    import numpy as np
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    from tests import ray_ref
    assert torch.cuda.is_available(), "gpu_rays.py needs a GPU"
    dev = torch.device("cuda", 0)

    def timed(fn):
        return gpu_common.timed(fn, a.reps, a.warmup)

    dense_dir = os.path.join(a.out, "_scenes")
    cases = [("bunny", os.path.join(ROOT, "scene", "bunny.json")),
             ("bunny_dense64k", scenes.make_dense_bunny(dense_dir, rounds=3, width=1920, height=1080))]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "scenes": {}}
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
        prim = ds.cast_rays(o, d)
        ta = timed(lambda: ds.cast_rays(o, d))
        tb = timed(lambda: ds.cast_rays(op, dp))
        # (the two orders give the same answers ray for ray)
        pb = ds.cast_rays(op, dp)
        same = all(torch.equal(prim[k][perm].view(torch.int32), pb[k].view(torch.int32)) for k in prim)
        hit = prim["object"] >= 0
        ho, hn = prim["point"][hit], prim["normal"][hit]
        g = torch.Generator(device=dev).manual_seed(2)
        r = torch.randn(ho.shape, device=dev, generator=g)
        r = r / r.norm(dim=1, keepdim=True)
        r = torch.where(((r * hn).sum(1) < 0)[:, None], -r, r).contiguous()
        ho = ho.contiguous()
        tc = timed(lambda: ds.shadow(ho, r, max_t=0.5))
        occl = float(ds.shadow(ho, r, max_t=0.5).mean())
        depth = torch.empty(n, device=dev)
        color = torch.empty(n * 3, device=dev)
        normal = torch.empty(n * 3, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        td = timed(lambda: ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=stream, fudge=1e-3, bounces=0))
        same_depth = torch.equal(depth.view(torch.int32), prim["t"].view(torch.int32))
        nh = int(hit.sum())
        rec = {"rays_a": n, "hits": nh, "rays_c": nh, "occluded_fraction_c": occl,
               "a_image_order_ms": ta[0], "b_permuted_ms": tb[0], "c_ao_shadow_ms": tc[0], "d_render_b0_ms": td[0],
               "a_grays_s": n / ta[0] / 1e6, "b_grays_s": n / tb[0] / 1e6, "c_grays_s": nh / tc[0] / 1e6,
               "min_max_ms": {"a": ta[1:], "b": tb[1:], "c": tc[1:], "d": td[1:]},
               "permuted_same_bits": bool(same), "a_depth_equals_render_depth": bool(same_depth),
               "stack_slots_note": "per lane, from the deepest mesh tree (scene_flatten.cpp ray_stack_slots)"}
        result["scenes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        ds.close()
    with open(os.path.join(a.out, "rays.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"ray queries on {result['device']}: HIP-event kernel time, median of {a.reps} after {a.warmup} warm-up launches", ""]
    lines.append(f"{'scene':16s} {'rays':>9s} {'(a) ms':>8s} {'Grays/s':>8s} {'(b) ms':>8s} {'Grays/s':>8s} {'(c) rays':>9s} "
                 f"{'(c) ms':>8s} {'Grays/s':>8s} {'(d) ms':>8s}")
    for name, r in result["scenes"].items():
        lines.append(f"{name:16s} {r['rays_a']:9d} {r['a_image_order_ms']:8.3f} {r['a_grays_s']:8.2f} {r['b_permuted_ms']:8.3f} "
                     f"{r['b_grays_s']:8.2f} {r['rays_c']:9d} {r['c_ao_shadow_ms']:8.3f} {r['c_grays_s']:8.2f} {r['d_render_b0_ms']:8.3f}")
    lines += ["", "(a) primary rays in image order, every output; (b) the same permuted; (c) one hemisphere shadow ray per hit,",
              "max_t 0.5; (d) ctr_render_device(bounces=0) of the same frame (primary rays + one shadow ray per light and hit)"]
    with open(os.path.join(a.out, "rays.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
