"""Time of nearest-point queries (ctr_nearest_points) on one MI355X: the default walk through the meshes' trees against
linear=True, the only alternative the library offers, on the same points.

Per scene (bunny.json and its 64 000-triangle version), two sets of 2.07 M points, each in image order and randomly permuted,
skip_planes on (a room's walls otherwise win almost everywhere), every output:
  (surface)  the primary hit points of the 1920x1080 frame pushed 0.05 along their normals
  (uniform)  as many uniform points in the box that holds those hit points (the room)
HIP-event time of a whole call, median with its spread (min, max) of --reps calls after --warmup; the linear walk of the dense
scene takes a third of a second per call and gets --linear-reps after one warm-up call.  The two walks are compared bit for bit once per case.  Writes
<out>/nearest.json and <out>/nearest.txt.  `--resources` (no GPU needed): the compiler's resource report of the kernel's two
instantiations into <out>/resources.txt.

  python scripts/gpu_nearest.py --out profiles/nearest [--reps 20 --warmup 3 --linear-reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)


def resources(out):
    note = ("\n(hipcc --offload-arch=gfx950 with the library's flags.  Occupancy is waves per SIMD; ScratchSize is bytes per lane.  LDS Size\n"
            " is the static part: the walk stack is dynamic, stack_slots x 128 lanes x 4 bytes per workgroup, none under LINEAR.\n"
            " Neither instantiation uses scratch.)\n")
    gpu_common.write_report(out, "resources.txt", gpu_common.resource_report("ray_nearest.hip", "ray_nearest_kernel", ((1, "LINEAR"),), "default walk",
                                                                             note, by_number=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--linear-reps", type=int, default=3)
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
    assert torch.cuda.is_available(), "gpu_nearest.py needs a GPU"
    dev = torch.device("cuda", 0)
    dense_dir = os.path.join(a.out, "_scenes")
    cases = [("bunny", os.path.join(ROOT, "scene", "bunny.json")),
             ("bunny_dense64k", scenes.make_dense_bunny(dense_dir, rounds=3, width=1920, height=1080))]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "linear_reps": a.linear_reps, "cases": []}
    for name, path in cases:
        s = ca.HostScene.load(path)
        assert s.ok
        s.set_size(1920, 1080)
        ds = ca.DeviceScene(s)
        rs = ray_ref.RefScene(s)
        tris = sum(o["tri_count"] for o in rs.objects if o["type"] == ray_ref.OBJ_MESH)
        o_np, d_np = ray_ref.camera_rays(rs.cam)
        hit = ds.cast_rays(torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev), outputs=("point", "normal", "object"))
        surface = torch.where((hit["object"] >= 0)[:, None], hit["point"] + 0.05 * hit["normal"], hit["point"]).contiguous()
        n = surface.shape[0]
        lo, hi = surface.min(0).values, surface.max(0).values
        g = torch.Generator().manual_seed(2)
        uniform = (lo + (hi - lo) * torch.rand(n, 3, generator=g).to(dev)).contiguous()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
        del hit
        for which, pts in (("surface", surface), ("uniform", uniform)):
            for order, p in (("image", pts), ("permuted", pts[perm].contiguous())):
                tree = ds.nearest_points(p, skip_planes=True)
                lin = ds.nearest_points(p, skip_planes=True, linear=True)   # (also the linear walk's warm-up)
                same = all(torch.equal(tree[k].view(torch.int32), lin[k].view(torch.int32)) for k in tree)
                on_mesh = int((tree["prim"] >= 0).sum())
                med_d = float(tree["distance"].median())
                del tree, lin
                t_tree = gpu_common.timed(lambda: ds.nearest_points(p, skip_planes=True), a.reps, a.warmup)
                slow = tris > 10000
                t_lin = gpu_common.timed(lambda: ds.nearest_points(p, skip_planes=True, linear=True), a.linear_reps if slow else a.reps,
                                         0 if slow else a.warmup)
                rec = {"scene": name, "triangles": int(tris), "points": which, "order": order, "n": n, "nearest_is_mesh": on_mesh,
                       "median_distance": med_d, "same_bits": bool(same), "tree_ms": t_tree[0], "linear_ms": t_lin[0],
                       "linear_over_tree": t_lin[0] / t_tree[0], "min_max_ms": {"tree": t_tree[1:], "linear": t_lin[1:]},
                       "linear_reps": a.linear_reps if slow else a.reps}
                result["cases"].append(rec)
                print(json.dumps(rec), flush=True)
        ds.close()
    with open(os.path.join(a.out, "nearest.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"nearest-point queries on {result['device']}: HIP-event time of a whole call, skip_planes on, every output;",
             f"median [min .. max] of {a.reps} calls after {a.warmup} warm-up calls (the linear walk of the dense scene: of {a.linear_reps} after 1)", "",
             f"{'scene':16s} {'triangles':>9s} {'points':8s} {'order':9s} {'n':>8s} {'tree walk ms':>28s} {'linear ms':>34s} {'linear / tree':>14s} {'same bits':>10s} {'median dist':>12s}"]
    for r in result["cases"]:
        t, ln = r["min_max_ms"]["tree"], r["min_max_ms"]["linear"]
        lines.append(f"{r['scene']:16s} {r['triangles']:9d} {r['points']:8s} {r['order']:9s} {r['n']:8d} "
                     f"{r['tree_ms']:9.3f} [{t[0]:7.3f} .. {t[1]:7.3f}] {r['linear_ms']:11.3f} [{ln[0]:9.3f} .. {ln[1]:9.3f}] "
                     f"{r['linear_over_tree']:14.1f} {str(r['same_bits']):>10s} {r['median_distance']:12.4f}")
    lines += ["", "tree walk: DeviceScene.nearest_points(p, skip_planes=True).  linear: the same with linear=True, every triangle of the mesh per",
              "point.  surface: the frame's primary hit points pushed 0.05 along their normals (most of them wall points, well away from the",
              "mesh); uniform: uniform points in the box of those hit points.  Both times include the calls' own",
              "torch allocations."]
    with open(os.path.join(a.out, "nearest.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
