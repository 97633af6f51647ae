"""Time of hit lists (ctr_list_hits) on one MI355X against the same lists made by a loop of ctr_cast_rays.

Per scene (bunny.json and its 64 000-triangle version, 1920x1080: 2.07 M camera rays), in image order and randomly permuted,
for K = 4 and K = 8, HIP-event time from the first launch to the last, median of --reps after --warmup:
  (one)   DeviceScene.list_hits(o, d, K), every output: one launch
  (loop)  K rounds of DeviceScene.cast_rays(o, d, min_t=m), every output, m a per-ray tensor; after each round the rays whose
          chain has ended are masked to the miss values and get m = +inf, the others m = (float)((double)t + 1e-3); the slots are
          stacked slot-major.  Everything stays on the device: no host synchronisation inside a repetition.
The two are compared bit for bit once per case.  Writes <out>/hits.json and <out>/hits.txt.  `--resources` (no GPU needed): the
compiler's resource report of the hit-list kernel's instantiations beside ray_query_kernel's own, into <out>/resources.txt.

  python scripts/gpu_hits.py --out profiles/hits [--reps 20 --warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)

OUT = ("t", "object", "prim", "point", "normal", "uv")
MISS = {"t": float("inf"), "object": -1, "prim": -1, "point": 0.0, "normal": 0.0, "uv": 0.0}


def resources(out):
    note = ("\n(hipcc --offload-arch=gfx950 with the library's flags.  Occupancy is waves per SIMD; ScratchSize is bytes per lane.  LDS Size\n"
            " is the static part: the walk stack is dynamic, stack_slots x 128 lanes x 4 bytes per workgroup for both kernels, none under\n"
            " LINEAR.  Neither kernel uses scratch.)\n")
    txt = gpu_common.resource_report("ray_hits.hip", "ray_hits_kernel", ((1, "LINEAR"),), "default walk", "\n", by_number=True)
    txt += gpu_common.resource_report("ray_query.hip", "ray_query_kernel", ((1, "LINEAR"), (2, "SHADOW"), (4, "ANYHIT")), "nearest", note,
                                      by_number=True)
    gpu_common.write_report(out, "resources.txt", txt)


def loop_of_casts(ds, o, d, K, step=1e-3):
    import torch
    n = o.shape[0]
    m = torch.full((n,), 1e-3, dtype=torch.float32, device=o.device)
    live = torch.ones(n, dtype=torch.bool, device=o.device)
    count = torch.zeros(n, dtype=torch.int32, device=o.device)
    slots = {k: [] for k in OUT}
    for _ in range(K):
        r = ds.cast_rays(o, d, min_t=m)
        live = live & (r["object"] >= 0)
        for k in OUT:
            keep = live if r[k].dim() == 1 else live[:, None]
            slots[k].append(torch.where(keep, r[k], torch.full_like(r[k], MISS[k])))
        count += live.to(torch.int32)
        m = torch.where(live, (r["t"].double() + step).float(), torch.full_like(m, float("inf")))
    out = {k: torch.stack(v) for k, v in slots.items()}
    out["count"] = count
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    assert torch.cuda.is_available(), "gpu_hits.py needs a GPU"
    dev = torch.device("cuda", 0)
    dense_dir = os.path.join(a.out, "_scenes")
    cases = [("bunny", os.path.join(ROOT, "scene", "bunny.json")),
             ("bunny_dense64k", scenes.make_dense_bunny(dense_dir, rounds=3, width=1920, height=1080))]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cases": []}
    for name, path in cases:
        s = ca.HostScene.load(path)
        assert s.ok
        s.set_size(1920, 1080)
        ds = ca.DeviceScene(s)
        o_np, d_np = ray_ref.camera_rays(ray_ref.RefScene(s).cam)
        o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
        n = o.shape[0]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
        for order, (oo, dd) in (("image", (o, d)), ("permuted", (o[perm].contiguous(), d[perm].contiguous()))):
            for K in (4, 8):
                one = ds.list_hits(oo, dd, K)
                loop = loop_of_casts(ds, oo, dd, K)
                same = all(torch.equal(one[k].view(torch.int32), loop[k].view(torch.int32)) for k in one)
                hist = torch.bincount(one["count"], minlength=K + 1).tolist()
                del one, loop
                t_one = gpu_common.timed(lambda: ds.list_hits(oo, dd, K), a.reps, a.warmup)
                t_loop = gpu_common.timed(lambda: loop_of_casts(ds, oo, dd, K), a.reps, a.warmup)
                rec = {"scene": name, "order": order, "K": K, "rays": n, "lists_by_length": hist, "same_bits": bool(same),
                       "one_launch_ms": t_one[0], "loop_ms": t_loop[0], "loop_over_one": t_loop[0] / t_one[0],
                       "min_max_ms": {"one": t_one[1:], "loop": t_loop[1:]}}
                result["cases"].append(rec)
                print(json.dumps(rec), flush=True)
        ds.close()
    with open(os.path.join(a.out, "hits.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = [f"hit lists on {result['device']}: HIP-event time of a whole call, median of {a.reps} after {a.warmup} warm-up calls", "",
             f"{'scene':16s} {'order':9s} {'K':>2s} {'rays':>9s} {'one launch ms':>14s} {'loop of casts ms':>17s} {'loop / one':>11s} {'same bits':>10s}  lists by length 0..K"]
    for r in result["cases"]:
        lines.append(f"{r['scene']:16s} {r['order']:9s} {r['K']:2d} {r['rays']:9d} {r['one_launch_ms']:14.3f} {r['loop_ms']:17.3f} "
                     f"{r['loop_over_one']:11.2f} {str(r['same_bits']):>10s}  {r['lists_by_length']}")
    lines += ["", "one launch: DeviceScene.list_hits(o, d, K), every output.  loop of casts: K rounds of DeviceScene.cast_rays with a per-ray",
              "min_t tensor, every output, ended rays masked and given min_t = +inf, slots stacked slot-major; all on the device, no host",
              "synchronisation inside a repetition.  Both times include the calls' own torch allocations."]
    with open(os.path.join(a.out, "hits.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
