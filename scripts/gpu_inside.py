"""Time of the inside queries (ctr_count_crossings, ctr_inside_points; include/cutrace_inside.h) on one MI355X, each against what
a caller would otherwise run.  There is no pass bar: every case is reported, the ones the tree or the single launch loses included.

Per scene (bunny.json, 1 000 triangles, and its 64 000-triangle version):
  count_crossings   the 2.07 M camera rays of the 1920x1080 frame, in image order and randomly permuted, min_t 1e-3:
                    the default walk | linear=True | list_hits(outputs=(), max_hits=16) on the same rays, the only crossing
                    count the library had (its chain rules make it another number: `same as list_hits` says how often)
  inside, R = 3     the frame's primary hit points pushed 0.05 off the surface, image order and permuted, and as many
                    uniform points in the box of those hit points (the room):
                    one launch | the same asking for `votes` (all three rays of every point: what the early stop saves) |
                    linear=True | three count_crossings launches plus torch parity and a vote
  signed_distance   the same points: signed_distance | nearest_points(skip_planes=True, outputs=("distance",)) alone: the
                    difference is the price of the sign
HIP-event time of a whole call, median with its spread (min, max) of --reps calls after --warmup; the linear walks of the dense
scene get --linear-reps after one warm-up call.  The walks are compared once per case.  Each scene is a run of its own
(--scene), so that a job gives each its own time limit; a run replaces its scene's cases in <out>/inside.json and rewrites
<out>/inside.txt from all of them.  `--resources` (no GPU needed): the compiler's resource report of the four kernels into
<out>/resources.txt.

  python scripts/gpu_inside.py --out profiles/inside --scene bunny [--reps 20 --warmup 3 --linear-reps 3]
  python scripts/gpu_inside.py --out profiles/inside --scene bunny_dense64k
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)

SCENES = ("bunny", "bunny_dense64k")


def resources(out):
    from cutrace_amd import build as b
    cmd = [b.hipcc(), *b.HIP_FLAGS, "--offload-device-only", "-c", "-o", os.devnull, os.path.join(b.CSRC, "ray_cross.hip"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, check=True)
    lines = []
    for line in r.stderr.splitlines():
        m = gpu_common.REMARK.search(line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            v = re.search(r"(ray_cross_kernel|ray_inside_kernel)ILb([01])E", m.group(2))
            lines.append(f"{v.group(1)}<{'true' if v.group(2) == '1' else 'false'}> ({'LINEAR' if v.group(2) == '1' else 'default walk'})" if v else m.group(2))
        else:
            lines.append(f"    {m.group(1)}: {m.group(2)}")
    note = ("\n(hipcc --offload-arch=gfx950 with the library's flags.  Occupancy is waves per SIMD; ScratchSize is bytes per lane.  LDS Size\n"
            " is the static part: the walk stack is dynamic, stack_slots x 128 lanes x 4 bytes per workgroup, none under LINEAR.\n"
            " No instantiation uses scratch.)\n")
    gpu_common.write_report(out, "resources.txt", "\n".join(lines) + note)


def report(result, out):
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}]"
    lines = [f"inside queries on {result['device']}: HIP-event time of a whole call in ms, median [min .. max] of {result['reps']} calls after "
             f"{result['warmup']} warm-up calls", f"(linear walks of the dense scene: of {result['linear_reps']} after 1)", "",
             "count_crossings(outputs=(\"count\", \"signed\"), min_t=1e-3) on the frame's camera rays",
             f"{'scene':16s} {'triangles':>9s} {'order':9s} {'n':>8s} {'tree walk':>31s} {'linear':>31s} {'list_hits K=16':>31s} {'linear/tree':>11s} {'hits/tree':>9s} {'tree = linear':>13s} {'same as list_hits':>17s}"]
    for r in result["cases"]:
        if r["call"] == "count_crossings":
            lines.append(f"{r['scene']:16s} {r['triangles']:9d} {r['order']:9s} {r['n']:8d} {fmt(r['tree_ms']):>31s} {fmt(r['linear_ms']):>31s} "
                         f"{fmt(r['list_hits_ms']):>31s} {r['linear_ms'][0] / r['tree_ms'][0]:11.1f} {r['list_hits_ms'][0] / r['tree_ms'][0]:9.2f} "
                         f"{str(r['tree_equals_linear']):>13s} {r['same_as_list_hits']:17.4f}")
    lines += ["", "inside at R = 3 (the default directions)",
              f"{'scene':16s} {'triangles':>9s} {'points':8s} {'order':9s} {'n':>8s} {'inside':>31s} {'with votes (no early stop)':>31s} {'linear':>31s} {'3 x count_crossings + torch':>31s} {'3 launches/inside':>17s} {'votes/inside':>12s} {'same':>5s} {'inside %':>8s}"]
    for r in result["cases"]:
        if r["call"] == "inside":
            lines.append(f"{r['scene']:16s} {r['triangles']:9d} {r['points']:8s} {r['order']:9s} {r['n']:8d} {fmt(r['inside_ms']):>31s} {fmt(r['votes_ms']):>31s} "
                         f"{fmt(r['linear_ms']):>31s} {fmt(r['three_launches_ms']):>31s} {r['three_launches_ms'][0] / r['inside_ms'][0]:17.2f} "
                         f"{r['votes_ms'][0] / r['inside_ms'][0]:12.2f} {str(r['same']):>5s} {100.0 * r['inside_fraction']:8.2f}")
    lines += ["", "signed_distance against nearest_points(skip_planes=True, outputs=(\"distance\",)) alone",
              f"{'scene':16s} {'triangles':>9s} {'points':8s} {'order':9s} {'n':>8s} {'signed_distance':>31s} {'nearest_points':>31s} {'signed/nearest':>14s}"]
    for r in result["cases"]:
        if r["call"] == "signed_distance":
            lines.append(f"{r['scene']:16s} {r['triangles']:9d} {r['points']:8s} {r['order']:9s} {r['n']:8d} {fmt(r['signed_ms']):>31s} {fmt(r['nearest_ms']):>31s} "
                         f"{r['signed_ms'][0] / r['nearest_ms'][0]:14.2f}")
    lines += ["", "tree = linear / same: the default walk's integers equal the linear walk's (and, for inside, the three launches' vote).",
              "same as list_hits: the fraction of rays whose count equals list_hits' (another definition: a surface less than `step` behind a hit",
              "is skipped there, a chain ends at K).  surface: the frame's primary hit points pushed 0.05 along their normals; uniform: uniform",
              "points in the box of those hit points.  All times include the calls' own torch allocations."]
    with open(os.path.join(out, "inside.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inside"))
    ap.add_argument("--scene", choices=SCENES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--linear-reps", type=int, default=3)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        resources(a.out)
        return
    if not a.scene:
        ap.error("--scene or --resources")
    import torch
    import cutrace_amd as ca
    from cutrace_amd import scenes
    from tests import ray_ref
    assert torch.cuda.is_available(), "gpu_inside.py needs a GPU"
    dev = torch.device("cuda", 0)
    path = os.path.join(ROOT, "scene", "bunny.json") if a.scene == "bunny" else \
        scenes.make_dense_bunny(tempfile.mkdtemp(prefix="inside_scenes_"), rounds=3, width=1920, height=1080)
    s = ca.HostScene.load(path)
    assert s.ok
    s.set_size(1920, 1080)
    ds = ca.DeviceScene(s)
    rs = ray_ref.RefScene(s)
    tris = int(sum(o["tri_count"] for o in rs.objects if o["type"] == ray_ref.OBJ_MESH))
    slow = tris > 10000
    lin_reps, lin_warm = (a.linear_reps, 1) if slow else (a.reps, a.warmup)
    head = {"scene": a.scene, "triangles": tris}
    cases = []

    def add(rec):
        cases.append(rec)
        print(json.dumps(rec), flush=True)

    o_np, d_np = ray_ref.camera_rays(rs.cam)
    ro, rd = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    n = ro.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    both = ("count", "signed")
    for order, (o, d) in (("image", (ro, rd)), ("permuted", (ro[perm].contiguous(), rd[perm].contiguous()))):
        tree = ds.count_crossings(o, d, min_t=1e-3, outputs=both)
        lin = ds.count_crossings(o, d, min_t=1e-3, outputs=both, linear=True)
        hits = ds.list_hits(o, d, 16, outputs=())["count"]
        rec = dict(head, call="count_crossings", order=order, n=n, tree_equals_linear=all(bool(torch.equal(tree[k], lin[k])) for k in both),
                   same_as_list_hits=float((tree["count"] == hits).float().mean()), mean_count=float(tree["count"].float().mean()))
        del tree, lin, hits
        rec["tree_ms"] = gpu_common.timed(lambda: ds.count_crossings(o, d, min_t=1e-3, outputs=both), a.reps, a.warmup)
        rec["linear_ms"] = gpu_common.timed(lambda: ds.count_crossings(o, d, min_t=1e-3, outputs=both, linear=True), lin_reps, lin_warm)
        rec["list_hits_ms"] = gpu_common.timed(lambda: ds.list_hits(o, d, 16, outputs=()), a.reps, a.warmup)
        add(rec)
    hit = ds.cast_rays(ro, rd, outputs=("point", "normal", "object"))
    surface = torch.where((hit["object"] >= 0)[:, None], hit["point"] + 0.05 * hit["normal"], hit["point"]).contiguous()
    lo, hi = surface.min(0).values, surface.max(0).values
    uniform = (lo + (hi - lo) * torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(dev)).contiguous()
    del hit, ro, rd
    table = [torch.from_numpy(v).to(dev).expand(n, 3).contiguous() for v in ca.inside_default_dirs()]

    def three_launches(p):
        votes = sum((ds.count_crossings(p, dv, skip_planes=True, skip_triangles=True)["count"] & 1) for dv in table)
        return votes >= 2

    for which, pts in (("surface", surface), ("uniform", uniform)):
        for order, p in (("image", pts), ("permuted", pts[perm].contiguous())):
            one = ds.inside(p)["inside"]
            full = ds.inside(p, outputs=("inside", "votes"))
            lin = ds.inside(p, outputs=("inside", "votes"), linear=True)
            same = bool(torch.equal(one, full["inside"])) and all(bool(torch.equal(full[k], lin[k])) for k in full) and bool(torch.equal(one, three_launches(p)))
            rec = dict(head, call="inside", points=which, order=order, n=n, same=same, inside_fraction=float(one.float().mean()),
                       split_votes=int(((full["votes"] == 1) | (full["votes"] == 2)).sum()))
            del one, full, lin
            rec["inside_ms"] = gpu_common.timed(lambda: ds.inside(p), a.reps, a.warmup)
            rec["votes_ms"] = gpu_common.timed(lambda: ds.inside(p, outputs=("inside", "votes")), a.reps, a.warmup)
            rec["linear_ms"] = gpu_common.timed(lambda: ds.inside(p, linear=True), lin_reps, lin_warm)
            rec["three_launches_ms"] = gpu_common.timed(lambda: three_launches(p), a.reps, a.warmup)
            add(rec)
            rec = dict(head, call="signed_distance", points=which, order=order, n=n)
            rec["signed_ms"] = gpu_common.timed(lambda: ds.signed_distance(p), a.reps, a.warmup)
            rec["nearest_ms"] = gpu_common.timed(lambda: ds.nearest_points(p, skip_planes=True, outputs=("distance",)), a.reps, a.warmup)
            add(rec)
    ds.close()
    js = os.path.join(a.out, "inside.json")
    result = json.load(open(js)) if os.path.exists(js) else {"cases": []}
    result.update(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, linear_reps=a.linear_reps)
    result["cases"] = sorted([c for c in result["cases"] if c["scene"] != a.scene] + cases, key=lambda c: SCENES.index(c["scene"]))
    with open(js, "w") as f:
        json.dump(result, f, indent=1)
    report(result, a.out)


if __name__ == "__main__":
    main()
