"""Time of surface shading queries (ctr_shade_points) on one MI355X, against the two calls they sit between.

bunny.json at 1920x1080, the points being the camera's primary hits (cast_rays' point, normal and object; the view
direction is the ray's).  HIP-event time of one call, median of --reps after --warmup calls, once with the rays in image
order and once randomly permuted:
  (a) DeviceScene.shade_points(objects=..., colour only) on the hits
  (b) DeviceScene.shade_rays(bounces=0) on the same rays: the same shading behind that call's own cast
  (c) DeviceScene.cast_rays(object, point, normal) alone
  (d) with --parent-lib: (b) on another build of libcutrace_amd.so (the parent commit's), in a process of its own before
      and after the measurements above
Writes <out>/points.json and <out>/points.txt.  `--resources` (no GPU needed): the compiler's resource report of every
instantiation of the kernel into <out>/resources.txt.

  python scripts/gpu_points.py --out profiles/points [--reps 50 --warmup 10] [--parent-lib build_variants/parent/libcutrace_amd.so]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpu_common  # noqa: E402  (beside this file)
ORDERS = ("image_order", "permuted")


def resources(out):
    gpu_common.write_report(out, "resources.txt", gpu_common.resource_report(
        "ray_points.hip", "ray_points_kernel", ((1, "LINEAR"), (2, "EXACT_POW")), "default",
        "\n(hipcc --offload-arch=gfx950 with the library's flags.  Occupancy is waves per SIMD; ScratchSize is bytes per lane.  LDS Size\n"
        " is the static part: the walk stack is dynamic, stack_slots x 128 lanes x 4 bytes per workgroup, none under LINEAR.\n"
        " Workgroup: 128 lanes = 2 waves, as ray_query.hip's.  The VGPRs set 4 (default, LINEAR | EXACT_POW), 3 (EXACT_POW) and 6\n"
        " (LINEAR) waves per SIMD, i.e. 16 / 12 / 24 per CU: each a whole number of two-wave workgroups, so the block size costs\n"
        " no occupancy; the walk stack takes the same LDS per wave whatever the block size; and a finished workgroup frees its\n"
        " registers and its stack after two waves' tails instead of four or more.  No kernel uses scratch.)\n"))


def measure(a, only_shade_rays=False):
    import torch
    import cutrace_amd as ca
    from tests import ray_ref
    assert torch.cuda.is_available(), "gpu_points.py needs a GPU"
    dev = torch.device("cuda", 0)

    def timed(fn):
        return dict(zip(("median_ms", "min_ms", "max_ms"), gpu_common.timed(fn, a.reps, a.warmup)))

    s = ca.HostScene.load(os.path.join(ROOT, "scene", "bunny.json"))
    assert s.ok
    s.set_size(1920, 1080)
    ds = ca.DeviceScene(s)
    o_np, d_np = ray_ref.camera_rays(ray_ref.RefScene(s).cam)
    o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    n = o.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    rays = {"image_order": (o, d), "permuted": (o[perm].contiguous(), d[perm].contiguous())}
    rec = {"device": torch.cuda.get_device_name(0), "rays": n, "reps": a.reps, "warmup": a.warmup, "lib": os.environ.get("CUTRACE_AMD_LIB", "")}
    for order in ORDERS:
        oo, dd = rays[order]
        r = {"shade_rays_b0": timed(lambda: ds.shade_rays(oo, dd, bounces=0))}
        if not only_shade_rays:
            hit = ds.cast_rays(oo, dd, outputs=("object", "point", "normal"))
            r["hits"] = int((hit["object"] >= 0).sum())
            r["shade_points"] = timed(lambda: ds.shade_points(hit["point"], hit["normal"], dd, objects=hit["object"]))
            r["cast_rays"] = timed(lambda: ds.cast_rays(oo, dd, outputs=("object", "point", "normal")))
            got = ds.shade_points(hit["point"], hit["normal"], dd, objects=hit["object"])["color"]
            want = ds.shade_rays(oo, dd, bounces=0)["color"]
            r["same_bits_as_shade_rays"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        rec[order] = r
    ds.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="another build of libcutrace_amd.so whose shade_rays(bounces=0) is timed beside")
    ap.add_argument("--only-shade-rays", action="store_true", help="print the shade_rays(bounces=0) times as JSON (what --parent-lib runs)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.resources:
        resources(a.out)
        return
    if a.only_shade_rays:
        print("RESULT " + json.dumps(measure(a, only_shade_rays=True)))
        return

    def parent():
        env = dict(os.environ, CUTRACE_AMD_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-shade-rays", "--reps", str(a.reps), "--warmup", str(a.warmup),
                            "--out", a.out], env=env, capture_output=True, text=True, check=True, timeout=300)
        return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])

    result = {"parent_before": parent() if a.parent_lib else None}
    result["this"] = measure(a)
    result["parent_after"] = parent() if a.parent_lib else None
    with open(os.path.join(a.out, "points.json"), "w") as f:
        json.dump(result, f, indent=1)
    t = result["this"]
    lines = [f"surface shading queries on {t['device']}: bunny.json at 1920x1080, {t['rays']} camera rays, the points are their primary hits",
             f"HIP-event time of one call (launch to completion on the stream, output allocation included), median of {a.reps} after "
             f"{a.warmup} warm-up calls [min .. max]", ""]

    def cell(x):
        return f"{x['median_ms']:8.3f} [{x['min_ms']:.3f} .. {x['max_ms']:.3f}]"
    for order in ORDERS:
        r = t[order]
        lines += [f"{order}: {r['hits']} of {t['rays']} rays hit; shade_points after cast_rays equals shade_rays(bounces=0) bit for bit: "
                  f"{r['same_bits_as_shade_rays']}",
                  f"  (a) shade_points(objects, colour)           {cell(r['shade_points'])} ms   {t['rays'] / r['shade_points']['median_ms'] / 1e3:8.1f} Mpoints/s",
                  f"  (b) shade_rays(bounces=0), its cast included {cell(r['shade_rays_b0'])} ms",
                  f"  (c) cast_rays(object, point, normal)        {cell(r['cast_rays'])} ms",
                  f"      (a) + (c) over (b)                      {(r['shade_points']['median_ms'] + r['cast_rays']['median_ms']) / r['shade_rays_b0']['median_ms']:8.2f}"]
        for k in ("parent_before", "parent_after"):
            if result[k]:
                lines.append(f"  (d) shade_rays(bounces=0), parent build, {k[7:]:6s} {cell(result[k][order]['shade_rays_b0'])} ms")
        lines.append("")
    lines += ["(d) is a process of its own on the parent commit's library, run before and after the process that measured (a)-(c).",
              "Reported, not gated."]
    with open(os.path.join(a.out, "points.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
