"""Shared comparison helpers and scene builders for the parity tests."""
import glob
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-4  # per-channel float tolerance stated by BASELINE.json:north_star


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def depth_report(got, want):
    """depth: +inf must match +inf; finite compared. Returns (n_bad_bitexact, n_bad_tol, max_abs)."""
    fin_g, fin_w = np.isfinite(got), np.isfinite(want)
    mism_inf = int((fin_g != fin_w).sum())
    both = fin_g & fin_w
    diff = np.zeros(got.shape, np.float64)
    diff[both] = np.abs(got[both].astype(np.float64) - want[both].astype(np.float64))
    nbits = int((bits(got) != bits(want)).sum())
    return dict(inf_mismatch=mism_inf, not_bitexact=nbits, over_tol=int((diff > TOL).sum()) + mism_inf,
                max_abs=float(diff.max()) if diff.size else 0.0)


def float_report(got, want, tol=TOL):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d = np.where(np.isnan(d), np.inf, d)
    px_bad = (d.reshape(d.shape[0], d.shape[1], -1) > tol).any(-1) if d.ndim == 3 else (d > tol)
    return dict(not_bitexact=int((bits(got) != bits(want)).sum()), over_tol=int(px_bad.sum()),
                max_abs=float(d.max()) if d.size else 0.0)


def assert_parity(got, want, what="", color_tol=TOL):
    """The bar: depth and normal bit-exact (pure +,-,*,/,sqrt arithmetic), colour within 1e-4
    per channel (pow() differs by ≤1 ulp between glibc and the device)."""
    dr = depth_report(got["depth"], want["depth"])
    nr = float_report(got["normal"], want["normal"])
    cr = float_report(got["color"], want["color"], color_tol)
    msg = f"{what}: depth {dr} normal {nr} color {cr}"
    assert dr["not_bitexact"] == 0, msg
    assert nr["not_bitexact"] == 0, msg
    assert cr["over_tol"] == 0, msg
    return dict(depth=dr, normal=nr, color=cr)


def uv_close(got, want, tol=1e-4):
    """uv within the parity bar; NaN where the reference has NaN (plane normal without x and y, default_schema.hpp:170)"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{int((nan_g != nan_w).sum())} uv values are NaN on one side only"
    d = np.abs(np.where(nan_w, 0, got) - np.where(nan_w, 0, want))
    lim = tol * np.maximum(1.0, np.abs(np.where(nan_w, 0, want)))
    assert (d <= lim).all(), f"uv differs by up to {float(d.max()):.3e}"
    return float(d.max())


def mesh_scene(stl_path, w, h, tris, extra_objects=(), fudge_note=""):
    import json
    from cutrace_amd import scenes
    scenes.write_stl(stl_path, np.asarray(tris, np.float32).reshape(-1, 3, 3))
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
            {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10}]
    objs = [{"type": "mesh", "file": stl_path, "material": 0},
            {"type": "plane", "point": [0, -1.0, 0], "normal": [0, 1, 0], "material": 1}] + list(extra_objects)
    lights = [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
              {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}]
    cam = {"eye": [0.3, 0.8, 4.0], "up": [0, 1, 0], "look": [-0.05, -0.15, -1.0], "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


def corner_meshes():
    """Triangle lists for the mesh corner-case tests: quad, duplicates, degenerate, fan, far."""
    quad = [[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]]
    dup = quad + quad + [[[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]]] * 3          # duplicates and triplicates
    degenerate = quad + [[[0, 0, 1], [0, 0, 1], [0, 0, 1]], [[0, 0, 1], [1, 1, 1], [2, 2, 1]]]  # point, collinear
    fan = [[[0, 0, 0.3], [float(np.cos(a)), float(np.sin(a)), 0.0], [float(np.cos(a + 0.7)), float(np.sin(a + 0.7)), 0.0]]
           for a in np.arange(0, 6.28, 0.7)]
    far = (np.asarray(quad, np.float32) * 500.0 + np.float32([3000, 0, -9000])).tolist()
    return quad, dup, degenerate, fan, far


def _random_scene(seed, w=72, h=48, opaque_mesh=False, extra_planes=False):
    """Seeded random scene mixing every primitive, light and material feature (incl. reflect +
    transparency on the same material, coincident planes, a mesh and stand-alone triangles)."""
    import json
    rng = np.random.RandomState(seed)

    def v(lo, hi):
        return [float(x) for x in rng.uniform(lo, hi, 3)]

    mats = []
    for _ in range(int(rng.randint(2, 6))):
        mats.append({"type": "solid", "color": v(0.05, 1.0), "specular": float(rng.uniform(0, 1)),
                     "reflect": float(rng.choice([0.0, 0.0, 0.3, 0.9])), "phong": float(rng.choice([0.0, 1.0, 20.0, 300.0])),
                     "transparency": 0.0 if opaque_mesh else float(rng.choice([0.0, 0.0, 0.0, 0.5]))})
    nm = len(mats)
    objs = []
    for _ in range(int(rng.randint(1, 5))):
        objs.append({"type": "sphere", "center": v(-1.5, 1.5), "radius": float(rng.uniform(0.2, 0.8)), "material": int(rng.randint(nm))})
    for _ in range(int(rng.randint(1, 4))):
        objs.append({"type": "triangle", "p1": v(-2, 2), "p2": v(-2, 2), "p3": v(-2, 2), "material": int(rng.randint(nm))})
    floor = {"type": "plane", "point": [0, -1.2, 0], "normal": [0, 1, 0], "material": int(rng.randint(nm))}
    objs.append(floor)
    if rng.rand() < 0.5:
        objs.append(dict(floor, material=int(rng.randint(nm))))  # coincident plane: exact tie on t
    objs.append({"type": "plane", "point": [0, 0, -3], "normal": [0, 0, 1], "material": int(rng.randint(nm))})
    if extra_planes:
        # more walls, axis-aligned (zeros of either sign, any length of normal) and not, anywhere in the object list
        rng2 = np.random.RandomState(seed + 7919)
        for _ in range(int(rng2.randint(1, 7))):
            if rng2.rand() < 0.7:
                a = int(rng2.randint(3))
                n = [float(rng2.choice([0.0, -0.0])) for _ in range(3)]
                n[a] = float(rng2.choice([-1.0, 1.0]) * rng2.choice([1.0, 0.25, 3.0, 1e-3]))
                pt = [float(x) for x in rng2.uniform(-1, 1, 3)]
                pt[a] = float(-np.sign(n[a]) * rng2.uniform(2.0, 6.0))
            else:
                n = [float(x) for x in rng2.uniform(-1, 1, 3)]
                pt = [float(-4.0 * x) for x in n]
            objs.insert(int(rng2.randint(len(objs) + 1)), {"type": "plane", "point": pt, "normal": n, "material": int(rng2.randint(nm))})
    if opaque_mesh or rng.rand() < 0.7:
        objs.insert(int(rng.randint(len(objs) + 1)), {"type": "mesh", "file": "scene/skull.stl", "material": int(rng.randint(nm))})
    lights = [{"type": "sun", "direction": v(-1, 1), "color": v(0.2, 1)}]
    for _ in range(int(rng.randint(0, 3))):
        lights.append({"type": "point", "point": v(-3, 3), "color": v(0.2, 1)})
    cam = {"eye": [float(rng.uniform(-1, 3)), float(rng.uniform(-0.5, 2)), 4.0], "up": [0, 1, 0], "look": v(-0.5, 0.5),
           "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": float(rng.uniform(0, 0.3))}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


def _coplanar_scene(ca, tmp_path, w, h, row, n_tris, seed):
    """A mesh whose triangles all lie (to float rounding) in the plane that contains EVERY primary ray of image row
    `row`: for those rays alpha = det[a b c] of default_schema.hpp:59 is pure rounding noise, and so are beta, gamma
    and t — the regime in which the reference's float test can report a hit for a ray that passes far from the
    triangle (BVH caveat)."""
    import ctypes as C
    from cutrace_amd import _lib, scenes
    rng = np.random.default_rng(seed)
    eye, up, look = (0.3, 0.8, 4.0), (0.0, 1.0, 0.0), (-0.05, -0.15, -1.0)
    cam = _lib.Camera()
    _lib.host_lib().ctr_camera_look_at(C.byref(cam), _lib.Vec3(*eye), _lib.Vec3(*up), _lib.Vec3(*look))
    f32 = np.float32
    E, R, U, F = (np.array(v.tup(), f32) for v in (cam.pos, cam.right, cam.up, cam.forward))
    v = (f32(0.5) - f32(row) / f32(h)) * U + F           # the row's rays: E + s*right*k + t*v
    tris = []
    for _ in range(n_tris):
        s0, t0 = f32(rng.uniform(-1.2, 1.2)), f32(rng.uniform(2.0, 5.0))
        pts = []
        for _ in range(3):
            s, t = s0 + f32(rng.uniform(-0.25, 0.25)), t0 + f32(rng.uniform(-0.4, 0.4))
            pts.append((E + s * R + t * v).astype(f32))
        tris.append(pts)
    stl = str(tmp_path / f"coplanar_{seed}.stl")
    scenes.write_stl(stl, np.asarray(tris, f32))
    sc = {"camera": {"eye": list(eye), "up": list(up), "look": list(look), "near_plane": 0.1, "far_plane": 100.0,
                     "width": w, "height": h, "ambient": 0.1},
          "lights": [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
                     {"type": "point", "point": [float(E[0] + 0.5 * R[0] + 1.0 * v[0]), float(E[1] + 0.5 * R[1] + 1.0 * v[1]),
                                                  float(E[2] + 0.5 * R[2] + 1.0 * v[2])]}],   # a light IN the plane too
          "materials": [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
                        {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.2, "phong": 10}],
          "objects": [{"type": "mesh", "file": stl, "material": 0},
                      {"type": "plane", "point": [0, -1.0, 0], "normal": [0, 1, 0], "material": 1},
                      {"type": "plane", "point": [0, 0, -6.0], "normal": [0, 0, 1], "material": 1}]}
    return parse(ca, sc)


def _mirror_coplanar_scene(ca, tmp_path, w, h, row, n_tris, seed, transparent, two_mirrors=False):
    """The same regime for SECONDARY rays, which no upload-time guard can see (guard.cpp plan_guards checks eyes
    and lights): a tilted mirror reflects every primary ray of image row `row` into ONE plane — the mirror image of the
    row's plane, through the mirror image of the eye — and the mesh's triangles lie in that plane to float rounding, some
    on the reflected rays' way, some far to the side of it.  For those reflected rays (and, with `transparent`, for the
    pass-through rays that continue from an in-plane hit in the same plane) alpha and all three numerators of
    default_schema.hpp:57-78 are rounding noise.  Neither the eye nor any light lies in that plane."""
    import ctypes as C
    from cutrace_amd import _lib, scenes
    rng = np.random.default_rng(seed)
    eye, up, look = (0.2, 0.9, 3.5), (0.0, 1.0, 0.0), (0.02, -0.1, -1.0)
    cam = _lib.Camera()
    _lib.host_lib().ctr_camera_look_at(C.byref(cam), _lib.Vec3(*eye), _lib.Vec3(*up), _lib.Vec3(*look))
    f32, f64 = np.float32, np.float64
    E, R, U, F = (np.array(v.tup(), f64) for v in (cam.pos, cam.right, cam.up, cam.forward))
    v = (0.5 - row / h) * U + F                           # the row's rays: E + s*R + t*v
    pm = np.array([0.0, 0.0, -2.0])                       # the mirror: a plane through pm, tilted towards the ceiling
    nm = np.array([0.0, 0.35, 1.0])
    mirrors = [(pm, nm)]
    if two_mirrors:                                       # ... and a second one above that sends the rays down again
        mirrors.append((np.array([0.0, 3.0, 0.0]), np.array([0.0, -1.0, 0.25])))
    E2, R2, v2, t_mirror = E, R, v, 0.0
    for (p_, n_) in mirrors:                              # images of the eye and of the row's plane, mirror after mirror
        nh = n_ / np.linalg.norm(n_)
        t_mirror = np.dot(p_ - E2, nh) / np.dot(v2, nh)   # where the row's central ray meets this mirror
        assert t_mirror > 0, f"the row's central ray does not meet the mirror: t = {t_mirror}"
        E2 = E2 - 2.0 * np.dot(E2 - p_, nh) * nh
        R2, v2 = R2 - 2.0 * np.dot(R2, nh) * nh, v2 - 2.0 * np.dot(v2, nh) * nh
    tris = []
    for _ in range(n_tris):
        s0, t0 = rng.uniform(-1.5, 1.5), t_mirror + rng.uniform(0.4, 3.5)   # beyond the mirror point = on the reflected side
        pts = []
        for _ in range(3):
            s_, t_ = s0 + rng.uniform(-0.3, 0.3), t0 + rng.uniform(-0.35, 0.35)
            pts.append((E2 + s_ * R2 + t_ * v2).astype(f32))
        tris.append(pts)
    stl = str(tmp_path / f"mirror_coplanar_{seed}_{int(transparent)}.stl")
    scenes.write_stl(stl, np.asarray(tris, f32))
    mesh_mat = {"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40}
    if transparent:
        mesh_mat["transparency"] = 0.4
    sc = {"camera": {"eye": list(eye), "up": list(up), "look": list(look), "near_plane": 0.1, "far_plane": 100.0,
                     "width": w, "height": h, "ambient": 0.1},
          "lights": [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
                     {"type": "sun", "direction": [0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}],
          "materials": [mesh_mat,
                        {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10},
                        {"type": "solid", "color": [0.9, 0.9, 0.9], "specular": 0.1, "reflect": 0.9, "phong": 20}],
          "objects": [{"type": "mesh", "file": stl, "material": 0},
                      {"type": "plane", "point": [0, -1.5, 0], "normal": [0, 1, 0], "material": 1}] +
                     [{"type": "plane", "point": [float(x) for x in p_], "normal": [float(x) for x in n_], "material": 2}
                      for (p_, n_) in mirrors]}
    return parse(ca, sc)


def _multi_mesh_scene(tmp_path, seed, w=96, h=64, opaque=False, n_mesh=4):
    """n_mesh meshes cut out of scene/bunny.stl and scene/skull.stl, translated so that their boxes overlap, at random
    places of the object list, mixed with planes, a sphere and a stand-alone triangle."""
    from cutrace_amd import scenes
    rng = np.random.RandomState(seed)
    src = [scenes.read_stl(os.path.join(ROOT, "scene", f)) for f in ("bunny.stl", "skull.stl")]
    mats = [{"type": "solid", "color": [float(x) for x in rng.uniform(0.1, 1, 3)], "specular": float(rng.uniform(0, 1)),
             "reflect": float(rng.choice([0.0, 0.3, 0.8])), "phong": float(rng.choice([1.0, 20.0, 200.0])),
             "transparency": 0.0 if opaque else float(rng.choice([0.0, 0.0, 0.4]))} for _ in range(4)]
    objs = [{"type": "plane", "point": [0, -1.3, 0], "normal": [0, 1, 0], "material": 0},
            {"type": "plane", "point": [0, 0, -4], "normal": [0, 0, 1], "material": 1},
            {"type": "sphere", "center": [1.2, 0.4, -0.5], "radius": 0.5, "material": 2},
            {"type": "triangle", "p1": [-2, -1, -1], "p2": [-1, 1.5, -1.5], "p3": [-2.5, 1, 0], "material": 3}]
    for m in range(n_mesh):
        t = src[int(rng.randint(2))]
        t = t[rng.rand(len(t)) < rng.uniform(0.2, 0.7)]           # a random part of the mesh (open surface)
        c = t.reshape(-1, 3).mean(0)
        scale = np.float32(1.2 / np.abs(t.reshape(-1, 3) - c).max())
        t = ((t - c) * scale + np.float32(rng.uniform(-0.7, 0.7, 3))).astype(np.float32)
        path = str(tmp_path / f"mm_{seed}_{m}.stl")
        scenes.write_stl(path, t)
        objs.insert(int(rng.randint(len(objs) + 1)), {"type": "mesh", "file": path, "material": int(rng.randint(4))})
    if rng.rand() < 0.5:   # the same mesh twice: exact ties on t between two MESHES (the first in scene order wins)
        first = next(o for o in objs if o["type"] == "mesh")
        objs.append(dict(first, material=int(rng.randint(4))))
    lights = [{"type": "sun", "direction": [float(x) for x in rng.uniform(-1, 1, 3)], "color": [0.7, 0.7, 0.7]},
              {"type": "point", "point": [float(x) for x in rng.uniform(-3, 3, 3)], "color": [0.6, 0.5, 0.4]}]
    cam = {"eye": [float(rng.uniform(-1, 1)), float(rng.uniform(-0.3, 1.0)), 4.0], "up": [0, 1, 0],
           "look": [float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.2, 0.1)), -1.0], "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.15}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


# ---- ray and radiance queries: the generator and the comparers of tests/test_gpu_rays.py, test_gpu_shade.py and
# test_gpu_query_ranges.py ----
f32 = np.float32


def to_np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def f32_bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def sphere_mask(rs, obj):
    from tests import ray_ref
    return np.isin(obj, [i for i, o in enumerate(rs.objects) if o["type"] == ray_ref.OBJ_SPHERE])


def assert_same(rs, got, want, what):
    """every output of `want` present in `got` with the same bits (sphere uv: 1e-4); returns the number of hits"""
    _bits = f32_bits
    obj = np.asarray(want["object"])
    assert np.array_equal(got["object"], obj), f"{what}: object differs in {int((got['object'] != obj).sum())} rays"
    if "prim" in want:
        assert np.array_equal(got["prim"], want["prim"]), f"{what}: prim"
    for k in ("t", "point", "normal"):
        if k in want:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs in {int((_bits(got[k]) != _bits(want[k])).any(-1).sum() if got[k].ndim > 1 else (_bits(got[k]) != _bits(want[k])).sum())} rays"
    if "uv" in want:
        sph = sphere_mask(rs, obj)
        g, w = got["uv"], np.asarray(want["uv"], f32)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: uv NaNs"
        assert np.array_equal(_bits(np.nan_to_num(g[~sph])), _bits(np.nan_to_num(w[~sph]))), f"{what}: uv"
        if sph.any():
            assert np.abs(g[sph].astype(np.float64) - w[sph]).max() <= 1e-4, f"{what}: sphere uv"
    return int((obj >= 0).sum())


def ref_dict(r):
    return {k: (v.astype(np.int32) if k in ("object", "prim") else v) for k, v in r.items()}


def assert_bitwise(got, want, what):
    g, w = f32_bits(got), f32_bits(np.asarray(want, f32).reshape(np.shape(got)))
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.reshape(len(g), -1).any(-1).sum())} of {len(g)} rays differ"


def max_diff(got, want, what):
    """largest per-channel difference; NaN positions must agree"""
    want = np.asarray(want, f32).reshape(got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    d = np.abs(np.nan_to_num(got).astype(np.float64) - np.nan_to_num(want).astype(np.float64))
    m = float(d.max()) if d.size else 0.0
    print(f"{what}: colour max|diff| {m:.3e}")
    return m


def refusal(entry, scene, query, what=""):
    """ctr_last_error() after `entry` (ctr_cast_rays, ctr_shade_rays or ctr_shade_points of the HIP library) refused the
    query record (None: a null query) on the scene handle with CTR_E_INVALID"""
    import ctypes as C
    from cutrace_amd import _lib
    status = entry(scene, C.byref(query) if query is not None else None, None)
    assert status == 1, f"{what}: status {status}, not CTR_E_INVALID (1)"
    return _lib.hip_lib().ctr_last_error().decode()


def bad(entry, scene, query, text):
    """... and `text` is part of the message"""
    msg = refusal(entry, scene, query, text)
    assert text in msg, (text, msg)


def first_hit_same(got, want, what):
    assert np.array_equal(got["object"], np.asarray(want["object"]).astype(np.int32)), f"{what}: object"
    assert_bitwise(got["t"], want["t"], f"{what}: t")
    assert_bitwise(got["normal"], want["normal"], f"{what}: normal")


def random_rays(rng, n, rs, lo, hi, lengths=(0.01, 1.0, 30.0)):
    """(origins, directions, per-ray min_t): origins uniform in [lo, hi]^3 and inside spheres and mesh boxes, Gaussian
    directions times one of `lengths`, a component exactly zero (either sign) in 10 % of them"""
    from tests import ray_ref
    o = rng.uniform(lo, hi, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32) * rng.choice(list(lengths), (n, 1)).astype(f32)
    z = rng.rand(n) < 0.1                                      # a direction component exactly zero (either sign)
    d[z, rng.randint(0, 3, int(z.sum()))] = rng.choice([0.0, -0.0], int(z.sum())).astype(f32)
    k = 0
    for ob in rs.objects:                                      # origins inside spheres and inside mesh boxes
        if ob["type"] == ray_ref.OBJ_SPHERE:
            m = n // 20
            o[k:k + m] = ob["v0"] + rng.uniform(-0.3, 0.3, (m, 3)).astype(f32) * ob["f0"]
            k += m
        elif ob["type"] == ray_ref.OBJ_MESH:
            m = n // 10
            o[k:k + m] = rng.uniform(ob["v0"], ob["v1"], (m, 3)).astype(f32)
            k += m
    mt = rng.choice([1e-3, 0.0, -0.5, 0.25], n).astype(f32)  # per-ray min_t, zero and negative included
    return o, d, mt

# ---- the range sweeps of tests/test_gpu_query_ranges.py.  tests/test_query_ranges_cpu.py proves, exponent by exponent,
# that tests/ray_ref.py neither overflows nor goes denormal on these inputs: an exponent that fails there leaves both
# lists, it is not tolerated ----
DIR_EXPONENTS = (-104, -100, -96, -64, -24, 24, 64, 100)   # directions are multiplied by 2^j
SCALE_EXPONENTS = (-20, -12, 0, 12, 24)   # every position by 2^k (at -30 and 30 the checker's own normals go denormal / overflow)


def pow2(j):
    return f32(np.ldexp(1.0, int(j)))


def sweep_rays(seed, n, rs, min_ratio=2.0 ** -6, aim=0.5):
    """The sweeps' base rays on scene `rs`: random_rays with directions of length about 1.  The fraction `aim` of the rays
    (none with a zero component) then points at a vertex of one of the scene's meshes, and a direction whose smallest
    non-zero component is below min_ratio x its largest is drawn again, so that no product of the reference goes denormal
    when the direction is scaled.  `sel` in {0, 1, 2} picks each ray's min_t and max_t."""
    from tests import ray_ref

    def narrow(v):
        a = np.abs(v)
        return np.where(a > 0, a, np.inf).min(-1) < f32(min_ratio) * a.max(-1)

    rng = np.random.RandomState(seed)
    o, d, _ = random_rays(rng, n, rs, -3.0, 3.0, lengths=(1.0,))
    zero = d == 0
    meshes = [ob for ob in rs.objects if ob["type"] == ray_ref.OBJ_MESH and ob["tri_count"]]
    if meshes:
        verts = np.concatenate([rs.tris[ob["tri_begin"]:ob["tri_begin"] + ob["tri_count"]].reshape(-1, 3) for ob in meshes])
        todo = np.nonzero((rng.rand(n) < aim) & ~zero.any(-1))[0]
        while len(todo):
            v = verts[rng.randint(0, len(verts), len(todo))] - o[todo]
            v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
            ok = np.isfinite(v).all(-1) & ~narrow(v)
            d[todo[ok]] = v[ok]
            todo = todo[~ok]
    todo = np.nonzero(narrow(d))[0]
    while len(todo):
        v = rng.normal(size=(len(todo), 3)).astype(f32)
        # a draw that changes nothing: it keeps the stream, and so the rays, those on which the counts of
        # profiles/rays/direction_length_before_fix.txt were measured — do not remove it without measuring them again
        rng.choice([1.0], (len(todo), 1))
        d[todo] = np.where(zero[todo], d[todo], v)
        todo = todo[narrow(d[todo])]
    return o, d, rng.randint(0, 3, n)


def sweep_min_t(sel, j):
    """per-ray min_t from {0, 1e-3, 1e-3 * 2^-j}; j may be per ray"""
    return np.where(sel == 0, f32(0.0), np.where(sel == 1, f32(1e-3), f32(1e-3) * np.ldexp(f32(1.0), -np.asarray(j)).astype(f32))).astype(f32)


def sweep_max_t(sel, j):
    """per-ray max_t from {inf, 2 * 2^-j, 100 * 2^-j}"""
    s = np.ldexp(f32(1.0), -np.asarray(j)).astype(f32)
    return np.where(sel == 0, f32(np.inf), np.where(sel == 1, f32(2.0) * s, f32(100.0) * s)).astype(f32)


def scaled_scene_json(tmp_path, k, w=32, h=32):
    """One scene of every primitive, light and material kind, every position and the radius multiplied by 2^k: half of
    scene/bunny.stl, a plane, a stand-alone triangle, a sphere; a point light and a sun; an opaque, a reflecting and a
    transmitting material."""
    from cutrace_amd import scenes
    s = float(pow2(k))
    tris = scenes.read_stl(os.path.join(ROOT, "scene", "bunny.stl"))[::2]
    stl = str(tmp_path / f"scaled_{k}.stl")
    scenes.write_stl(stl, (tris * pow2(k)).astype(np.float32))

    def p(*v):
        return [float(np.float32(x)) * s for x in v]
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40},
            {"type": "solid", "color": [0.9, 0.9, 0.95], "specular": 0.3, "reflect": 0.7, "phong": 60},
            {"type": "solid", "color": [0.3, 0.8, 0.5], "specular": 0.6, "reflect": 0.0, "phong": 30, "transparency": 0.5}]
    objs = [{"type": "mesh", "file": stl, "material": 0},
            {"type": "plane", "point": p(0, -1.25, 0), "normal": [0.0, 1.0, 0.0], "material": 1},
            {"type": "triangle", "p1": p(-2.5, -1, -1.5), "p2": p(2.5, -1, -1.5), "p3": p(0.25, 2.5, -1.75), "material": 2},
            {"type": "sphere", "center": p(1.5, 0.25, 0.5), "radius": p(0.5)[0], "material": 2}]
    lights = [{"type": "point", "point": p(0.5, 2.5, 2.0), "color": [0.8, 0.8, 0.8]},
              {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}]
    cam = {"eye": p(0.5, 0.75, 4.0), "up": [0, 1, 0], "look": [-0.05, -0.15, -1.0], "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


# ---- the render-side range sweeps of tests/test_gpu_render_ranges.py.  tests/test_render_ranges_cpu.py proves, case by
# case, that the oracle stays inside its own arithmetic and that its frame shows every kind of object: a case that fails
# there leaves the list with a comment that says why, it is not tolerated ----
OFFSET_CASES = ((0, 10), (0, 14), (0, 18), (12, 10), (-12, 14))   # (k, e): the scene scaled by 2^k sits 2^e * 2^k off the origin
# (k, offset exponent or None, whether fudge scales with the scene: 1e-3 * 2^k, or stays 1e-3)
RENDER_RANGE_CASES = (tuple((k, None, True) for k in SCALE_EXPONENTS) + tuple((k, e, True) for k, e in OFFSET_CASES) +
                      tuple((k, None, False) for k in (-20, -12, 12, 24)))
RANGE_FLAVOURS = ("mixed", "opaque")
ALL_MISS_CASE = (-20, None, False)   # the scene is 2^-20 across and min_t is 1e-3: everything is nearer than min_t


# Supersampled frames (case, flavour, samples per axis) whose REDUCED oracle frame changes in some bit when the oracle's
# specular term is (float)pow((double)x, (double)e) — what VAR_EXACT_POW computes — in place of glibc's powf, which is not
# correctly rounded (about one result in a thousand is the neighbouring float).  tests/test_render_ranges_cpu.py proves on
# the CPU that these are exactly the frames that do: on them the bitwise colour comparison under VAR_EXACT_POW says nothing
# about the kernel; there the exact-pow launch is compared bit for bit with the oracle whose specular term is that rounded-once
# pow (oracle_render(pow_rounded_once=True), proved there to differ from the oracle in those colour words only), and with
# the oracle itself within TOL.  They stay in every other comparison.
# No 48 x 48 frame of any case depends on it.  (colour words that differ: 1, 1, 3, 1)
RANGE_POW_DEPENDENT = (((0, 10, True), "mixed", 2), ((0, 10, True), "opaque", 2), ((12, 10, True), "mixed", 2), ((12, 10, True), "opaque", 2))


def range_fudge(case):
    k, _, scaled = case
    return float(f32(1e-3) * pow2(k)) if scaled else 1e-3


def range_case_id(case):
    k, e, scaled = case
    return f"k={k},e={e},fudge={'1e-3*2^k' if scaled else '1e-3'}"


def range_offset(k, offset_exp):
    """the float32 offset of a case: 2^e * (1, -0.75, 0.5) * 2^k, or zeros"""
    if offset_exp is None:
        return np.zeros(3, f32)
    return (np.array([1.0, -0.75, 0.5], f32) * pow2(offset_exp)) * pow2(k)


def render_range_scene_json(tmp_path, k, offset_exp=None, opaque=False, w=48, h=48):
    """scaled_scene_json for the render: the mesh is two meshes (the even and the odd triangles of scene/bunny.stl, 1000
    triangles together), the camera's look point scales with the scene, so that every k shows the same view, and an
    offset 2^offset_exp * (1, -0.75, 0.5) * 2^k is added in float32 to every position: the mesh vertices after scaling, the
    plane's point, the triangle's corners, the sphere's centre, the point light, the eye and the look point.
    opaque: every transparency is 0."""
    from cutrace_amd import scenes
    s, off = pow2(k), range_offset(k, offset_exp)
    tris = scenes.read_stl(os.path.join(ROOT, "scene", "bunny.stl"))
    stls = []
    for part in (0, 1):
        stl = str(tmp_path / f"range_{k}_{offset_exp}_{part}.stl")
        scenes.write_stl(stl, ((tris[part::2] * s).astype(f32) + off).astype(f32))
        stls.append(stl)

    def p(*v):
        return [float(x) for x in (np.array(v, f32) * s + off).astype(f32)]
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40},
            {"type": "solid", "color": [0.9, 0.9, 0.95], "specular": 0.3, "reflect": 0.7, "phong": 60},
            {"type": "solid", "color": [0.3, 0.8, 0.5], "specular": 0.6, "reflect": 0.0, "phong": 30, "transparency": 0.0 if opaque else 0.5}]
    objs = [{"type": "mesh", "file": stls[0], "material": 0},
            {"type": "mesh", "file": stls[1], "material": 0},
            {"type": "plane", "point": p(0, -1.25, 0), "normal": [0.0, 1.0, 0.0], "material": 1},
            {"type": "triangle", "p1": p(-2.5, -1, -1.5), "p2": p(2.5, -1, -1.5), "p3": p(0.25, 2.5, -1.75), "material": 2},
            {"type": "sphere", "center": p(1.5, 0.25, 0.5), "radius": float(f32(0.5) * s), "material": 2}]
    lights = [{"type": "point", "point": p(0.5, 2.5, 2.0), "color": [0.8, 0.8, 0.8]},
              {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}]
    cam = {"eye": p(0.5, 0.75, 4.0), "up": [0, 1, 0], "look": p(-0.05, -0.15, -1.0), "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


RANGE_KINDS = {"mesh": (0, 1), "plane": (2,), "triangle": (3,), "sphere": (4,)}   # object indices of render_range_scene_json


def hall_of_mirrors_json(w, h, middle=None):
    """two facing mirror walls, a floor, and between them a sphere that both reflects and transmits (or the object `middle`,
    which gets that material): every level to bounces 15 is live"""
    mats = [{"type": "solid", "color": [0.9, 0.9, 0.95], "specular": 0.3, "reflect": 0.8, "phong": 60},
            {"type": "solid", "color": [0.7, 0.5, 0.3], "specular": 0.1, "reflect": 0.0, "phong": 5},
            {"type": "solid", "color": [0.3, 0.8, 0.5], "specular": 0.6, "reflect": 0.3, "phong": 30, "transparency": 0.5}]
    objs = [{"type": "plane", "point": [-2, 0, 0], "normal": [1, 0, 0], "material": 0},
            {"type": "plane", "point": [2, 0, 0], "normal": [-1, 0, 0], "material": 0},
            {"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": 1},
            dict(middle, material=2) if middle else {"type": "sphere", "center": [0.2, -0.3, 0.0], "radius": 0.6, "material": 2}]
    lights = [{"type": "point", "point": [0.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
              {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}]
    cam = {"eye": [0.9, 0.4, 4.0], "up": [0, 1, 0], "look": [-0.6, -0.2, -1.0], "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs})


# ---- the shading-parameter sweeps of tests/test_gpu_shading_ranges.py: materials, lights and phong exponents outside the
# box every other scene draws them from.  tests/test_shading_ranges_cpu.py proves the builders' claims (which sheet's
# partial sum reaches 1, how many occluders lie over which floor pixel, how many constructed rays sit in a highlight) and
# pins tests/shade_ref.py and, where built, the reference's own headers to the oracle on every case.  Out of scope, because
# they put NaN rays into the kernels: a sun of zero direction, a light exactly on a hit point, non-finite parameters, a
# negative phong exponent (DESIGN.md "Shading parameters the kernels are pinned over") ----
SHADE_W, SHADE_H = 48, 36


def _solid(color=(0.8, 0.8, 0.8), specular=0.0, reflect=0.0, phong=10.0, transparency=0.0):
    return {"type": "solid", "color": [float(x) for x in color], "specular": float(specular), "reflect": float(reflect),
            "phong": float(phong), "transparency": float(transparency)}


def _camera(eye, look, up=(0, 1, 0), w=SHADE_W, h=SHADE_H, ambient=0.1):
    return {"eye": [float(x) for x in eye], "up": [float(x) for x in up], "look": [float(x) for x in look], "near_plane": 0.1,
            "far_plane": 100.0, "width": w, "height": h, "ambient": float(ambient)}


def light_scale(host_scene):
    """Lambda: the sum over the lights of the largest |colour channel|.  The colour is linear in the light colours, so the
    colour bar of a case is TOL * max(1, Lambda)."""
    d = host_scene.desc.contents
    return float(sum(max(abs(c) for c in d.lights[i].color.tup()) for i in range(d.n_lights)))


# scene_flatten.h CTR_FAST_POW_KAPPA, restated: max |fs_fast - fs_ref| / e of the fast specular term, measured
# (profiles/shading_ranges/fastpow.txt)
FAST_POW_KAPPA = 2.42e-7


def fast_pow_kept(host_scene):
    """the chooser's rule (scene_flatten.h fast_pow_in_bar), restated: the fast specular path stays while
    2 kappa * max over the materials of |phong * specular| * largest |colour channel| * Lambda <= TOL"""
    d = host_scene.desc.contents
    worst = max((abs(float(d.materials[i].phong_exp) * float(d.materials[i].specular)) * max(abs(c) for c in d.materials[i].color.tup())
                 for i in range(d.n_materials)), default=0.0)
    return 2.0 * FAST_POW_KAPPA * worst * light_scale(host_scene) <= TOL


def _quad(x0, x1, y, z0, z1):
    return [[[x0, y, z0], [x1, y, z0], [x1, y, z1]], [[x0, y, z0], [x1, y, z1], [x0, y, z1]]]


# family 1, occluder stacks: sheets from the floor upwards, (kind, transparency).  "meshA" / "meshB": one quad of that mesh per
# entry — several entries of one name are several quads of ONE mesh, which share its material; "sphere": two crossings;
# "plane": horizontal and unbounded, so every floor point lies under it and the counts of such a stack start at 1.
# gaps: vertical distance to the sheet below (default 0.4); light_above: the point light sits above that many sheets.
STACK_CASES = {
    "0.75x4": dict(sheets=[("triangle", 0.75), ("meshA", 0.75), ("meshB", 0.75), ("meshA", 0.75)]),   # the sum IS 1.0 at sheet 4
    "0.5x2": dict(sheets=[("triangle", 0.5), ("meshA", 0.5)]),
    "0.9x12": dict(sheets=[("meshA", 0.9)] * 12),           # twelve quads of one mesh; the f32 sum of 1 - 0.9f
    "0.7x4": dict(sheets=[("triangle", 0.7), ("meshA", 0.7), ("meshA", 0.7), ("plane", 0.7)]),   # passes 1 between sheets
    "1.0x5": dict(sheets=[("triangle", 1.0), ("meshA", 1.0), ("meshB", 1.0), ("sphere", 1.0)]),   # never reaches 1
    "1.5x3": dict(sheets=[("meshA", 1.5), ("meshB", 1.5), ("triangle", 1.5)]),   # negative intensity, factor above 1
    "1e-7x2": dict(sheets=[("triangle", 1e-7), ("meshA", 1e-7)]),   # 1 - 1e-7 rounds below 1: an ordered loop, no bounce
    "mixed": dict(sheets=[("triangle", 0.9), ("meshA", 0.2), ("meshB", 0.6)]),
    "mixed_reversed": dict(sheets=[("triangle", 0.6), ("meshA", 0.2), ("meshB", 0.9)]),
    "close": dict(sheets=[("triangle", 0.6), ("meshA", 0.6)], gaps=[None, 5e-4]),   # the restart at last_hit + 1e-3 skips the second
    # the point light between sheets 2 and 3, over the staircase's second step, so that the floor lies under 0, 1 or 2 on its way
    "light_between": dict(sheets=[("triangle", 0.75), ("meshA", 0.75), ("meshB", 0.75), ("meshA", 0.75)], gaps=[None, 0.4, 1.2, 0.4],
                          light_above=2, light_x=-1.0),
}
# the sum is exactly 1.0 at the second sheet and a factor above 1 follows: a loop that went on at == 1.0 would come back below 1
STACK_CASES["exact_then_negative"] = dict(sheets=[("triangle", 0.5), ("meshA", 0.5), ("meshB", 1.5)])
# two unbounded, slightly tilted sheets, the first between 1.06e-3 and 1.94e-3 above the floor, the second 1e-3 above the first,
# under a vertical sun: the second is met at t1 + 1e-3 to within a few float32 ulps, t1 changing from pixel to pixel.  For t1 in
# [2^-10, 2^-9) the float sum t1 + 1e-3f is a tie for every other t1 while the DOUBLE sum t1 + 1e-3, narrowed once, never is:
# whether the loop sees the second sheet depends, on some pixels, on the restart being the double sum.
# (No camera fits beneath it: this case has the upper camera only, and no point light.)
STACK_CASES["restart_step"] = dict(sheets=[("plane", 0.5), ("plane", 0.5)], y0=1.5e-3, gaps=[None, 1e-3], sun=[0.0, -1.0, 0.0], plane_normal=[1.5e-4, 1.0, 5e-5],
                                   cameras=("above",), no_point=True)
STACK_CAMERAS = ("below", "above")


def stack_cameras(name):
    return STACK_CASES[name].get("cameras", STACK_CAMERAS)
STACK_FLOOR = 0   # the floor's object index in every stack scene
STACK_Y0 = 2.0    # height of the lowest sheet; the lower camera sits beneath it


def stack_crossings(name):
    """occluder crossings of a vertical ray through the whole stack (a sphere counts twice)"""
    return sum(2 if kind == "sphere" else 1 for kind, _ in STACK_CASES[name]["sheets"])


def stack_partial_sums(transparencies):
    """the shadow loop's float32 running sum of 1 - transparency, sheet after sheet (no early exit)"""
    s, out = f32(0.0), []
    for t in transparencies:
        s = f32(s + (f32(1.0) - f32(t)))
        out.append(s)
    return out


def first_full_sheet(transparencies):
    """1-based index of the sheet at which the running sum first reaches 1.0f, or None"""
    return next((i + 1 for i, s in enumerate(stack_partial_sums(transparencies)) if s >= f32(1.0)), None)


def stack_scene_json(tmp_path, name, camera, w=SHADE_W, h=SHADE_H):
    """(scene JSON, bounces).  An opaque matte floor y = 0, a point light and a sun above it, and between them the sheets of
    STACK_CASES[name]: flat sheet j of n covers x >= -1.5 + 3 j / n, so the floor under x in step j lies under j of them (a
    sphere over the last two steps adds two).  camera "below": under the lowest sheet, looking at the floor, so only
    shadow rays traverse the stack; "above": looking down through it, bounces = min(6, crossings)."""
    from cutrace_amd import scenes
    case = STACK_CASES[name]
    sheets = case["sheets"]
    gaps = case.get("gaps") or [None] * len(sheets)
    n_flat = sum(1 for kind, _ in sheets if kind in ("triangle", "meshA", "meshB"))
    mats = [_solid((0.9, 0.85, 0.8))]
    objs = [{"type": "plane", "point": [0, 0, 0], "normal": [0, 1, 0], "material": 0}]
    mesh_tris, mesh_mat, heights = {}, {}, []
    y, j = case.get("y0", STACK_Y0), 0
    for i, (kind, tr) in enumerate(sheets):
        if i:
            y += 0.4 if gaps[i] is None else gaps[i]
        heights.append(y)
        if kind in mesh_tris:
            assert mats[mesh_mat[kind]]["transparency"] == float(tr), "the quads of one mesh share its material"
        else:
            mats.append(_solid((0.3 + 0.1 * (i % 5), 0.8 - 0.1 * (i % 4), 0.5), specular=0.5, phong=30.0, transparency=tr))
        m = len(mats) - 1
        x0 = -1.5 + 3.0 * j / max(n_flat, 1)
        if kind == "triangle":
            objs.append({"type": "triangle", "p1": [x0, y, -9.0], "p2": [x0, y, 9.0], "p3": [x0 + 18.0, y, 0.0], "material": m})
            j += 1
        elif kind in ("meshA", "meshB"):
            if kind not in mesh_tris:
                mesh_tris[kind], mesh_mat[kind] = [], m
                objs.append({"type": "mesh", "file": str(tmp_path / f"stack_{name}_{kind}.stl"), "material": m})
            mesh_tris[kind] += _quad(x0, 5.0, y, -4.0, 4.0)
            j += 1
        elif kind == "sphere":
            objs.append({"type": "sphere", "center": [0.5, y + 1.0, 1.4], "radius": 0.9, "material": m})
            y += 2.0
        else:
            objs.append({"type": "plane", "point": [0, y, 0], "normal": case.get("plane_normal", [0, 1, 0]), "material": m})
    for kind, tris in mesh_tris.items():
        scenes.write_stl(str(tmp_path / f"stack_{name}_{kind}.stl"), np.asarray(tris, f32))
    top = y
    above = case.get("light_above")
    ly = top + 6.0 if above is None else 0.5 * (heights[above - 1] + heights[above])
    lights = [{"type": "point", "point": [case.get("light_x", -0.4), ly, 0.5], "color": [0.9, 0.9, 0.9]},
              {"type": "sun", "direction": case.get("sun", [0.15, -1.0, -0.1]), "color": [0.5, 0.5, 0.5]}][1 if case.get("no_point") else 0:]
    if camera == "below":
        cam, bounces = _camera((-3.5, STACK_Y0 - 0.2, 2.5), (-1.2, 0.0, 0.8), w=w, h=h), 2
    else:
        cam, bounces = _camera((-0.2, top + 3.0, 0.4), (-0.19, 0.0, 0.4), up=(0, 0, -1), w=w, h=h), min(6, stack_crossings(name))
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs}), bounces


# family 2, bounce thresholds: reflect, transparency, or both of one material take each of these values
_E6 = f32(1e-6)   # below the double 1e-6 the reference compares with: off; the next float up is on
THRESHOLD_VALUES = tuple(float(f32(v)) for v in (0.0, -0.0, 1e-7, _E6, np.nextafter(_E6, f32(1.0)), 0.25, 1.0, 1.5, -0.5))   # float32 values
THRESHOLD_MODES = ("reflect", "transparency", "both")
THRESHOLD_BOUNCES = (0, 1, 4)
THRESHOLD_MATERIAL = 2
THR_W, THR_H = 32, 24


def threshold_room_json(mode, value, w=THR_W, h=THR_H):
    """hall_of_mirrors_json closed to a room (a back wall, a ceiling, a wall behind the camera; the point light is inside,
    the sun is shut out); the middle sphere's material gets `value` as reflect, transparency or both"""
    sc = json.loads(hall_of_mirrors_json(w, h))
    m = sc["materials"][THRESHOLD_MATERIAL]
    m["reflect"], m["transparency"] = 0.0, 0.0
    for key in (("reflect", "transparency") if mode == "both" else (mode,)):
        m[key] = float(value)
    sc["objects"] += [{"type": "plane", "point": [0, 0, -3], "normal": [0, 0, 1], "material": 1},
                      {"type": "plane", "point": [0, 3, 0], "normal": [0, -1, 0], "material": 1},
                      {"type": "plane", "point": [0, 0, 6], "normal": [0, 0, -1], "material": 1}]
    return json.dumps(sc)


# family 3, the phong exponent
PHONG_EXPONENTS = (0.0, 0.5, 1.0, 2.0, 32.0, 300.0, 1000.0, 3000.0, 10000.0, 100000.0)
PHONG_LIGHTS = ("point", "sun")
PHONG_FRAME_MAX = 3000.0          # plain camera frames up to here: above it the highlight is narrower than a pixel
PHONG_THETAS = np.concatenate([[0.0], np.logspace(-5, np.log10(0.35), 15)])   # half vector off the normal by these angles
PHONG_POINTS = 72                 # 24 per surface: the plane, the sphere, the quad mesh
PHONG_RAYS_W, PHONG_RAYS_H = 48, 24   # the constructed rays as a lens frame: 72 * 16 = 48 * 24
_PHONG_POINT = np.array([0.5, 8.0, 3.0])
_PHONG_SUN = np.array([-0.05, -1.0, -0.35])
_PHONG_SPHERE = (np.array([-1.6, 0.2, 0.0]), 0.8)
_PHONG_QUAD = np.array([[0.8, -0.3, 1.0], [2.4, -0.5, 0.6], [2.6, 0.3, -0.8], [1.0, 0.5, -0.4]])   # a planar quad facing the lights


def _phong_quad_tris():
    """the quad as two triangles, wound so that the reference's normal (ray_ref.tri_normal) faces the lights"""
    from tests import ray_ref
    q = _PHONG_QUAD.copy()
    q[3] = q[0] + (q[2] - q[1])   # a parallelogram: planar
    q = q.astype(f32)
    tris = np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], f32)
    if ray_ref.tri_normal(tris[0, 0], tris[0, 1], tris[0, 2])[1] < 0:
        tris = tris[:, ::-1].copy()
    return tris


def phong_scene_json(tmp_path, e, light, w=SHADE_W, h=SHADE_H):
    """a plane, a sphere and a quad mesh of ONE material (specular 1, colour (1, 1, 1), phong e), one light of colour (1, 1, 1)"""
    from cutrace_amd import scenes
    stl = str(tmp_path / "phong_quad.stl")
    scenes.write_stl(stl, _phong_quad_tris())
    c, r = _PHONG_SPHERE
    objs = [{"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": 0},
            {"type": "sphere", "center": [float(x) for x in c], "radius": r, "material": 0},
            {"type": "mesh", "file": stl, "material": 0},
            # a triangle that turns its back on the camera and on the light: there max(0, n.h) is 0, and 0^e is 1 at e = 0
            {"type": "triangle", "p1": [0.6, 0.9, -1.5], "p2": [-0.6, 0.9, -1.5], "p3": [0.0, 1.9, -1.5], "material": 0}]
    lights = [{"type": "point", "point": [float(x) for x in _PHONG_POINT], "color": [1, 1, 1]} if light == "point" else
              {"type": "sun", "direction": [float(x) for x in _PHONG_SUN], "color": [1, 1, 1]}]
    cam = _camera((0.3, 2.5, 5.0), (0.2, -0.4, 0.0), w=w, h=h)
    return json.dumps({"camera": cam, "lights": lights, "materials": [_solid((1, 1, 1), specular=1.0, phong=e)], "objects": objs})


def phong_rays(light, seed=5):
    """(origins, directions), float32 (PHONG_POINTS * len(PHONG_THETAS), 3): per surface point p with normal n and unit
    direction l to the light, and per angle theta of PHONG_THETAS, the half vector h is n turned by theta about a random
    axis, the view direction v = 2 (l.h) h - l, the ray starts at p + 3 v and runs along -v.  Ray k * 16 + i: point k, angle i."""
    rng = np.random.RandomState(seed)
    tris = _phong_quad_tris().astype(np.float64)
    qn = np.cross(tris[0, 1] - tris[0, 0], tris[0, 2] - tris[0, 0])
    qn = qn / np.linalg.norm(qn) * (1 if qn[1] > 0 else -1)
    c, r = _PHONG_SPHERE
    pts = []
    for k in range(PHONG_POINTS):
        kind = k % 3
        if kind == 0:
            p, n = np.array([rng.uniform(-3, 3), -1.0, rng.uniform(-1.5, 2.5)]), np.array([0.0, 1.0, 0.0])
        elif kind == 1:
            to_l = _PHONG_POINT - c if light == "point" else -_PHONG_SUN
            n = to_l / np.linalg.norm(to_l) + rng.uniform(-0.3, 0.3, 3)   # within about 25 degrees of the light
            n = n / np.linalg.norm(n)
            p = c + r * n
        else:
            a, b = rng.uniform(0.15, 0.85, 2)
            p, n = tris[0, 0] + a * (tris[0, 1] - tris[0, 0]) + b * (tris[1, 2] - tris[0, 0]), qn
        pts.append((p, n))
    o, d = [], []
    for p, n in pts:
        l = (_PHONG_POINT - p) if light == "point" else -_PHONG_SUN
        l = l / np.linalg.norm(l)
        t1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
        t1 = t1 / np.linalg.norm(t1)
        t2 = np.cross(n, t1)
        for th in PHONG_THETAS:
            phi = rng.uniform(0, 2 * np.pi)
            for turn in (0.0, np.pi):   # the axis that leaves the view direction further above the surface
                hv = np.cos(th) * n + np.sin(th) * (np.cos(phi + turn) * t1 + np.sin(phi + turn) * t2)
                v = 2.0 * np.dot(l, hv) * hv - l
                if turn == 0.0 or np.dot(n, v) > best[0]:
                    best = (np.dot(n, v), v)
            v = best[1]
            assert np.dot(n, v) > 0.05, "a view direction below the surface"
            o.append(p + 3.0 * v)
            d.append(-v)
    return np.asarray(o, f32), np.asarray(d, f32)


# family 4, lights and ambient
def _many_lights(n, seed=2):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        col = [float(x) for x in rng.uniform(0.05, 0.4, 3)]
        if i % 2 == 0:
            out.append({"type": "point", "point": [float(x) for x in rng.uniform([-3, 1, -1], [3, 5, 4])], "color": col})
        else:
            out.append({"type": "sun", "direction": [float(x) for x in rng.uniform([-1, -1, -1], [1, -0.2, 1])], "color": col})
    return out


def _sun(j):
    s = float(pow2(j))
    return [{"type": "sun", "direction": [-0.3 * s, -1.0 * s, -0.25 * s], "color": [0.6, 0.6, 0.5]},
            {"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.3, 0.3, 0.4]}]


_FAR = float(pow2(20))
LIGHT_CASES = {
    **{f"n{n}": dict(lights=_many_lights(n)) for n in (0, 1, 2, 3, 8, 33)},
    "colours": dict(lights=[{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0, 0, 0]},
                            {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [64.0, 32.0, 16.0]},
                            {"type": "point", "point": [-1.0, 3.0, 1.5], "color": [0.5, -0.7, 0.2]}]),
    "sun_2^-10": dict(lights=_sun(-10)), "sun_1": dict(lights=_sun(0)), "sun_2^10": dict(lights=_sun(10)),
    "point_2^20_away": dict(lights=[{"type": "point", "point": [0.25 * _FAR, 0.75 * _FAR, 0.5 * _FAR], "color": [0.8, 0.8, 0.8]}]),
    "point_2e-3_above_the_floor": dict(lights=[{"type": "point", "point": [1.5, -1.0 + 2e-3, 1.0], "color": [0.8, 0.8, 0.8]},
                                               {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.3, 0.3, 0.3]}]),
    "point_inside_the_sphere": dict(lights=[{"type": "point", "point": [0.35, 0.1, 0.05], "color": [0.8, 0.8, 0.8]},
                                            {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.3, 0.3, 0.3]}]),
    "point_inside_the_glass_sphere": dict(lights=[{"type": "point", "point": [0.35, 0.1, 0.05], "color": [0.8, 0.8, 0.8]}], glass=0.5),
    "point_behind_the_wall": dict(lights=[{"type": "point", "point": [-3.5, 0.5, 0.0], "color": [0.8, 0.8, 0.8]}]),
    **{f"ambient_{a}": dict(lights=_many_lights(2), ambient=a) for a in (0.0, 1.0, 2.5, -0.25)},
}
LIGHT_SUN_LENGTH_CASES = ("sun_2^-10", "sun_1", "sun_2^10")   # one frame, bit for bit: v / |v| does not see a power of two


def lights_scene_json(tmp_path, name, w=SHADE_W, h=SHADE_H):
    """a reflecting floor, a sphere (opaque, or transmitting `glass`), an opaque wall (a quad mesh) at x = -2.5, and the lights
    and the ambient factor of LIGHT_CASES[name]"""
    from cutrace_amd import scenes
    case = LIGHT_CASES[name]
    stl = str(tmp_path / "lights_wall.stl")
    scenes.write_stl(stl, np.asarray([[[-2.5, -1, -2], [-2.5, -1, 2], [-2.5, 2, 2]], [[-2.5, -1, -2], [-2.5, 2, 2], [-2.5, 2, -2]]], f32))
    mats = [_solid((0.7, 0.6, 0.5), specular=0.3, reflect=0.2, phong=20.0),
            _solid((0.3, 0.6, 0.9), specular=0.5, phong=40.0, transparency=case.get("glass", 0.0)),
            _solid((0.8, 0.3, 0.3), specular=0.2, phong=5.0)]
    objs = [{"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": 0},
            {"type": "sphere", "center": [0.3, 0.0, 0.0], "radius": 0.9, "material": 1},
            {"type": "mesh", "file": stl, "material": 2}]
    cam = _camera((1.0, 1.2, 5.0), (-0.5, -0.2, 0.0), w=w, h=h, ambient=case.get("ambient", 0.1))
    return json.dumps({"camera": cam, "lights": case["lights"], "materials": mats, "objects": objs})


# every frame case of the sweep: (family, ...) tuples, their ids, and one builder
SHADING_FRAME_CASES = (tuple(("stack", n, c) for n in STACK_CASES for c in stack_cameras(n)) +
                       tuple(("threshold", m, i, b) for m in THRESHOLD_MODES for i in range(len(THRESHOLD_VALUES)) for b in THRESHOLD_BOUNCES) +
                       tuple(("phong", e, l) for e in PHONG_EXPONENTS if e <= PHONG_FRAME_MAX for l in PHONG_LIGHTS) +
                       tuple(("lights", n) for n in LIGHT_CASES))


def shading_case_id(case):
    if case[0] == "threshold":
        return f"threshold,{case[1]}={THRESHOLD_VALUES[case[2]]!r},bounces={case[3]}"
    return ",".join(str(x) for x in case)


def shading_case_json(tmp_path, case):
    """(scene JSON, bounces) of a frame case"""
    if case[0] == "stack":
        return stack_scene_json(tmp_path, case[1], case[2])
    if case[0] == "threshold":
        return threshold_room_json(case[1], THRESHOLD_VALUES[case[2]]), case[3]
    if case[0] == "phong":
        return phong_scene_json(tmp_path, case[1], case[2]), 2
    return lights_scene_json(tmp_path, case[1]), 3


# ---- what CPU and GPU tests both need ----
def parse(ca, sc):
    """the HostScene of a scene description (JSON text, or the dict of one), which must parse"""
    s = ca.HostScene.parse(sc if isinstance(sc, str) else json.dumps(sc))
    assert s.ok, f"the scene description did not parse: status {s.status}"
    return s


GOLD = os.path.join(ROOT, "tests", "golden")
GOLD_SMALL = sorted(glob.glob(os.path.join(GOLD, "small_*.npz")))   # <scene>_<w>x<h>_b<bounces>: generated by tests/golden/make_golden.py


def golden_case(path):
    """(scene name, width, height, bounces) of a golden file's name"""
    m = re.match(r"(small|full)_(.+)_(\d+)x(\d+)_b(\d+)\.npz", os.path.basename(path))
    return m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))
