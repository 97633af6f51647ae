"""NumPy restatement of ctr_list_hits (include/cutrace_hits.h), vectorised over the live rays (TEST INFRASTRUCTURE): the chain
of nearest casts of the reference's shadow_intensity (inc/shading.hpp:22-45) over tests/ray_ref.py's ray_cast, the hits kept
instead of summed.  Also the scene the hit-list tests share and the running sum that turns a list back into shadow_intensity.
The checker of tests/test_gpu_hits.py; pinned against ray_ref.shadow_intensity by tests/test_hits_cpu.py."""
import json

import numpy as np

from tests import ray_ref

f32 = np.float32
OUTPUTS = ("t", "object", "prim", "point", "normal", "uv")
_MISS = {"t": f32(np.inf), "object": -1, "prim": -1, "point": f32(0), "normal": f32(0), "uv": f32(0)}
_COLS = {"t": (), "object": (), "prim": (), "point": (3,), "normal": (3,), "uv": (2,)}


def list_hits(scene, start, dirs, max_hits, min_t=f32(1e-3), max_t=f32(np.inf), step=1e-3, ignore_transparent=False):
    """count (n,) int32 and slot-major t, object, prim (K, n), point, normal (K, n, 3), uv (K, n, 2):
         m = min_t; for j < K: h = ray_cast(ray, m); stop unless h hits and h.t < max_t; slot j = h; m = (float)((double)h.t + step)
    Unfilled slots hold ray_cast's miss values."""
    start = np.ascontiguousarray(start, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    n, K = len(start), int(max_hits)
    m = np.broadcast_to(np.asarray(min_t, f32), (n,)).astype(f32)
    max_t = np.broadcast_to(np.asarray(max_t, f32), (n,)).astype(f32)
    out = {k: np.full((K, n) + _COLS[k], _MISS[k], np.int32 if k in ("object", "prim") else f32) for k in OUTPUTS}
    count = np.zeros(n, np.int32)
    live = np.arange(n)
    for j in range(K):
        if not len(live):
            break
        r = ray_ref.ray_cast(scene, start[live], dirs[live], m[live], ignore_transparent=ignore_transparent)
        with np.errstate(all="ignore"):
            go = (r["object"] >= 0) & (r["t"] < max_t[live])
        live = live[go]
        for k in OUTPUTS:
            out[k][j, live] = r[k][go]
        count[live] = j + 1
        m[live] = (r["t"][go].astype(np.float64) + np.float64(step)).astype(f32)   # shading.hpp:32: a double add, narrowed
    out["count"] = count
    return out


def shadow_from_lists(scene, count, objects):
    """shadow_intensity (shading.hpp:22-45) from a ray's list: the float32 running sum of 1 - transparency of the listed
    objects' materials, hit after hit, 1 as soon as it reaches 1.  Valid where the list did not end at its last slot."""
    K, n = objects.shape
    trans = np.array([scene.transparency[o["mat"]] for o in scene.objects], f32)
    inten = np.zeros(n, f32)
    open_ = np.ones(n, bool)
    for j in range(K):
        on = open_ & (j < count)
        inten[on] = inten[on] + (f32(1.0) - trans[objects[j, on]])
        full = on & (inten >= f32(1.0))
        inten[full] = f32(1.0)
        open_ &= ~full
    return inten


# ---- the scene of the hit-list tests: layers of every kind of object, opaque and transmitting ----
LAYERS_Z = (-0.5, -0.3, -0.1, 0.1, 0.3, 0.5)
COINCIDENT_PLANE = 5   # object 5 lies in object 4's plane: ray_cast prefers the lower index, and the restart skips the tie


def layered_description(tmp_path, w=16, h=16):
    """the description, as a dict, of: object 0: a mesh of six stacked quads over [-1, 1]^2 at z = -0.5 .. 0.5 (material 0); 1, 2: spheres; 3: a triangle;
    4, 5: two coincident planes; 6: a plane.  Material 0 is opaque, material 1 has transparency 0.5."""
    from cutrace_amd import scenes
    tris = []
    for z in LAYERS_Z:
        tris += [[[-1, -1, z], [1, -1, z], [1, 1, z]], [[-1, -1, z], [1, 1, z], [-1, 1, z]]]
    stl = str(tmp_path / "layers.stl")
    scenes.write_stl(stl, np.asarray(tris, f32))
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40, "transparency": 0.0},
            {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10, "transparency": 0.5}]
    objs = [{"type": "mesh", "file": stl, "material": 0},
            {"type": "sphere", "center": [1.5, 0.2, 0.0], "radius": 0.7, "material": 1},
            {"type": "sphere", "center": [-1.2, -0.3, 0.4], "radius": 0.5, "material": 0},
            {"type": "triangle", "p1": [-2, -2, 1], "p2": [2, -2, 1.2], "p3": [0, 2, 0.8], "material": 1},
            {"type": "plane", "point": [0, -1.2, 0], "normal": [0, 1, 0], "material": 0},
            {"type": "plane", "point": [0, -1.2, 0], "normal": [0, 1, 0], "material": 1},
            {"type": "plane", "point": [0, 0, -3], "normal": [0, 0, 1], "material": 0}]
    cam = {"eye": [0.3, 0.2, 9.0], "up": [0, 1, 0], "look": [0, 0, 0], "near_plane": 0.1, "far_plane": 100.0,
           "width": w, "height": h, "ambient": 0.2}
    return {"camera": cam, "lights": [{"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [1, 1, 1]}], "materials": mats, "objects": objs}


def layered_scene(ca, tmp_path, w=16, h=16):
    s = ca.HostScene.parse(json.dumps(layered_description(tmp_path, w, h)))
    assert s.ok, "the layered scene failed to parse"
    return s


def layered_rays(n=4000, seed=1):
    """origins uniform in [-3, 3]^3, Gaussian directions times one of 0.01, 1, 30"""
    rng = np.random.RandomState(seed)
    o = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3)).astype(f32) * rng.choice([0.01, 1.0, 30.0], (n, 1)).astype(f32)
    return o, d
