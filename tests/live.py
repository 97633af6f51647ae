"""What the live-edit GPU tests share (mesh update, rebuild and replace; lights, materials and objects; the handle's arrays): mesh
generators, scene builders, readers of a parsed description, and the ONE check that an edited handle equals a fresh one.  pytest
rewrites `assert` in test modules only, so every assert here says what it compared."""
import ctypes as C
import json

import numpy as np

from cutrace_amd import _lib, scenes
from tests.gpu_support import assert_same_frame, same_tensors
from tests.util import mesh_scene, parse

W, H = 96, 54
BOUNCES = 3
KV_MERGE = 512
f32 = np.float32
EYE = [0.3, 0.8, 4.03]            # in no plane z = const of the guard meshes below


# ---------------------------------------------------------------- meshes

def random_mesh(n, seed, spread=0.9, size=0.3):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-spread, spread, (n, 1, 3))
    return (centre + rng.uniform(-size, size, (n, 3, 3))).astype(f32)


def moved(tris, angle, wobble, seed=0, shift=(0.0, 0.0, 0.0)):
    """a rotation about (1, 2, 3) by `angle`, a translation and a per-vertex wobble"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    rng = np.random.default_rng(seed)
    return (tris.astype(np.float64) @ R.T + np.asarray(shift) + rng.uniform(-wobble, wobble, tris.shape)).astype(f32)


def staircase():
    """scripts/mesh_rebuild_check.cpp's: 63 tiny triangles, their centroids at 2^-m, m = 0 .. 20, on each coordinate axis of the unit
    cube.  Every Morton key has a highest bit of its own, one peels off per split, and the device's tree is refused."""
    out = []
    for m in range(21):
        for axis in range(3):
            c = np.zeros(3, f32)
            c[axis] = np.ldexp(f32(1), -m)
            e = np.where(c != 0, np.ldexp(c, -10), np.ldexp(f32(1), -30)).astype(f32)
            out.append([c - e, c + e, [c[0] + e[0], c[1] - e[1], c[2]]])
    return np.asarray(out, f32)


def cluster(n, seed):
    """triangle positions and sizes over ten octaves around the origin (scripts/mesh_rebuild_check.cpp "geometric cluster"): a key
    spends three bits per octave, so the device's tree is several times deeper than the host's and still inside the walk's stack"""
    rng = np.random.default_rng(seed)
    t = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.3, 0.3, (n, 3, 3)))     # (large enough for rays to find them)
    return (t * np.ldexp(1.0, -(np.arange(n) % 10))[:, None, None]).astype(f32)


SMALL_AT = f32([2.5, 0.0, 2.5])       # where room_scene's 12-triangle mesh gets its new set: beside the 70-triangle mesh, in front of the eye


def outgrowing_set():
    """12 triangles over ten octaves (cluster): the device's tree over them has four nodes, where the 12-triangle meshes of the
    scenes here were created with one (scripts/mesh_rebuild_check.cpp's text says so for both), so the tree leaves its range and
    the node array grows"""
    return (cluster(12, seed=3) + SMALL_AT).astype(f32)


def guard_tris(k, n_other=400, seed=0, zero_area=True):
    """tests/test_scene_flatten.py's _guard_mesh with tilted fillers: k triangles IN the plane z = 0.5 (file indices 0..k-1),
    n_other triangles in the planes z = 2 + 0.1 j + 0.2 x, which hold neither EYE nor a light of the tests and are parallel to no
    sun of theirs, and (zero_area) two triangles of no area in the plane z = 0.5"""
    rng = np.random.RandomState(seed)
    tris = []
    for _ in range(k):
        c = rng.uniform(-1, 1, 2)
        tris.append([[c[0] + dx, c[1] + dy, 0.5] for dx, dy in ((0, 0), (0.3, 0.05), (0.1, 0.35))])
    for j in range(n_other):
        c = rng.uniform(-1, 1, 2)
        tris.append([[c[0] + dx, c[1] + dy, 2.0 + 0.1 * j + 0.2 * (c[0] + dx)] for dx, dy in ((0, 0), (0.3, 0.05), (0.1, 0.35))])
    if zero_area:
        tris += [[[0.1, 0.1, 0.5]] * 3, [[0, 0, 0.5], [0.5, 0.5, 0.5], [1, 1, 0.5]]]     # a point, three points of a line
    return np.asarray(tris, f32)


def on_a_busy_stream(tris):
    """(tensor, stream): `tris` on device 0 after some arithmetic on a stream of its own, with no wait between that work and the return"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    src = torch.from_numpy(tris).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        t = src
        for _ in range(20):                                           # (some work for the stream to be busy with)
            t = t * f32(1.01) + f32(0.001)
        t = t.contiguous()
    return t, stream


# ---------------------------------------------------------------- scenes

def scene_with(ca, tmp_path, name, meshes, w=W, h=H):
    """util.mesh_scene: meshes[0] (reflecting material), a floor, two lights — and the other meshes behind them"""
    paths = []
    for k, t in enumerate(meshes):
        paths.append(str(tmp_path / f"{name}_{k}.stl"))
        scenes.write_stl(paths[-1], t)
    extra = [{"type": "mesh", "file": p, "material": 1} for p in paths[1:]]
    return parse(ca, mesh_scene(paths[0], w, h, meshes[0], extra_objects=extra))


def base_scene(tmp_path, name, tris, extra=(), w=W, h=H):
    """util.mesh_scene as a dict: the mesh (material 0, reflecting), a floor (material 1), a point light and a sun"""
    paths = []
    for k, t in enumerate(extra):
        paths.append(str(tmp_path / f"{name}_x{k}.stl"))
        scenes.write_stl(paths[-1], t)
    return json.loads(mesh_scene(str(tmp_path / f"{name}.stl"), w, h, tris,
                                 extra_objects=[{"type": "mesh", "file": p, "material": 1} for p in paths]))


ROW = 12


def _row_plane(h):
    """eye, right and the in-plane direction of image row ROW, as util._coplanar_scene (test_rays_coplanar_with_triangles) builds them"""
    cam = _lib.Camera()
    _lib.host_lib().ctr_camera_look_at(C.byref(cam), _lib.Vec3(0.3, 0.8, 4.0), _lib.Vec3(0.0, 1.0, 0.0), _lib.Vec3(-0.05, -0.15, -1.0))
    E, R, U, F = (np.array(x.tup(), f32) for x in (cam.pos, cam.right, cam.up, cam.forward))
    return E, R, (f32(0.5) - f32(ROW) / f32(h)) * U + F


def in_plane_scene(ca, tmp_path, name, tris, w, h):
    """the scene of util._coplanar_scene around a mesh of our own: one of its lights lies in the plane of image row `ROW` too"""
    eye, up, look = (0.3, 0.8, 4.0), (0.0, 1.0, 0.0), (-0.05, -0.15, -1.0)
    E, R, v = _row_plane(h)
    stl = str(tmp_path / f"{name}.stl")
    scenes.write_stl(stl, tris)
    sc = {"camera": {"eye": list(eye), "up": list(up), "look": list(look), "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1},
          "lights": [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
                     {"type": "point", "point": [float(x) for x in (E + f32(0.5) * R + f32(1.0) * v)], "color": [0.5, 0.5, 0.5]}],
          "materials": [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
                        {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.2, "phong": 10}],
          "objects": [{"type": "mesh", "file": stl, "material": 0},
                      {"type": "plane", "point": [0, -1.0, 0], "normal": [0, 1, 0], "material": 1},
                      {"type": "plane", "point": [0, 0, -6.0], "normal": [0, 0, 1], "material": 1}]}
    return parse(ca, sc)


def with_in_plane(base, k, h, seed):
    """`base` with its first k triangles put into the plane that holds every primary ray of row ROW"""
    rng = np.random.default_rng(seed)
    E, R, v = _row_plane(h)
    out = base.copy()
    for i in range(k):
        s0, t0 = f32(rng.uniform(-1.2, 1.2)), f32(rng.uniform(2.0, 5.0))
        for p in range(3):
            s, t = s0 + f32(rng.uniform(-0.25, 0.25)), t0 + f32(rng.uniform(-0.4, 0.4))
            out[i, p] = (E + s * R + t * v).astype(f32)
    return out


OFF = [{"type": "point", "point": [3.0, -1.0, 1.0], "color": [0.9, 0.9, 0.9]}]   # in no plane of guard_tris


def guard_scene(tmp_path, name, meshes, lights, eye=EYE, w=48, h=27):
    objs = []
    for k, t in enumerate(meshes):
        path = str(tmp_path / f"{name}_{k}.stl")
        scenes.write_stl(path, t)
        objs.append({"type": "mesh", "file": path, "material": 0})
    objs.append({"type": "plane", "point": [0, -1.5, 0], "normal": [0, 1, 0], "material": 1})
    return {"camera": {"eye": list(eye), "up": [0, 1, 0], "look": [0.0, 0.0, 0.0], "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1},
            "lights": lights,
            "materials": [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40},
                          {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10}],
            "objects": objs}


# the object-edit scenes
OPAQUE, OTHER, GLASS, MIRROR = 0, 1, 2, 3
MATERIALS = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40},
             {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10},
             {"type": "solid", "color": [0.9, 0.9, 0.9], "specular": 0.3, "reflect": 0.0, "phong": 20, "transparency": 0.5},   # used by no object at first
             {"type": "solid", "color": [0.7, 0.7, 0.7], "specular": 0.3, "reflect": 0.4, "phong": 30}]
LIGHTS = [{"type": "point", "point": [3.0, -1.0, 1.0], "color": [0.9, 0.9, 0.9]}, {"type": "sun", "direction": [0.3, -0.8, 0.5], "color": [0.3, 0.3, 0.3]}]
ROOM_MESH, ROOM_SPHERE, ROOM_SMALL, ROOM_TRI, ROOM_WALL = 2, 4, 6, 7, 8
ROOM_PLANES = (0, 1, 3, 5, 8)


def camera(eye, look, w, h):
    return {"eye": list(eye), "up": [0, 1, 0], "look": list(look), "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1}


def room_scene(tmp_path, name, w=48, h=27):
    """(b) of scripts/object_edit_check.cpp: a box room of five axis-aligned planes, a 70-triangle mesh with five triangles in
    z = 0.5, a 12-triangle reflecting mesh, a sphere and a stand-alone triangle.  The eye's image in the wall z = -6, once that wall
    reflects and stands at z = 0, lies in z = 0.5."""
    big, small = str(tmp_path / f"{name}_70.stl"), str(tmp_path / f"{name}_12.stl")
    scenes.write_stl(big, guard_tris(5, n_other=65, seed=5, zero_area=False))
    scenes.write_stl(small, guard_tris(0, n_other=12, seed=6, zero_area=False) + f32([2.5, 0.0, 0.0]))
    objs = [{"type": "plane", "point": [-5, 0, 0], "normal": [1, 0, 0], "material": OTHER},
            {"type": "plane", "point": [5, 0, 0], "normal": [-1, 0, 0], "material": OTHER},
            {"type": "mesh", "file": big, "material": OPAQUE},
            {"type": "plane", "point": [0, -3, 0], "normal": [0, 1, 0], "material": OTHER},
            {"type": "sphere", "center": [-2.0, -1.0, 3.0], "radius": 0.7, "material": OPAQUE},
            {"type": "plane", "point": [0, 8, 0], "normal": [0, -1, 0], "material": OTHER},
            {"type": "mesh", "file": small, "material": MIRROR},
            {"type": "triangle", "p1": [-3, 0, 6], "p2": [-2, 0.5, 6.5], "p3": [-2.5, 2, 6], "material": OPAQUE},
            {"type": "plane", "point": [0, 0, -6], "normal": [0, 0, 1], "material": OTHER}]
    return {"camera": camera([0.3, 0.2, -0.5], [0.0, 0.1, 1.0], w, h), "lights": LIGHTS, "materials": MATERIALS, "objects": objs}


def edited(sc, **kw):
    out = json.loads(json.dumps(sc))
    out.update(kw)
    return out


def with_objects(sc, changes):
    """a copy of the scene with {object index: {field: value}} applied"""
    out = json.loads(json.dumps(sc))
    for i, kw in changes.items():
        out["objects"][i].update(kw)
    return out


# ---------------------------------------------------------------- a parsed description

def desc_lights(hs):
    d = hs.desc.contents
    return [d.lights[i] for i in range(int(d.n_lights))]


def desc_materials(hs):
    d = hs.desc.contents
    return [d.materials[i] for i in range(int(d.n_materials))]


def desc_objects(hs):
    """the description's objects as set_objects takes them (a mesh's tri_begin, v0 and v1 are ignored)"""
    d = hs.desc.contents
    return [d.objects[i] for i in range(int(d.n_objects))]


def mesh_objects(hs):
    d = hs.desc.contents
    return [i for i in range(d.n_objects) if d.objects[i].type == 1]


def desc_tris(hs, obj):
    """the triangles of mesh `obj` as the description holds them, (n, 3, 3) float32: exactly what a fresh handle is built from"""
    d = hs.desc.contents
    o = d.objects[obj]
    n = int(o.tri_count)
    raw = C.string_at(C.addressof(d.triangles[int(o.tri_begin)]), n * C.sizeof(_lib.Triangle))
    return np.frombuffer(raw, f32).reshape(n, 3, 3).copy()


def desc_box(hs, obj):
    o = hs.desc.contents.objects[obj]
    return np.array(o.v0.tup(), f32), np.array(o.v1.tup(), f32)


# ---------------------------------------------------------------- an edited handle against a fresh one

def frame(ds, bits, bounces=BOUNCES):
    ds.set_variant(bits)
    return ds.render(bounces=bounces)


def each_scan(monkeypatch, body):
    """body() with the guard's scan on the device, then on the host; what it returns (the guard states it went through) must
    be the same both times"""
    seen = {}
    for scan in ("device", "host"):
        monkeypatch.setenv("CUTRACE_GUARD_SCAN", scan)
        seen[scan] = body()
    assert seen["device"] == seen["host"], f"the scan on the device went through {seen['device']}, the scan on the host through {seen['host']}"
    assert seen["device"], "the case looked at no guard state"


def assert_box(upd, obj, fresh_scene, what):
    lo, hi = upd.mesh_box(obj)
    want_lo, want_hi = desc_box(fresh_scene, obj)                    # the loader's ctr_mesh_bounds
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), f"{what}: box {lo} {hi}, ctr_mesh_bounds {want_lo} {want_hi}"


def assert_equals_fresh(ca, upd, fresh, what, bounces=BOUNCES, base=0, same_trees=False, counters_of=None):
    """The edited handle `upd` against `fresh`, a handle created from the edited description.  Returns the guard state of every mesh.
    Always: depth, normal, colour and ray count under VAR_AUTO and VAR_EXACT_POW, bit for bit against `fresh` and against the
    handle's own VAR_NO_CLUSTER walk; and the guard state of every mesh.
    same_trees (every tree of `upd` is the builder's own, as every tree of `fresh` is) or counters_of: the kernel build of each of
    those launches too, the frame and the build under VAR_STATS, and its work counters — those of `fresh`, or those of the handle
    `counters_of`, which walks the trees `upd` walks (a mesh that update_mesh refitted is walked through another tree than a fresh
    build's: same frame, other work).  Without either, trees may differ, and a tree changes no result, only the work.
    base: variant bits both handles carry throughout (VAR_MERGE)."""
    work = same_trees or counters_of is not None
    for bits in (ca.VAR_AUTO, ca.VAR_EXACT_POW):
        u, f = frame(upd, base | bits, bounces), frame(fresh, base | bits, bounces)
        assert_same_frame(u, f, f"{what}, variant {bits}: edited vs fresh")
        if work:
            assert upd.last_kernel() == fresh.last_kernel(), f"{what}, variant {bits}: kernel {upd.last_kernel():#x} vs fresh {fresh.last_kernel():#x}"
        assert_same_frame(u, frame(upd, base | bits | ca.VAR_NO_CLUSTER, bounces), f"{what}, variant {bits}: edited vs its own linear walk")
    if work:
        u, f = frame(upd, base | ca.VAR_STATS, bounces), frame(fresh, base | ca.VAR_STATS, bounces)
        assert_same_frame(u, f, f"{what}, VAR_STATS")
        assert upd.last_kernel() == fresh.last_kernel(), f"{what}, VAR_STATS: kernel {upd.last_kernel():#x} vs fresh {fresh.last_kernel():#x}"
        if counters_of is not None:
            assert_same_frame(frame(counters_of, base | ca.VAR_STATS, bounces), f, f"{what}, VAR_STATS: the handle that gives the counters")
        want = (counters_of or fresh).last_counters()
        assert np.array_equal(upd.last_counters(), want), f"{what}: counters {upd.last_counters()} against {want}"
    upd.set_variant(base)
    fresh.set_variant(base)
    meshes = [k for k in range(upd.object_count()) if int(upd.get_object(k).type) == 1]
    state, want = [upd.guard_state(m) for m in meshes], [fresh.guard_state(m) for m in meshes]
    assert state == want, f"{what}: guard states {state} against the fresh handle's {want}"
    return state


def rays_at_the_mesh(n, seed, target=1.2):
    rng = np.random.default_rng(seed)
    o = (np.array([0.3, 0.8, 4.0]) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    return o, (rng.uniform(-target, target, (n, 3)) - o).astype(f32)


def assert_queries_equal_fresh(upd, fresh, n_lights, what):
    import torch
    rng = np.random.default_rng(15)
    n = 1024
    o = (np.array(EYE) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    d = (rng.uniform(-1.2, 1.2, (n, 3)) - o).astype(f32)
    cu, cf = upd.cast_rays(o, d), fresh.cast_rays(o, d)
    same_tensors(cu, cf, f"{what}: cast_rays")
    su, sf = upd.shadow(o, d, 50.0), fresh.shadow(o, d, 50.0)
    assert torch.equal(su, sf), f"{what}: shadow differs in {int((su != sf).sum())} rays"
    outs = ("color", "t", "object", "normal")
    same_tensors(upd.shade_rays(o, d, bounces=2, outputs=outs), fresh.shade_rays(o, d, bounces=2, outputs=outs), f"{what}: shade_rays")
    args = dict(normals=cf["normal"], view_dirs=torch.from_numpy(d), objects=cf["object"], outputs=("color", "light_shadow"))
    pu, pf = upd.shade_points(cf["point"], **args), fresh.shade_points(cf["point"], **args)
    assert tuple(pu["light_shadow"].shape) == (n, n_lights), f"{what}: light_shadow is {tuple(pu['light_shadow'].shape)}, not {(n, n_lights)}"
    same_tensors(pu, pf, f"{what}: shade_points")
