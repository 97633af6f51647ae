"""Ray queries on the GPU (ctr_cast_rays, DeviceScene.cast_rays / shadow) against the reference's ray_cast and
shadow_intensity: the C oracle where it covers the case (camera rays), tests/ray_ref.py (its NumPy restatement, pinned
against the oracle by tests/test_rays_cpu.py) everywhere else.  "Same bits": bitwise, except the sphere's texture
coordinates (atan2f / asinf on the device, 1e-4)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle
from tests import ray_ref, util
from tests.conftest import load_scene
from tests.util import (assert_same as _assert_same, f32_bits as _bits, random_rays as _random_rays, ref_dict as _ref_dict,
                        to_np as _np)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
THREADS = os.cpu_count() or 4


# ---- 1. camera rays in image order ----
@pytest.mark.parametrize("name,w,h", [("bunny", 96, 54), ("mirror", 96, 54), ("sphere_plane", 96, 54)])
def test_camera_rays_equal_the_render_and_the_oracle(ca, name, w, h):
    s = load_scene(ca, name, w, h)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(rs.cam)
    got = _np(ds.cast_rays(o, d, min_t=1e-3))
    r = ds.render_uv(bounces=0, fudge=1e-3)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=0, threads=THREADS, hit_ids=True, uv=True)
    want = dict(t=r["depth"].reshape(-1), normal=r["normal"].reshape(-1, 3), uv=r["uv"].reshape(-1, 2),
                object=g["hit_id"].reshape(-1))
    assert _assert_same(rs, got, want, name) > 0
    assert np.array_equal(_bits(got["t"]), _bits(g["depth"].reshape(-1)))
    ds.close()


def test_camera_rays_of_the_dense_bunny(ca, tmp_path):
    """the 64 000-triangle bunny: the whole frame against the render, sampled rows against the oracle's hit ids"""
    from cutrace_amd import scenes
    w, h = 192, 108
    s = ca.HostScene.load(scenes.make_dense_bunny(str(tmp_path), rounds=3, width=w, height=h))
    assert s.ok
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(rs.cam)
    got = _np(ds.cast_rays(o, d, min_t=1e-3))
    r = ds.render_uv(bounces=0, fudge=1e-3)
    for k, n in (("t", 1), ("normal", 3), ("uv", 2)):
        src = r["depth" if k == "t" else k].reshape(-1, n) if n > 1 else r["depth"].reshape(-1)
        assert np.array_equal(_bits(got[k]), _bits(src)), k
    for r0 in (20, 54, 80):
        g = oracle.oracle_render(s, fudge=1e-3, bounces=0, rows=(r0, r0 + 2), threads=THREADS, hit_ids=True)
        assert np.array_equal(got["object"][r0 * w:(r0 + 2) * w], g["hit_id"].reshape(-1))
        assert np.array_equal(_bits(got["t"][r0 * w:(r0 + 2) * w]), _bits(g["depth"].reshape(-1)))
    assert (got["prim"][got["object"] == 0] >= 0).all()
    ds.close()


# ---- 2. an incoherent batch: many cameras, permuted ----
def test_incoherent_batch_of_many_cameras(ca):
    from cutrace_amd import _lib
    w, h = 48, 32
    s = load_scene(ca, "bunny", w, h)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(11)
    desc = s.desc.contents
    keep = _lib.Camera()
    C.memmove(C.byref(keep), C.byref(desc.cam), C.sizeof(_lib.Camera))
    origins, dirs, want = [], [], []
    for _ in range(6):
        cam = _lib.Camera()
        C.memmove(C.byref(cam), C.byref(keep), C.sizeof(_lib.Camera))
        eye = _lib.Vec3(*[float(x) for x in rng.uniform([-2.5, -0.5, 1.0], [2.5, 2.0, 5.0])])
        look = _lib.Vec3(*[float(x) for x in rng.uniform(-0.4, 0.4, 3)])
        _lib.host_lib().ctr_camera_look_at(C.byref(cam), eye, _lib.Vec3(0.0, 1.0, 0.0), look)
        desc.cam = cam
        rs = ray_ref.RefScene(s)
        o, d = ray_ref.camera_rays(rs.cam)
        g = oracle.oracle_render(s, fudge=1e-3, bounces=0, threads=THREADS, hit_ids=True, uv=True)
        origins.append(o)
        dirs.append(d)
        want.append(dict(t=g["depth"].reshape(-1), normal=g["normal"].reshape(-1, 3), uv=g["uv"].reshape(-1, 2),
                         object=g["hit_id"].reshape(-1)))
    desc.cam = keep
    o, d = np.concatenate(origins), np.concatenate(dirs)
    perm = rng.permutation(len(o))
    got = _np(ds.cast_rays(o[perm], d[perm], min_t=1e-3))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    rs = ray_ref.RefScene(s)
    for c in range(6):
        sl = inv[c * w * h:(c + 1) * w * h]
        _assert_same(rs, {k: v[sl] for k, v in got.items()}, want[c], f"camera {c}")
    ordered = _np(ds.cast_rays(o, d, min_t=1e-3))
    for k in ordered:
        assert np.array_equal(_bits(ordered[k][perm]) if ordered[k].dtype == f32 else ordered[k][perm],
                              _bits(got[k]) if got[k].dtype == f32 else got[k]), k
    ds.close()


# ---- 3. random rays against ray_ref ----
@pytest.mark.parametrize("which", ["bunny", "random0", "random5"])
def test_random_rays_against_ray_ref(ca, which):
    from tests.util import _random_scene
    s = load_scene(ca, "bunny", 32, 32) if which == "bunny" else ca.HostScene.parse(_random_scene(int(which[6:]), w=32, h=32))
    assert s.ok
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(3)
    n = 20000 if which == "bunny" else 6000
    o, d, mt = _random_rays(rng, n, rs, -3.0, 3.0)
    want = _ref_dict(ray_ref.ray_cast(rs, o, d, mt))
    for linear in (False, True):
        got = _np(ds.cast_rays(o, d, min_t=mt, linear=linear))
        assert _assert_same(rs, got, want, f"{which} linear={linear}") > n // 10
    ds.close()


# ---- 4. the reference's rules ----
def _axis_scene(ca, tmp_path, name, meshes, extra=()):
    import json
    from cutrace_amd import scenes
    objs = []
    for k, tris in enumerate(meshes):
        path = str(tmp_path / f"{name}_{k}.stl")
        scenes.write_stl(path, np.asarray(tris, f32))
        objs.append({"type": "mesh", "file": path, "material": k % 2})
    objs += list(extra)
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40},
            {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10}]
    cam = {"eye": [0.3, 0.2, 9.0], "up": [0, 1, 0], "look": [0, 0, 0], "near_plane": 0.1, "far_plane": 100.0,
           "width": 16, "height": 16, "ambient": 0.2}
    s = ca.HostScene.parse(json.dumps({"camera": cam, "lights": [{"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [1, 1, 1]}],
                                       "materials": mats, "objects": objs}))
    assert s.ok
    return s


def test_ties_go_to_the_lower_object_and_the_lower_file_index(ca, tmp_path):
    quad = [[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]]
    dup = quad + quad + [[[-1, -1, 0.0], [1, -1, 0.0], [0, 1, 0.0]]]
    plane = {"type": "plane", "point": [0, 0, 0], "normal": [0, 0, 1], "material": 0}
    tri = {"type": "triangle", "p1": [-1, -1, 0], "p2": [1, -1, 0], "p3": [1, 1, 0], "material": 1}
    s = _axis_scene(ca, tmp_path, "ties", [dup, dup], extra=(tri, plane, plane))
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(5)
    n = 4000
    o = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(0.5, 4.0, (n, 1))], 1).astype(f32)
    d = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), -np.ones((n, 1))], 1).astype(f32)
    want = _ref_dict(ray_ref.ray_cast(rs, o, d, f32(1e-3)))
    for linear in (False, True):
        got = _np(ds.cast_rays(o, d, linear=linear))
        _assert_same(rs, got, want, f"ties linear={linear}")
        hit = got["object"] >= 0
        assert set(np.unique(got["object"][hit])) <= {0, 3} and (got["object"] == 0).any()   # mesh 0, or the plane beyond it
        assert set(np.unique(got["prim"][got["object"] == 0])) <= {0, 1, 4}                 # first copies in file order
    ds.close()


def test_mesh_whose_nearest_valid_t_equals_min_t_is_rejected_whole(ca, tmp_path):
    big = lambda z: [[-4, -4, z], [4, -4, z], [0, 5, z]]
    s = _axis_scene(ca, tmp_path, "mint", [[big(-1.0), big(-2.0)], [big(-3.0)]])
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    o = np.zeros((3, 3), f32)
    d = np.tile(f32([0, 0, -1]), (3, 1))
    mt = f32([1.0, 0.5, 2.0])
    for linear in (False, True):
        got = _np(ds.cast_rays(o, d, min_t=mt, linear=linear))
        assert got["t"].tolist() == [3.0, 1.0, 3.0] and got["object"].tolist() == [1, 0, 1], got
        _assert_same(rs, got, _ref_dict(ray_ref.ray_cast(rs, o, d, mt)), "t0 == min_t")
    ds.close()


def test_mesh_whose_box_test_fails_is_missed_whatever_its_triangles_say(ca, tmp_path):
    """dir.z exactly 0 and the origin in the box's z-min plane: (bmin.z - start.z) * (1/0) = NaN, `tmin <= tmax` false —
    the mesh is missed although the ray meets its triangle's edge in that plane; the mesh behind is what it sees"""
    edge_on = [[2, -1, 0], [2, 1, 0], [2, 0, 1]]
    behind = [[5, -9, -9], [5, 9, -9], [5, 0, 12]]
    s = _axis_scene(ca, tmp_path, "nanbox", [[edge_on], [behind]])
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    y = np.linspace(-0.4, 0.4, 33).astype(f32)
    o = np.zeros((33, 3), f32)
    d = np.stack([np.ones(33, f32), y, np.zeros(33, f32)], 1)
    want = _ref_dict(ray_ref.ray_cast(rs, o, d, f32(1e-3)))
    assert (want["object"] == 1).all()
    for linear in (False, True):
        _assert_same(rs, _np(ds.cast_rays(o, d, linear=linear)), want, f"NaN box linear={linear}")
    ds.close()


# ---- 5. ignore_transparent ----
def test_ignore_transparent_against_ray_ref_and_the_render(ca):
    from tests.util import _random_scene
    for seed in (2, 4, 9):
        s = ca.HostScene.parse(_random_scene(seed + 40, w=64, h=40))
        assert s.ok
        rs = ray_ref.RefScene(s)
        ds = ca.DeviceScene(s)
        o, d = ray_ref.camera_rays(rs.cam)
        got = _np(ds.cast_rays(o, d, ignore_transparent=True))
        _assert_same(rs, got, _ref_dict(ray_ref.ray_cast(rs, o, d, f32(1e-3), ignore_transparent=True)), f"ign {seed}")
        ds.set_variant(ca.VAR_IGNORE_TRANSPARENT)
        r = ds.render_uv(bounces=0)
        _assert_same(rs, got, dict(t=r["depth"].reshape(-1), normal=r["normal"].reshape(-1, 3), uv=r["uv"].reshape(-1, 2),
                                   object=got["object"]), f"ign render {seed}")
        rng = np.random.RandomState(seed)
        o2, d2, mt = _random_rays(rng, 3000, rs, -2.5, 2.5)
        _assert_same(rs, _np(ds.cast_rays(o2, d2, min_t=mt, ignore_transparent=True)),
                     _ref_dict(ray_ref.ray_cast(rs, o2, d2, mt, ignore_transparent=True)), f"ign random {seed}")
        ds.close()


# ---- 6. shadow ----
@pytest.mark.parametrize("seed,opaque", [(1, False), (7, False), (2, True), (5, True)])
def test_shadow_against_ray_ref_and_a_loop_of_casts(ca, seed, opaque):
    import torch
    from tests.util import _random_scene
    s = ca.HostScene.parse(_random_scene(seed, w=32, h=32, opaque_mesh=opaque))
    assert s.ok
    rs = ray_ref.RefScene(s)
    assert (rs.transparency == 0).all() == opaque  # all opaque: the any-hit path
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(seed)
    o, d, _ = _random_rays(rng, 3000, rs, -2.5, 2.5)
    max_t = rng.choice([0.5, 2.0, 100.0, np.inf], len(o)).astype(f32)
    want = ray_ref.shadow_intensity(rs, o, d, max_t)
    for linear in (False, True):
        got = ds.shadow(o, d, max_t=torch.from_numpy(max_t), linear=linear).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), f"seed {seed} linear={linear}: {int((_bits(got) != _bits(want)).sum())} rays"
    assert ((want > 0) & (want < 1)).any() != opaque and (want == 1).any() and (want == 0).any()
    # the reference's loop made of cast_rays calls: min_dist = (float)((double)last_hit + 1e-3)
    inten = np.zeros(len(o), f32)
    last = np.zeros(len(o), f32)
    live = np.ones(len(o), bool)
    while live.any():
        idx = np.nonzero(live)[0]
        r = _np(ds.cast_rays(o[idx], d[idx], min_t=(last[idx].astype(np.float64) + 1e-3).astype(f32), outputs=("t", "object")))
        go = (r["object"] >= 0) & (r["t"] < max_t[idx])
        live[idx[~go]] = False
        idx, t, ob = idx[go], r["t"][go], r["object"][go]
        inten[idx] = inten[idx] + (f32(1) - rs.transparency[[rs.objects[i]["mat"] for i in ob]])
        full = inten[idx] >= 1
        inten[idx[full]] = 1
        live[idx[full]] = False
        last[idx] = t
    assert np.array_equal(_bits(inten), _bits(want))
    ds.close()


# ---- 7. rays in a triangle's plane ----
def test_in_plane_rays_linear_is_exact(ca, tmp_path):
    """Origins in the plane of a mesh's triangles (a plane that holds no eye and no light), directions in that plane: the
    regime where the reference's float test is rounding noise.  linear=True is bit-identical to ray_ref; how many
    results of the default walk differ is reported, not asserted (the documented caveat)."""
    import json
    from cutrace_amd import scenes
    rng = np.random.default_rng(7)
    P = f32([0.2, -0.1, 0.3])
    U = (f32([0.8, 0.15, -0.3]) / np.linalg.norm([0.8, 0.15, -0.3])).astype(f32)
    V = np.cross(U, f32([0.1, 0.9, 0.4])).astype(f32)
    V = (V / np.linalg.norm(V)).astype(f32)
    pt = lambda a, b: (P + f32(a) * U + f32(b) * V).astype(f32)
    tris = []
    for _ in range(64):
        a0, b0 = rng.uniform(-2, 2, 2)
        tris.append([pt(a0 + rng.uniform(-0.2, 0.2), b0 + rng.uniform(-0.2, 0.2)) for _ in range(3)])
    stl = str(tmp_path / "inplane.stl")
    scenes.write_stl(stl, np.asarray(tris, f32))
    sc = {"camera": {"eye": [0.5, 3.0, 6.0], "up": [0, 1, 0], "look": [0, 0, 0], "near_plane": 0.1, "far_plane": 100.0,
                     "width": 16, "height": 16, "ambient": 0.1},
          "lights": [{"type": "point", "point": [2.0, 4.0, 1.0], "color": [1, 1, 1]}],
          "materials": [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40}],
          "objects": [{"type": "mesh", "file": stl, "material": 0}]}
    s = ca.HostScene.parse(json.dumps(sc))
    assert s.ok
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    n = 8000
    ab = rng.uniform(-2.5, 2.5, (n, 2))
    o = np.stack([pt(a, b) for a, b in ab]).astype(f32)
    ang = rng.uniform(0, 2 * np.pi, n)
    d = (np.cos(ang)[:, None] * U + np.sin(ang)[:, None] * V).astype(f32)
    want = _ref_dict(ray_ref.ray_cast(rs, o, d, f32(1e-3)))
    lin = _np(ds.cast_rays(o, d, linear=True))
    hits = _assert_same(rs, lin, want, "in-plane, linear")
    dflt = _np(ds.cast_rays(o, d))
    differ = int(((dflt["object"] != want["object"]) | (_bits(dflt["t"]) != _bits(want["t"]))).sum())
    print(f"in-plane rays: {n}, reference hits {hits}, default walk differs in {differ}")
    ds.close()


# ---- 8. the two walks agree ----
def test_linear_and_default_walk_agree_on_the_dense_bunny(ca, tmp_path):
    import torch
    from cutrace_amd import scenes
    s = ca.HostScene.load(scenes.make_dense_bunny(str(tmp_path), rounds=3, width=64, height=36))
    assert s.ok
    ds = ca.DeviceScene(s)
    g = torch.Generator().manual_seed(8)
    n = 100000
    o = (torch.rand(n, 3, generator=g) * 2.4 - 1.2).cuda()
    o[:, 1] += 0.5
    d = torch.randn(n, 3, generator=g).cuda()
    a = ds.cast_rays(o, d)
    b = ds.cast_rays(o, d, linear=True)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert int((a["object"] == 0).sum()) > n // 20
    ds.close()


# ---- 9. edge cases ----
def test_sizes_output_subsets_and_graph_capture(ca):
    import torch
    s = load_scene(ca, "sphere_plane", 32, 18)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(9)
    o, d, mt = _random_rays(rng, 1000, rs, -3.0, 3.0)
    full = _np(ds.cast_rays(o, d, min_t=mt))
    _assert_same(rs, full, _ref_dict(ray_ref.ray_cast(rs, o, d, mt)), "1000 rays")
    empty = ds.cast_rays(o[:0], d[:0])
    assert all(v.shape[0] == 0 for v in empty.values()) and ds.shadow(o[:0], d[:0], 1.0).shape == (0,)
    one = _np(ds.cast_rays(o[:1], d[:1], min_t=mt[:1]))
    for k in full:
        assert np.array_equal(one[k], full[k][:1]), k
    for m in (1, 63, 129, 999):
        part = _np(ds.cast_rays(o[:m], d[:m], min_t=mt[:m]))
        for k in full:
            assert np.array_equal(part[k], full[k][:m]), (m, k)
    for k in ca.RAY_OUTPUTS:
        sub = _np(ds.cast_rays(o, d, min_t=mt, outputs=(k,)))
        assert list(sub) == [k] and np.array_equal(sub[k], full[k]), k
    sub = _np(ds.cast_rays(o, d, min_t=mt, outputs=("uv", "prim")))
    assert np.array_equal(sub["uv"], full["uv"]) and np.array_equal(sub["prim"], full["prim"])
    # a single-stream graph capture, replayed once
    od, dd, md = (torch.from_numpy(x).cuda() for x in (o, d, mt))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ds.cast_rays(od, dd, min_t=md)   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ds.cast_rays(od, dd, min_t=md)
    graph.replay()
    torch.cuda.synchronize()
    for k in full:
        assert np.array_equal(cap[k].cpu().numpy(), full[k]), k
    ds.close()


def test_bad_arguments(ca):
    import torch
    from cutrace_amd import _lib
    L = _lib.hip_lib()
    s = load_scene(ca, "sphere_plane", 32, 18)
    ds = ca.DeviceScene(s)
    n = 100
    o = torch.zeros(n, 3, device="cuda")
    d = torch.ones(n, 3, device="cuda")
    t = torch.empty(n, device="cuda")
    sh = torch.empty(n, device="cuda")
    host = np.zeros((n, 3), f32)

    def q(**kw):
        x = _lib.RayQuery()
        x.n_rays = n
        x.d_origin, x.d_dir = o.data_ptr(), d.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = functools.partial(util.bad, L.ctr_cast_rays, ds._h)

    assert L.ctr_cast_rays(ds._h, C.byref(q(d_t=t.data_ptr())), None) == 0
    bad(q(d_t=t.data_ptr(), d_origin=None), "null rays")
    bad(q(d_t=t.data_ptr(), flags=16), "unknown flag")
    bad(q(d_shadow=sh.data_ptr(), flags=5), "exclude each other")
    bad(q(d_shadow=sh.data_ptr(), d_t=t.data_ptr(), flags=4), "CTR_RAY_SHADOW")
    bad(q(flags=4), "CTR_RAY_SHADOW")
    bad(q(), "nearest-hit query")
    bad(q(d_t=t.data_ptr(), d_shadow=sh.data_ptr()), "nearest-hit query")
    bad(q(d_t=host.ctypes.data), "d_t is not device memory")
    bad(q(d_t=t.data_ptr(), d_origin=host.ctypes.data), "d_origin is not device memory")
    bad(q(d_t=t.data_ptr(), n_rays=1 << 31), "2^31")
    assert L.ctr_cast_rays(ds._h, C.byref(q(d_t=t.data_ptr(), n_rays=0)), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ds.cast_rays(o.double(), d)
    with pytest.raises(ValueError):
        ds.cast_rays(o[:, :2], d[:, :2])
    with pytest.raises(ValueError):
        ds.cast_rays(o, d[:10])
    with pytest.raises(ValueError):
        ds.cast_rays(o, d, outputs=("depth",))
    with pytest.raises(ValueError):
        ds.shadow(o, d, max_t=torch.ones(7, device="cuda"))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ds.cast_rays(o.to("cuda:1"), d)
    ds.close()


# ---- 10. renders are undisturbed ----
def test_renders_before_and_after_queries_are_identical(ca):
    s = load_scene(ca, "bunny", 128, 72)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=5)
    ca_ = ds.last_counters()
    rng = np.random.RandomState(10)
    o, d, mt = _random_rays(rng, 50000, rs, -3.0, 3.0)
    ds.cast_rays(o, d, min_t=mt)
    ds.shadow(o, d, max_t=2.0)
    ds.cast_rays(o, d, linear=True)
    b = ds.render(bounces=5)
    cb = ds.last_counters()
    for k in ("depth", "color", "normal"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["ray_count"] == b["ray_count"] and np.array_equal(ca_[:2], cb[:2])
    ds.close()
