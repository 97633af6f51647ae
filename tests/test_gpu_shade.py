"""Radiance queries on the GPU (ctr_shade_rays, DeviceScene.shade_rays) against the reference's ray_color: the C oracle
where it covers the case (camera rays), tests/shade_ref.py (its NumPy restatement, pinned against the oracle by
tests/test_shade_cpu.py) everywhere else, and the render kernel of the same build beyond the oracle's depth.
"Bitwise": identical float bits, NaN positions equal.  "Within TOL": tests/util.TOL per channel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle
from tests import ray_ref, shade_ref, util
from tests.conftest import load_scene
from tests.util import (TOL, assert_bitwise as _bitwise, f32_bits as _bits, first_hit_same as _first_hit_same,
                        max_diff as _max_diff, random_rays, to_np as _np)

pytestmark = pytest.mark.gpu
f32 = np.float32
THREADS = os.cpu_count() or 4
FIRST = ("t", "object", "normal")
ALL = ("color",) + FIRST


# ---- 5. camera rays in image order ----
@pytest.mark.parametrize("name,bounces", [("bunny", 0), ("bunny", 5), ("mirror", 0), ("mirror", 5), ("mirror", 8),
                                          ("sphere_plane", 0), ("sphere_plane", 5)])
def test_camera_rays_equal_the_oracle(ca, name, bounces):
    s = load_scene(ca, name, 96, 54)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(rs.cam)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=bounces, threads=THREADS, hit_ids=True)
    want = dict(t=g["depth"].reshape(-1), normal=g["normal"].reshape(-1, 3), object=g["hit_id"].reshape(-1))
    assert (want["object"] >= 0).any()
    for linear in (False, True):
        what = f"{name} bounces {bounces} linear={linear}"
        exact = _np(ds.shade_rays(o, d, bounces=bounces, min_t=1e-3, exact_pow=True, linear=linear, outputs=ALL))
        _bitwise(exact["color"], g["color"], what + " exact_pow: color")
        _first_hit_same(exact, want, what + " exact_pow")
        fast = _np(ds.shade_rays(o, d, bounces=bounces, min_t=1e-3, linear=linear, outputs=ALL))
        assert _max_diff(fast["color"], g["color"], what) <= TOL
        _first_hit_same(fast, want, what)
    ds.close()


# ---- 6. an incoherent batch: many cameras, permuted ----
@pytest.mark.parametrize("name", ["bunny", "sphere_plane"])
def test_incoherent_batch_of_many_cameras(ca, name):
    from cutrace_amd import _lib
    w, h = 48, 32
    s = load_scene(ca, name, w, h)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(11)
    desc = s.desc.contents
    keep = _lib.Camera()
    C.memmove(C.byref(keep), C.byref(desc.cam), C.sizeof(_lib.Camera))
    origins, dirs, want, cams = [], [], [], []
    for _ in range(6):
        cam = _lib.Camera()
        C.memmove(C.byref(cam), C.byref(keep), C.sizeof(_lib.Camera))
        eye = _lib.Vec3(*[float(x) for x in rng.uniform([-2.5, -0.5, 1.0], [2.5, 2.0, 5.0])])
        look = _lib.Vec3(*[float(x) for x in rng.uniform(-0.4, 0.4, 3)])
        _lib.host_lib().ctr_camera_look_at(C.byref(cam), eye, _lib.Vec3(0.0, 1.0, 0.0), look)
        cams.append(cam)
        desc.cam = cam
        o, d = ray_ref.camera_rays(ray_ref.RefScene(s).cam)
        g = oracle.oracle_render(s, fudge=1e-3, bounces=5, threads=THREADS, hit_ids=True)
        origins.append(o)
        dirs.append(d)
        want.append(dict(color=g["color"].reshape(-1, 3), t=g["depth"].reshape(-1), normal=g["normal"].reshape(-1, 3),
                         object=g["hit_id"].reshape(-1)))
    desc.cam = keep
    ds.set_cameras(cams)  # the guards now cover the six eyes and their mirror images
    o, d = np.concatenate(origins), np.concatenate(dirs)
    perm = rng.permutation(len(o))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    for exact in (True, False):
        got = _np(ds.shade_rays(o[perm], d[perm], bounces=5, min_t=1e-3, exact_pow=exact, outputs=ALL))
        ordered = _np(ds.shade_rays(o, d, bounces=5, min_t=1e-3, exact_pow=exact, outputs=ALL))
        for k in ALL:
            if k == "object":
                assert np.array_equal(ordered[k][perm], got[k]), k
            else:
                _bitwise(got[k], ordered[k][perm], f"{name} exact_pow={exact}: permuted against ordered, {k}")
        for c in range(6):
            sl = inv[c * w * h:(c + 1) * w * h]
            part = {k: v[sl] for k, v in got.items()}
            _first_hit_same(part, want[c], f"{name} camera {c}")
            if exact:
                _bitwise(part["color"], want[c]["color"], f"{name} camera {c}: color")
            else:
                assert _max_diff(part["color"], want[c]["color"], f"{name} camera {c}") <= TOL
    ds.close()


# ---- 7. random rays against shade_ref ----
@pytest.mark.parametrize("which", ["bunny", "random0", "random1", "random5"])
def test_random_rays_against_shade_ref(ca, which):
    from tests.util import _random_scene
    s = load_scene(ca, "bunny", 32, 32) if which == "bunny" else ca.HostScene.parse(_random_scene(int(which[6:]), w=32, h=32))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(3)
    n = 4000 if which == "bunny" else 3000
    bounces = 3
    o, d, _ = random_rays(rng, n, sc, -3.0, 3.0)
    want = shade_ref.ray_color(sc, o, d, min_t=1e-3, bounces=bounces)
    assert int((want["object"] >= 0).sum()) > n // 10
    for exact in (False, True):
        what = f"{which} exact_pow={exact}"
        lin = _np(ds.shade_rays(o, d, bounces=bounces, min_t=1e-3, exact_pow=exact, linear=True, outputs=ALL))
        _first_hit_same(lin, want, what + " linear")
        assert _max_diff(lin["color"], want["color"], what + " linear") <= TOL
        dflt = _np(ds.shade_rays(o, d, bounces=bounces, min_t=1e-3, exact_pow=exact, outputs=ALL))
        assert np.array_equal(dflt["object"], lin["object"]), what
        for k in ("color", "t", "normal"):
            _bitwise(dflt[k], lin[k], f"{what}: default walk against linear, {k}")
    ds.close()


# ---- 8. deep recursion ----
def _hall_of_mirrors(ca, w, h):
    """two facing mirror walls, a floor, and a sphere that both reflects and transmits: every level to bounces 15 is live"""
    from tests.util import hall_of_mirrors_json
    s = ca.HostScene.parse(hall_of_mirrors_json(w, h))
    assert s.ok
    return s


@pytest.mark.parametrize("name", ["mirror", "hall"])
def test_bounces_15_equal_the_render_of_the_same_build(ca, name):
    import torch
    w, h = 64, 36
    s = load_scene(ca, "mirror", w, h) if name == "mirror" else _hall_of_mirrors(ca, w, h)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    ds.set_variant(ca.VAR_EXACT_POW)
    depth = torch.empty(h * w, device="cuda")
    color = torch.empty(h * w * 3, device="cuda")
    normal = torch.empty(h * w * 3, device="cuda")
    deep = {}
    for b in (15, 11):
        ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
                         fudge=1e-3, bounces=b)
        torch.cuda.synchronize()
        o, d = ray_ref.camera_rays(rs.cam)
        got = _np(ds.shade_rays(o, d, bounces=b, min_t=1e-3, exact_pow=True, outputs=ALL))
        _bitwise(got["color"], color.cpu().numpy(), f"{name} bounces {b}: color against the render")
        _bitwise(got["t"], depth.cpu().numpy(), f"{name} bounces {b}: t against the render's depth")
        _bitwise(got["normal"], normal.cpu().numpy(), f"{name} bounces {b}: normal")
        deep[b] = got["color"]
    if name == "hall":
        assert not np.array_equal(deep[15], deep[11]), "the hall does not recurse below depth 11: the test shows nothing"
    ds.close()


def test_bounces_8_with_reflecting_and_transmitting_material_equal_the_oracle(ca):
    s = load_scene(ca, "sphere_plane", 48, 27)
    sc = shade_ref.ShadeScene(s)
    both = (sc.mat_reflexivity.astype(np.float64) >= 1e-6) & (sc.transparency.astype(np.float64) >= 1e-6)
    assert both.any(), "sphere_plane has no material that both reflects and transmits"
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(sc.cam)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=8, threads=THREADS, hit_ids=True)
    for linear in (False, True):
        got = _np(ds.shade_rays(o, d, bounces=8, min_t=1e-3, exact_pow=True, linear=linear, outputs=ALL))
        _bitwise(got["color"], g["color"], f"sphere_plane bounces 8 linear={linear}: color")
        _first_hit_same(got, dict(t=g["depth"].reshape(-1), normal=g["normal"].reshape(-1, 3), object=g["hit_id"].reshape(-1)),
                        "sphere_plane bounces 8")
    ds.close()


# ---- 9. plumbing ----
def test_streams_graph_capture_sizes_and_output_subsets(ca):
    import torch
    s = load_scene(ca, "sphere_plane", 32, 18)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(9)
    o, d, _ = random_rays(rng, 1000, sc, -3.0, 3.0)
    full = _np(ds.shade_rays(o, d, outputs=ALL))
    assert list(ds.shade_rays(o, d)) == ["color"]
    empty = ds.shade_rays(o[:0], d[:0], outputs=ALL)
    assert set(empty) == set(ALL) and all(v.shape[0] == 0 for v in empty.values())
    for m in (1, 63, 65, 999):
        part = _np(ds.shade_rays(o[:m], d[:m], outputs=ALL))
        for k in ALL:
            assert np.array_equal(part[k].view(np.uint32), full[k][:m].view(np.uint32)), (m, k)
    sub = _np(ds.shade_rays(o, d, outputs=("normal",)))
    assert list(sub) == ["color", "normal"] and np.array_equal(_bits(sub["normal"]), _bits(full["normal"]))
    # ambient: None is the scene camera's; another value changes lit pixels
    amb = float(s.desc.contents.cam.ambient)
    _bitwise(_np(ds.shade_rays(o, d, ambient=amb))["color"], full["color"], "ambient given explicitly")
    assert not np.array_equal(_np(ds.shade_rays(o, d, ambient=amb + 0.25))["color"], full["color"])
    # a non-default stream
    od, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = ds.shade_rays(od, dd, outputs=ALL, stream=side)
    side.synchronize()
    for k in ALL:
        assert np.array_equal(on_side[k].cpu().numpy().view(np.uint32), full[k].view(np.uint32)), k
    torch.cuda.current_stream().wait_stream(side)
    # a single-branch graph capture, replayed once
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ds.shade_rays(od, dd, outputs=ALL)
    graph.replay()
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(cap[k].cpu().numpy().view(np.uint32), full[k].view(np.uint32)), k
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
    col = torch.empty(n, 3, device="cuda")
    host = np.zeros((n, 3), f32)

    def q(**kw):
        x = _lib.ShadeQuery()
        x.n_rays = n
        x.bounces = 5
        x.min_t = 1e-3
        x.d_origin, x.d_dir, x.d_color = o.data_ptr(), d.data_ptr(), col.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = functools.partial(util.bad, L.ctr_shade_rays, ds._h)

    assert L.ctr_shade_rays(ds._h, C.byref(q()), None) == 0
    bad(q(d_origin=None), "null rays")
    bad(q(d_dir=None), "null rays")
    bad(q(flags=4), "unknown flag")
    bad(q(bounces=-1), "bounces -1")
    bad(q(bounces=16), "bounces 16")
    bad(q(d_color=None), "d_color")
    bad(q(d_color=host.ctypes.data), "d_color is not device memory")
    bad(q(d_origin=host.ctypes.data), "d_origin is not device memory")
    bad(q(d_normal=host.ctypes.data), "d_normal is not device memory")
    bad(q(n_rays=1 << 31), "2^31")
    assert L.ctr_shade_rays(ds._h, C.byref(q(n_rays=0)), None) == 0
    assert L.ctr_shade_rays(ds._h, C.byref(q(bounces=15, flags=3)), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ds.shade_rays(o.double(), d)
    with pytest.raises(ValueError):
        ds.shade_rays(o, d[:10])
    with pytest.raises(ValueError):
        ds.shade_rays(o, d, outputs=("depth",))
    with pytest.raises(ValueError):
        ds.shade_rays(o, d, bounces=16)
    ds.close()


def test_renders_before_and_after_a_radiance_query_are_identical(ca):
    s = load_scene(ca, "bunny", 128, 72)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=5)
    ca_ = ds.last_counters()
    rng = np.random.RandomState(10)
    o, d, _ = random_rays(rng, 50000, sc, -3.0, 3.0)
    ds.shade_rays(o, d, bounces=5)
    ds.shade_rays(o, d, bounces=2, linear=True, exact_pow=True, outputs=ALL)
    b = ds.render(bounces=5)
    cb = ds.last_counters()
    for k in ("depth", "color", "normal"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["ray_count"] == b["ray_count"] and np.array_equal(ca_[:2], cb[:2])
    ds.close()
