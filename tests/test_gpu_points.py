"""Surface shading queries on the GPU (ctr_shade_points, DeviceScene.shade_points) against the reference's phong: the C
oracle where it covers the case (the primary hits of a camera's rays at bounces = 0), tests/points_ref.py (shade_ref.phong
and ray_ref.shadow_intensity driven by material indices, pinned against the oracle by tests/test_points_cpu.py) everywhere
else, and the radiance query of the same build for the composition with cast_rays.
"Bitwise": identical float bits, NaN positions equal.  "Within TOL": tests/util.TOL per channel; where a scene's light
colours sum to more than 1 the fast specular term is held to TOL * max(1, Lambda) (tests/util.light_scale: the colour is
linear in the light colours, the bar of tests/test_gpu_shading_ranges.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle
from tests import points_ref, ray_ref, shade_ref, util
from tests.conftest import load_scene
from tests.util import (LIGHT_CASES, SCALE_EXPONENTS, STACK_CASES, TOL, _random_scene, assert_bitwise as _bitwise, f32_bits as _bits,
                        fast_pow_kept, light_scale, lights_scene_json, max_diff as _max_diff, pow2, random_rays, scaled_scene_json,
                        stack_cameras, stack_scene_json, to_np as _np)

pytestmark = pytest.mark.gpu
f32 = np.float32
THREADS = os.cpu_count() or 4
BOTH = ("color", "light_shadow")
LENGTHS = (0.01, 1.0, 30.0)


def _scene(ca, which, w=32, h=32):
    s = load_scene(ca, which, w, h) if not which.startswith("random") else ca.HostScene.parse(_random_scene(int(which[6:]), w=w, h=h))
    assert s.ok
    return s


def _free_points(rng, n, sc):
    """n points uniform in [-3, 3]^3, the box these scenes live in (tests/util.random_rays draws its origins from it): not on
    surfaces; Gaussian normals and view directions of length about 0.01, 1 and 30; random valid materials"""
    p = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3)).astype(f32) * rng.choice(list(LENGTHS), (n, 1)).astype(f32)
    view = rng.normal(size=(n, 3)).astype(f32) * rng.choice(list(LENGTHS), (n, 1)).astype(f32)
    mat = rng.randint(0, len(sc.mat_specular), n).astype(np.int32)
    return p, nrm, view, mat


@functools.lru_cache(maxsize=None)
def _primary(name, w, h):
    """the camera's primary hits of a stock scene and the oracle's frame at bounces = 0, computed once"""
    import cutrace_amd as ca
    s = load_scene(ca, name, w, h)
    sc = shade_ref.ShadeScene(s)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=0, threads=THREADS, hit_ids=True)
    _, d, r, hit = points_ref.oracle_hits(sc, g)
    for v in (d, hit, g["color"], *r.values()):
        v.setflags(write=False)
    return s, sc, d, r, hit, g["color"].reshape(-1, 3)


# ---- 1. against the C oracle, bit for bit ----
@pytest.mark.parametrize("name", ["bunny", "mirror", "sphere_plane"])
def test_primary_hits_equal_the_oracle(ca, name):
    s, sc, d, r, hit, want = _primary(name, 96, 54)
    assert hit.sum() > 100, "no hit pixels: the test shows nothing"
    ds = ca.DeviceScene(s)
    args = (r["point"][hit], r["normal"][hit], d[hit])
    mat = sc.obj_mat[r["object"][hit]].astype(np.int32)
    for linear in (False, True):
        what = f"{name} linear={linear}"
        exact = _np(ds.shade_points(*args, materials=mat, exact_pow=True, linear=linear))
        _bitwise(exact["color"], want[hit], what + " exact_pow: color")
        fast = _np(ds.shade_points(*args, materials=mat, linear=linear))
        assert _max_diff(fast["color"], want[hit], what) <= TOL
    ds.close()


# ---- 2. composition: cast_rays, then shade_points, is shade_rays(bounces=0) ----
@pytest.mark.parametrize("which", ["bunny", "random1"])
def test_shade_points_after_cast_rays_is_shade_rays_without_bounces(ca, which):
    s = _scene(ca, which, 64, 36)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    for rays in ("camera", "random"):
        o, d = ray_ref.camera_rays(sc.cam) if rays == "camera" else random_rays(np.random.RandomState(12), 3000, sc, -3.0, 3.0)[:2]
        hit = ds.cast_rays(o, d, outputs=("object", "point", "normal"))
        n_hit = int((hit["object"] >= 0).sum())
        assert n_hit > 0 and (n_hit < len(o) or rays == "camera"), "hits are needed, and among the random rays misses"
        for exact in (False, True):
            got = _np(ds.shade_points(hit["point"], hit["normal"], d, objects=hit["object"], exact_pow=exact))
            want = _np(ds.shade_rays(o, d, bounces=0, exact_pow=exact))
            _bitwise(got["color"], want["color"], f"{which} {rays} rays exact_pow={exact}")
    ds.close()


# ---- 3. free points ----
@pytest.mark.parametrize("which", ["bunny", "random0", "random1", "random5"])
def test_free_points_against_points_ref(ca, which):
    s = _scene(ca, which)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    n = 3000
    p, nrm, view, mat = _free_points(np.random.RandomState(4), n, sc)
    want_c = points_ref.shade_points(sc, p, nrm, view, mat)
    want_ls = points_ref.light_shadow(sc, p)
    for exact in (False, True):
        what = f"{which} exact_pow={exact}"
        lin = _np(ds.shade_points(p, nrm, view, materials=mat, exact_pow=exact, linear=True, outputs=BOTH))
        assert lin["light_shadow"].shape == (n, len(sc.lights))
        assert _max_diff(lin["color"], want_c, what + " linear") <= TOL
        _bitwise(lin["light_shadow"], want_ls, what + " linear: light_shadow")
        dflt = _np(ds.shade_points(p, nrm, view, materials=mat, exact_pow=exact, outputs=BOTH))
        for k in BOTH:
            _bitwise(dflt[k], lin[k], f"{what}: default walk against linear, {k}")
    part = float(((want_ls > 0) & (want_ls < 1)).mean())
    print(f"{which}: {part:.3f} of the light_shadow entries strictly between 0 and 1, {float((want_ls == 1).mean()):.3f} exactly 1")
    # (random5 has transmitting objects too, but its only light is a sun behind its transmitting back wall: every shadow ray
    # that crosses the transmitting sphere goes on through the wall, 0.5 + 0.5 = 1, and the checker finds no partial entry)
    if which in ("random0", "random1"):
        assert any(sc.transparent(i) for i in range(len(sc.objects)))
        assert part >= 0.05, "hardly any partial shadow: the test shows nothing"
    if which == "bunny":
        assert (want_ls == 0).sum() > n // 10 and (want_ls == 1).sum() > n // 10
    ds.close()


# ---- 4. degenerate points inside an ordinary batch ----
@pytest.mark.parametrize("mode", ["materials", "objects"])
def test_degenerate_points_inside_an_ordinary_batch(ca, mode):
    s = _scene(ca, "bunny")
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    lamp = next(l["v"] for l in sc.lights if l["type"] == shade_ref.LIGHT_POINT)
    n = 500
    p, nrm, view, mat = _free_points(np.random.RandomState(6), n, sc)
    rng = np.random.RandomState(7)
    n_idx = len(sc.objects) if mode == "objects" else len(sc.mat_specular)
    idx = rng.randint(0, n_idx, n).astype(np.int32)
    # (row of the batch, what is wrong with it); the rows spread over several waves, two of them adjacent
    rows = {3: "zero normal", 70: "zero view", 130: "nan point", 131: "inf point", 200: "at the light", 321: "index one past the end",
            322: "index -2", 400: "index 2^31 - 1", 480: "object -1"}
    clean = np.array([k not in rows for k in range(n)])
    for k, what in rows.items():
        if what == "zero normal":
            nrm[k] = 0.0
        elif what == "zero view":
            view[k] = [0.0, -0.0, 0.0]
        elif what == "nan point":
            p[k, 1] = np.nan
        elif what == "inf point":
            p[k] = [np.inf, 1.0, -np.inf]
        elif what == "at the light":
            p[k] = lamp
        elif what.startswith("index"):
            idx[k] = {"index one past the end": n_idx, "index -2": -2, "index 2^31 - 1": 2 ** 31 - 1}[what]
        elif mode == "objects":
            idx[k] = -1
    kw = {mode: idx}
    got = _np(ds.shade_points(p, nrm, view, exact_pow=True, outputs=BOTH, **kw))   # (it returns: no lane spins)
    alone = _np(ds.shade_points(p[clean], nrm[clean], view[clean], exact_pow=True, outputs=BOTH, **{mode: idx[clean]}))
    for k in BOTH:
        _bitwise(got[k][clean], alone[k], f"{mode}: the ordinary points of the batch, {k}")
    _bitwise(got["light_shadow"], points_ref.light_shadow(sc, p), f"{mode}: light_shadow of every row")
    in_range = (idx >= 0) & (idx < n_idx)
    valid = np.where(in_range, idx, 0)
    want = points_ref.shade_points(sc, p, nrm, view, sc.obj_mat[valid] if mode == "objects" else valid)
    want[~in_range] = np.nan
    if mode == "objects":
        want[idx == -1] = 0.0
        assert (got["color"][480] == 0).all() and not np.signbit(got["color"][480]).any()
    for k in (321, 322, 400):
        assert np.isnan(got["color"][k]).all(), rows[k]
    assert _max_diff(got["color"], want, f"{mode}: every row against points_ref") <= TOL
    ds.close()


# ---- 5. lights ----
@functools.lru_cache(maxsize=None)
def _floor_points(seed, n, x=(-2.0, 2.0), y=(-0.99, 1.5), z=(-2.0, 3.0)):
    rng = np.random.RandomState(seed)
    p = rng.uniform([x[0], y[0], z[0]], [x[1], y[1], z[1]], (n, 3)).astype(f32)
    p[: n // 3, 1] = y[0]   # a third of them just above the floor
    nrm = rng.normal(size=(n, 3)).astype(f32)
    nrm[: n // 3] = [0.0, 1.0, 0.0]
    view = rng.normal(size=(n, 3)).astype(f32)
    return p, nrm, view


@pytest.mark.parametrize("name", ["n0", "n1", "n8", "n33", "colours", "point_inside_the_glass_sphere", "ambient_2.5"])
def test_lights(ca, tmp_path, name):
    s = ca.HostScene.parse(lights_scene_json(tmp_path, name))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    n = 600
    p, nrm, view = _floor_points(8, n)
    mat = np.random.RandomState(9).randint(0, 3, n).astype(np.int32)
    n_lights = len(LIGHT_CASES[name]["lights"])
    assert len(sc.lights) == n_lights == ds.n_lights
    exact = _np(ds.shade_points(p, nrm, view, materials=mat, exact_pow=True, outputs=BOTH))
    dflt = _np(ds.shade_points(p, nrm, view, materials=mat, outputs=BOTH))
    assert exact["light_shadow"].shape == dflt["light_shadow"].shape == (n, n_lights)
    if n_lights == 0:
        amb = (sc.mat_color[mat] * sc.ambient).astype(f32)   # phong's `final` before the first light
        _bitwise(exact["color"], amb, "no lights: ambient * diffuse")
        _bitwise(dflt["color"], amb, "no lights: ambient * diffuse")
        only = ds.shade_points(p, outputs=("light_shadow",))
        assert list(only) == ["light_shadow"] and tuple(only["light_shadow"].shape) == (n, 0)
    else:
        want_ls = points_ref.light_shadow(sc, p)
        _bitwise(exact["light_shadow"], want_ls, f"{name}: light_shadow")
        _bitwise(dflt["light_shadow"], want_ls, f"{name}: light_shadow")
        want = points_ref.shade_points(sc, p, nrm, view, mat)
        assert _max_diff(exact["color"], want, f"{name} exact_pow") <= TOL
        if fast_pow_kept(s):
            assert _max_diff(dflt["color"], want, name) <= TOL * max(1.0, light_scale(s))
    if name == "colours":
        assert not fast_pow_kept(s), "this scene is meant to leave the fast specular term's domain"
    if not fast_pow_kept(s):   # the launch takes the exact term by itself
        _bitwise(dflt["color"], exact["color"], f"{name}: the default call outside the fast term's domain")
    ds.close()


# ---- 6. transparent stacks ----
@pytest.mark.parametrize("name", list(STACK_CASES))
def test_transparent_stacks(ca, tmp_path, name):
    text, _ = stack_scene_json(tmp_path, name, stack_cameras(name)[0])
    s = ca.HostScene.parse(text)
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    # just above the floor, under every step of the staircase (sheet j of n begins at x = -1.5 + 3 j / n) and beside it
    n = 400
    rng = np.random.RandomState(13)
    p = rng.uniform([-2.5, 1e-4, -1.5], [2.5, 1e-4, 1.5], (n, 3)).astype(f32)
    want = points_ref.light_shadow(sc, p)
    for linear in (False, True):
        got = _np(ds.shade_points(p, linear=linear, outputs=("light_shadow",)))
        _bitwise(got["light_shadow"], want, f"{name} linear={linear}: light_shadow")
    print(f"{name}: light_shadow values {np.unique(want)[:12]}")
    if name in ("0.75x4", "0.5x2", "0.7x4"):   # the partial sums land on 1 (the first two) or pass it
        assert (want == 1).any() and ((want > 0) & (want < 1)).any()
    if name == "1.0x5":                         # they never reach it
        assert want.max() < 1
    ds.close()


# ---- 7. scene scale ----
@pytest.mark.parametrize("k", [SCALE_EXPONENTS[0], 0, SCALE_EXPONENTS[-1]])
def test_scene_scale(ca, tmp_path, k):
    """Points on the surfaces of the scene scaled by 2^k.  The shadow loop starts at the fixed 1e-3 whatever the scale: at
    2^-20 it starts beyond the whole scene and nothing shadows anything — kernel and checker must agree on that too."""
    assert SCALE_EXPONENTS[0] < 0 < SCALE_EXPONENTS[-1] and 0 in SCALE_EXPONENTS
    s = ca.HostScene.parse(scaled_scene_json(tmp_path, k))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(sc.cam)
    r = ray_ref.ray_cast(sc, o, d, f32(1e-3) * pow2(k))   # (a min_t of the scene's size: these casts only place the points)
    hit = r["object"] >= 0
    assert len(set(r["object"][hit])) == len(sc.objects), "every kind of surface carries points"
    p, nrm, view = r["point"][hit], r["normal"][hit], d[hit]
    mat = sc.obj_mat[r["object"][hit]].astype(np.int32)
    want = points_ref.shade_points(sc, p, nrm, view, mat)
    want_ls = points_ref.light_shadow(sc, p)
    print(f"scale 2^{k}: {int(hit.sum())} points, light_shadow mean {float(want_ls.mean()):.3f}, {int(np.isnan(want).sum())} NaNs")
    assert fast_pow_kept(s)
    for linear in (False, True):
        what = f"scale 2^{k} linear={linear}"
        exact = _np(ds.shade_points(p, nrm, view, materials=mat, exact_pow=True, linear=linear, outputs=BOTH))
        _bitwise(exact["light_shadow"], want_ls, what + ": light_shadow")
        assert _max_diff(exact["color"], want, what + " exact_pow") <= TOL
        fast = _np(ds.shade_points(p, nrm, view, materials=mat, linear=linear, outputs=BOTH))
        _bitwise(fast["light_shadow"], want_ls, what + ": light_shadow")
        assert _max_diff(fast["color"], want, what) <= TOL * max(1.0, light_scale(s))
    if k == 0:
        assert ((want_ls > 0) & (want_ls < 1)).any() and (want_ls == 1).any() and (want_ls == 0).any()
    ds.close()


# ---- 8. plumbing ----
def test_prefix_subsets_scalar_material_ambient_stream_and_graph(ca):
    import torch
    s = _scene(ca, "sphere_plane", 32, 18)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    n = 999
    p, nrm, view, mat = _free_points(np.random.RandomState(9), n, sc)
    full = _np(ds.shade_points(p, nrm, view, materials=mat, outputs=BOTH))
    assert list(ds.shade_points(p, nrm, view, materials=mat)) == ["color"]
    # the first m results of the batch are the results of a batch of m (across the wave and the workgroup size)
    for m in (0, 1, 63, 65, 257):
        part = _np(ds.shade_points(p[:m], nrm[:m], view[:m], materials=mat[:m], outputs=BOTH))
        assert part["color"].shape == (m, 3) and part["light_shadow"].shape == (m, ds.n_lights)
        for k in BOTH:
            assert np.array_equal(_bits(part[k]), _bits(full[k][:m])), (m, k)
    # light_shadow alone needs the points only
    only = _np(ds.shade_points(p, outputs=("light_shadow",)))
    assert list(only) == ["light_shadow"] and np.array_equal(_bits(only["light_shadow"]), _bits(full["light_shadow"]))
    # a scalar material against the same value as a tensor
    one = _np(ds.shade_points(p, nrm, view, materials=1))
    _bitwise(one["color"], _np(ds.shade_points(p, nrm, view, materials=np.full(n, 1, np.int32)))["color"], "scalar material")
    assert not np.array_equal(one["color"], full["color"])
    # ambient: None is the scene camera's; another value changes the colours
    amb = float(s.desc.contents.cam.ambient)
    _bitwise(_np(ds.shade_points(p, nrm, view, materials=mat, ambient=amb))["color"], full["color"], "ambient given explicitly")
    assert not np.array_equal(_np(ds.shade_points(p, nrm, view, materials=mat, ambient=amb + 0.25))["color"], full["color"])
    # a non-default stream
    dev = [torch.from_numpy(x).cuda() for x in (p, nrm, view, mat)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = ds.shade_points(dev[0], dev[1], dev[2], materials=dev[3], outputs=BOTH, stream=side)
    side.synchronize()
    for k in BOTH:
        assert np.array_equal(_bits(on_side[k].cpu().numpy()), _bits(full[k])), k
    torch.cuda.current_stream().wait_stream(side)
    # a single-branch graph capture, replayed once
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ds.shade_points(dev[0], dev[1], dev[2], materials=dev[3], outputs=BOTH)
    graph.replay()
    torch.cuda.synchronize()
    for k in BOTH:
        assert np.array_equal(_bits(cap[k].cpu().numpy()), _bits(full[k])), k
    ds.close()


# ---- 9. bad arguments through the C-ABI on a live scene ----
def test_bad_arguments(ca):
    import torch
    from cutrace_amd import _lib
    L = _lib.hip_lib()
    s = _scene(ca, "sphere_plane", 32, 18)
    ds = ca.DeviceScene(s)
    n_mat = int(s.desc.contents.n_materials)
    n = 100
    p = torch.zeros(n, 3, device="cuda")
    v = torch.ones(n, 3, device="cuda")
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    col = torch.empty(n, 3, device="cuda")
    ls = torch.empty(n, max(ds.n_lights, 1), device="cuda")
    host = np.zeros((n, 3), f32)

    def q(**kw):
        x = _lib.PointQuery()
        x.n_points = n
        x.d_point, x.d_normal, x.d_view, x.d_color, x.d_light_shadow = p.data_ptr(), v.data_ptr(), v.data_ptr(), col.data_ptr(), ls.data_ptr()
        for k, val in kw.items():
            setattr(x, k, val)
        return x

    bad = functools.partial(util.bad, L.ctr_shade_points, ds._h)

    assert L.ctr_shade_points(ds._h, C.byref(q()), None) == 0
    assert L.ctr_shade_points(ds._h, C.byref(q(flags=3, d_material=idx.data_ptr())), None) == 0
    assert L.ctr_shade_points(ds._h, C.byref(q(d_object=idx.data_ptr(), d_light_shadow=None)), None) == 0
    assert L.ctr_shade_points(ds._h, C.byref(q(d_color=None, d_normal=None, d_view=None, material=-5)), None) == 0   # the scalar is not in use
    assert L.ctr_shade_points(ds._h, C.byref(q(n_points=0, d_point=None)), None) == 0
    assert L.ctr_shade_points(ds._h, C.byref(q(material=n_mat, d_material=idx.data_ptr())), None) == 0                # nor here
    bad(q(d_point=None), "null d_point")
    bad(q(flags=4), "unknown flag")
    bad(q(d_color=None, d_light_shadow=None), "no output")
    bad(q(d_normal=None), "d_color needs d_normal and d_view")
    bad(q(d_view=None), "d_color needs d_normal and d_view")
    bad(q(d_material=idx.data_ptr(), d_object=idx.data_ptr()), "exclude each other")
    bad(q(material=n_mat), f"material {n_mat} outside")
    bad(q(material=-1), "material -1 outside")
    bad(q(n_points=1 << 31), "2^31")
    for slot in ("d_point", "d_normal", "d_view", "d_material", "d_object", "d_color", "d_light_shadow"):
        bad(q(**{slot: host.ctypes.data}), f"{slot} is not device memory")
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ds.shade_points(p.double(), v, v, materials=0)
    with pytest.raises(ValueError):
        ds.shade_points(p, v[:10], v, materials=0)
    with pytest.raises(ValueError):
        ds.shade_points(p, v, v, materials=idx, objects=idx)
    with pytest.raises(ValueError):
        ds.shade_points(p, v, v)
    with pytest.raises(ValueError):
        ds.shade_points(p, v, v, materials=0, outputs=("t",))
    with pytest.raises(RuntimeError):
        ds.shade_points(p, v, v, materials=n_mat)
    ds.close()


# ---- 10. renders are undisturbed ----
def test_renders_before_and_after_a_batch_of_points_are_identical(ca):
    s = load_scene(ca, "bunny", 128, 72)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=5)
    ca_ = ds.last_counters()
    p, nrm, view, mat = _free_points(np.random.RandomState(10), 50000, sc)
    ds.shade_points(p, nrm, view, materials=mat)
    ds.shade_points(p, nrm, view, materials=mat, linear=True, exact_pow=True, outputs=BOTH)
    b = ds.render(bounces=5)
    cb = ds.last_counters()
    for k in ("depth", "color", "normal"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["ray_count"] == b["ray_count"] and np.array_equal(ca_[:2], cb[:2])
    ds.close()
