"""The shading state machines across material, light and phong-exponent ranges (-m gpu): the shadow loop through
transparent occluders, the specular term, the >= 1e-6 bounce thresholds and the per-light loop, which exist twice — in the
render kernel (render_kernel.hip, ACT_LIGHT / ACT_BOUNCE / ACT_UNWIND) and in ray_shade.hip — on the cases of tests/util.py
"the shading-parameter sweeps": stacks of up to twelve transparent occluders whose 1 - transparency sums land on, pass or
never reach 1 (transparencies of 1, 1.5 and 1e-7 included, two sheets closer than the loop's restart step, a point light
between sheets); reflect and transparency around the double 1e-6 and outside [0, 1]; phong exponents from 0 to 100 000 on
rays constructed to sit inside the highlight; up to 33 lights, colours of 0, 64 and below 0, suns of length 2^-10 and 2^10,
point lights far away, next to a surface, inside a sphere and behind a wall; ambient factors of 0, 1, 2.5 and -0.25.

Every frame case goes through every entry point that shades: the plain render (default build; exact pow; exact with the
reference's walk; exact without any-hit), the supersampled frame, the lens render on the camera's own rays, the radiance
query with both walks, exact and fast; where they apply render_uv, the IGNORE_TRANSPARENT variant, and on the stacks the
cast query with ignore_transparent and the shadow query.

The checker is the CPU oracle; tests/test_shading_ranges_cpu.py pins tests/shade_ref.py and the reference's own headers
to it on every case and proves the builders' claims.  Bar: depth, normal and ray count equal the oracle's bit for bit;
the exact-pow colour equals oracle_render(pow_rounded_once=True) bit for bit and the plain oracle within TOL * max(1, Lambda),
Lambda the sum over the lights of the largest |colour channel| (the colour is linear in the light colours); the lens render
equals the render of the same build bit for bit, the exact radiance query the exact render.  The fast specular path
(exp2(e * log2(x)) on a half vector normalised with v_rsq_f32) is held to TOL * max(1, Lambda) where the launch keeps it:
the build chooser drops it where phong * specular * colour * Lambda says it would leave the bar (kernel_choice.h
fast_pow_ok; measured per exponent on the constructed rays, profiles/shading_ranges/fastpow.txt)."""
import os

import numpy as np
import pytest

import oracle
from cutrace_amd import lenses
from tests import aa_ref, ray_ref, shade_ref
from tests.gpu_support import expected_kernel, gpu  # noqa: F401  (gpu: the fixture)
from tests.util import (PHONG_EXPONENTS, PHONG_LIGHTS, PHONG_RAYS_H, PHONG_RAYS_W, SHADING_FRAME_CASES, STACK_CASES, STACK_FLOOR,
                        TOL, assert_same, f32, fast_pow_kept, light_scale, parse, phong_rays, phong_scene_json, ref_dict, shading_case_id, shading_case_json,
                        stack_cameras, stack_scene_json, to_np, uv_close)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = min(os.cpu_count() or 4, 16)
KV_ANYHIT, KV_FASTPOW, KV_HOSTOUT, KV_UV, KV_IGNTR, KV_SS, KV_RAYS = 2, 32, 128, 256, 1024, 2048, 4096
FRAME = ("depth", "normal", "color")
FRAME_CASES = [pytest.param(c, id=shading_case_id(c)) for c in SHADING_FRAME_CASES]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kernel_choice.npz"))["choice"].reshape(6, 512, 8, 2, 4)


def same_bits_nan(a, b):
    """identical float bits; NaNs by position and sign, not payload"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32).reshape(np.shape(a))
    na, nb = np.isnan(a), np.isnan(b)
    return (np.array_equal(na, nb) and np.array_equal(np.signbit(a[na]), np.signbit(b[nb])) and
            np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def max_diff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    d = np.abs(a - b)
    return float(np.where(np.isnan(d), np.inf, d).max()) if d.size else 0.0


def assert_bits(got, want, what, keys=FRAME):
    for k in keys:
        assert same_bits_nan(got[k], want[k]), f"{what}: {k} differs in {int((np.asarray(got[k]) != np.asarray(want[k]).reshape(np.shape(got[k]))).sum())} values, by up to {max_diff(got[k], want[k]):.3e}"


def assert_frame(got, want, tol, what):
    """depth and normal bit for bit, colour within tol"""
    assert_bits(got, want, what, ("depth", "normal"))
    d = max_diff(got["color"], want["color"])
    print(f"{what}: colour max|diff| {d:.3e} (bar {tol:.3e})")
    assert d <= tol, f"{what}: colour max|diff| {d:.3e} above {tol:.3e}"


def as_numpy(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def frozen(o):
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


# ---- every frame case through every entry point that shades ----
@pytest.mark.parametrize("case", FRAME_CASES)
def test_frame_case(gpu, golden, tmp_path, case):
    what = shading_case_id(case)
    family = case[0]
    text, bounces = shading_case_json(tmp_path, case)
    s = parse(gpu, text)
    w, h = s.size
    tol = TOL * max(1.0, light_scale(s))
    kw = dict(fudge=1e-3, bounces=bounces)
    want = frozen(oracle.oracle_render(s, threads=NT, **kw))
    once = frozen(oracle.oracle_render(s, threads=NT, pow_rounded_once=True, **kw))
    for k in FRAME:
        assert not np.isnan(want[k]).any(), k
    assert max_diff(once["color"], want["color"]) <= tol
    d = s.desc.contents
    all_opaque = all(d.materials[i].transparency == 0.0 for i in range(d.n_materials))
    ds = gpu.DeviceScene(s)
    exact = gpu.VAR_EXACT_POW

    # a. the plain render: the default build ...
    r = ds.render(**kw)
    kv_default = ds.last_kernel()
    print(f"{what}: kernel {kv_default:#x}, {r['ray_count']} casts, Lambda {light_scale(s):.3f}")
    # (outside the fast specular path's domain the launch is the one VAR_EXACT_POW gets: test_gpu_kernel_choice._expected)
    assert kv_default == expected_kernel(gpu, golden, s, 0, "render", bounces) and bool(kv_default & KV_FASTPOW) == fast_pow_kept(s), hex(kv_default)
    assert bool(kv_default & KV_ANYHIT) == all_opaque, "any-hit only when every transparency is exactly +-0"
    assert_frame(r, want, tol, f"{what}, default build")
    assert r["ray_count"] == want["ray_count"], what
    # ... and exact pow: with the shipped walk, the reference's walk, and without any-hit
    for name, var in (("exact pow", exact), ("the reference's walk", exact | gpu.VAR_NO_PREFILTER | gpu.VAR_NO_CLUSTER), ("no any-hit", exact | gpu.VAR_NO_ANYHIT)):
        ds.set_variant(var)
        e = ds.render(**kw)
        assert ds.last_kernel() == expected_kernel(gpu, golden, s, var, "render", bounces), (what, name, hex(ds.last_kernel()))
        assert_bits(e, once, f"{what}, {name}, against the oracle with the pow rounded once")
        assert_frame(e, want, tol, f"{what}, {name}")
        assert e["ray_count"] == want["ray_count"], (what, name)
    exact_frame = e

    # b. the supersampled frame
    s.set_size(2 * w, 2 * h)
    big = oracle.oracle_render(s, threads=NT, **kw)
    big_once = oracle.oracle_render(s, threads=NT, pow_rounded_once=True, **kw)
    s.set_size(w, h)
    ds.set_variant(gpu.VAR_AUTO)
    r2 = ds.render(samples=2, **kw)
    assert ds.last_kernel() & KV_SS
    assert_frame(r2, aa_ref.reduce_frame(big, 2), tol, f"{what}, samples=2")
    assert r2["ray_count"] == big["ray_count"], what
    ds.set_variant(exact)
    e2 = ds.render(samples=2, **kw)
    assert_bits(e2, aa_ref.reduce_frame(big_once, 2), f"{what}, samples=2, exact pow")
    assert_frame(e2, aa_ref.reduce_frame(big, 2), tol, f"{what}, samples=2, exact pow")

    # c. the lens render on the camera's own rays: the render of the same build, bit for bit
    o, dirs = lenses.pinhole(d.cam, w, h)
    for var in (gpu.VAR_AUTO, exact):
        ds.set_variant(var)
        plain = ds.render(**kw)
        kv_plain = ds.last_kernel() & ~KV_HOSTOUT
        got = as_numpy(ds.render_lens(o, dirs, **kw))
        assert ds.last_kernel() == kv_plain | KV_RAYS, (hex(ds.last_kernel()), hex(kv_plain))
        assert_bits(got, plain, f"{what}, lens render on pinhole rays, var={var}")
        assert got["ray_count"] == plain["ray_count"] and got["max_depth"] == plain["max_depth"], (what, var)

    # d. the radiance query on the camera's rays, both walks: exact = the exact render bit for bit; fast within the bar
    sc = shade_ref.ShadeScene(s)
    co, cd = ray_ref.camera_rays(sc.cam)
    first = dict(t=want["depth"].reshape(-1), normal=want["normal"].reshape(-1, 3))
    for linear in (False, True):
        for ex in (True, False):
            q = to_np(ds.shade_rays(co, cd, bounces=bounces, min_t=1e-3, exact_pow=ex, linear=linear, outputs=("color", "t", "object", "normal")))
            name = f"{what}, radiance query linear={linear} exact={ex}"
            assert np.array_equal(q["object"], want["hit_id"].reshape(-1).astype(np.int32)), name
            assert same_bits_nan(q["t"], first["t"]) and same_bits_nan(q["normal"], first["normal"]), name
            if ex:
                assert same_bits_nan(q["color"], exact_frame["color"]), f"{name}: colour differs from the exact render's by up to {max_diff(q['color'], exact_frame['color']):.3e}"
                assert same_bits_nan(q["color"], once["color"]), name
            elif fast_pow_kept(s):
                dq = max_diff(q["color"], want["color"])
                print(f"{name}: colour max|diff| {dq:.3e} (bar {tol:.3e})")
                assert dq <= tol, name
            else:   # outside the fast path's domain the launch takes the exact one
                assert same_bits_nan(q["color"], once["color"]), f"{name}: the fast path ran outside its domain"

    # e. texture coordinates, and the primary cast that ignores transparent objects
    if family in ("stack", "lights"):
        ds.set_variant(gpu.VAR_AUTO)
        wuv = oracle.oracle_render(s, threads=NT, uv=True, **kw)
        ruv = ds.render_uv(**kw)
        assert ds.last_kernel() & KV_UV
        uv_close(ruv["uv"], wuv["uv"])
        assert_frame(ruv, wuv, tol, f"{what}, render_uv")
        assert ruv["ray_count"] == wuv["ray_count"]
    if family in ("stack", "threshold"):
        wig = oracle.oracle_render(s, threads=NT, uv=True, ignore_transparent_primary=True, **kw)
        wig_once = oracle.oracle_render(s, threads=NT, uv=True, ignore_transparent_primary=True, pow_rounded_once=True, **kw)
        for var in (gpu.VAR_IGNORE_TRANSPARENT, gpu.VAR_IGNORE_TRANSPARENT | exact):
            ds.set_variant(var)
            rig = ds.render_uv(**kw)
            assert ds.last_kernel() & KV_IGNTR
            uv_close(rig["uv"], wig["uv"])
            if var & exact:
                assert_bits(rig, wig_once, f"{what}, ignore transparent, exact pow")
            assert_frame(rig, wig, tol, f"{what}, ignore transparent, var={var}")
            assert rig["ray_count"] == wig["ray_count"]
    ds.close()


# ---- the cast query that ignores transparent objects, and the shadow query, on the stacks ----
@pytest.mark.parametrize("name", list(STACK_CASES))
def test_stack_queries(gpu, tmp_path, name):
    for camera in stack_cameras(name):
        s = parse(gpu, stack_scene_json(tmp_path, name, camera)[0])
        sc = shade_ref.ShadeScene(s)
        ds = gpu.DeviceScene(s)
        o, d = ray_ref.camera_rays(sc.cam)
        want = ref_dict(ray_ref.ray_cast(sc, o, d, f32(1e-3), ignore_transparent=True))
        if all(float(f32(t)) >= 1e-6 for _, t in STACK_CASES[name]["sheets"]):   # (1e-7 is not transparent to ray_cast)
            assert (want["object"] == STACK_FLOOR).all(), "every sheet transmits: the floor alone is left"
        for linear in (False, True):
            assert_same(sc, to_np(ds.cast_rays(o, d, min_t=1e-3, ignore_transparent=True, linear=linear)), want, f"{name} {camera} linear={linear}")
        hit = want["point"]
        for li, l in enumerate(sc.lights):   # the shadow rays phong casts from the floor, shading.hpp:79-85
            if l["type"] == shade_ref.LIGHT_SUN:
                direction, dist = np.broadcast_to(-l["v"], hit.shape).astype(f32), np.full(len(hit), np.inf, f32)
            else:
                diff = ray_ref.vsub(np.broadcast_to(l["v"], hit.shape), hit)
                direction, dist = ray_ref.vnormalized(diff).astype(f32), ray_ref.vnorm(diff)
            nd = ray_ref.vnormalized(direction).astype(f32)
            max_t = (dist * ray_ref.vnorm(direction)).astype(f32)
            ws = ray_ref.shadow_intensity(sc, hit, nd, max_t)
            print(f"{name} {camera}, light {li}: shadow factors {np.unique(ws).tolist()[:14]}")
            for linear in (False, True):
                got = ds.shadow(hit, nd, max_t, linear=linear).cpu().numpy()
                assert same_bits_nan(got, ws), f"{name} {camera}, light {li}, linear={linear}: {int((got != ws).sum())} shadow factors differ"
        ds.close()


# ---- the phong exponent on rays constructed to sit inside the highlight ----
_phong_want = {}


@pytest.mark.parametrize("light", PHONG_LIGHTS)
@pytest.mark.parametrize("e", PHONG_EXPONENTS)
def test_phong_exponent_on_constructed_rays(gpu, tmp_path, e, light):
    """the radiance query with both walks, and the rays as a lens frame.  Exact pow: tests/shade_ref.py bit for bit (the f64 pow
    rounded once, what oracle_render(pow_rounded_once=True) computes: tests/test_shading_ranges_cpu.py).  The fast path:
    max |colour_fast - colour_ref| is printed per exponent (profiles/shading_ranges/fastpow.txt holds the table) and held to
    TOL where the chooser's rule keeps the fast build."""
    what = f"e={e:g} {light}"
    s = parse(gpu, phong_scene_json(tmp_path, e, light, w=PHONG_RAYS_W, h=PHONG_RAYS_H))
    o, d = phong_rays(light)
    dn = ray_ref.vnormalized(d).astype(f32)   # what the lens render makes of its directions
    want = shade_ref.ray_color(shade_ref.ShadeScene(s), o, dn, min_t=1e-3, bounces=2)
    assert (want["object"] >= 0).all() and not np.isnan(want["color"]).any()
    assert light_scale(s) == 1.0
    keep = fast_pow_kept(s)
    ds = gpu.DeviceScene(s)
    out = ("color", "t", "object", "normal")
    for linear in (False, True):
        q = to_np(ds.shade_rays(o, dn, bounces=2, min_t=1e-3, exact_pow=True, linear=linear, outputs=out))
        assert np.array_equal(q["object"], want["object"].astype(np.int32)), what
        assert same_bits_nan(q["t"], want["t"]) and same_bits_nan(q["normal"], want["normal"]), what
        assert same_bits_nan(q["color"], want["color"]), f"{what} linear={linear}: exact colour differs by up to {max_diff(q['color'], want['color']):.3e}"
        fast = to_np(ds.shade_rays(o, dn, bounces=2, min_t=1e-3, exact_pow=False, linear=linear, outputs=out))
        assert same_bits_nan(fast["t"], want["t"]) and same_bits_nan(fast["normal"], want["normal"]), what
        df = max_diff(fast["color"], want["color"])
        print(f"fastpow query e={e:g} {light} linear={linear}: max|colour_fast - colour_ref| {df:.3e}")
        if keep:
            assert df <= TOL, f"{what}: the fast path is {df:.3e} off inside the domain the chooser keeps it in"
        else:   # the launch drops the fast path where the rule says it would leave the bar
            assert same_bits_nan(fast["color"], q["color"]), f"{what}: the fast path ran outside its domain"
    exact_q = q
    for var in (gpu.VAR_AUTO, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        r = as_numpy(ds.render_lens(o.reshape(PHONG_RAYS_H, PHONG_RAYS_W, 3), d.reshape(PHONG_RAYS_H, PHONG_RAYS_W, 3), bounces=2))
        kv = ds.last_kernel()
        assert kv & KV_RAYS and bool(kv & KV_FASTPOW) == (var == gpu.VAR_AUTO and keep), hex(kv)
        assert same_bits_nan(r["depth"], want["t"]) and same_bits_nan(r["normal"], want["normal"]), (what, var)
        dl = max_diff(r["color"], want["color"])
        print(f"fastpow lens e={e:g} {light} kernel {kv:#x}: max|colour - colour_ref| {dl:.3e}")
        if not kv & KV_FASTPOW:
            assert same_bits_nan(r["color"], exact_q["color"]), f"{what} var={var}: the lens frame differs from the exact query by up to {max_diff(r['color'], exact_q['color']):.3e}"
        else:
            assert dl <= TOL, f"{what}: the default build is {dl:.3e} off"
    ds.close()
