"""The render kernel across scene scale and offset (-m gpu): every entry point that runs render_kernel<KV> — the plain
render and its variants, the delivering build, the texture coordinates, the supersampled frame and the lens render — on
scenes scaled by 2^-20 to 2^24, scenes that sit up to 2^18 units off the origin, and with a min_t that does or does not
scale with the scene (tests/util.py RENDER_RANGE_CASES, each all-opaque and with a transmitting material).  The kernel's
shortcuts (clamped reciprocals, the lazy-exact box test, widened node boxes, the division-free plane classification, the
axis-plane path, the deferred exact triangle test, the any-hit placeholder, the normalisation shortcut) are each a relative
margin plus an absolute constant: here they meet coordinates that are not of order 1.

The checker is the CPU oracle; tests/test_render_ranges_cpu.py proves case by case that it is exact and that its frame
shows every kind of object.  Bar: util.assert_parity (depth and normal bit-exact, colour within util.TOL), and bit for bit
in all three outputs under VAR_EXACT_POW.  Every pixel of the 48 x 48 frames is compared.

Before the node boxes' margin of the BVH walk covered the rounding of the ray origin's own term (render_kernel.hip, "mesh
entered: walk set-up"; DESIGN.md §4 "Range the render is pinned over"), the walk missed triangles of scenes far off the
origin.  Measured once on one MI355X with the library before the fix, pixels that differed from the oracle, mixed and
opaque flavour alike, in the case k = 0, e = 18: plain render, render_uv and every build with the BVH walk (exact pow, no
any-hit, no 6-wave, merged) 2 of 2304 (colour, by up to 0.14; depth and normal equal), samples = 2: 12 of 2304, fisheye
lens against the linear radiance query: colour by up to 0.148; the reference's walk (NO_PREFILTER | NO_CLUSTER) and
NO_CLUSTER alone: 0.  Rendered at 96 x 96: 13 of 9216, four of them with another depth; k = 0, e = 14 at 192 x 192: 1 of
36864 (depth).  Every other case: 0."""
import os

import numpy as np
import pytest

import oracle
from cutrace_amd import lenses
from tests import aa_ref
from tests.gpu_support import gpu  # noqa: F401  (the fixture)
from tests.lens_rays import assert_frames, frame_from_rays, normalised
from tests.util import (ALL_MISS_CASE, RANGE_FLAVOURS, RANGE_POW_DEPENDENT, RENDER_RANGE_CASES, assert_parity, uv_close, f32, pow2, range_case_id, range_fudge,
                        render_range_scene_json, same_bits)

pytestmark = pytest.mark.gpu

W = H = 48
BOUNCES = 5
NT = min(os.cpu_count() or 4, 16)
KV_ANYHIT, KV_OCC6, KV_HOSTOUT, KV_UV, KV_MERGE, KV_IGNTR, KV_SS, KV_RAYS = 2, 64, 128, 256, 512, 1024, 2048, 4096
CASES = [pytest.param(c, f, id=f"{range_case_id(c)},{f}") for c in RENDER_RANGE_CASES for f in RANGE_FLAVOURS]
FRAME = ("depth", "normal", "color")


def host_scene(ca, tmp_path, case, flavour):
    s = ca.HostScene.parse(render_range_scene_json(tmp_path, case[0], case[1], opaque=flavour == "opaque", w=W, h=H))
    assert s.ok
    return s


_want = {}


def wanted(ca, tmp_path, case, flavour, ss=1, **kw):
    """the oracle's frame of a case at ss*W x ss*H, rendered once per (case, flavour, ss, options) and left unchanged
    (the key has no tmp_path in it: the frame depends on the case alone, not on where its STL files were written)"""
    key = (case, flavour, ss, tuple(sorted(kw.items())))
    if key not in _want:
        s = host_scene(ca, tmp_path, case, flavour)
        s.set_size(ss * W, ss * H)
        o = oracle.oracle_render(s, fudge=range_fudge(case), bounces=BOUNCES, threads=NT, **kw)
        for k in FRAME:
            assert not np.isnan(o[k]).any(), (case, flavour, ss, k)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = o
    return _want[key]


def max_depth_of(frame):
    fin = frame["depth"][np.isfinite(frame["depth"]) & (frame["depth"] > 0)]
    return float(fin.max()) if fin.size else 0.0


def assert_bits(got, want, what):
    for k in FRAME:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert same_bits(g, w), f"{what}: {k} differs in {int((g.view(np.uint32) != w.view(np.uint32)).sum())} words of {g.size}"


def as_numpy(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


# ---- a. the plain render, default variant ----
@pytest.mark.parametrize("case,flavour", CASES)
def test_plain_render(gpu, tmp_path, case, flavour):
    what = f"{range_case_id(case)} {flavour}"
    want = wanted(gpu, tmp_path, case, flavour)
    ds = gpu.DeviceScene(host_scene(gpu, tmp_path, case, flavour))
    r = ds.render(fudge=range_fudge(case), bounces=BOUNCES)
    kv = ds.last_kernel()
    ds.close()
    print(f"{what}: kernel {kv:#x}, {r['ray_count']} casts, the oracle {want['ray_count']}")
    assert_parity(r, want, what=what)
    assert r["ray_count"] == want["ray_count"], what
    assert r["max_depth"] == max_depth_of(want), what
    # the shipped 6-wave any-hit build (1000 mesh triangles, all opaque), or the 5-wave ordered one
    assert kv & (KV_OCC6 | KV_ANYHIT) == (KV_OCC6 | KV_ANYHIT if flavour == "opaque" else 0), hex(kv)
    if case == ALL_MISS_CASE:
        assert np.isposinf(r["depth"]).all() and not r["color"].any() and not r["normal"].any()
        assert r["ray_count"] == 2 * W * H


# ---- b. the other builds of the plain render ----
@pytest.mark.parametrize("case,flavour", CASES)
def test_render_variants(gpu, tmp_path, case, flavour):
    what = f"{range_case_id(case)} {flavour}"
    want = wanted(gpu, tmp_path, case, flavour)
    fudge = range_fudge(case)
    ds = gpu.DeviceScene(host_scene(gpu, tmp_path, case, flavour))
    exact = gpu.VAR_EXACT_POW
    for name, var in (("exact pow", exact), ("the reference's walk", exact | gpu.VAR_NO_PREFILTER | gpu.VAR_NO_CLUSTER),
                      ("no any-hit", exact | gpu.VAR_NO_ANYHIT), ("no 6-wave build", exact | gpu.VAR_NO_OCC6), ("merged", exact | gpu.VAR_MERGE)):
        ds.set_variant(var)
        r = ds.render(fudge=fudge, bounces=BOUNCES)
        assert_bits(r, want, f"{what}, {name}")
        assert r["ray_count"] == want["ray_count"], (what, name)
        if var & gpu.VAR_MERGE:
            assert ds.last_kernel() & KV_MERGE, f"{what}: the merged tree was not walked"
    ds.set_variant(gpu.VAR_AUTO)
    r = ds.render(fudge=fudge, bounces=BOUNCES, pinned=True)   # the delivering build
    assert ds.last_kernel() & KV_HOSTOUT, hex(ds.last_kernel())
    assert_parity(r, want, what=f"{what}, delivered by the kernel")
    assert r["ray_count"] == want["ray_count"]
    ds.close()


# ---- c. texture coordinates ----
@pytest.mark.parametrize("case,flavour", CASES)
def test_texture_coordinates(gpu, tmp_path, case, flavour):
    """the bar of test_gpu_parity.py test_texture_coordinates_random_scenes_vs_oracle: uv within 1e-4 (relative above 1),
    NaN where the oracle has NaN, depth and normal bit-exact"""
    what = f"{range_case_id(case)} {flavour}"
    fudge = range_fudge(case)
    ds = gpu.DeviceScene(host_scene(gpu, tmp_path, case, flavour))
    want = wanted(gpu, tmp_path, case, flavour, uv=True)
    r = ds.render_uv(fudge=fudge, bounces=BOUNCES)
    assert ds.last_kernel() & KV_UV
    uv_close(r["uv"], want["uv"])
    assert_parity(r, want, what=what + " uv")
    assert r["ray_count"] == want["ray_count"]
    if flavour == "mixed":
        want = wanted(gpu, tmp_path, case, flavour, uv=True, ignore_transparent_primary=True)
        for var in (gpu.VAR_IGNORE_TRANSPARENT, gpu.VAR_IGNORE_TRANSPARENT | gpu.VAR_EXACT_POW):
            ds.set_variant(var)
            r = ds.render_uv(fudge=fudge, bounces=BOUNCES)
            assert ds.last_kernel() & KV_IGNTR
            uv_close(r["uv"], want["uv"])
            if var & gpu.VAR_EXACT_POW:
                assert_bits(r, want, what + " ignore transparent, exact pow")
            else:
                assert_parity(r, want, what=what + " ignore transparent")
            assert r["ray_count"] == want["ray_count"]
    ds.close()


# ---- d. the supersampled frame ----
@pytest.mark.parametrize("case,flavour", CASES)
def test_supersampled_render(gpu, tmp_path, case, flavour):
    what = f"{range_case_id(case)} {flavour}"
    fudge = range_fudge(case)
    ds = gpu.DeviceScene(host_scene(gpu, tmp_path, case, flavour))
    for ss in (2, 4):
        big = wanted(gpu, tmp_path, case, flavour, ss=ss)
        want = aa_ref.reduce_frame(big, ss)
        ds.set_variant(gpu.VAR_AUTO)
        r = ds.render(fudge=fudge, bounces=BOUNCES, samples=ss)
        assert ds.last_kernel() & KV_SS
        assert r["depth"].shape == (H, W)
        assert_parity(r, want, what=f"{what} s={ss}")
        assert r["ray_count"] == big["ray_count"], (what, ss)
        ds.set_variant(gpu.VAR_EXACT_POW)
        e = ds.render(fudge=fudge, bounces=BOUNCES, samples=ss)
        if (case, flavour, ss) in RANGE_POW_DEPENDENT:
            # the oracle's own colour depends on how its pow is rounded (util.py): within TOL of it, and bit for bit what the
            # oracle gives with the device's pow, the f64 pow rounded once
            assert_parity(e, want, what=f"{what} s={ss} exact pow")
            once = aa_ref.reduce_frame(wanted(gpu, tmp_path, case, flavour, ss=ss, pow_rounded_once=True), ss)
            assert not same_bits(once["color"], want["color"])
            assert_bits(e, once, f"{what} s={ss} exact pow, against the oracle with the pow rounded once")
        else:
            assert_bits(e, want, f"{what} s={ss} exact pow")
    ds.close()


# ---- e. the lens render ----
@pytest.mark.parametrize("case,flavour", CASES)
def test_lens_render(gpu, tmp_path, case, flavour):
    """pinhole rays: the plain render of the same handle, bit for bit.  A fisheye and a two-samples-per-axis thin lens (aperture
    and focus scaled with the scene): the radiance query with the linear walk on the normalised directions, as
    test_gpu_lens.py test_other_lenses_against_the_linear_radiance_query compares; tests/test_gpu_query_ranges.py swept that
    query against tests/shade_ref.py across these scales."""
    what = f"{range_case_id(case)} {flavour}"
    fudge, sk = range_fudge(case), float(pow2(case[0]))
    s = host_scene(gpu, tmp_path, case, flavour)
    cam = s.desc.contents.cam
    ds = gpu.DeviceScene(s)
    o, d = lenses.pinhole(cam, W, H)
    for var in (gpu.VAR_AUTO, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        plain = ds.render(fudge=fudge, bounces=BOUNCES)
        kv_plain = ds.last_kernel() & ~KV_HOSTOUT
        got = as_numpy(ds.render_lens(o, d, fudge=fudge, bounces=BOUNCES))
        assert ds.last_kernel() == kv_plain | KV_RAYS, (hex(ds.last_kernel()), hex(kv_plain))
        assert_bits(got, plain, f"{what} pinhole var={var}")
        assert got["ray_count"] == plain["ray_count"] and got["max_depth"] == plain["max_depth"], (what, var)
    for lname, ss, (o, d) in (("fisheye", 1, lenses.fisheye(cam, W, H, 150.0)),
                              ("thin lens", 2, lenses.thin_lens(cam, W, H, 2, 0.15 * sk, 4.0 * sk, seed=11))):
        keep = ~lenses.is_masked(o, d).reshape(-1)
        assert (lname == "fisheye") == (not keep.all()) and keep.sum() > ss * ss * H * W // 3
        of, df = o.reshape(-1, 3)[keep], normalised(d.reshape(-1, 3)[keep])
        for exact in (False, True):
            kw = dict(bounces=BOUNCES, min_t=fudge, exact_pow=exact, outputs=("color", "t", "normal"))
            ref = as_numpy(ds.shade_rays(of, df, linear=True, **kw))
            bvh = as_numpy(ds.shade_rays(of, df, linear=False, **kw))
            for k in ("t", "normal"):   # the reference side does not depend on the walk for these rays
                assert same_bits(ref[k], bvh[k]), (what, lname, k)
            want = aa_ref.reduce_frame(frame_from_rays(ss * H, ss * W, keep, ref["t"], ref["normal"], ref["color"]), ss)
            ds.set_variant(gpu.VAR_EXACT_POW if exact else gpu.VAR_AUTO)
            got = as_numpy(ds.render_lens(o, d, fudge=fudge, bounces=BOUNCES, samples=ss))
            kv = ds.last_kernel()
            assert kv & KV_RAYS and bool(kv & KV_SS) == (ss > 1)
            assert_frames(got, want, f"{what} {lname} exact={exact}", color="bits" if exact else "tol")
            if case != ALL_MISS_CASE:
                assert np.isfinite(got["depth"]).sum() > H * W // 10, f"{what} {lname}: the lens sees too little"
    ds.close()


# ---- f. the length of the lens render's directions ----
LENS_DIR_EXPONENTS = (-56, -24, 24, 56)


@pytest.mark.parametrize("j", LENS_DIR_EXPONENTS + ("mixed",))
def test_lens_directions_of_length_2_to_the_j(gpu, tmp_path, j):
    """v * (1 / sqrt(v.v)) of a direction times a power of two is the same unit vector bit for bit as long as v.v stays
    normal, and 2^+-112 does: the frame of the k = 0 scene must not change.  "mixed": every pixel its own exponent."""
    case = (0, None, True)
    s = host_scene(gpu, tmp_path, case, "mixed")
    ds = gpu.DeviceScene(s)
    o, d = lenses.pinhole(s.desc.contents.cam, W, H)
    if j == "mixed":
        jj = np.random.RandomState(7).choice(LENS_DIR_EXPONENTS + (0,), (H, W))
        assert all((jj == e).sum() > 100 for e in LENS_DIR_EXPONENTS)
    else:
        jj = np.full((H, W), j)
    dj = (d * np.ldexp(f32(1.0), jj).astype(f32)[..., None]).astype(f32)
    assert np.isfinite(dj).all() and (np.abs(dj[dj != 0]) > 1e-37).all()
    for var in (gpu.VAR_AUTO, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        base = as_numpy(ds.render_lens(o, d, bounces=BOUNCES))
        got = as_numpy(ds.render_lens(o, dj, bounces=BOUNCES))
        assert np.isfinite(base["depth"]).sum() > H * W // 2
        assert_bits(got, base, f"j={j} var={var}")
        assert got["ray_count"] == base["ray_count"] and got["max_depth"] == base["max_depth"]
    want = wanted(gpu, tmp_path, case, "mixed")
    assert_bits(got, want, f"j={j} against the oracle")   # (the last launch: exact pow)
    ds.close()

