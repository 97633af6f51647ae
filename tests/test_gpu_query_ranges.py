"""Ray and radiance queries (ctr_cast_rays, ctr_shade_rays) across the range of their inputs: directions of length 2^-104
to 2^100, scenes scaled by 2^-20 to 2^24 and far off centre, non-finite and zero rays inside ordinary batches, and the
largest LDS launch ctr_shade_rays can make.  The checker is tests/ray_ref.py / tests/shade_ref.py;
tests/test_query_ranges_cpu.py proves that it is exact at every exponent used here (tests/util.py DIR_EXPONENTS,
SCALE_EXPONENTS), so a mismatch is the kernel's.  "Bitwise" as in test_gpu_rays.py and test_gpu_shade.py."""
import json

import numpy as np
import pytest

from tests import ray_ref, shade_ref
from tests.conftest import load_scene
from tests.util import (DIR_EXPONENTS, SCALE_EXPONENTS, TOL, _random_scene, assert_bitwise, assert_same, corner_meshes, f32,
                        f32_bits, first_hit_same, hall_of_mirrors_json, max_diff, pow2, range_offset, ref_dict, render_range_scene_json, scaled_scene_json, sphere_mask,
                        sweep_max_t, sweep_min_t, sweep_rays, to_np)

pytestmark = pytest.mark.gpu
ALL = ("color", "t", "object", "normal")
N = 4096
SWEEP_SCENES = ("bunny", "sphere_plane", "random0", "random5")


def sweep_scene(ca, which):
    s = ca.HostScene.parse(_random_scene(int(which[6:]), w=32, h=32)) if which.startswith("random") else load_scene(ca, which, 32, 32)
    assert s.ok
    return s


def direction_batch(sc, j, n=N, seed=3):
    """(origins, directions * 2^j, min_t, max_t, shade_rays' min_t) of one batch; j = "mixed": every ray its own exponent.
    shade_rays takes one min_t for all rays and all levels: 1e-3 as the render, but no more than 1e-3 * 2^-j of the
    longest direction, whose first hits it would otherwise cut off."""
    o, d, sel = sweep_rays(seed, n, sc)
    jj = np.random.RandomState(seed + 1).choice(DIR_EXPONENTS, n) if j == "mixed" else np.full(n, j)
    d = (d * np.ldexp(f32(1.0), jj).astype(f32)[:, None]).astype(f32)
    return o, d, sweep_min_t(sel, jj), sweep_max_t(sel, jj), float(min(f32(1e-3), f32(1e-3) * pow2(-int(jj.max()))))


def check_batch(ds, sc, o, d, mt, max_t, shade_min_t, what, bounces=3):
    """cast_rays, shadow and shade_rays of one batch, both walks, against the reference: the assertions of every sweep"""
    import torch
    n = len(o)
    want = ref_dict(ray_ref.ray_cast(sc, o, d, mt))
    meshes = [i for i, ob in enumerate(sc.objects) if ob["type"] == ray_ref.OBJ_MESH]
    on_mesh, hits = int(np.isin(want["object"], meshes).sum()), int((want["object"] >= 0).sum())
    print(f"{what}: {n} rays, the reference hits something in {hits}, a mesh in {on_mesh}")
    assert hits >= n // 10 and (on_mesh >= n // 20 or not meshes), f"{what}: the batch shows too little"
    for linear in (False, True):
        assert_same(sc, to_np(ds.cast_rays(o, d, min_t=mt, linear=linear)), want, f"{what}: cast_rays linear={linear}")
    want_s = ray_ref.shadow_intensity(sc, o, d, max_t)
    for linear in (False, True):
        got = ds.shadow(o, d, max_t=torch.from_numpy(max_t), linear=linear).cpu().numpy()
        assert_bitwise(got, want_s, f"{what}: shadow linear={linear}")
    want_c = shade_ref.ray_color(sc, o, d, min_t=shade_min_t, bounces=bounces)
    for exact in (False, True):
        w = f"{what}: shade_rays exact_pow={exact}"
        lin = to_np(ds.shade_rays(o, d, bounces=bounces, min_t=shade_min_t, exact_pow=exact, linear=True, outputs=ALL))
        first_hit_same(lin, want_c, w + " linear")
        assert max_diff(lin["color"], want_c["color"], w + " linear") <= TOL
        dflt = to_np(ds.shade_rays(o, d, bounces=bounces, min_t=shade_min_t, exact_pow=exact, outputs=ALL))
        assert np.array_equal(dflt["object"], lin["object"]), w + ": default walk against linear, object"
        for k in ("color", "t", "normal"):
            assert_bitwise(dflt[k], lin[k], f"{w}: default walk against linear, {k}")


# ---- 1. direction length ----
@pytest.mark.parametrize("j", DIR_EXPONENTS + ("mixed",))
@pytest.mark.parametrize("which", SWEEP_SCENES)
def test_directions_of_length_2_to_the_j(ca, which, j):
    """Before the walk's box test scaled the direction to unit size (ray_walk.h box_ray), its reciprocals' clamp at +-1e30 made
    the default walk miss meshes for directions shorter than about 2^-99.  Measured on one MI355X with the library before
    the fix, rays of these batches whose default walk differed from the linear walk, cast_rays / shadow / shade_rays:
    bunny j=-104: 313 / 42 / 308, -100: 302 / 42 / 302, -96: 17 / 4 / 17, mixed: 74 / 12 / 74; random5 j=-104: 1177 / 322 /
    1173, -100: 1167 / 317 / 1167, -96: 150 / 28 / 150, mixed: 303 / 71 / 303; every other exponent and scene: 0."""
    s = sweep_scene(ca, which)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    check_batch(ds, sc, *direction_batch(sc, j), f"{which} j={j}")
    ds.close()


# ---- 2. scene scale ----
@pytest.mark.parametrize("k", SCALE_EXPONENTS)
def test_scenes_scaled_by_2_to_the_k(ca, tmp_path, k):
    """origins and min_t scale with the scene, directions do not; the shadow loop's 1e-3 step is absolute, so shadows and
    colours change with k — and must still be the reference's"""
    base = shade_ref.ShadeScene(ca.HostScene.parse(scaled_scene_json(tmp_path, 0)))
    s = ca.HostScene.parse(scaled_scene_json(tmp_path, k))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    o, d, sel = sweep_rays(4, N, base)
    sk = pow2(k)
    check_batch(ds, sc, o * sk, d, sweep_min_t(sel, 0) * sk, sweep_max_t(sel, 0) * sk, float(f32(1e-3) * sk), f"scale k={k}")
    ds.close()


@pytest.mark.parametrize("e", [10, 18])
def test_a_scene_2_to_the_e_off_the_origin(ca, tmp_path, e):
    """the scene of the render range sweep (tests/util.py render_range_scene_json) moved 2^e * (1, -0.75, 0.5) off the origin,
    the rays' origins with it.  The node boxes' margin of the default walk (ray_walk.h cast_mesh) is folded into the ray
    origin's own term, whose rounding grows with the origin's coordinates: before the margin covered that, the default walk
    differed from the linear one at e = 18 (seen on the thin-lens rays of tests/test_gpu_render_ranges.py)."""
    base = shade_ref.ShadeScene(ca.HostScene.parse(render_range_scene_json(tmp_path, 0, None, w=32, h=32)))
    s = ca.HostScene.parse(render_range_scene_json(tmp_path, 0, e, w=32, h=32))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    o, d, sel = sweep_rays(7, N, base)
    check_batch(ds, sc, (o + range_offset(0, e)).astype(f32), d, sweep_min_t(sel, 0), sweep_max_t(sel, 0), 1e-3, f"offset e={e}")
    ds.close()


def test_a_mesh_far_off_centre_next_to_one_at_the_origin(ca, tmp_path):
    from cutrace_amd import scenes
    quad, dup, degenerate, fan, far = corner_meshes()
    objs = []
    for name, tris in (("fan", fan), ("far", far)):
        path = str(tmp_path / f"{name}.stl")
        scenes.write_stl(path, np.asarray(tris, f32))
        objs.append({"type": "mesh", "file": path, "material": len(objs)})
    objs.append({"type": "plane", "point": [0, -1.0, 0], "normal": [0, 1, 0], "material": 1})
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
            {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.0, "phong": 10, "transparency": 0.4}]
    lights = [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
              {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}]
    cam = {"eye": [0.3, 0.8, 4.0], "up": [0, 1, 0], "look": [-0.05, -0.15, -1.0], "near_plane": 0.1, "far_plane": 100.0,
           "width": 32, "height": 32, "ambient": 0.1}
    s = ca.HostScene.parse(json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs}))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    o, d, sel = sweep_rays(5, N, sc)
    want = ray_ref.ray_cast(sc, o, d, sweep_min_t(sel, 0))
    assert (want["object"] == 0).sum() >= 50 and (want["object"] == 1).sum() >= 50   # both meshes are seen
    check_batch(ds, sc, o, d, sweep_min_t(sel, 0), sweep_max_t(sel, 0), 1e-3, "fan and far")
    ds.close()


# ---- 3. odd rays inside ordinary batches ----
NAN, INF = f32(np.nan), f32(np.inf)
ODD = [("origin", 0, NAN), ("origin", 2, NAN), ("dir", 1, NAN), ("dir", 2, NAN), ("origin", 0, INF), ("origin", 1, -INF),
       ("dir", 0, INF), ("dir", 2, -INF), ("zero", 0, f32(0.0)), ("zero", 0, f32(-0.0)), ("axis", 0, None), ("axis", 1, None),
       ("axis", 2, None), ("tiny", 0, None)]


def with_odd_rays(o, d):
    """every seventh ray replaced by one of ODD, in turn: (origins, directions, mask of the replaced)"""
    o, d = o.copy(), d.copy()
    odd = np.zeros(len(o), bool)
    for n, i in enumerate(range(3, len(o), 7)):
        kind, c, v = ODD[n % len(ODD)]
        odd[i] = True
        if kind == "origin":
            o[i, c] = v
        elif kind == "dir":
            d[i, c] = v
        elif kind == "zero":                                   # the all-zero direction, (0, 0, 0) and (-0, 0, 0)
            d[i] = (v, 0.0, 0.0)
        elif kind == "axis":                                   # two zero components
            keep = d[i, c]
            d[i] = (0.0, -0.0, 0.0)
            d[i, c] = keep
        else:                                                  # length 1e-38: every component denormal
            d[i] = (d[i].astype(np.float64) / np.linalg.norm(d[i].astype(np.float64)) * 1e-38).astype(f32)
    return o, d, odd


def same_or_both_nan(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    if g.dtype != np.float32:
        assert np.array_equal(g, w.astype(g.dtype)), what
        return
    w = w.astype(f32).reshape(g.shape)
    bad = (f32_bits(g) != f32_bits(w)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), f"{what}: {int(bad.reshape(len(g), -1).any(-1).sum())} of {len(g)} rays differ"


@pytest.mark.parametrize("which", ["bunny", "random5"])
def test_odd_rays_inside_ordinary_batches(ca, which):
    """NaN, infinite, zero, axis-parallel and denormal rays: (a) every ray's answer is the reference's, NaN for NaN;
    (b) the ordinary rays around them get bit for bit what they get in a batch without them"""
    import torch
    s = sweep_scene(ca, which)
    sc = shade_ref.ShadeScene(s)
    ds = ca.DeviceScene(s)
    o0, d0, sel = sweep_rays(6, N, sc)
    mt, max_t = sweep_min_t(sel, 0), sweep_max_t(sel, 0)
    o, d, odd = with_odd_rays(o0, d0)
    assert odd.sum() >= 20 * len(ODD) and not odd[::7].any()
    want = ref_dict(ray_ref.ray_cast(sc, o, d, mt))
    want_s = ray_ref.shadow_intensity(sc, o, d, max_t)
    want_c = shade_ref.ray_color(sc, o, d, min_t=1e-3, bounces=3)
    sph = sphere_mask(sc, want["object"])
    for linear in (False, True):
        what = f"{which} linear={linear}"
        got, clean = to_np(ds.cast_rays(o, d, min_t=mt, linear=linear)), to_np(ds.cast_rays(o0, d0, min_t=mt, linear=linear))
        assert_same(sc, {k: v[~odd] for k, v in got.items()}, {k: v[~odd] for k, v in want.items()}, what + ": ordinary rays")
        for k in got:
            m = odd & ~sph if k == "uv" else odd
            same_or_both_nan(got[k][m], want[k][m], f"{what}: odd rays, {k}")
            same_or_both_nan(got[k][~odd], clean[k][~odd], f"{what}: ordinary rays with and without odd neighbours, {k}")
        if (odd & sph).any():
            g, w = got["uv"][odd & sph], want["uv"][odd & sph].astype(f32)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.abs(np.nan_to_num(g) - np.nan_to_num(w)).max() <= 1e-4, what + ": sphere uv"
        sh = ds.shadow(o, d, max_t=torch.from_numpy(max_t), linear=linear).cpu().numpy()
        clean_sh = ds.shadow(o0, d0, max_t=torch.from_numpy(max_t), linear=linear).cpu().numpy()
        same_or_both_nan(sh, want_s, what + ": shadow")
        same_or_both_nan(sh[~odd], clean_sh[~odd], what + ": shadow of ordinary rays with and without odd neighbours")
        for exact in (False, True):
            w = f"{what} exact_pow={exact}"
            col = to_np(ds.shade_rays(o, d, bounces=3, min_t=1e-3, exact_pow=exact, linear=linear, outputs=ALL))
            clean_col = to_np(ds.shade_rays(o0, d0, bounces=3, min_t=1e-3, exact_pow=exact, linear=linear, outputs=ALL))
            for k in ("t", "object", "normal"):
                same_or_both_nan(col[k], want_c[k], f"{w}: first hit, {k}")
            assert max_diff(col["color"], want_c["color"], w) <= TOL
            for k in ALL:
                same_or_both_nan(col[k][~odd], clean_col[k][~odd], f"{w}: ordinary rays with and without odd neighbours, {k}")
    ds.close()


# ---- 4. the largest LDS launch ----
def test_the_largest_lds_launch(ca, tmp_path):
    """the deepest tree this project builds (the 64 000-triangle bunny: 33 stack slots), 10-dword frames (its material
    reflects and transmits) and bounces 15, between two mirror walls"""
    from cutrace_amd import scenes
    w, h = 64, 36
    scenes.make_dense_bunny(str(tmp_path), rounds=3)
    mesh = {"type": "mesh", "file": str(tmp_path / "bunny_sub3.stl")}
    s = ca.HostScene.parse(hall_of_mirrors_json(w, h, middle=mesh))
    assert s.ok
    sc = shade_ref.ShadeScene(s)
    assert ((sc.mat_reflexivity.astype(np.float64) >= 1e-6) & (sc.transparency.astype(np.float64) >= 1e-6)).any()
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(sc.cam)
    deep = {}
    for b in (15, 11):
        dflt = to_np(ds.shade_rays(o, d, bounces=b, min_t=1e-3, exact_pow=True, outputs=ALL))
        lin = to_np(ds.shade_rays(o, d, bounces=b, min_t=1e-3, exact_pow=True, linear=True, outputs=ALL))
        assert np.array_equal(dflt["object"], lin["object"]) and (dflt["object"] == 3).sum() > 50
        for k in ("color", "t", "normal"):
            assert_bitwise(dflt[k], lin[k], f"bounces {b}: default walk against linear, {k}")
        deep[b] = dflt["color"]
    assert not np.array_equal(deep[15], deep[11]), "the scene does not recurse below depth 11: the test shows nothing"
    want = shade_ref.ray_color(sc, o, d, min_t=1e-3, bounces=2)
    lin = to_np(ds.shade_rays(o, d, bounces=2, min_t=1e-3, exact_pow=True, linear=True, outputs=ALL))
    first_hit_same(lin, want, "bounces 2 linear")
    assert max_diff(lin["color"], want["color"], "bounces 2 linear") <= TOL
    ds.close()
