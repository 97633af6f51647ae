"""The checkers and the case builders of tests/test_gpu_shading_ranges.py (CPU, no GPU).

The photometric counterpart of tests/test_render_ranges_cpu.py.  The GPU sweep runs materials, lights and phong exponents
outside the box every other scene draws them from (tests/util.py, "the shading-parameter sweeps"); here, case by case,
  - tests/shade_ref.py, the checker of the radiance queries, equals oracle_render(pow_rounded_once=True) bit for bit on the
    camera's rays, and, where oracle/_ref is built, the reference's own headers equal the oracle bit for bit: the C
    restatement had never met these values either;
  - the builders' claims hold: at which sheet the float32 partial sums reach 1, that the lower camera of a stack sees floor
    under every occluder count, that the constructed rays of the phong family sit inside the highlight, that the values
    around 1e-6 and the negative zero arrive in the scene description as the floats they are meant to be;
  - the flattened scene's all_opaque / need_cold / any_bounce follow exactly-zero and the double comparison.

A case that fails here leaves the lists of tests/util.py with a comment that says why: it is not tolerated."""
import numpy as np
import pytest

import oracle
from tests import ray_ref, shade_ref
from tests.checkers import harness, run  # noqa: F401  (the fixture that builds scripts/flatten_check.cpp)
from tests.util import (LIGHT_CASES, LIGHT_SUN_LENGTH_CASES, PHONG_EXPONENTS, PHONG_LIGHTS, PHONG_POINTS, PHONG_RAYS_H, PHONG_RAYS_W, PHONG_THETAS,
                        SHADING_FRAME_CASES, STACK_CASES, fast_pow_kept, STACK_FLOOR, THRESHOLD_MATERIAL, THRESHOLD_MODES, THRESHOLD_VALUES, f32, first_full_sheet,
                        lights_scene_json, parse, phong_rays, phong_scene_json, same_bits, shading_case_id, shading_case_json, stack_crossings,
                        stack_cameras, stack_partial_sums, stack_scene_json, threshold_room_json)

FRAME_CASES = [pytest.param(c, id=shading_case_id(c)) for c in SHADING_FRAME_CASES]
FRAME = ("depth", "normal", "color")


def same_bits_nan(a, b):
    """identical float bits; NaNs by position and sign, not payload"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32).reshape(np.shape(a))
    na, nb = np.isnan(a), np.isnan(b)
    return (np.array_equal(na, nb) and np.array_equal(np.signbit(a[na]), np.signbit(b[nb])) and
            np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


# ---- the checkers against each other ----
@pytest.mark.parametrize("case", FRAME_CASES)
def test_shade_ref_equals_the_oracle_with_the_pow_rounded_once(ca, tmp_path, case):
    text, bounces = shading_case_json(tmp_path, case)
    s = parse(ca, text)
    sc = shade_ref.ShadeScene(s)
    o, d = ray_ref.camera_rays(sc.cam)
    r = shade_ref.ray_color(sc, o, d, min_t=1e-3, bounces=bounces)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=bounces, pow_rounded_once=True)
    assert (g["hit_id"] >= 0).sum() > g["hit_id"].size // 4
    assert same_bits_nan(r["color"], g["color"]), f"colour differs by up to {np.nanmax(np.abs(r['color'].reshape(g['color'].shape) - g['color']))}"
    assert same_bits_nan(r["t"], g["depth"]) and same_bits_nan(r["normal"], g["normal"])
    assert np.array_equal(r["object"], g["hit_id"].reshape(-1))
    for k in FRAME:   # what the sweep leaves out of scope would show here: no case may make a NaN
        assert not np.isnan(g[k]).any(), k
    plain = oracle.oracle_render(s, fudge=1e-3, bounces=bounces)   # glibc's powf against the pow rounded once: an ulp of the term
    assert same_bits(plain["depth"], g["depth"]) and same_bits(plain["normal"], g["normal"]) and plain["ray_count"] == g["ray_count"]
    assert np.abs(plain["color"].astype(np.float64) - g["color"]).max() <= 1e-6 * max(1.0, float(np.abs(g["color"]).max()))


@pytest.mark.parametrize("case", FRAME_CASES)
def test_ref_render_equals_oracle_render(ca, tmp_path, case):
    """the restatement against the reference's own headers, where those have been built"""
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built here (needs the reference tree at build time)")
    text, bounces = shading_case_json(tmp_path, case)
    s = parse(ca, text)
    o, r = oracle.oracle_render(s, bounces=bounces), oracle.ref_render(s, bounces=bounces)
    for k in FRAME:
        assert same_bits_nan(o[k], r[k]), k
    assert np.array_equal(o["hit_id"], r["hit_id"]) and o["ray_count"] == r["ray_count"]
    if hasattr(oracle.ref_lib(), "ref_render_ex") and case[0] in ("stack", "threshold"):   # the frames of the uv and ignore-transparent runs
        kw = dict(bounces=bounces, uv=True, ignore_transparent_primary=True)
        o, r = oracle.oracle_render(s, **kw), oracle.ref_render(s, **kw)
        for k in FRAME + ("uv",):
            assert same_bits_nan(o[k], r[k]), f"uv, ignore transparent: {k}"


@pytest.mark.parametrize("light", PHONG_LIGHTS)
@pytest.mark.parametrize("e", PHONG_EXPONENTS)
def test_the_constructed_rays_sit_in_the_highlight(ca, tmp_path, e, light):
    """at least 32 rays per exponent with a specular term above 0.25 in tests/shade_ref.py: the scene's material has
    specular 1 and colour 1 and its one light colour 1, so the term is colour minus the same scene's colour with specular 0"""
    o, d = phong_rays(light)
    assert o.shape == (PHONG_POINTS * len(PHONG_THETAS), 3) and len(o) == PHONG_RAYS_W * PHONG_RAYS_H
    d = ray_ref.vnormalized(d).astype(f32)
    s = parse(ca, phong_scene_json(tmp_path, e, light))
    with_spec = shade_ref.ray_color(shade_ref.ShadeScene(s), o, d, bounces=0)
    s.set_material(0, specular=0.0)
    without = shade_ref.ray_color(shade_ref.ShadeScene(s), o, d, bounces=0)
    assert (with_spec["object"] >= 0).all() and not np.isnan(with_spec["color"]).any()
    fs = with_spec["color"][:, 0].astype(np.float64) - without["color"][:, 0]
    n = int((fs > 0.25).sum())
    print(f"e = {e:g}, {light}: {n} of {len(o)} rays with a specular term above 0.25, the largest {fs.max():.4f}; objects {np.bincount(with_spec['object'])}")
    assert n >= 32
    assert all(int((with_spec["object"] == k).sum()) >= len(o) // 6 for k in (0, 1, 2)), "a surface is hardly hit"
    if e > 0:
        assert fs.max() > 0.99, "no ray on the highlight's peak"


# ---- the builders' claims ----
def test_the_lists_keep_what_the_sweep_is_for():
    assert set(STACK_CASES) == {"0.75x4", "0.5x2", "0.9x12", "0.7x4", "1.0x5", "1.5x3", "1e-7x2", "mixed", "mixed_reversed", "close", "light_between",
                                "exact_then_negative", "restart_step"}
    kinds = {k for c in STACK_CASES.values() for k, _ in c["sheets"]}
    assert kinds == {"triangle", "meshA", "meshB", "sphere", "plane"}
    assert any(sum(k == "meshA" for k, _ in c["sheets"]) > 1 for c in STACK_CASES.values()), "several quads of one mesh"
    assert [float(f32(v)) for v in THRESHOLD_VALUES] == list(THRESHOLD_VALUES) and len(THRESHOLD_VALUES) == 9
    assert np.signbit(THRESHOLD_VALUES[1]) and THRESHOLD_VALUES[1] == 0
    assert THRESHOLD_VALUES[3] < 1e-6 < THRESHOLD_VALUES[4] and np.nextafter(f32(THRESHOLD_VALUES[3]), f32(1)) == f32(THRESHOLD_VALUES[4])
    assert PHONG_EXPONENTS == (0.0, 0.5, 1.0, 2.0, 32.0, 300.0, 1000.0, 3000.0, 10000.0, 100000.0)
    assert PHONG_THETAS[0] == 0 and len(PHONG_THETAS) == 16
    assert {f"n{n}" for n in (0, 1, 2, 3, 8, 33)} <= set(LIGHT_CASES) and {f"ambient_{a}" for a in (0.0, 1.0, 2.5, -0.25)} <= set(LIGHT_CASES)
    assert [len(LIGHT_CASES[f"n{n}"]["lights"]) for n in (0, 1, 2, 3, 8, 33)] == [0, 1, 2, 3, 8, 33]
    assert {l["type"] for l in LIGHT_CASES["n33"]["lights"]} == {"sun", "point"}
    assert len(SHADING_FRAME_CASES) == 25 + 81 + 16 + 19


def test_the_partial_sums_reach_one_where_the_cases_say():
    tr = {n: [t for k, t in c["sheets"] for _ in range(2 if k == "sphere" else 1)] for n, c in STACK_CASES.items()}
    assert stack_partial_sums(tr["0.75x4"])[3] == f32(1.0) and first_full_sheet(tr["0.75x4"]) == 4    # exactly 1.0, at the fourth
    assert first_full_sheet(tr["0.5x2"]) == 2 and stack_partial_sums(tr["0.5x2"])[1] == f32(1.0)
    # 1 - 0.9f is 0.100000024: ten of them are the first float32 sum at or above 1 (the exact sum of ten is 1.00000024)
    assert f32(1.0) - f32(0.9) > f32(0.1)
    assert first_full_sheet(tr["0.9x12"]) == 10 and stack_partial_sums(tr["0.9x12"])[8] < f32(1.0)
    sums = stack_partial_sums(tr["0.7x4"])
    assert first_full_sheet(tr["0.7x4"]) == 4 and sums[2] < f32(1.0) < sums[3]                       # passes 1 between sheets
    assert first_full_sheet(tr["1.0x5"]) is None and len(tr["1.0x5"]) == 5 and all(s == 0 for s in stack_partial_sums(tr["1.0x5"]))
    sums = stack_partial_sums(tr["exact_then_negative"])   # 1.0 exactly at the second sheet; going on would give 0.5
    assert first_full_sheet(tr["exact_then_negative"]) == 2 and sums[1] == f32(1.0) and sums[2] == f32(0.5)
    assert first_full_sheet(tr["1.5x3"]) is None and all(s < 0 for s in stack_partial_sums(tr["1.5x3"]))
    # 1e-7: one occluder leaves the sum below 1 (the loop goes on, in hit order), two reach it; and 1e-7 makes no bounce
    assert f32(1.0) - f32(1e-7) < f32(1.0) and first_full_sheet(tr["1e-7x2"]) == 2 and float(f32(1e-7)) < 1e-6
    # the same three sheets in both orders: full shadow at the third, or already at the second; under two sheets 0.9 or 1
    assert first_full_sheet(tr["mixed"]) == 3 and first_full_sheet(tr["mixed_reversed"]) == 2
    assert stack_partial_sums(tr["mixed"])[1] < f32(1.0) <= stack_partial_sums(tr["mixed_reversed"])[1]


def occluders(sc, start, nd, light_dist, step):
    """hits of shadow_intensity's loop without its early exit: casts from min_t = (float)(last_hit + step)"""
    n = len(start)
    count, last, live = np.zeros(n, int), np.zeros(n, f32), np.ones(n, bool)
    while live.any():
        idx = np.nonzero(live)[0]
        r = ray_ref.ray_cast(sc, start[idx], nd[idx], (last[idx].astype(np.float64) + step).astype(f32))
        go = (r["object"] >= 0) & (r["t"] < light_dist[idx])
        live[idx[~go]] = False
        count[idx[go]] += 1
        last[idx[go]] = r["t"][go]
    return count


@pytest.mark.parametrize("name", [n for n in STACK_CASES if "below" in stack_cameras(n)])
def test_the_lower_camera_sees_floor_under_every_occluder_count(ca, tmp_path, name):
    """the floor pixels of the camera under the stack, per light: how many occluders the shadow loop meets on the way to it"""
    text, _ = stack_scene_json(tmp_path, name, "below")
    s = parse(ca, text)
    sc = shade_ref.ShadeScene(s)
    g = oracle.oracle_render(s, bounces=0)
    assert (g["hit_id"] == STACK_FLOOR).all(), "the lower camera sees something else than the floor"
    o, d = ray_ref.camera_rays(sc.cam)
    hit = ray_ref.ray_cast(sc, o, d, f32(1e-3))["point"]
    k = stack_crossings(name)
    has_plane = any(kind == "plane" for kind, _ in STACK_CASES[name]["sheets"])
    for li, l in enumerate(sc.lights):
        if l["type"] == shade_ref.LIGHT_SUN:
            nd = np.broadcast_to(ray_ref.vnormalized(-l["v"]), hit.shape).astype(f32)
            dist = np.full(len(hit), np.inf, f32)
        else:
            diff = ray_ref.vsub(np.broadcast_to(l["v"], hit.shape), hit)
            nd, dist = ray_ref.vnormalized(ray_ref.vnormalized(diff)).astype(f32), ray_ref.vnorm(diff)
        seen = np.bincount(occluders(sc, hit, nd, dist, 1e-3), minlength=k + 1)
        print(f"{name}, light {li}: floor pixels per occluder count {seen.tolist()}")
        above = STACK_CASES[name].get("light_above")
        top = k if (above is None or l["type"] == shade_ref.LIGHT_SUN) else above
        if name == "close":
            # two sheets 5e-4 apart: the restart at last_hit + 1e-3 steps over the second one, as the reference's loop does
            assert seen[2] == 0 and seen[0] >= 20 and seen[1] >= 20
            assert np.bincount(occluders(sc, hit, nd, dist, 0.0), minlength=3)[2] >= 20, "without the step both are met"
            continue
        # an unbounded plane lies between every floor point and the lights: such a stack has no floor under 0 occluders
        for c in range(1 if has_plane else 0, top + 1):
            assert seen[c] >= 20, f"light {li}: {seen[c]} floor pixels under {c} occluders"
        assert not seen[top + 1:].any()


def test_the_threshold_values_arrive_as_the_floats_they_are(ca):
    for mode in THRESHOLD_MODES:
        for v in THRESHOLD_VALUES:
            m = parse(ca, threshold_room_json(mode, v)).desc.contents.materials[THRESHOLD_MATERIAL]
            for key, field in (("reflect", m.reflexivity), ("transparency", m.transparency)):
                want = f32(v) if mode in (key, "both") else f32(0.0)
                assert f32(field).view(np.uint32) == want.view(np.uint32), (mode, v, key)


@pytest.mark.parametrize("mode", THRESHOLD_MODES)
def test_the_flattened_facts_follow_exact_zero_and_the_double_comparison(ca, harness, tmp_path, mode):  # noqa: F811
    """all_opaque: every transparency exactly +-0; need_cold: the material both reflects and transmits, each (double)x >= 1e-6;
    any_bounce: the room's mirrors reflect, so always.  Without the mirrors: the material alone decides."""
    import json
    for v in THRESHOLD_VALUES:
        on = float(v) >= 1e-6
        assert on == (v in THRESHOLD_VALUES[4:8])
        flat, _ = run(harness, tmp_path, parse(ca, threshold_room_json(mode, v)))
        got = tuple(flat["scalars"][k] for k in ("all_opaque", "need_cold", "any_bounce"))
        assert got == (int(mode == "reflect" or v == 0), int(mode == "both" and on), 1), (mode, v, got)
        sc = json.loads(threshold_room_json(mode, v))
        sc["materials"][0]["reflect"] = 0.0
        flat, _ = run(harness, tmp_path, parse(ca, json.dumps(sc)))
        assert flat["scalars"]["any_bounce"] == int(on), (mode, v)


def test_a_sun_of_any_length_gives_one_frame(ca, tmp_path):
    frames = [oracle.oracle_render(parse(ca, lights_scene_json(tmp_path, n)), bounces=3) for n in LIGHT_SUN_LENGTH_CASES]
    for f in frames[1:]:
        for k in FRAME:
            assert same_bits(f[k], frames[0][k]), k


def test_the_restart_step_case_sits_on_the_rounding_of_the_restart(ca, tmp_path):
    """restart_step: under the vertical sun the second sheet is met within an ulp of the restart (float)((double)t1 + 1e-3); on a
    good part of the floor pixels the float sum t1 + 1e-3f is the neighbouring float and would decide the other way"""
    text, _ = stack_scene_json(tmp_path, "restart_step", "above")
    sc = shade_ref.ShadeScene(parse(ca, text))
    o, d = ray_ref.camera_rays(sc.cam)
    floor = ray_ref.ray_cast(sc, o, d, f32(1e-3), ignore_transparent=True)
    assert (floor["object"] == STACK_FLOOR).all()
    hit, up = floor["point"], np.broadcast_to(np.array([0, 1, 0], f32), (len(o), 3)).astype(f32)
    t1 = ray_ref.ray_cast(sc, hit, up, f32(1e-3))["t"]
    as_double, as_float = (t1.astype(np.float64) + 1e-3).astype(f32), t1 + f32(1e-3)
    t2 = ray_ref.ray_cast(sc, hit, up, np.nextafter(t1, f32(np.inf)))["t"]
    differ = (t2 > as_double) != (t2 > as_float)
    print(f"restart_step: the second sheet is seen by {int((t2 > as_double).sum())} of {len(o)} pixels; a float restart decides otherwise on {int(differ.sum())}")
    assert differ.sum() >= 20 and (t2 > as_double).sum() >= 20 and (~(t2 > as_double)).sum() >= 20


def test_the_flattened_scene_knows_where_the_fast_specular_path_stays_in_the_bar(ca, harness, tmp_path):  # noqa: F811
    """fast_pow_ok of the flattened scene against the rule restated in tests/util.py, on the phong family and on the shipped
    scenes; scene/bunny.json, the benchmark's, keeps the fast build"""
    from tests.conftest import load_scene
    seen = set()
    scenes = [(f"phong e={e:g} {l}", parse(ca, phong_scene_json(tmp_path, e, l))) for e in PHONG_EXPONENTS for l in PHONG_LIGHTS]
    scenes += [(n, load_scene(ca, n, 16, 16)) for n in ("bunny", "mirror", "sphere_plane", "triangle")]
    scenes += [(n, parse(ca, lights_scene_json(tmp_path, n))) for n in ("n0", "n33", "colours")]
    for name, s in scenes:
        flat, _ = run(harness, tmp_path, s)
        assert flat["scalars"]["fast_pow_ok"] == int(fast_pow_kept(s)), name
        seen.add(fast_pow_kept(s))
        if name == "bunny":
            assert fast_pow_kept(s), "the benchmark's scene would change its build"
    assert fast_pow_kept(parse(ca, phong_scene_json(tmp_path, 0.0, "sun"))) and fast_pow_kept(parse(ca, lights_scene_json(tmp_path, "n0")))
