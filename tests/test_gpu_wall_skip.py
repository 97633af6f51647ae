"""Shadow trips that skip their plane tests (render_kernel.hip "room-safe lanes"; the room facts of scene_flatten.cpp, DESIGN.md
"Shadow casts from inside a plane room").  The skip removes only tests whose outcome the facts fix beforehand, so every case
renders with two handles — A created normally, B under CUTRACE_NO_WALL_SKIP=1 (read when a handle is created: zero facts) — and
compares depth, colour, normal BITWISE and the ray count; live edits are compared with a fresh handle as well.  Against the
oracle: the default variant — the launch that skips: the code exists only in the one-mesh builds launched with room facts and in
the any-hit statistics builds — within the parity bar (its specular term is the fast one; depth, normal and the ray count bit for
bit), and the VAR_EXACT_POW launch, a general build that carries no facts, bit for bit in all three buffers with the oracle whose
pow is rounded once (tests/util.py).  Frames are 64 x 48 at bounces 3."""
import json

import numpy as np
import pytest

import oracle
from cutrace_amd import _lib
from tests.conftest import load_scene
from tests.gpu_support import LIGHTS_IN, RIGHT, assert_same_frame, env, gpu, held, octahedra, room  # noqa: F401  (gpu: the fixture)
from tests.util import assert_parity, parse

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 64, 48
BOUNCES = 3


def handles(ca, s, variant=0):
    a = ca.DeviceScene(s)
    with env("CUTRACE_NO_WALL_SKIP"):
        b = ca.DeviceScene(s)
    a.set_variant(variant)
    b.set_variant(variant)
    return a, b


def no_facts(f):
    return not f["c"].any() and f["r"] == 0.0 and f["delta"] == 0.0 and f["lights"] == 0


def skipped(ca, s, render):
    """(any-hit shadow trips, those that skipped their plane tests) of `render` on a VAR_STATS handle, and its frame"""
    ds = ca.DeviceScene(s)
    ds.set_variant(ca.VAR_STATS)
    ca.DeviceScene.lane_stats(reset=True)
    got = held(render(ds))
    st = ca.DeviceScene.lane_stats(reset=True)
    ds.close()
    return st["anyhit_shadow_trips"], st["anyhit_shadow_trips_without_planes"], got


def against_the_oracle(ca, s, got, what, anyhit=True):
    want = oracle.oracle_render(s, fudge=1e-3, bounces=BOUNCES, threads=4)
    assert_parity(got, want, what=f"{what}: default variant / oracle")
    assert got["ray_count"] == want["ray_count"], what
    once = oracle.oracle_render(s, fudge=1e-3, bounces=BOUNCES, threads=4, pow_rounded_once=True)
    a, b = handles(ca, s, ca.VAR_EXACT_POW)
    try:
        e = held(a.render(bounces=BOUNCES))
        assert bool(a.last_kernel() & 2) == anyhit and not a.last_kernel() & 32, hex(a.last_kernel())   # any-hit or not; exact pow
        assert_same_frame(e, once, f"{what}: exact pow / oracle with the pow rounded once")
        assert_same_frame(e, held(b.render(bounces=BOUNCES)), f"{what}: exact pow, skip on / off")
    finally:
        a.close()
        b.close()


def a_against_b(ca, s, what, render=lambda ds: ds.render(bounces=BOUNCES), with_oracle=True, variant=0, anyhit=True):
    """`render` on A and B: the same frame; B carries no facts.  Returns A's frame and A's room facts."""
    a, b = handles(ca, s, variant)
    try:
        got, ref = held(render(a)), held(render(b))
        assert_same_frame(got, ref, f"{what}: skip on / off")
        assert a.last_kernel() == b.last_kernel(), what
        facts = a.room_facts()
        assert no_facts(b.room_facts()), what
    finally:
        a.close()
        b.close()
    if with_oracle:
        against_the_oracle(ca, s, got, what, anyhit)
    return got, facts


def the_room(ca, tmp_path, name, lights=LIGHTS_IN, **kw):
    return parse(ca, room(tmp_path, name, [octahedra(RIGHT)], lights=lights, **kw)[0])


def point(x, y, z, c=0.5):
    return {"type": "point", "point": [float(x), float(y), float(z)], "color": [c, c, c]}


# 1
def test_bunny_room(gpu):
    s = load_scene(gpu, "bunny", W, H)
    _, facts = a_against_b(gpu, s, "bunny")
    assert facts["lights"] == 0xF and facts["delta"] >= 2e-6 and facts["r"] > 0, facts
    trips, without, got = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))
    assert trips > 0 and without > 0, (trips, without)
    print(f"bunny {W}x{H} b{BOUNCES}: {without} of {trips} any-hit shadow trips skipped their plane tests")
    plain, _ = a_against_b(gpu, s, "bunny", with_oracle=False)
    assert_same_frame(got, plain, "VAR_STATS / default")


def test_octahedra_room(gpu, tmp_path):
    s = the_room(gpu, tmp_path, "plain")
    _, facts = a_against_b(gpu, s, "room")
    assert facts["lights"] == 0b11, facts
    trips, without, _ = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))
    assert 0 < without <= trips


# 2
def test_one_light_just_outside_a_wall(gpu, tmp_path):
    s = the_room(gpu, tmp_path, "outside", lights=LIGHTS_IN + [point(-1.001, 0.2, 0.5)])
    _, facts = a_against_b(gpu, s, "a light 1e-3 outside the wall x = -1")
    assert facts["lights"] == 0b011, facts


# 3
def test_a_light_at_the_margin(gpu, tmp_path):
    """the smallest float32 distance from the wall x = -1 at which the light keeps its bit, found by bisection on the facts of
    a live handle; three ulp nearer the bit is clear, three ulp farther it is set, and both frames are the oracle's"""
    def lights_at(x):
        return [_lib.Light(1, _lib.Vec3(float(x), 0.2, 0.5), _lib.Vec3(0.5, 0.5, 0.5))]

    ds = gpu.DeviceScene(the_room(gpu, tmp_path, "margin0", lights=[point(-0.5, 0.2, 0.5)]))

    def has_bit(x):
        ds.set_lights(lights_at(x))
        ds.render(bounces=0)
        return ds.room_facts()["lights"] == 1

    lo, hi = f32(-1.0), f32(-0.5)   # no bit on the wall, a bit half a unit inside
    assert not has_bit(lo) and has_bit(hi)
    while np.nextafter(lo, f32(0)) != hi:
        mid = f32(0.5 * (np.float64(lo) + np.float64(hi)))
        lo, hi = (lo, mid) if has_bit(mid) else (mid, hi)
    ds.close()
    assert 0 < hi + 1.0 < 1e-3, hi   # the margin is a small multiple of the float spacing of the room, far below a light's usual distance

    def ulps(x, k):
        for _ in range(abs(k)):
            x = np.nextafter(x, f32(1) if k > 0 else f32(-2))
        return x

    for k, bit in ((3, 1), (-3, 0)):
        s = the_room(gpu, tmp_path, f"margin{k}", lights=[point(ulps(hi, k), 0.2, 0.5)])
        _, facts = a_against_b(gpu, s, f"light {k:+d} ulp from the margin")
        assert facts["lights"] == bit, (k, facts)


# 4
def test_an_oblique_plane_clears_the_facts(gpu, tmp_path):
    text = json.loads(room(tmp_path, "oblique", [octahedra(RIGHT)])[0])
    text["objects"].append({"type": "plane", "point": [0, -0.95, 0], "normal": [0.1, 1.0, 0.05], "material": 1})
    s = parse(gpu, json.dumps(text))
    _, facts = a_against_b(gpu, s, "room + oblique plane")
    assert no_facts(facts), facts
    trips, without, _ = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))
    assert trips > 0 and without == 0


# 5
def test_looking_out_of_the_open_side(gpu, tmp_path):
    """the eye stands at the back wall and looks out through the open side: reflected rays leave the room, some hit nothing,
    some meet a wall's plane far outside the origin box — those hit points fail the box test and cast with the plane tests"""
    text = json.loads(room(tmp_path, "out", [octahedra(RIGHT)], eye=(0.0, 0.0, -0.8))[0])
    text["camera"]["look"] = [0.15, -0.1, 1.0]
    for m in text["materials"]:
        m["reflect"] = 0.6
    s = parse(gpu, json.dumps(text))
    got, facts = a_against_b(gpu, s, "looking out")
    assert facts["lights"] == 0b11
    far = np.isfinite(got["depth"]) & (got["depth"] > 4 * facts["r"])
    assert np.isinf(got["depth"]).any() or far.any(), "some primary rays were meant to leave the room"
    trips, without, _ = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))
    assert 0 < without < trips


# 6
@pytest.mark.parametrize("scale,offset", [(1e-3, 0.0), (1e3, 0.0), (1.0, 1e4)], ids=["x1e-3", "x1e3", "+1e4"])
def test_scaled_and_offset_rooms(gpu, tmp_path, scale, offset):
    text = json.loads(room(tmp_path, "scaled", [octahedra(RIGHT)])[0])
    off = np.array([offset, -0.75 * offset, 0.5 * offset])

    def move(p):
        return [float(v) for v in (np.asarray(p, np.float64) * scale + off).astype(f32)]

    from cutrace_amd import scenes
    path = str(tmp_path / "scaled_mesh.stl")
    scenes.write_stl(path, (octahedra(RIGHT).astype(np.float64) * scale + off).astype(f32))
    for o in text["objects"]:
        if o["type"] == "mesh":
            o["file"] = path
        else:
            o["point"] = move(o["point"])
    for light in text["lights"]:
        light["point"] = move(light["point"])
    text["camera"]["eye"] = move(text["camera"]["eye"])
    s = parse(gpu, json.dumps(text))
    _, facts = a_against_b(gpu, s, f"room x {scale} + {offset}")
    assert facts["lights"] == 0b11 and facts["delta"] > 0, facts
    assert 1.9 * scale <= facts["r"] <= 8 * scale, facts   # the box follows the room


def test_a_sphere_takes_the_general_build_without_the_skip(gpu, tmp_path):
    """not a one-mesh launch: the general any-hit build, which has no code for the facts, so the launch carries none"""
    s = the_room(gpu, tmp_path, "sphere", sphere=True)
    a = gpu.DeviceScene(s)
    a.render(bounces=BOUNCES)
    assert a.last_kernel() & 2 and a.last_shape() == 0 and no_facts(a.room_facts()), hex(a.last_kernel())
    a.close()
    a_against_b(gpu, s, "room + sphere")
    trips, without, _ = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))   # (the statistics build does skip, in any shape)
    assert 0 < without <= trips


# 7
def test_a_transparent_material_takes_a_build_without_the_skip(gpu, tmp_path):
    s = the_room(gpu, tmp_path, "transparent", transparent=True)   # material 2, which two of the walls have
    a = gpu.DeviceScene(s)
    a.render(bounces=BOUNCES)
    assert not a.last_kernel() & 2 and no_facts(a.room_facts()), hex(a.last_kernel())
    a.close()
    a_against_b(gpu, s, "a transparent wall material", anyhit=False)
    trips, without, _ = skipped(gpu, s, lambda ds: ds.render(bounces=BOUNCES))
    assert trips == 0 and without == 0   # (the counters are the any-hit builds')


# 8
def test_live_edits_equal_a_fresh_handle(gpu, tmp_path):
    """a light across a wall and back, a wall moved inwards past a light, a material made transparent and opaque again: after
    every edit the frame and the facts are a fresh handle's on the edited scene"""
    inside, outside = point(-0.6, 0.7, 1.0), point(-1.3, 0.7, 1.0)
    base = dict(lights=[point(0.5, 0.8, 1.5), inside])
    steps = [("light outside", dict(lights=[base["lights"][0], outside])),
             ("light back", base),
             ("floor above a light", dict(base, floor_y=0.75)),      # the light at y = 0.7 is now under the floor
             ("floor back", base),
             ("transparent", dict(base, transparent=True)),
             ("opaque again", base)]
    ds = gpu.DeviceScene(the_room(gpu, tmp_path, "live0", **base))
    ds.render(bounces=BOUNCES)
    assert ds.room_facts()["lights"] == 0b11
    floor = 1 + 4   # room(): the mesh, then the five walls, the floor last
    seen = []
    for k, (what, kw) in enumerate(steps):
        edited = the_room(gpu, tmp_path, f"live{k + 1}", **kw)   # (transparent=True: material 2, which two of the walls have)
        ds.set_lights([_lib.Light(1, _lib.Vec3(*l["point"]), _lib.Vec3(*l["color"])) for l in kw["lights"]])
        ds.set_object(floor, point=(0.0, kw.get("floor_y", -1.0), 0.0))
        ds.set_material(2, transparency=0.5 if kw.get("transparent") else 0.0)
        got = held(ds.render(bounces=BOUNCES))
        fresh = gpu.DeviceScene(edited)
        want = held(fresh.render(bounces=BOUNCES))
        assert_same_frame(got, want, f"{what}: edited / fresh handle")
        f_live, f_fresh = ds.room_facts(), fresh.room_facts()
        assert ds.last_kernel() == fresh.last_kernel(), what
        fresh.close()
        assert np.array_equal(f_live["c"], f_fresh["c"]) and (f_live["r"], f_live["delta"], f_live["lights"]) == (f_fresh["r"], f_fresh["delta"], f_fresh["lights"]), (what, f_live, f_fresh)
        with env("CUTRACE_NO_WALL_SKIP"):
            off = gpu.DeviceScene(edited)
        assert_same_frame(got, held(off.render(bounces=BOUNCES)), f"{what}: edited / fresh handle without the skip")
        off.close()
        seen.append(f_live["lights"])
    ds.close()
    assert seen == [0b01, 0b11, 0b01, 0b11, 0, 0b11], seen


# 9
def test_supersampled_lens_and_host_delivery_launches(gpu):
    import torch
    from cutrace_amd import lenses
    s = load_scene(gpu, "bunny", W, H)
    plain, _ = a_against_b(gpu, s, "bunny", with_oracle=False)
    a_against_b(gpu, s, "2 x 2 samples", lambda ds: ds.render(bounces=BOUNCES, samples=2), with_oracle=False)
    pinned, _ = a_against_b(gpu, s, "page-locked buffers", lambda ds: ds.render(bounces=BOUNCES, pinned=True), with_oracle=False)
    assert_same_frame(pinned, plain, "host delivery / plain")
    o, d = lenses.pinhole(s.desc.contents.cam, W, H)

    def lens(ds):
        r = ds.render_lens(o, d, bounces=BOUNCES)
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}

    got, _ = a_against_b(gpu, s, "pinhole lens", lens, with_oracle=False)
    assert_same_frame(got, plain, "lens / plain")
