"""The phased builds of the render kernel (cutrace_amd/csrc/kernel_choice.h phased_build, render_kernel.hip "Phased builds",
render_trip.h; DESIGN.md "Phased opaque builds"): an opaque build is launched as its phased twin, in which the kind of a trip
— a radiance trip, or the shadow trip towards light k — is one scalar of the wave and a radiance trip and a shadow trip are code
of their own.  Every trip, every cast and the arithmetic of every taken path stay what they are, so every case renders with two
handles of the same kind — A created normally, B under CUTRACE_NO_PHASE_SPLIT=1 (read when a handle is created: the opaque
build as it is without the twin) — and compares depth, normal and colour BITWISE, the ray count and the counters, the build,
the shape and the opaque build, and reads back which instantiation ran (last_phased: 1 for A, 0 for B).

Frames are 64 x 40 and 64 x 48 (8 x 5 and 8 x 6 tiles), as in tests/test_gpu_opaque_build.py, and 52 x 27, whose edge tiles
hold lanes outside the image — lanes that are inactive from the first trip on.  The invariant the builds rest on is checked on
the CPU (tests/test_phase_cpu.py) and, with the counter the statistics build has had all along, on the device: no trip of an
all-opaque scene mixes kinds, and a scene with a transparent material has trips that do."""
import json

import numpy as np
import pytest

import oracle
from tests.conftest import load_scene
from tests.gpu_support import LIGHTS_IN, RIGHT, assert_same_frame, camera_of, env, gpu, held, octahedra, room  # noqa: F401  (gpu: the fixture)
from tests.live import desc_lights
from tests.util import assert_parity, parse

pytestmark = pytest.mark.gpu

f32 = np.float32
# scene_device.h KV_*: the default variant, with or without the 6-wave build (64), with or without host delivery (128)
DEFAULT = 1 | 2 | 8 | 32
W, H = 64, 40


def handles(ca, s):
    a = ca.DeviceScene(s)
    with env("CUTRACE_NO_PHASE_SPLIT"):
        b = ca.DeviceScene(s)
    return a, b


def compare(a, b, what, render, kernel=None, counters=True):
    """`render` on A and on B: the same frame, ray count, counters, build, shape and opaque build; A phased, B not.  A's frame."""
    got = held(render(a))
    got_words = a.last_counters().copy()
    ref = held(render(b))
    ref_words = b.last_counters().copy()
    assert_same_frame(got, ref, f"{what}: phase split on / off")
    for k in ("max_depth", "rows"):
        if k in ref:
            assert got[k] == ref[k], (what, k, got[k], ref[k])
    if counters:   # (host-form renders: the 16 counter words of the launch; device-form ones bring their own)
        assert (got_words == ref_words).all(), (what, got_words, ref_words)
    assert got.get("words") == ref.get("words"), (what, got.get("words"), ref.get("words"))
    assert (a.last_kernel(), a.last_shape(), a.last_opaque()) == (b.last_kernel(), b.last_shape(), b.last_opaque()), what
    assert (a.last_phased(), b.last_phased()) == (1, 0), (what, hex(a.last_kernel()), a.last_shape(), a.last_opaque())
    assert a.last_opaque() == 1 and a.last_shape() == 1 and a.last_kernel() & 2, (what, hex(a.last_kernel()))
    if kernel is not None:
        assert a.last_kernel() == kernel, (what, hex(a.last_kernel()))
    return got


def a_against_b(ca, s, what, render, **kw):
    a, b = handles(ca, s)
    try:
        return compare(a, b, what, render, **kw)
    finally:
        a.close()
        b.close()


# ---- the scenes: every one all-opaque, one mesh, planes ----
SUNS_AND_POINTS = [{"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.5, 0.5, 0.4]},
                   {"type": "point", "point": [0.5, 0.8, 1.5], "color": [0.6, 0.6, 0.6]},
                   # below the floor's level and behind the mesh as the camera sees it: dark for the faces that look away
                   {"type": "point", "point": [0.9, -0.9, -0.9], "color": [0.3, 0.4, 0.3]},
                   {"type": "sun", "direction": [0.4, 0.2, 1.0], "color": [0.2, 0.2, 0.3]}]


def many_lights(n):
    rng = np.random.default_rng(n)
    out = []
    for k in range(n):
        c = [float(x) for x in rng.uniform(0.02, 0.08, 3)]
        if k % 3 == 1:
            out.append({"type": "sun", "direction": [float(x) for x in rng.uniform(-1, 1, 3)], "color": c})
        else:
            out.append({"type": "point", "point": [float(x) for x in rng.uniform(-0.9, 0.9, 3)], "color": c})
    return out


def edited_room(tmp_path, name, change=None, **kw):
    text = json.loads(room(tmp_path, name, [octahedra(RIGHT)], **kw)[0])
    if change:
        change(text)
    return text


def mat(i, **kw):
    def change(text):
        text["materials"][i].update(kw)
    return change


REFLECT_EDGE = float(f32(1e-6))                       # as a double below 1e-6: the material does not reflect
REFLECT_NEXT = float(np.nextafter(f32(1e-6), f32(1)))  # the next float up: it does
ROOMS = {
    "open room": dict(),                                              # open towards the camera: reflections escape
    "a wall that does not reflect": dict(change=mat(2, reflect=0.0)),   # (walls 1 and 3)
    "mesh reflect 0": dict(change=mat(0, reflect=0.0)),
    "mesh reflect f32(1e-6)": dict(change=mat(0, reflect=REFLECT_EDGE)),
    "mesh reflect next float up": dict(change=mat(0, reflect=REFLECT_NEXT)),
    "no light": dict(lights=[]),
    "one light": dict(lights=LIGHTS_IN[:1]),
    "four lights, suns and points": dict(lights=SUNS_AND_POINTS),
    "33 lights": dict(lights=many_lights(33)),
    "52 x 27": dict(w=52, h=27),
}


def room_scene(ca, tmp_path, name):
    return parse(ca, edited_room(tmp_path, name.replace(" ", "_"), **ROOMS[name]))


@pytest.fixture(scope="module")
def bunny(gpu):
    """the flagship room at 64 x 40: walls, mesh silhouettes and reflections of the mesh in the walls"""
    s = load_scene(gpu, "bunny", W, H)
    a, b = handles(gpu, s)
    yield s, a, b
    a.close()
    b.close()


# ---- the flagship room ----
@pytest.mark.parametrize("bounces,kernel", [(0, DEFAULT | 64), (1, DEFAULT | 64), (5, DEFAULT | 64), (6, DEFAULT), (15, DEFAULT)])
def test_bunny_room(bunny, bounces, kernel):
    """bounces 5: the headline launch, the 6-wave build; 0: no frame is ever pushed; 6: the chooser's 5-wave build; 15: the
    deepest recursion there is"""
    _, a, b = bunny
    compare(a, b, f"bunny bounces {bounces}", lambda ds: ds.render(bounces=bounces), kernel=kernel)


def test_bunny_room_into_page_locked_buffers(bunny):
    """host delivery: the KV_HOSTOUT twin of the 6-wave build; the same frame as through pageable buffers"""
    _, a, b = bunny
    pinned = compare(a, b, "bunny, page-locked", lambda ds: ds.render(bounces=5, pinned=True), kernel=DEFAULT | 64 | 128)
    pageable = compare(a, b, "bunny, pageable", lambda ds: ds.render(bounces=5), kernel=DEFAULT | 64)
    assert_same_frame(pinned, pageable, "bunny: page-locked / pageable")


def test_bunny_room_with_lanes_outside_the_image(gpu):
    """52 x 27: 7 x 4 tiles, the last column 4 pixels wide and the last row 3 high"""
    s = load_scene(gpu, "bunny", 52, 27)
    for bounces in (5, 6):
        a_against_b(gpu, s, f"bunny 52 x 27, bounces {bounces}", lambda ds: ds.render(bounces=bounces))


def test_default_build_against_the_oracle(bunny):
    """the launch every caller gets: depth, normal and ray count bit for bit, the colour within the parity bar"""
    s, a, _ = bunny
    got = held(a.render(bounces=5))
    assert a.last_phased() == 1 and a.last_opaque() == 1 and a.last_kernel() == DEFAULT | 64
    want = oracle.oracle_render(s, fudge=1e-3, bounces=5, threads=4)
    assert_parity(got, want, what="bunny 64x40 b5: phased build / oracle")
    assert got["ray_count"] == want["ray_count"]


# ---- lanes that end at different times; light count and type ----
@pytest.mark.parametrize("name", list(ROOMS))
def test_rooms(gpu, tmp_path, name):
    s = room_scene(gpu, tmp_path, name)
    a, b = handles(gpu, s)
    try:
        for bounces in (3, 6):
            compare(a, b, f"{name}, bounces {bounces}", lambda ds: ds.render(bounces=bounces), kernel=DEFAULT)
        compare(a, b, f"{name}, page-locked", lambda ds: ds.render(bounces=3, pinned=True), kernel=DEFAULT | 128)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["four lights, suns and points", "33 lights", "no light"])
def test_lights_with_room_facts_and_without(gpu, tmp_path, name):
    """the same launches with the room facts in the scene head (shadow trips from inside the room skip their plane tests) and,
    under CUTRACE_NO_WALL_SKIP=1, without: the ROOM twins of the builds.  One light of the mixed four is dark for the faces of
    the mesh that look away from it (the statistics build counts such pairs below)."""
    s = room_scene(gpu, tmp_path, name)
    a, b = handles(gpu, s)
    try:
        with_facts = compare(a, b, f"{name}, room facts", lambda ds: ds.render(bounces=3))
        if name == "four lights, suns and points":   # its first point light is well inside the walls: the ROOM twins ran
            assert a.room_facts()["lights"] != 0 and b.room_facts()["lights"] != 0, (name, a.room_facts())
    finally:
        a.close()
        b.close()
    with env("CUTRACE_NO_WALL_SKIP"):
        a, b = handles(gpu, s)
    try:
        without = compare(a, b, f"{name}, no wall skip", lambda ds: ds.render(bounces=3))
        assert a.room_facts()["lights"] == 0
        if name == "four lights, suns and points":
            assert (a.dark_skip(), b.dark_skip()) == (1, 1)   # the DARK twins: one of the four is dark for part of the mesh
    finally:
        a.close()
        b.close()
    assert_same_frame(with_facts, without, f"{name}: room facts / none")


# ---- every way into these builds ----
def device_frame(ds, w, n_rows, n_frames, call):
    import torch
    dev = torch.device("cuda:0")
    px = n_frames * n_rows * w
    depth = torch.zeros(px, dtype=torch.float32, device=dev)
    color = torch.zeros(3 * px, dtype=torch.float32, device=dev)
    normal = torch.zeros(3 * px, dtype=torch.float32, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    call(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), counters.data_ptr())
    torch.cuda.synchronize()
    words = counters.cpu().numpy()
    return dict(depth=depth.cpu().numpy(), color=color.cpu().numpy(), normal=normal.cpu().numpy(), ray_count=int(words[0]),
                words=[int(x) for x in words])


def test_render_device(gpu, bunny):
    s, a, b = bunny

    def call(ds):
        return device_frame(ds, W, H, 1, lambda d, c, n, k: ds.render_device(d, c, n, d_counters=k, bounces=5))

    got = compare(a, b, "render_device", call, kernel=DEFAULT | 64, counters=False)
    host = held(a.render(bounces=5))
    assert (got["depth"].view(np.uint32) == host["depth"].reshape(-1).view(np.uint32)).all() and got["ray_count"] == host["ray_count"]


def test_batch_of_two_frames_with_part_stride(gpu, tmp_path):
    """render_device_batch: two cameras in one launch, the part rotating from frame to frame (part_stride 1)"""
    s = parse(gpu, room(tmp_path, "batch", [octahedra(RIGHT)])[0])
    cams = [camera_of(gpu, s), camera_of(gpu, parse(gpu, room(tmp_path, "batch2", [octahedra(RIGHT)], eye=(-0.4, 0.3, 2.6))[0]))]
    w, h, n_rows, part = 64, 48, 24, 0   # 48 rows in 8-row blocks, 2 parts: 24 rows each

    def batch(ds):
        ds.set_cameras(cams)
        return device_frame(ds, w, n_rows, 2, lambda d, c, n, k: ds.render_device_batch(
            d, c, n, n_frames=2, frame_stride_px=n_rows * w, d_counters=k, bounces=3, rows=(0, h, 8, part, 2), part_stride=1))

    got = a_against_b(gpu, s, "batch of two frames", batch, kernel=DEFAULT, counters=False)
    assert got["ray_count"] > 2 * n_rows * w and np.isfinite(got["depth"]).all()


def test_lights_then_a_material_edited_on_a_live_handle(gpu, tmp_path):
    """set_lights (two lights become the mixed four: the phase rule's n_light changes), then set_material (the mesh stops
    reflecting): each frame is a fresh handle's on the edited scene, which in turn is held against its unsplit twin"""
    before = edited_room(tmp_path, "live0")
    after = edited_room(tmp_path, "live1", lights=SUNS_AND_POINTS)
    final = edited_room(tmp_path, "live2", lights=SUNS_AND_POINTS, change=mat(0, reflect=0.0))
    ds = gpu.DeviceScene(parse(gpu, before))
    try:
        ds.render(bounces=4)
        assert ds.last_phased() == 1
        after_scene = parse(gpu, after)   # (kept: desc_lights returns views of its records)
        steps = (("lights", lambda: ds.set_lights([gpu.Light.from_buffer_copy(l) for l in desc_lights(after_scene)]), after_scene),
                 ("material", lambda: ds.set_material(0, reflexivity=0.0), parse(gpu, final)))
        for what, edit, edited in steps:
            edit()
            got = held(ds.render(bounces=4))
            a, b = handles(gpu, edited)
            try:
                want = compare(a, b, f"{what}: fresh handles", lambda h: h.render(bounces=4), kernel=DEFAULT)
                assert_same_frame(got, want, f"{what}: edited / fresh handle")
                assert (ds.last_kernel(), ds.last_shape(), ds.last_opaque(), ds.last_phased()) == (a.last_kernel(), 1, 1, 1), what
            finally:
                a.close()
                b.close()
    finally:
        ds.close()


# ---- scenes the phased builds are not for ----
def test_launches_that_are_no_opaque_build_are_not_phased(gpu, tmp_path):
    s = parse(gpu, room(tmp_path, "sph", [octahedra(RIGHT)], sphere=True)[0])
    ds = gpu.DeviceScene(s)
    try:
        ds.render(bounces=3)
        assert (ds.last_shape(), ds.last_opaque(), ds.last_phased()) == (0, 0, 0)
    finally:
        ds.close()
    with env("CUTRACE_NO_OPAQUE_BUILD"):
        ds = gpu.DeviceScene(parse(gpu, room(tmp_path, "noopq", [octahedra(RIGHT)])[0]))
    try:
        ds.render(bounces=3)
        assert (ds.last_shape(), ds.last_opaque(), ds.last_phased()) == (1, 0, 0)
    finally:
        ds.close()


# ---- the invariant on the device ----
def mixing(gpu, s, bounces):
    ds = gpu.DeviceScene(s)
    try:
        ds.set_variant(gpu.VAR_STATS)
        gpu.DeviceScene.lane_stats(reset=True)
        ds.render(bounces=bounces)
        assert ds.last_phased() == 0 and ds.last_opaque() == 0
        return gpu.DeviceScene.lane_stats(reset=True)
    finally:
        ds.close()


def test_no_trip_of_an_all_opaque_scene_mixes_kinds(gpu, bunny, tmp_path):
    """the statistics build counts the trips whose live lanes cast for more than one (kind, depth): none in any scene above"""
    scenes = [("bunny", bunny[0]), ("bunny 52 x 27", load_scene(gpu, "bunny", 52, 27))] + [(n, room_scene(gpu, tmp_path, n)) for n in ROOMS]
    dark_pairs = {}
    for name, s in scenes:
        for bounces in (5, 15):
            st = mixing(gpu, s, bounces)
            assert st["wave_trips"] > 0 and st["trips_mixing_kinds"] == 0, (name, bounces, st["trips_mixing_kinds"], st["wave_trips"])
            dark_pairs[name] = st["dark_lights"]["lane_light_pairs"]
    assert dark_pairs["four lights, suns and points"] > 0, dark_pairs   # a light that is dark for part of the mesh


def test_the_counter_sees_a_mixed_trip_where_a_material_transmits(gpu):
    st = mixing(gpu, load_scene(gpu, "sphere_plane", W, H), 5)
    assert st["trips_mixing_kinds"] > 0, st
