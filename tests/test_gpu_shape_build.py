"""The one-mesh launch shape of the render kernel (cutrace_amd/csrc/kernel_choice.h KS_ONE_MESH, launch_shape): on a scene of one
mesh, planes and nothing else, the default variant's launches run render_kernel<KV, 1>, from which the object loop and the
top-level walk are compiled out.  Only code that such a scene never runs is removed, so every case renders with two handles —
A created normally, B under CUTRACE_NO_SHAPE_BUILD=1 (read when a handle is created: shape 0) — and compares depth, colour
and normal BITWISE, the ray count and the build (last_kernel), and reads the shape back (last_shape: 1 for A, 0 for B).
Scenes and variants the shape is not for must report shape 0 on both.  Frames are 96 x 54 or smaller."""

import numpy as np
import pytest

from tests.conftest import load_scene
from tests.gpu_support import LIGHTS_IN, RIGHT, assert_same_frame, camera_of, env, gpu, held, octahedra, room  # noqa: F401  (gpu: the fixture)
from tests.live import desc_tris
from tests.util import _coplanar_scene, parse

pytestmark = pytest.mark.gpu

f32 = np.float32
# scene_device.h KV_*: the default variant, with or without the 6-wave build (64), with or without host delivery (128)
DEFAULT = 1 | 2 | 8 | 32
ONE_MESH_BUILDS = {DEFAULT, DEFAULT | 64, DEFAULT | 128, DEFAULT | 64 | 128}
W, H = 64, 48
LIGHT_BEHIND_WALL = {"type": "point", "point": [-3.0, 0.2, 0.5], "color": [0.7, 0.7, 0.7]}   # the wall x = -1 lies between it and the room


def handles(ca, s, variant=0):
    a = ca.DeviceScene(s)
    with env("CUTRACE_NO_SHAPE_BUILD"):
        b = ca.DeviceScene(s)
    a.set_variant(variant)
    b.set_variant(variant)
    return a, b


def a_against_b(ca, s, what, render, shape=1, variant=0):
    """`render` on A and on B: the same frame, the same build; A in `shape`, B in shape 0.  Returns A's frame."""
    a, b = handles(ca, s, variant)
    try:
        got, ref = held(render(a)), held(render(b))
        assert_same_frame(got, ref, f"{what}: shape build on / off")
        assert a.last_kernel() == b.last_kernel(), what
        assert (a.last_shape(), b.last_shape()) == (shape, 0), (what, hex(a.last_kernel()))
        if shape:
            assert a.last_kernel() in ONE_MESH_BUILDS, (what, hex(a.last_kernel()))
    finally:
        a.close()
        b.close()
    return got


# ---- the flagship scene ----
@pytest.mark.parametrize("bounces", [0, 1, 5])
@pytest.mark.parametrize("size", [(96, 54), (37, 21)], ids=["96x54", "37x21"])
def test_bunny(gpu, size, bounces):
    """whole tiles and a few rows over; partial tiles in both directions"""
    a_against_b(gpu, load_scene(gpu, "bunny", *size), f"bunny {size} bounces {bounces}", lambda ds: ds.render(bounces=bounces))


def test_bunny_five_wave_build(gpu):
    """VAR_NO_OCC6 keeps the default variant's 5-wave build: one of the four, so the shape applies"""
    a = a_against_b(gpu, load_scene(gpu, "bunny", 96, 54), "bunny, no 6-wave build", lambda ds: ds.render(bounces=5), variant=gpu.VAR_NO_OCC6)
    b = a_against_b(gpu, load_scene(gpu, "bunny", 96, 54), "bunny", lambda ds: ds.render(bounces=5))
    assert_same_frame(a, b, "5-wave / 6-wave build")


# ---- tiles that exercise the paths the shape touches ----
def test_tiles_that_only_see_walls(gpu, tmp_path):
    """the mesh fills part of the right half: in the first trip of every tile of the leftmost columns no lane's ray passes the
    mesh's box, so the wave leaves the mesh code at `bb_m == 0` — and the loop that is no loop any more must end there"""
    text, _, _ = room(tmp_path, "walls", [octahedra(RIGHT)])
    got = a_against_b(gpu, parse(gpu, text), "walls-only tiles", lambda ds: ds.render(bounces=3))
    axis = (got["normal"] != 0).sum(-1) == 1                                  # a wall's normal has one component
    assert axis[:, :16].all(), "the two leftmost tile columns were meant to see walls only"
    assert not axis.all() and np.isfinite(got["depth"]).all(), "the mesh was meant to be in the frame"


def test_shadow_trip_that_ends_at_the_planes(gpu, tmp_path):
    """the first light stands behind a wall: every shadow ray towards it meets that wall, so in the trip that casts them all
    lanes retire at the planes (`alive_m == 0`) and the wave never reaches the mesh"""
    text, _, _ = room(tmp_path, "behind", [octahedra(RIGHT)], lights=[LIGHT_BEHIND_WALL] + LIGHTS_IN)
    a_against_b(gpu, parse(gpu, text), "light behind a wall", lambda ds: ds.render(bounces=2))
    text, _, _ = room(tmp_path, "behind_only", [octahedra(RIGHT)], lights=[LIGHT_BEHIND_WALL])
    a_against_b(gpu, parse(gpu, text), "only the light behind a wall", lambda ds: ds.render(bounces=0))


def test_mesh_with_guard_records(gpu, tmp_path):
    """the coplanar mesh of the parity tests (an eye and a light in its triangles' plane): the walk starts at the mesh's extra
    guard node, whose index the head's record carries; 12 triangles, so the 5-wave build"""
    s = _coplanar_scene(gpu, tmp_path, W, H, row=20, n_tris=12, seed=5)
    ds = gpu.DeviceScene(s)
    guards, linear = ds.guard_state(0)
    ds.close()
    assert guards or linear, "the mesh was meant to have guard records"
    a_against_b(gpu, s, "guarded mesh", lambda ds: ds.render(bounces=4))


# ---- the other ways into the kernel ----
def test_rows_in_two_parts(gpu):
    """8-row blocks dealt to 2 parts (54 rows: 30 and 24)"""
    for part in (0, 1):
        a_against_b(gpu, load_scene(gpu, "bunny", 96, 54), f"part {part} of 2", lambda ds: ds.render(bounces=3, rows=(0, 54, 8, part, 2)))


def test_batch_of_two_frames_with_part_stride(gpu, tmp_path):
    """render_device_batch: two cameras in one launch, the part rotating from frame to frame (part_stride 1)"""
    import torch
    s = parse(gpu, room(tmp_path, "batch", [octahedra(RIGHT)])[0])
    cams = [camera_of(gpu, s), camera_of(gpu, parse(gpu, room(tmp_path, "batch2", [octahedra(RIGHT)], eye=(-0.4, 0.3, 2.6))[0]))]
    dev = torch.device("cuda:0")
    n_rows = 24   # 48 rows in 8-row blocks, 2 parts: 24 rows each

    def batch(ds):
        ds.set_cameras(cams)
        px = 2 * n_rows * W
        depth = torch.zeros(px, dtype=torch.float32, device=dev)
        color = torch.zeros(3 * px, dtype=torch.float32, device=dev)
        normal = torch.zeros(3 * px, dtype=torch.float32, device=dev)
        counters = torch.zeros(16, dtype=torch.int64, device=dev)
        ds.render_device_batch(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), n_frames=2, frame_stride_px=n_rows * W,
                               d_counters=counters.data_ptr(), bounces=3, rows=(0, H, 8, 0, 2), part_stride=1)
        torch.cuda.synchronize()
        return dict(depth=depth.cpu().numpy(), color=color.cpu().numpy(), normal=normal.cpu().numpy(), ray_count=int(counters[0].item()))

    got = a_against_b(gpu, s, "batch of two frames", batch)
    assert got["ray_count"] > 2 * n_rows * W and np.isfinite(got["depth"]).all()


def test_host_call_into_page_locked_and_pageable_buffers(gpu, tmp_path):
    """page-locked buffers: the kernel delivers the frame itself (the KV_HOSTOUT twins, 6-wave for the bunny, 5-wave for 48
    triangles); pageable ones: device buffers and a copy.  All four are the same frame per scene."""
    for name, s in (("bunny", load_scene(gpu, "bunny", 96, 54)), ("room", parse(gpu, room(tmp_path, "host", [octahedra(RIGHT)])[0]))):
        pinned = a_against_b(gpu, s, f"{name}, page-locked", lambda ds: ds.render(bounces=3, pinned=True))
        pageable = a_against_b(gpu, s, f"{name}, pageable", lambda ds: ds.render(bounces=3))
        assert_same_frame(pinned, pageable, f"{name}: page-locked / pageable")
    ds = gpu.DeviceScene(load_scene(gpu, "bunny", 96, 54))
    ds.render(bounces=3, pinned=True)
    assert ds.last_kernel() & 128, "the page-locked call was meant to take the host-delivery build"
    ds.close()


# ---- edits of a live one-mesh handle ----
def test_edits_keep_the_shape_and_equal_a_fresh_handle(gpu, tmp_path):
    """update_mesh (refit), rebuild_mesh (a new tree) and a moved plane on ONE handle: still shape 1, and each frame is a
    fresh handle's on the edited scene"""
    base = octahedra(RIGHT)
    rng = np.random.default_rng(7)
    moved = (base + f32([-0.5, 0.1, 0.2]) + rng.uniform(-0.02, 0.02, base.shape)).astype(f32)
    folded = (moved[::-1] * f32([1.0, -1.0, 1.0]) + f32([-0.3, 0.0, -0.2])).astype(f32)
    text0, mesh, floor = room(tmp_path, "edit0", [base])
    steps = (("update_mesh", moved, -1.0), ("rebuild_mesh", folded, -1.0), ("moved floor", folded, -0.8))
    ds = gpu.DeviceScene(parse(gpu, text0))
    ds.render(bounces=3)
    assert ds.last_shape() == 1
    for k, (what, tris, floor_y) in enumerate(steps):
        edited = parse(gpu, room(tmp_path, f"edit{k + 1}", [tris], floor_y=floor_y)[0])
        if what == "update_mesh":
            ds.update_mesh(mesh, desc_tris(edited, mesh))
        elif what == "rebuild_mesh":
            ds.rebuild_mesh(mesh, desc_tris(edited, mesh))
        else:
            ds.set_object(floor, point=(0.0, floor_y, 0.0))
        got = ds.render(bounces=3)
        assert ds.last_shape() == 1, what
        fresh = gpu.DeviceScene(edited)
        assert_same_frame(got, fresh.render(bounces=3), f"{what}: edited / fresh handle")
        assert fresh.last_shape() == 1 and fresh.last_kernel() == ds.last_kernel(), what
        fresh.close()
    ds.close()


# ---- scenes and variants the shape is not for ----
def test_scenes_that_stay_in_shape_0(gpu, tmp_path):
    two = [octahedra(RIGHT[:3]), octahedra(RIGHT[3:])]
    cases = (("one mesh and a sphere", parse(gpu, room(tmp_path, "sph", [octahedra(RIGHT)], sphere=True)[0])),
             ("two meshes", parse(gpu, room(tmp_path, "two", two)[0])),
             ("one mesh, one transparent material", parse(gpu, room(tmp_path, "tr", [octahedra(RIGHT)], transparent=True)[0])))
    for what, s in cases:
        a_against_b(gpu, s, what, lambda ds: ds.render(bounces=3), shape=0)
    s = gpu.HostScene.load("scene/sphere_plane.json")
    assert s.ok
    s.set_size(64, 36)
    a_against_b(gpu, s, "sphere_plane.json", lambda ds: ds.render(bounces=3), shape=0)


def test_variants_outside_the_four_builds_stay_in_shape_0(gpu):
    s = load_scene(gpu, "bunny", 96, 54)
    want = a_against_b(gpu, s, "default", lambda ds: ds.render(bounces=3))
    for name in ("VAR_STATS", "VAR_NO_PREFILTER", "VAR_NO_ANYHIT", "VAR_EXACT_POW"):
        got = a_against_b(gpu, s, name, lambda ds: ds.render(bounces=3), shape=0, variant=getattr(gpu, name))
        if name != "VAR_EXACT_POW":   # (the exact specular term differs from the fast one in the colour's last bits)
            assert_same_frame(got, want, f"{name} / default")


def test_no_direct_on_the_host_path_takes_the_twin_without_delivery(gpu):
    """VAR_NO_DIRECT with page-locked buffers: the frame leaves through device buffers, i.e. the launch is the default
    variant's build without KV_HOSTOUT — one of the four builds, for which launch_shape's rule is shape 1"""
    s = load_scene(gpu, "bunny", 96, 54)
    got = a_against_b(gpu, s, "VAR_NO_DIRECT", lambda ds: ds.render(bounces=3, pinned=True), variant=gpu.VAR_NO_DIRECT)
    ds = gpu.DeviceScene(s)
    ds.set_variant(gpu.VAR_NO_DIRECT)
    ds.render(bounces=3, pinned=True)
    assert not ds.last_kernel() & 128
    ds.close()
    assert_same_frame(got, a_against_b(gpu, s, "default", lambda ds: ds.render(bounces=3, pinned=True)), "VAR_NO_DIRECT / default")


def test_a_handle_without_scene_head_stays_in_shape_0(gpu):
    """CUTRACE_NO_SCENE_HEAD=1: the mesh record is read by pointer, which the one-mesh build has no code for"""
    s = load_scene(gpu, "bunny", 96, 54)
    with env("CUTRACE_NO_SCENE_HEAD"):
        got = a_against_b(gpu, s, "no scene head", lambda ds: ds.render(bounces=3), shape=0)
    assert_same_frame(got, a_against_b(gpu, s, "default", lambda ds: ds.render(bounces=3)), "no scene head / default")
