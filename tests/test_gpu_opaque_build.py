"""The opaque build of the render kernel (cutrace_amd/csrc/kernel_choice.h KO_OPAQUE, opaque_build; DESIGN.md "The opaque one-mesh
build"): a one-mesh launch of an any-hit build runs render_kernel<KV, 1, ROOM, 1>, from which the pass-through half of ray_color
is compiled out — an any-hit build is chosen only when no material transmits — and in which the hit point lives in the ray
origin alone.  Only code such a launch never runs is removed, so every case renders with two handles
of the same kind — A created normally, B under CUTRACE_NO_OPAQUE_BUILD=1 (read when a handle is created: the parent's
instantiation) — and compares depth, normal and colour BITWISE and the ray count, the build (last_kernel) and the shape, and
reads back which instantiation ran (last_opaque: 1 for A, 0 for B).

An opaque build asks for the LDS of its parent twin at every bounce count (tests/test_opaque_choice_cpu.py), so there is no
bounce count at which a launch falls back to the parent's instantiation: bounces 5 is the largest at which the 6-wave build
(KV_OCC6) is chosen, at bounces 6 the chooser takes the build without it, and both run as opaque builds.  Frames are 64 x 40
(8 x 5 tiles) or 64 x 48."""
import json

import numpy as np
import pytest

import oracle
from tests.conftest import load_scene
from tests.gpu_support import RIGHT, assert_same_frame, camera_of, env, gpu, held, octahedra, room  # noqa: F401  (gpu: the fixture)
from tests.live import desc_tris
from tests.util import assert_parity, parse

pytestmark = pytest.mark.gpu

f32 = np.float32
# scene_device.h KV_*: the default variant, with or without the 6-wave build (64), with or without host delivery (128)
DEFAULT = 1 | 2 | 8 | 32
W, H = 64, 40


def handles(ca, s):
    a = ca.DeviceScene(s)
    with env("CUTRACE_NO_OPAQUE_BUILD"):
        b = ca.DeviceScene(s)
    return a, b


def compare(a, b, what, render, opaque=1, kernel=None):
    """`render` on A and on B: the same frame, build and shape; A as the opaque build (or not: `opaque`), B never.  A's frame."""
    got, ref = held(render(a)), held(render(b))
    assert_same_frame(got, ref, f"{what}: opaque build on / off")
    assert a.last_kernel() == b.last_kernel() and a.last_shape() == b.last_shape(), what
    assert (a.last_opaque(), b.last_opaque()) == (opaque, 0), (what, hex(a.last_kernel()), a.last_shape())
    if opaque:
        assert a.last_shape() == 1 and a.last_kernel() & 2, (what, hex(a.last_kernel()))
    if kernel is not None:
        assert a.last_kernel() == kernel, (what, hex(a.last_kernel()))
    return got


@pytest.fixture(scope="module")
def bunny(gpu):
    """the flagship room at 64 x 40: walls, mesh silhouettes and reflections of the mesh in the walls"""
    s = load_scene(gpu, "bunny", W, H)
    a, b = handles(gpu, s)
    yield s, a, b
    a.close()
    b.close()


def a_against_b(ca, s, what, render, **kw):
    a, b = handles(ca, s)
    try:
        return compare(a, b, what, render, **kw)
    finally:
        a.close()
        b.close()


# ---- the flagship room ----
@pytest.mark.parametrize("bounces,kernel", [(5, DEFAULT | 64), (0, DEFAULT | 64), (1, DEFAULT | 64), (6, DEFAULT), (15, DEFAULT)])
def test_bunny_room(bunny, bounces, kernel):
    """bounces 5: the headline launch, the 6-wave build; 0: no frame is ever pushed (the stack's one frame is unused);
    1: one push, one unwind; 6: one more than the 6-wave build has room for — the chooser's 5-wave build, an opaque build as well;
    15: the deepest recursion there is"""
    _, a, b = bunny
    compare(a, b, f"bunny bounces {bounces}", lambda ds: ds.render(bounces=bounces), kernel=kernel)


def test_default_build_against_the_oracle(bunny):
    """the launch every caller gets: depth, normal and ray count bit for bit, the colour within the parity bar"""
    s, a, _ = bunny
    got = held(a.render(bounces=5))
    assert a.last_opaque() == 1 and a.last_kernel() == DEFAULT | 64
    want = oracle.oracle_render(s, fudge=1e-3, bounces=5, threads=4)
    assert_parity(got, want, what="bunny 64x40 b5: opaque build / oracle")
    assert got["ray_count"] == want["ray_count"]


# ---- the other ways into the kernel (tests/test_gpu_shape_build.py's) ----
def test_rows_in_two_parts(bunny):
    """8-row blocks dealt to 2 parts (40 rows: 24 and 16)"""
    _, a, b = bunny
    for part in (0, 1):
        compare(a, b, f"part {part} of 2", lambda ds: ds.render(bounces=3, rows=(0, H, 8, part, 2)))


def test_batch_of_two_frames_with_part_stride(gpu, tmp_path):
    """render_device_batch: two cameras in one launch, the part rotating from frame to frame (part_stride 1)"""
    import torch
    s = parse(gpu, room(tmp_path, "batch", [octahedra(RIGHT)])[0])
    cams = [camera_of(gpu, s), camera_of(gpu, parse(gpu, room(tmp_path, "batch2", [octahedra(RIGHT)], eye=(-0.4, 0.3, 2.6))[0]))]
    dev = torch.device("cuda:0")
    w, h, n_rows = 64, 48, 24   # 48 rows in 8-row blocks, 2 parts: 24 rows each

    def batch(ds):
        ds.set_cameras(cams)
        px = 2 * n_rows * w
        depth = torch.zeros(px, dtype=torch.float32, device=dev)
        color = torch.zeros(3 * px, dtype=torch.float32, device=dev)
        normal = torch.zeros(3 * px, dtype=torch.float32, device=dev)
        counters = torch.zeros(16, dtype=torch.int64, device=dev)
        ds.render_device_batch(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), n_frames=2, frame_stride_px=n_rows * w,
                               d_counters=counters.data_ptr(), bounces=3, rows=(0, h, 8, 0, 2), part_stride=1)
        torch.cuda.synchronize()
        return dict(depth=depth.cpu().numpy(), color=color.cpu().numpy(), normal=normal.cpu().numpy(), ray_count=int(counters[0].item()))

    got = a_against_b(gpu, s, "batch of two frames", batch, kernel=DEFAULT)
    assert got["ray_count"] > 2 * n_rows * w and np.isfinite(got["depth"]).all()


def test_host_call_into_page_locked_and_pageable_buffers(gpu, bunny, tmp_path):
    """page-locked buffers: the kernel delivers the frame itself (the KV_HOSTOUT twins, 6-wave for the bunny, 5-wave for 48
    triangles); pageable ones: device buffers and a copy.  All four are the same frame per scene."""
    _, a, b = bunny
    pinned = compare(a, b, "bunny, page-locked", lambda ds: ds.render(bounces=3, pinned=True), kernel=DEFAULT | 64 | 128)
    pageable = compare(a, b, "bunny, pageable", lambda ds: ds.render(bounces=3), kernel=DEFAULT | 64)
    assert_same_frame(pinned, pageable, "bunny: page-locked / pageable")
    s = parse(gpu, room(tmp_path, "host", [octahedra(RIGHT)])[0])
    pinned = a_against_b(gpu, s, "room, page-locked", lambda ds: ds.render(bounces=3, pinned=True), kernel=DEFAULT | 128)
    pageable = a_against_b(gpu, s, "room, pageable", lambda ds: ds.render(bounces=3), kernel=DEFAULT)
    assert_same_frame(pinned, pageable, "room: page-locked / pageable")


# ---- edits of a live handle ----
def test_a_mesh_update_keeps_the_opaque_build(gpu, tmp_path):
    base = octahedra(RIGHT)
    rng = np.random.default_rng(7)
    moved = (base + f32([-0.5, 0.1, 0.2]) + rng.uniform(-0.02, 0.02, base.shape)).astype(f32)
    text0, mesh, _ = room(tmp_path, "edit0", [base])
    edited = parse(gpu, room(tmp_path, "edit1", [moved])[0])
    ds = gpu.DeviceScene(parse(gpu, text0))
    ds.render(bounces=3)
    assert ds.last_opaque() == 1
    ds.update_mesh(mesh, desc_tris(edited, mesh))
    got = held(ds.render(bounces=3))
    assert ds.last_opaque() == 1 and ds.last_shape() == 1
    a_fresh, b_fresh = handles(gpu, edited)
    try:
        want = compare(a_fresh, b_fresh, "updated mesh, fresh handles", lambda h: h.render(bounces=3))
        assert_same_frame(got, want, "update_mesh: edited / fresh handle")
        assert a_fresh.last_kernel() == ds.last_kernel()
    finally:
        ds.close()
        a_fresh.close()
        b_fresh.close()


def test_a_material_made_transparent_leaves_the_any_hit_build_and_comes_back(gpu):
    """transparency 0.25 on a wall's material: the next launch is no any-hit build (so no opaque build, whose code could not
    shade it); back to 0: the opaque build again.  Each frame is a fresh handle's on the edited scene."""
    ds = gpu.DeviceScene(load_scene(gpu, "bunny", W, H))
    ds.render(bounces=5)
    assert ds.last_opaque() == 1 and ds.last_kernel() & 2
    seen = []
    for what, t in (("transparent", 0.25), ("opaque again", 0.0)):
        ds.set_material(1, transparency=t)
        got = held(ds.render(bounces=5))
        edited = load_scene(gpu, "bunny", W, H)
        edited.set_material(1, transparency=t)
        fresh = gpu.DeviceScene(edited)
        try:
            assert_same_frame(got, held(fresh.render(bounces=5)), f"{what}: edited / fresh handle")
            assert (ds.last_kernel(), ds.last_shape(), ds.last_opaque()) == (fresh.last_kernel(), fresh.last_shape(), fresh.last_opaque()), what
        finally:
            fresh.close()
        seen.append((bool(ds.last_kernel() & 2), ds.last_opaque()))
    ds.close()
    assert seen == [(False, 0), (True, 1)], seen


# ---- scenes the opaque build is not for ----
def test_a_scene_with_a_sphere_stays_on_the_parents_code(gpu, tmp_path):
    s = parse(gpu, room(tmp_path, "sph", [octahedra(RIGHT)], sphere=True)[0])
    a_against_b(gpu, s, "one mesh and a sphere", lambda ds: ds.render(bounces=3), opaque=0)
    ds = gpu.DeviceScene(s)
    ds.render(bounces=3)
    assert ds.last_kernel() & 2 and ds.last_shape() == 0 and ds.last_opaque() == 0, hex(ds.last_kernel())
    ds.close()


def test_a_transparent_material_and_the_statistics_build_stay_on_the_parents_code(gpu, tmp_path):
    text = json.loads(room(tmp_path, "tr", [octahedra(RIGHT)])[0])
    text["materials"][2]["transparency"] = 0.25
    a_against_b(gpu, parse(gpu, json.dumps(text)), "a transparent wall material", lambda ds: ds.render(bounces=3), opaque=0)

    def stats(ds):
        ds.set_variant(gpu.VAR_STATS)
        return ds.render(bounces=3)

    a_against_b(gpu, parse(gpu, room(tmp_path, "st", [octahedra(RIGHT)])[0]), "VAR_STATS", stats, opaque=0)
