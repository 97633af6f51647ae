"""The scene head (scene_device.h DSceneHead): the first axis triple of planes and the first mesh record carried in the
kernel-argument block.  The head holds COPIES of records the kernel otherwise reads by pointer, so every case is
compared three ways: against the oracle (tests/util.assert_parity), bitwise — depth, normal, colour, ray count —
against a handle created with CUTRACE_NO_SCENE_HEAD=1 (every record by pointer), and, wherever a handle's state
changed between two renders, bitwise against a fresh handle.  Frames are 64x48 or smaller."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle

from tests.gpu_support import assert_same_frame, env
from tests.util import _coplanar_scene, _multi_mesh_scene, assert_parity, parse, same_bits

pytestmark = pytest.mark.gpu
NT = min(os.cpu_count() or 4, 16)
W, H = 64, 48

EYE, UP, LOOK = [0.4, 0.3, 3.2], [0, 1, 0], [-0.1, -0.1, -1.0]
MATS = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
        {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.1, "phong": 10},
        {"type": "solid", "color": [0.9, 0.9, 0.9], "specular": 0.5, "reflect": 0.0, "phong": 80},
        {"type": "solid", "color": [0.4, 0.9, 0.5], "specular": 0.3, "reflect": 0.0, "phong": 20, "transparency": 0.5}]
# the walls of a room around the camera, two normal to each axis (one axis triple), then a third one normal to y
AXIS_PLANES = [([0, -1.0, 0], [0, 1, 0]), ([0, 0, -3.0], [0, 0, 1]), ([-2.5, 0, 0], [1, 0, 0]), ([2.5, 0, 0], [-1, 0, 0]),
               ([0, 3.0, 0], [0, -1, 0]), ([0, 0, 6.0], [0, 0, -1]), ([0, -1.25, 0], [0, 2, 0])]
OBLIQUE_PLANES = [([0, -1.1, 0], [0.3, 1, 0.2]), ([0, 0, -2.8], [-0.2, 0.1, 1]), ([2.2, 0, 0], [-1, 0.3, 0.1])]
LIGHTS = {"none": [],
          "one": [{"type": "point", "point": [0.5, 2.0, 2.0], "color": [0.8, 0.8, 0.8]}],
          "sun+points": [{"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]},
                         {"type": "point", "point": [0.5, 2.0, 2.0], "color": [0.6, 0.6, 0.6]},
                         {"type": "point", "point": [-1.5, 0.5, 1.0], "color": [0.3, 0.4, 0.5]}]}


def room(n_axis=5, n_oblique=0, mesh=True, lights="sun+points", w=W, h=H, eye=None, look=None, plane_mats=None, mesh_mat=0,
         mesh_file="scene/bunny.stl"):
    planes = AXIS_PLANES[:n_axis] + OBLIQUE_PLANES[:n_oblique]
    objs = [{"type": "plane", "point": p, "normal": n, "material": (plane_mats[i] if plane_mats else 1 + i % 2)}
            for i, (p, n) in enumerate(planes)]
    if mesh:
        objs.insert(len(objs) // 2, {"type": "mesh", "file": mesh_file, "material": mesh_mat})
    objs.append({"type": "sphere", "center": [1.3, -0.4, 0.2], "radius": 0.4, "material": 2})
    cam = {"eye": eye or EYE, "up": UP, "look": look or LOOK, "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": LIGHTS[lights], "materials": MATS, "objects": objs})


def three_ways(ca, s, what, bounces=4, variant=0, render=None, oracle_kw=None, want=None):
    """oracle parity of a handle with the head; the same bits from a handle without it.  Returns the frame."""
    render = render or (lambda ds: ds.render(bounces=bounces))
    ds = ca.DeviceScene(s)
    ds.set_variant(variant)
    got = render(ds)
    ds.close()
    with env("CUTRACE_NO_SCENE_HEAD"):
        off = ca.DeviceScene(s)
    off.set_variant(variant)
    ref = render(off)
    off.close()
    if want is None:
        want = oracle.oracle_render(s, bounces=bounces, threads=NT, **(oracle_kw or {}))
    assert_parity(got, want, what=what)
    assert got["ray_count"] == want["ray_count"], what
    assert_same_frame(got, ref, f"{what}: head on / off")
    return got


@pytest.mark.parametrize("n_axis,n_oblique", [(0, 0), (1, 0), (2, 0), (5, 0), (6, 0), (7, 0), (2, 3)])
def test_planes(ca, n_axis, n_oblique):
    """0 .. 7 axis-aligned planes (5: the flagship's room; 7: a second triple, read by pointer) and 2 axis + 3 oblique
    planes, of which the head holds the axis triple only"""
    three_ways(ca, parse(ca, room(n_axis, n_oblique)), f"{n_axis} axis + {n_oblique} oblique planes")


@pytest.mark.parametrize("lights", list(LIGHTS))
def test_lights(ca, lights):
    three_ways(ca, parse(ca, room(lights=lights)), f"lights: {lights}")


def test_fudge_zero_takes_the_general_plane_code(ca):
    """fudge = 0: no axis fast path, so the head's triple goes unused although it is filled"""
    s = parse(ca, room())
    want = oracle.oracle_render(s, fudge=0.0, bounces=3, threads=NT)
    three_ways(ca, s, "fudge 0", render=lambda ds: ds.render(fudge=0.0, bounces=3), want=want)


def test_no_mesh(ca):
    three_ways(ca, parse(ca, room(mesh=False)), "no mesh")


def test_one_mesh_with_guard_records(ca, tmp_path):
    """a mesh whose triangles' plane contains the eye and a light: the walk starts at the mesh's spare node, so the head's
    record must carry the bvh_root the guard selection wrote"""
    s = _coplanar_scene(ca, tmp_path, W, H, row=20, n_tris=12, seed=5)
    three_ways(ca, s, "guarded mesh")


@pytest.mark.parametrize("n_mesh", [2, 4])
def test_several_meshes_read_by_pointer(ca, tmp_path, n_mesh):
    s = parse(ca, _multi_mesh_scene(tmp_path, seed=3 + n_mesh, w=W, h=H, n_mesh=n_mesh))
    three_ways(ca, s, f"{n_mesh} meshes")


def test_merged_tree_and_back(ca, tmp_path):
    """CTR_VAR_MERGE with 4 meshes: the head holds the merged pseudo mesh; set_variant to the merged tree and back on ONE
    handle gives what fresh handles give"""
    s = parse(ca, _multi_mesh_scene(tmp_path, seed=11, w=W, h=H, opaque=True, n_mesh=4))
    want = oracle.oracle_render(s, bounces=4, threads=NT)
    plain = three_ways(ca, s, "4 meshes", want=want)
    merged = three_ways(ca, s, "4 meshes, merged tree", variant=ca.VAR_MERGE, want=want)
    assert_same_frame(plain, merged, "merged tree / two-level walk")
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=4)
    ds.set_variant(ca.VAR_MERGE)
    b = ds.render(bounces=4)
    ds.set_variant(0)
    c = ds.render(bounces=4)
    ds.close()
    for got, name in ((a, "before"), (b, "merged"), (c, "back")):
        assert_same_frame(got, plain, f"set_variant: {name}")


def test_ignore_transparent_reads_the_heads_words(ca):
    """CTR_VAR_IGNORE_TRANSPARENT with a transparent plane (slot 1 of the axis triple) and a transparent mesh"""
    s = parse(ca, room(plane_mats=[1, 3, 2, 1, 2], mesh_mat=3))
    plain = ca.DeviceScene(s).render(bounces=3)
    got = three_ways(ca, s, "ignore transparent", bounces=3, variant=ca.VAR_IGNORE_TRANSPARENT,
                     oracle_kw={"ignore_transparent_primary": True})
    assert int((got["depth"].view(np.uint32) != plain["depth"].view(np.uint32)).sum()) > 100  # the objects really are skipped


def _camera_of(ca, s):
    c = ca.Camera()
    C.memmove(C.byref(c), C.byref(s.desc.contents.cam), C.sizeof(ca.Camera))
    return c


def _eye_plane_mesh(tmp_path):
    """an octahedron and, sticking out of it, six triangles that lie exactly in the horizontal plane through EYE (and
    through no light): only while the eye is there does the mesh get guard records"""
    from cutrace_amd import scenes
    c, r = np.float32([-0.3, 0.0, 0.0]), np.float32(0.6)
    ax = [np.float32(v) * r for v in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]
    tris = [[c + ax[i], c + ax[j], c + ax[k]] for i in (0, 1) for j in (2, 3) for k in (4, 5)]
    y = np.float32(EYE[1])
    for k in range(6):
        a0, a1 = 1.0 * k, 1.0 * k + 0.8
        tris.append([[-0.3, y, 0.0], [-0.3 + 1.3 * np.cos(a0), y, 1.3 * np.sin(a0)], [-0.3 + 1.3 * np.cos(a1), y, 1.3 * np.sin(a1)]])
    path = str(tmp_path / "eye_plane.stl")
    scenes.write_stl(path, np.asarray(tris, np.float32))
    return path


def test_set_cameras_changes_the_guard_selection(ca, tmp_path):
    """render; set_cameras with an eye outside the triangles' plane (the guard records go, bvh_root returns to the root)
    and back into it; every render equals the oracle's, a fresh handle's and a handle's without the head"""
    stl = _eye_plane_mesh(tmp_path)
    s_in = parse(ca, room(mesh_file=stl))
    s_out = parse(ca, room(mesh_file=stl, eye=[1.1, 1.4, 3.6], look=[-0.3, -0.35, -1.0]))
    cam_in, cam_out = _camera_of(ca, s_in), _camera_of(ca, s_out)
    ds = ca.DeviceScene(s_in)
    first = ds.render(bounces=3)
    ds.set_cameras([cam_out])
    second = ds.render(bounces=3)
    ds.set_cameras([cam_in])
    third = ds.render(bounces=3)
    ds.close()
    assert_parity(first, oracle.oracle_render(s_in, bounces=3, threads=NT), what="eye in the plane")
    assert_parity(second, oracle.oracle_render(s_out, bounces=3, threads=NT), what="eye out of the plane")
    assert_same_frame(third, first, "back in the plane")
    fresh = ca.DeviceScene(s_out)
    assert_same_frame(second, fresh.render(bounces=3), "eye out of the plane: against a fresh handle")
    fresh.close()
    with env("CUTRACE_NO_SCENE_HEAD"):
        off = ca.DeviceScene(s_in)
    assert_same_frame(first, off.render(bounces=3), "eye in the plane: head on / off")
    off.set_cameras([cam_out])
    assert_same_frame(second, off.render(bounces=3), "eye out of the plane: head on / off")
    off.close()


def test_batch_of_two_cameras(ca):
    """two frames with different cameras in one launch: one head serves both"""
    import torch
    a, b = parse(ca, room()), parse(ca, room(eye=[-0.8, 0.9, 3.5]))
    cams = [_camera_of(ca, a), _camera_of(ca, b)]
    want = [oracle.oracle_render(x, bounces=3, threads=NT) for x in (a, b)]
    dev = torch.device("cuda:0")

    def batch(ds):
        ds.set_cameras(cams)
        depth = torch.zeros(2 * H * W, dtype=torch.float32, device=dev)
        color = torch.zeros(2 * H * W * 3, dtype=torch.float32, device=dev)
        normal = torch.zeros(2 * H * W * 3, dtype=torch.float32, device=dev)
        counters = torch.zeros(16, dtype=torch.int64, device=dev)
        ds.render_device_batch(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), n_frames=2, frame_stride_px=H * W,
                               d_counters=counters.data_ptr(), bounces=3)
        torch.cuda.synchronize()
        return [dict(depth=depth.cpu().numpy().reshape(2, H, W)[f], color=color.cpu().numpy().reshape(2, H, W, 3)[f],
                     normal=normal.cpu().numpy().reshape(2, H, W, 3)[f], ray_count=int(counters[0].item())) for f in range(2)]

    ds = ca.DeviceScene(a)
    got = batch(ds)
    ds.close()
    with env("CUTRACE_NO_SCENE_HEAD"):
        off = ca.DeviceScene(a)
    ref = batch(off)
    off.close()
    assert got[0]["ray_count"] == want[0]["ray_count"] + want[1]["ray_count"]
    for f in range(2):
        assert_parity(got[f], want[f], what=f"batch frame {f}")
        assert_same_frame(got[f], ref[f], f"batch frame {f}: head on / off")
        fresh = ca.DeviceScene((a, b)[f])
        one = fresh.render(bounces=3)
        fresh.close()
        for k in ("depth", "normal", "color"):
            assert same_bits(got[f][k], one[k]), f"batch frame {f} against a fresh handle: {k}"


def test_supersampled(ca):
    """s = 2 at 16x16 output pixels"""
    from tests import aa_ref
    big = parse(ca, room(w=32, h=32))
    o = oracle.oracle_render(big, bounces=3, threads=NT)
    want = aa_ref.reduce_frame(o, 2)
    want["ray_count"] = o["ray_count"]
    three_ways(ca, parse(ca, room(w=16, h=16)), "supersampled s=2", render=lambda ds: ds.render(bounces=3, samples=2), want=want)


def test_host_delivery(ca):
    """a page-locked destination at 64x16: the kernel delivers the frame itself (KV_HOSTOUT build)"""
    def pinned(ds):
        r = ds.render(bounces=3, pinned=True)
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}  # (views of the handle's block)
    s = parse(ca, room(w=64, h=16))
    got = three_ways(ca, s, "host delivery", bounces=3, render=pinned)
    ds = ca.DeviceScene(s)
    assert_same_frame(got, ds.render(bounces=3), "host delivery / device buffers")
    ds.close()
