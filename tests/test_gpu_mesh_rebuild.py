"""Mesh rebuilds on the GPU (include/cutrace_rebuild.h): a handle whose mesh got new vertices AND a new tree through
rebuild_mesh — the device's linear BVH or the host's builder — against a handle freshly created from the replaced description.
Every comparison is BITWISE: a tree cannot change a result, only the time a walk takes.  Frames are 96 x 54 or smaller; the shapes
are the smallest at which each part can go wrong (tests/test_gpu_mesh_update.py's; the helpers are those of tests/live.py)."""
import ctypes as C

import numpy as np
import pytest

from cutrace_amd import _lib, scenes
from tests.gpu_support import assert_same_frame, gpu, same_tensors  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, H, KV_MERGE, W, assert_box, assert_equals_fresh, cluster, desc_tris, frame, in_plane_scene, mesh_objects, moved,
                        on_a_busy_stream, random_mesh, rays_at_the_mesh, scene_with, staircase, with_in_plane)
from tests.util import mesh_scene, parse

pytestmark = pytest.mark.gpu

f32 = np.float32


# ---- 1 ----
@pytest.mark.parametrize("builder", ["device", "host"])
@pytest.mark.parametrize("n", [1, 4, 5, 64, 65, 1000])
def test_moved_mesh_equals_a_fresh_handle(gpu, tmp_path, n, builder):
    """no internal node; one leaf; two leaves; the wave boundary of the builder's kernels; several levels"""
    mesh = random_mesh(n, seed=n)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "base", [mesh]))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    fresh_scene = scene_with(gpu, tmp_path, "moved", [moved(mesh, 0.6, 0.05, seed=n)])
    info = upd.rebuild_mesh(0, desc_tris(fresh_scene, 0), builder=builder)
    assert info["builder"] == (1 if builder == "host" else 0) and info["fell_back"] == 0, info
    assert info["node_count"] >= 1 and info["levels"] >= 1 and (n > 4 or (info["node_count"], info["levels"]) == (1, 1)), info
    assert_box(upd, 0, fresh_scene, f"{n} triangles, {builder}")
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"{n} triangles, {builder}")


# ---- 2 ----
def test_host_builder_on_the_same_triangles_changes_nothing_at_all(gpu, tmp_path):
    """the same builder over the same triangles gives the same tree, and the refit the builder's boxes (tests/test_mesh_update_cpu.py):
    the frames AND the work counters of the walk are those of the untouched handle"""
    s = scene_with(gpu, tmp_path, "identity", [random_mesh(1000, seed=3)])
    untouched, upd = gpu.DeviceScene(s), gpu.DeviceScene(s)
    info = upd.rebuild_mesh(0, desc_tris(s, 0), builder="host")
    assert info["builder"] == 1 and info["moved"] == 0 and info["fell_back"] == 0, info
    for bits in (gpu.VAR_AUTO, gpu.VAR_STATS):
        a, b = frame(untouched, bits), frame(upd, bits)
        assert_same_frame(b, a, f"identity, variant {bits}")
        assert np.array_equal(upd.last_counters(), untouched.last_counters()), (bits, upd.last_counters(), untouched.last_counters())


# ---- 3 ----
@pytest.mark.parametrize("name", ["70 identical triangles", "flat in x"])
def test_degenerate_sets_through_the_device_builder(gpu, tmp_path, name):
    """all keys equal (split by position), an axis of zero extent (no key bits, no NaN): equals fresh, and ties on t go to file index 0"""
    if name == "flat in x":
        tris = random_mesh(200, seed=21, spread=0.8, size=0.3)
        tris[:, :, 0] = f32(0.25)
        tris[0] = tris[1] = f32([[0.25, -0.9, -0.9], [0.25, 0.9, -0.9], [0.25, 0.0, 0.9]])   # one exact duplicate, large: ties on t
    else:
        tris = np.broadcast_to(f32([[-0.6, -0.2, 0.1], [0.7, -0.3, 0.2], [0.1, 0.9, -0.1]]), (70, 3, 3)).copy()
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "deg_base", [random_mesh(len(tris), seed=20)]))
    fresh_scene = scene_with(gpu, tmp_path, "deg", [tris])
    info = upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))
    assert info["builder"] == 0 and info["fell_back"] == 0, info
    fresh = gpu.DeviceScene(fresh_scene)
    assert_equals_fresh(gpu, upd, fresh, name)
    o, d = rays_at_the_mesh(4096, seed=22, target=0.6)
    got, want = upd.cast_rays(o, d, outputs=("t", "prim", "object")), fresh.cast_rays(o, d, outputs=("t", "prim", "object"))
    same_tensors(got, want, name)
    prim = got["prim"][got["object"] == 0].cpu().numpy()
    assert prim.size > 100, "the rays are aimed at the mesh"
    if name == "flat in x":
        assert 0 in prim and 1 not in prim, "a tie on t goes to the lower file index"
    else:
        assert (prim == 0).all(), f"ties on t go to file index 0, got {np.unique(prim)}"


# ---- 4 ----
def test_a_refused_device_tree_falls_back_to_the_host_builder(gpu, tmp_path):
    tris = staircase()
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "stair_base", [random_mesh(len(tris), seed=23)]))
    upd.render(bounces=BOUNCES)
    fresh_scene = scene_with(gpu, tmp_path, "stair", [tris])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), tris.view(np.uint32))
    info = upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))
    assert info["fell_back"] == 1 and info["builder"] == 1, info
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "staircase")
    again = scene_with(gpu, tmp_path, "stair_again", [moved(random_mesh(len(tris), seed=24), 0.3, 0.02)])
    info = upd.rebuild_mesh(0, desc_tris(again, 0))
    assert info["fell_back"] == 0 and info["builder"] == 0, info
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(again), "a further rebuild after the fallback")


# ---- 5 ----
@pytest.mark.parametrize("first", ["rebuild", "update"])
def test_rebuilds_and_updates_in_a_row_carry_nothing_over(gpu, tmp_path, first):
    mesh = random_mesh(65, seed=8)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "row", [mesh]))
    steps = ("rebuild", "update", "rebuild", "update") if first == "rebuild" else ("update", "rebuild")
    for k, (step, (angle, wobble)) in enumerate(zip(steps, ((2.0, 0.3), (-1.0, 0.0), (0.2, 0.6), (0.9, 0.1)))):
        fresh_scene = scene_with(gpu, tmp_path, f"row_{k}", [moved(mesh, angle, wobble, seed=k)])
        if step == "rebuild":
            assert upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))["fell_back"] == 0
        else:
            upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_box(upd, 0, fresh_scene, f"step {k}: {step}")
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {k}: {step}")


# ---- 6 ----
def test_two_meshes_rebuilt_one_after_the_other(gpu, tmp_path):
    """whether a tree fits its range or moves to the end of the node array, the other mesh is untouched"""
    a, b = random_mesh(64, seed=5, spread=0.5), moved(random_mesh(65, seed=6, spread=0.5), 0.0, 0.0, shift=(0.9, 0.2, 0.0))
    s = scene_with(gpu, tmp_path, "two", [a, b])
    upd = gpu.DeviceScene(s)
    upd.render(bounces=BOUNCES)
    objs = mesh_objects(s)
    now = [a, b]
    for k, (which, builder) in enumerate(((0, "device"), (1, "device"), (0, "host"), (1, "device"))):
        other = objs[1 - which]
        state, box = upd.guard_state(other), upd.mesh_box(other)
        now[which] = moved(now[which], 0.7, 0.1, seed=k)
        fresh_scene = scene_with(gpu, tmp_path, f"two_{k}", now)
        info = upd.rebuild_mesh(objs[which], desc_tris(fresh_scene, objs[which]), builder=builder)
        assert info["fell_back"] == 0 and info["moved"] in (0, 1), info
        assert upd.guard_state(other) == state and all(np.array_equal(x, y) for x, y in zip(upd.mesh_box(other), box)), f"step {k}"
        assert_box(upd, objs[which], fresh_scene, f"step {k}")
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {k}: mesh {which} rebuilt on the {builder}, moved {info['moved']}")


# ---- 7 ----
@pytest.mark.parametrize("scan", ["host", "device"])
def test_triangles_rebuilt_into_the_eyes_plane_and_out_again(gpu, tmp_path, monkeypatch, scan):
    """guard records (3), the linear fallback (70 > CTR_GUARD_SLOTS), a linear mesh rebuilt into another linear state — the new
    tree's device nodes must get the unbounded payload — and back to culling (0); the guard's scan on either side"""
    monkeypatch.setenv("CUTRACE_GUARD_SCAN", scan)
    w, h = 96, 24
    mesh = moved(random_mesh(100, seed=9, spread=0.8, size=0.25), 0.0, 0.0, shift=(0.0, 1.2, 0.0))   # above the rows' plane
    upd = gpu.DeviceScene(in_plane_scene(gpu, tmp_path, "plane_base", mesh, w, h))
    upd.render(bounces=2)
    for step, (k, seed) in enumerate(((3, 1), (70, 2), (70, 3), (0, 4))):
        fresh_scene = in_plane_scene(gpu, tmp_path, f"plane_{step}", with_in_plane(moved(mesh, 0.05 * step, 0.0), k, h, seed), w, h)
        assert upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))["fell_back"] == 0
        fresh = gpu.DeviceScene(fresh_scene)
        state = upd.guard_state(0)
        assert state == fresh.guard_state(0), (step, state, fresh.guard_state(0))
        assert state[1] == (k > 64) and (state[1] or set(range(k)) <= set(state[0])), (step, state)
        assert_equals_fresh(gpu, upd, fresh, f"step {step}: {k} triangles in the eye's plane, scan on the {scan}", bounces=2)


def test_reflective_small_mesh_rebuilt(gpu, tmp_path):
    """a mesh of 12 reflecting triangles is 12 flat mirrors to the guard: the virtual eyes follow it"""
    mirror = random_mesh(12, seed=10, spread=0.6, size=0.5)
    other = moved(random_mesh(200, seed=11, spread=0.7), 0.0, 0.0, shift=(0.3, 0.4, -1.0))
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "mirror", [mirror, other]))
    fresh_scene = scene_with(gpu, tmp_path, "mirror_moved", [moved(mirror, 0.8, 0.0, shift=(0.2, 0.1, 0.3)), other])
    assert upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))["fell_back"] == 0
    fresh = gpu.DeviceScene(fresh_scene)
    assert [upd.guard_state(m) for m in mesh_objects(fresh_scene)] == [fresh.guard_state(m) for m in mesh_objects(fresh_scene)]
    assert_equals_fresh(gpu, upd, fresh, "reflective mesh of 12")


# ---- 8 ----
def test_a_deeper_tree_than_the_original_gets_the_stack_it_needs(gpu, tmp_path):
    """the ray queries size their LDS stacks from FlatScene::ray_slots per call: a stale value under a deeper tree loses entries"""
    tris = cluster(200, seed=25)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "cluster_base", [random_mesh(200, seed=26)]))
    fresh_scene = scene_with(gpu, tmp_path, "cluster", [tris])
    host_levels = gpu.DeviceScene(fresh_scene).rebuild_mesh(0, desc_tris(fresh_scene, 0), builder="host")["levels"]
    info = upd.rebuild_mesh(0, desc_tris(fresh_scene, 0))
    assert info["builder"] == 0 and info["fell_back"] == 0 and info["levels"] > host_levels, (info, host_levels)
    fresh = gpu.DeviceScene(fresh_scene)
    rng = np.random.default_rng(27)
    n = 8192
    o = (np.array([0.3, 0.8, 4.0]) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    aim = rng.uniform(-1, 1, (n, 3)) * np.ldexp(1.0, -(np.arange(n) % 10))[:, None]          # into every octave of the cluster
    d = (aim - o).astype(f32)
    cu = upd.cast_rays(o, d)
    same_tensors(cu, upd.cast_rays(o, d, linear=True), "cast_rays against its own linear walk")
    same_tensors(cu, fresh.cast_rays(o, d), "cast_rays against fresh")
    assert int((cu["object"] == 0).sum()) > n // 20, "the rays are aimed at the mesh"
    outputs = ("color", "t", "object", "normal")
    su = upd.shade_rays(o, d, bounces=2, outputs=outputs)
    same_tensors(su, upd.shade_rays(o, d, bounces=2, linear=True, outputs=outputs), "shade_rays against its own linear walk")
    same_tensors(su, fresh.shade_rays(o, d, bounces=2, outputs=outputs), "shade_rays against fresh")
    assert_equals_fresh(gpu, upd, fresh, "cluster of 200")


# ---- 9 ----
def test_merged_tree_is_retired_by_a_rebuild(gpu, tmp_path):
    a, b = random_mesh(64, seed=12, spread=0.5), moved(random_mesh(65, seed=13, spread=0.5), 0.0, 0.0, shift=(0.8, 0.2, 0.0))
    s = scene_with(gpu, tmp_path, "merge", [a, b])
    upd = gpu.DeviceScene(s)
    upd.set_variant(gpu.VAR_MERGE)
    upd.render(bounces=BOUNCES)
    assert upd.last_kernel() & KV_MERGE, "the scene of two meshes walks its merged tree before the rebuild"
    obj = mesh_objects(s)[1]
    fresh_scene = scene_with(gpu, tmp_path, "merge_moved", [a, moved(b, 0.5, 0.05, shift=(-0.6, 0.0, 0.2))])
    upd.rebuild_mesh(obj, desc_tris(fresh_scene, obj))
    upd.set_variant(gpu.VAR_MERGE)                                   # (accepted, and builds nothing)
    r = upd.render(bounces=BOUNCES)
    assert not upd.last_kernel() & KV_MERGE, hex(upd.last_kernel())
    fresh = gpu.DeviceScene(fresh_scene)
    assert_same_frame(r, frame(fresh, gpu.VAR_AUTO), "VAR_MERGE after a rebuild: the two-level walk")
    assert_equals_fresh(gpu, upd, fresh, "after the merged tree retired")


# ---- 10 ----
@pytest.mark.parametrize("builder", ["device", "host"])
def test_numpy_input_and_tensor_on_its_producing_stream(gpu, tmp_path, builder):
    """both input paths; the tensor is produced on a non-default stream and handed over without a wait in between"""
    mesh = random_mesh(1000, seed=16)
    s = scene_with(gpu, tmp_path, "in", [mesh])
    from_tensor, from_numpy = gpu.DeviceScene(s), gpu.DeviceScene(s)
    t, stream = on_a_busy_stream(mesh)
    a = from_tensor.rebuild_mesh(0, t, builder=builder, stream=stream)
    new = t.cpu().numpy()
    b = from_numpy.rebuild_mesh(0, new, builder=builder)
    assert a == b, (a, b)
    fresh_scene = scene_with(gpu, tmp_path, "in_new", [new])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), new.view(np.uint32))
    fresh = gpu.DeviceScene(fresh_scene)
    assert_equals_fresh(gpu, from_tensor, fresh, "device tensor on its own stream")
    assert_equals_fresh(gpu, from_numpy, fresh, "numpy array")


# ---- 11 ----
def test_rejected_rebuilds_leave_the_handle_untouched(gpu, tmp_path):
    import torch
    mesh = random_mesh(65, seed=17)
    s = scene_with(gpu, tmp_path, "bad", [mesh])
    ds = gpu.DeviceScene(s)
    before, box = frame(ds, gpu.VAR_AUTO), ds.mesh_box(0)
    stats = frame(ds, gpu.VAR_STATS)
    counters = ds.last_counters().copy()
    good = moved(mesh, 0.4, 0.0)
    bad = torch.from_numpy(good).to(torch.device("cuda", 0))
    bad[40, 1, 2] = float("nan")
    inf = good.copy()
    inf[64, 2, 0] = np.inf

    def untouched(what):
        assert_same_frame(frame(ds, gpu.VAR_AUTO), before, f"after the rejected rebuild ({what})")
        assert_same_frame(frame(ds, gpu.VAR_STATS), stats, f"after the rejected rebuild ({what}), VAR_STATS")
        assert np.array_equal(ds.last_counters(), counters), what
        assert all(np.array_equal(x, y) for x, y in zip(ds.mesh_box(0), box)), what
    for builder in ("device", "host"):
        for what, obj, tris in (("wrong count", 0, good[:64]), ("not a mesh", 1, mesh), ("object out of range", 99, mesh),
                                ("NaN vertex in a device tensor", 0, bad), ("infinite vertex in a host array", 0, inf)):
            with pytest.raises(RuntimeError, match=r"ctr_scene_rebuild_mesh failed \(1\)"):
                ds.rebuild_mesh(obj, tris, builder=builder)
            untouched(f"{what}, {builder}")
    with pytest.raises(ValueError, match="builder"):
        ds.rebuild_mesh(0, good, builder="sah")
    L = _lib.hip_lib()
    good = np.ascontiguousarray(good)
    for flags in (2, 5, 0x100):
        assert L.ctr_scene_rebuild_mesh(ds._h, 0, C.c_void_p(good.ctypes.data), len(good), flags, None, None) == 1
        assert b"unknown flag bits" in L.ctr_last_error()
        untouched(f"flags {flags:#x}")
    empty = str(tmp_path / "empty.stl")
    scenes.write_stl(empty, np.zeros((0, 3, 3), f32))
    es = parse(gpu, mesh_scene(str(tmp_path / "one.stl"), W, H, mesh, extra_objects=[{"type": "mesh", "file": empty, "material": 1}]))
    with pytest.raises(RuntimeError, match="empty mesh"):
        gpu.DeviceScene(es).rebuild_mesh(2, mesh[:1])
    assert ds.rebuild_mesh(0, good)["fell_back"] == 0                 # and the handle still takes a good one
