"""Mesh replaces on the GPU (include/cutrace_replace.h): a handle whose mesh got ANOTHER NUMBER of triangles through
replace_mesh — the device's linear BVH or the host's builder — against a handle freshly created from the replaced description.
Every comparison is BITWISE: neither a tree nor the place of a mesh's records in the scene's arrays can change a result.  Frames are
96 x 54 or smaller; the counts are the smallest at which each part can go wrong (tests/test_gpu_mesh_update.py's and
tests/test_gpu_mesh_rebuild.py's; the helpers are those of tests/live.py)."""
import ctypes as C

import numpy as np
import pytest

from cutrace_amd import _lib, scenes
from tests.gpu_support import assert_same_frame, gpu, same_tensors  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, H, KV_MERGE, W, assert_box, assert_equals_fresh, cluster, desc_tris, frame, in_plane_scene, mesh_objects, moved,
                        on_a_busy_stream, random_mesh, scene_with, staircase, with_in_plane)
from tests.util import mesh_scene, parse

pytestmark = pytest.mark.gpu

f32 = np.float32


def assert_ranges(info, n_before, cap_before, n, what):
    """the range rules of include/cutrace_replace.h: in place while the count fits, else max(n, 2 * tri_cap) records at the end"""
    grows = n > cap_before
    assert info["tris_moved"] == int(grows), (what, info)
    assert info["tri_cap"] == (max(n, 2 * cap_before) if grows else cap_before), (what, info)
    assert info["nodes_moved"] in (0, 1) and 1 <= info["node_count"] <= n and info["levels"] >= 1, (what, info)
    assert n > 4 or (info["node_count"], info["levels"]) == (1, 1), (what, info)


# ---- 1 ----
@pytest.mark.parametrize("builder", ["device", "host"])
@pytest.mark.parametrize("n0,n1", [(65, 1), (1, 65), (4, 5), (5, 4), (64, 65), (65, 64), (1000, 200), (200, 1000)])
def test_replaced_mesh_equals_a_fresh_handle(gpu, tmp_path, n0, n1, builder):
    """no inner node; one leaf against two; the wave boundary of the builder's kernels; in place against moved"""
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "base", [random_mesh(n0, seed=n0)]))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    fresh_scene = scene_with(gpu, tmp_path, "new", [moved(random_mesh(n1, seed=100 + n1), 0.6, 0.05, seed=n1)])
    info = upd.replace_mesh(0, desc_tris(fresh_scene, 0), builder=builder)
    what = f"{n0} -> {n1} triangles, {builder}"
    assert info["builder"] == (1 if builder == "host" else 0) and info["fell_back"] == 0, info
    assert_ranges(info, n0, n0, n1, what)
    assert_box(upd, 0, fresh_scene, what)
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), what)


# ---- 2 ----
def test_host_builder_gives_the_fresh_handles_work_counters_too(gpu, tmp_path):
    """the same builder over the same triangles gives the same tree, and the refit the builder's boxes (tests/test_mesh_update_cpu.py),
    as tests/test_gpu_mesh_rebuild.py test 2 argues: frames, work counters, kernel build and launch shape are the fresh handle's"""
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "big", [random_mesh(1000, seed=3)]))
    fresh_scene = scene_with(gpu, tmp_path, "small", [random_mesh(600, seed=4)])
    info = upd.replace_mesh(0, desc_tris(fresh_scene, 0), builder="host")
    assert info["builder"] == 1 and info["fell_back"] == 0 and info["tris_moved"] == 0 and info["tri_cap"] == 1000, info
    fresh = gpu.DeviceScene(fresh_scene)
    for bits in (gpu.VAR_AUTO, gpu.VAR_STATS):
        a, b = frame(fresh, bits), frame(upd, bits)
        assert_same_frame(b, a, f"1000 -> 600, variant {bits}")
        assert np.array_equal(upd.last_counters(), fresh.last_counters()), (bits, upd.last_counters(), fresh.last_counters())
        assert upd.last_kernel() == fresh.last_kernel() and upd.last_shape() == fresh.last_shape(), (bits, upd.last_kernel(), fresh.last_kernel())


# ---- 3 ----
def test_queries_see_the_replaced_mesh(gpu, tmp_path):
    """a deeper tree over more triangles in a moved range: the queries take ranges, counts and stack slots from the handle per call"""
    import torch
    tris = cluster(500, seed=25)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "q_base", [random_mesh(200, seed=26)]))
    fresh_scene = scene_with(gpu, tmp_path, "q_cluster", [tris])
    info = upd.replace_mesh(0, desc_tris(fresh_scene, 0))
    assert info["builder"] == 0 and info["fell_back"] == 0 and info["tris_moved"] == 1 and info["tri_cap"] == 500, info
    fresh = gpu.DeviceScene(fresh_scene)
    rng = np.random.default_rng(27)
    n = 8192
    o = (np.array([0.3, 0.8, 4.0]) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    aim = rng.uniform(-1, 1, (n, 3)) * np.ldexp(1.0, -(np.arange(n) % 10))[:, None]          # into every octave of the cluster
    d = (aim - o).astype(f32)
    cu, cf = upd.cast_rays(o, d), fresh.cast_rays(o, d)
    same_tensors(cu, upd.cast_rays(o, d, linear=True), "cast_rays against its own linear walk")
    same_tensors(cu, cf, "cast_rays against fresh")
    assert int((cu["object"] == 0).sum()) > n // 20, "the rays are aimed at the mesh"
    outputs = ("color", "t", "object", "normal")
    su = upd.shade_rays(o, d, bounces=2, outputs=outputs)
    same_tensors(su, upd.shade_rays(o, d, bounces=2, linear=True, outputs=outputs), "shade_rays against its own linear walk")
    same_tensors(su, fresh.shade_rays(o, d, bounces=2, outputs=outputs), "shade_rays against fresh")
    args = dict(normals=cf["normal"], view_dirs=torch.from_numpy(d), objects=cf["object"], outputs=("color", "light_shadow"))
    pu = upd.shade_points(cf["point"], **args)
    same_tensors(pu, upd.shade_points(cf["point"], linear=True, **args), "shade_points against its own linear walk")
    same_tensors(pu, fresh.shade_points(cf["point"], **args), "shade_points against fresh")
    assert_equals_fresh(gpu, upd, fresh, "200 -> cluster of 500")


# ---- 4 ----
def _mixed_scene(ca, tmp_path, name, a, b):
    """mesh a, (the floor,) a stand-alone triangle, mesh b, a sphere: the triangle's record lies between the two mesh ranges"""
    stl_b = str(tmp_path / f"{name}_b.stl")
    scenes.write_stl(stl_b, b)
    extra = [{"type": "triangle", "p1": [-1.6, 0.2, 0.5], "p2": [-0.9, 0.3, 0.8], "p3": [-1.3, 1.1, 0.4], "material": 0},
             {"type": "mesh", "file": stl_b, "material": 1},
             {"type": "sphere", "center": [1.4, 0.1, 0.6], "radius": 0.35, "material": 1}]
    return parse(ca, mesh_scene(str(tmp_path / f"{name}_a.stl"), W, H, a, extra_objects=extra))


def test_mixed_scene_keeps_what_lies_between_and_beside(gpu, tmp_path):
    a, b = random_mesh(40, seed=30, spread=0.5), moved(random_mesh(30, seed=31, spread=0.4), 0.0, 0.0, shift=(0.8, 0.3, -0.4))
    s = _mixed_scene(gpu, tmp_path, "mixed", a, b)
    upd = gpu.DeviceScene(s)
    upd.render(bounces=BOUNCES)
    first, second = mesh_objects(s)
    now = {first: a, second: b}
    steps = ((first, random_mesh(90, seed=32, spread=0.5), "device"), (second, moved(random_mesh(70, seed=33, spread=0.4), 0.0, 0.0, shift=(0.8, 0.3, -0.4)), "host"),
             (first, random_mesh(12, seed=34, spread=0.5), "device"))
    for k, (which, tris, builder) in enumerate(steps):
        other = second if which == first else first
        state, box = upd.guard_state(other), upd.mesh_box(other)
        n_before = len(now[which])
        now[which] = tris
        fresh_scene = _mixed_scene(gpu, tmp_path, f"mixed_{k}", now[first], now[second])
        info = upd.replace_mesh(which, desc_tris(fresh_scene, which), builder=builder)
        assert info["fell_back"] == 0 and info["tris_moved"] == int(len(tris) > n_before), (k, info)
        assert upd.guard_state(other) == state and all(np.array_equal(x, y) for x, y in zip(upd.mesh_box(other), box)), f"step {k}: the untouched mesh"
        assert_box(upd, which, fresh_scene, f"step {k}")
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {k}: object {which} replaced by {len(tris)} triangles on the {builder}")


# ---- 5 ----
@pytest.mark.parametrize("scan", ["host", "device"])
def test_guard_states_at_changing_counts(gpu, tmp_path, monkeypatch, scan):
    """guard records (3), the linear fallback (70 > CTR_GUARD_SLOTS), a linear mesh replaced into another linear state — the new tree's
    device nodes must get the unbounded payload — and back to culling (0), each at another count; the guard's scan on either side,
    whose flat plane array is laid out anew when a count changes"""
    monkeypatch.setenv("CUTRACE_GUARD_SCAN", scan)
    w, h = 96, 24
    lift = dict(shift=(0.0, 1.2, 0.0))                                # above the rows' plane
    upd = gpu.DeviceScene(in_plane_scene(gpu, tmp_path, "plane_base", moved(random_mesh(100, seed=9, spread=0.8, size=0.25), 0.0, 0.0, **lift), w, h))
    upd.render(bounces=2)
    for step, (n, k, seed) in enumerate(((40, 3, 1), (200, 70, 2), (150, 70, 3), (90, 0, 4))):
        mesh = moved(random_mesh(n, seed=40 + step, spread=0.8, size=0.25), 0.05 * step, 0.0, **lift)
        fresh_scene = in_plane_scene(gpu, tmp_path, f"plane_{step}", with_in_plane(mesh, k, h, seed), w, h)
        assert upd.replace_mesh(0, desc_tris(fresh_scene, 0))["fell_back"] == 0
        fresh = gpu.DeviceScene(fresh_scene)
        state = upd.guard_state(0)
        assert state == fresh.guard_state(0), (step, state, fresh.guard_state(0))
        assert state[1] == (k > 64) and (state[1] or set(range(k)) <= set(state[0])), (step, state)
        assert_equals_fresh(gpu, upd, fresh, f"step {step}: {k} of {n} triangles in the eye's plane, scan on the {scan}", bounces=2)


# ---- 6 ----
def test_reflecting_mesh_across_the_mirror_threshold(gpu, tmp_path):
    """a reflecting mesh of up to CTR_MIRROR_MESH_TRIS = 16 triangles is that many flat mirrors to the guard, a larger one none: the
    virtual eyes appear and vanish with the count, and the other mesh's guard state follows them"""
    other = moved(random_mesh(200, seed=11, spread=0.7), 0.0, 0.0, shift=(0.3, 0.4, -1.0))
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "mirror", [random_mesh(12, seed=10, spread=0.6, size=0.5), other]))
    upd.render(bounces=BOUNCES)
    for k, n in enumerate((20, 12)):
        fresh_scene = scene_with(gpu, tmp_path, f"mirror_{k}", [random_mesh(n, seed=50 + k, spread=0.6, size=0.5), other])
        info = upd.replace_mesh(0, desc_tris(fresh_scene, 0))
        assert info["fell_back"] == 0 and info["tris_moved"] == (1 if n == 20 else 0) and info["tri_cap"] == 24, info
        fresh = gpu.DeviceScene(fresh_scene)
        assert [upd.guard_state(m) for m in mesh_objects(fresh_scene)] == [fresh.guard_state(m) for m in mesh_objects(fresh_scene)]
        assert_equals_fresh(gpu, upd, fresh, f"reflecting mesh of {n}")


# ---- 7 ----
def test_replaces_updates_and_rebuilds_in_a_row(gpu, tmp_path):
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "row", [random_mesh(65, seed=8)]))
    mesh = {130: random_mesh(130, seed=60), 40: random_mesh(40, seed=61)}
    steps = (("replace", 130, 65), ("update", 130, 65), ("rebuild", 130, 65), ("replace", 40, 130), ("update", 40, 130))
    for k, (step, n, old) in enumerate(steps):
        fresh_scene = scene_with(gpu, tmp_path, f"row_{k}", [moved(mesh[n], 0.4 * k, 0.1, seed=k)])
        tris = desc_tris(fresh_scene, 0)
        if step == "replace":
            info = upd.replace_mesh(0, tris)
            assert info["fell_back"] == 0 and info["tris_moved"] == int(n > old) and info["tri_cap"] == 130, (k, info)
        else:
            # the OLD count is refused, by both calls, and leaves the handle as it is; then the new one is taken
            stale = random_mesh(old, seed=62)
            with pytest.raises(RuntimeError, match=r"ctr_scene_update_mesh failed \(1\)"):
                upd.update_mesh(0, stale)
            with pytest.raises(RuntimeError, match=r"ctr_scene_rebuild_mesh failed \(1\)"):
                upd.rebuild_mesh(0, stale)
            if step == "update":
                upd.update_mesh(0, tris)
            else:
                assert upd.rebuild_mesh(0, tris)["fell_back"] == 0
        assert_box(upd, 0, fresh_scene, f"step {k}: {step}")
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {k}: {step} at {n}")


# ---- 8 ----
def test_merged_tree_is_retired_by_a_replace(gpu, tmp_path):
    a, b = random_mesh(64, seed=12, spread=0.5), moved(random_mesh(65, seed=13, spread=0.5), 0.0, 0.0, shift=(0.8, 0.2, 0.0))
    s = scene_with(gpu, tmp_path, "merge", [a, b])
    upd = gpu.DeviceScene(s)
    upd.set_variant(gpu.VAR_MERGE)
    upd.render(bounces=BOUNCES)
    assert upd.last_kernel() & KV_MERGE, "the scene of two meshes walks its merged tree before the replace"
    obj = mesh_objects(s)[1]
    fresh_scene = scene_with(gpu, tmp_path, "merge_new", [a, moved(random_mesh(90, seed=14, spread=0.5), 0.5, 0.05, shift=(-0.6, 0.0, 0.2))])
    info = upd.replace_mesh(obj, desc_tris(fresh_scene, obj))
    assert info["tris_moved"] == 1 and info["tri_cap"] == 130, info   # (behind the merged tree's room, which stays where it is)
    upd.set_variant(gpu.VAR_MERGE)                                   # (accepted, and builds nothing)
    r = upd.render(bounces=BOUNCES)
    assert not upd.last_kernel() & KV_MERGE, hex(upd.last_kernel())
    fresh = gpu.DeviceScene(fresh_scene)
    assert_same_frame(r, frame(fresh, gpu.VAR_AUTO), "VAR_MERGE after a replace: the two-level walk")
    assert_equals_fresh(gpu, upd, fresh, "after the merged tree retired")


# ---- 9 ----
@pytest.mark.parametrize("builder", ["device", "host"])
def test_numpy_input_and_tensor_on_its_producing_stream(gpu, tmp_path, builder):
    """both input paths; the tensor is produced on a non-default stream and handed over without a wait in between"""
    s = scene_with(gpu, tmp_path, "in", [random_mesh(300, seed=15)])
    from_tensor, from_numpy = gpu.DeviceScene(s), gpu.DeviceScene(s)
    t, stream = on_a_busy_stream(random_mesh(1000, seed=16))
    a = from_tensor.replace_mesh(0, t, builder=builder, stream=stream)
    new = t.cpu().numpy()
    b = from_numpy.replace_mesh(0, new, builder=builder)
    assert a == b and a["tris_moved"] == 1 and a["tri_cap"] == 1000, (a, b)
    fresh_scene = scene_with(gpu, tmp_path, "in_new", [new])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), new.view(np.uint32))
    fresh = gpu.DeviceScene(fresh_scene)
    assert_equals_fresh(gpu, from_tensor, fresh, "device tensor on its own stream")
    assert_equals_fresh(gpu, from_numpy, fresh, "numpy array")


# ---- 10 ----
def test_refused_replaces_leave_the_handle_untouched(gpu, tmp_path):
    import torch
    mesh = random_mesh(65, seed=17)
    s = scene_with(gpu, tmp_path, "bad", [mesh])
    ds = gpu.DeviceScene(s)
    before, box = frame(ds, gpu.VAR_AUTO), ds.mesh_box(0)
    stats = frame(ds, gpu.VAR_STATS)
    counters = ds.last_counters().copy()
    good = random_mesh(150, seed=18)
    bad = torch.from_numpy(good).to(torch.device("cuda", 0))
    bad[140, 1, 2] = float("nan")
    inf = good.copy()
    inf[149, 2, 0] = np.inf

    def untouched(what):
        assert_same_frame(frame(ds, gpu.VAR_AUTO), before, f"after the refused replace ({what})")
        assert_same_frame(frame(ds, gpu.VAR_STATS), stats, f"after the refused replace ({what}), VAR_STATS")
        assert np.array_equal(ds.last_counters(), counters), what
        assert all(np.array_equal(x, y) for x, y in zip(ds.mesh_box(0), box)), what
    L = _lib.hip_lib()
    good_c = np.ascontiguousarray(good)
    for builder in ("device", "host"):
        for what, obj, tris in (("no triangles", 0, good[:0]), ("not a mesh", 1, good), ("object out of range", 99, good),
                                ("NaN vertex in a device tensor", 0, bad), ("infinite vertex in a host array", 0, inf)):
            with pytest.raises(RuntimeError, match=r"ctr_scene_replace_mesh failed \(1\)"):
                ds.replace_mesh(obj, tris, builder=builder)
            untouched(f"{what}, {builder}")
    assert L.ctr_scene_replace_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), 0, 0, None, None) == 1      # n = 0 behind a pointer that is not null
    assert b"0 triangles" in L.ctr_last_error(), L.ctr_last_error()
    untouched("n_tris = 0")
    assert L.ctr_scene_replace_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), 0x1000000, 0, None, None) == 1
    assert b"16777216 triangles" in L.ctr_last_error(), L.ctr_last_error()
    untouched("n_tris = 2^24")
    with pytest.raises(ValueError, match="builder"):
        ds.replace_mesh(0, good, builder="sah")
    for flags in (2, 5, 0x100):
        assert L.ctr_scene_replace_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), len(good_c), flags, None, None) == 1
        assert b"unknown flag bits" in L.ctr_last_error()
        untouched(f"flags {flags:#x}")
    empty = str(tmp_path / "empty.stl")
    scenes.write_stl(empty, np.zeros((0, 3, 3), f32))
    es = parse(gpu, mesh_scene(str(tmp_path / "one.stl"), W, H, mesh, extra_objects=[{"type": "mesh", "file": empty, "material": 1}]))
    with pytest.raises(RuntimeError, match="empty mesh"):
        gpu.DeviceScene(es).replace_mesh(2, mesh[:1])
    info = ds.replace_mesh(0, good)                                   # and the handle still takes a good one
    assert info["fell_back"] == 0 and info["tris_moved"] == 1 and info["tri_cap"] == 150, info
    fresh_scene = scene_with(gpu, tmp_path, "good", [good])
    assert_equals_fresh(gpu, ds, gpu.DeviceScene(fresh_scene), "a good replace after the refused ones")


# ---- 11 ----
def test_objects_report_the_new_count(gpu, tmp_path):
    a, b = random_mesh(64, seed=19, spread=0.5), moved(random_mesh(30, seed=20, spread=0.5), 0.0, 0.0, shift=(0.8, 0.2, 0.0))
    s = scene_with(gpu, tmp_path, "objs", [a, b])
    ds = gpu.DeviceScene(s)
    first, second = mesh_objects(s)
    new = random_mesh(77, seed=21, spread=0.5)
    fresh_scene = scene_with(gpu, tmp_path, "objs_new", [new, b])
    ds.replace_mesh(first, desc_tris(fresh_scene, first))
    assert int(ds.get_object(first).tri_count) == 77 and int(ds.get_object(second).tri_count) == 30
    objs = [ds.get_object(k) for k in range(ds.object_count())]
    ds.set_objects(objs)                                              # the list goes back unchanged ...
    stale = [ds.get_object(k) for k in range(ds.object_count())]
    stale[first].tri_count = 64
    with pytest.raises(RuntimeError, match=r"ctr_scene_set_objects failed \(1\)"):
        ds.set_objects(stale)                                         # ... and the old count does not
    assert_box(ds, first, fresh_scene, "after set_objects")
    assert_equals_fresh(gpu, ds, gpu.DeviceScene(fresh_scene), "after set_objects")


# ---- 12 ----
def test_a_refused_device_tree_falls_back_to_the_host_builder(gpu, tmp_path):
    tris = staircase()
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "stair_base", [random_mesh(100, seed=23)]))
    upd.render(bounces=BOUNCES)
    fresh_scene = scene_with(gpu, tmp_path, "stair", [tris])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), tris.view(np.uint32))
    info = upd.replace_mesh(0, desc_tris(fresh_scene, 0))
    assert info["fell_back"] == 1 and info["builder"] == 1 and info["tris_moved"] == 0 and info["tri_cap"] == 100, info
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "staircase of 63 into a handle of 100")
