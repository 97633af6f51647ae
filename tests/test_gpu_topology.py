"""A live object count on the GPU (include/cutrace_topology.h): a handle whose objects were removed and appended through
remove_object, add_object and add_mesh against a handle freshly created from the edited description — the removed objects deleted, the
added ones appended.  Every comparison is BITWISE and goes through tests/live.py's assert_equals_fresh and assert_queries_equal_fresh:
frames under two builds and the handle's own linear walk, the guard state of every mesh, with the host builder's trees also the kernel
build and the work counters, and the queries with the object indices they report.  Frames are 48 x 27 at bounces 3, meshes have 12
and 70 triangles, queries 1024 rays."""
import ctypes as C
import json

import numpy as np
import pytest

from cutrace_amd import _lib
from tests.gpu_support import assert_same_frame, gpu, same_tensors  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, KV_MERGE, MIRROR, OPAQUE, OTHER, ROOM_MESH, ROOM_SMALL, ROOM_SPHERE, ROOM_TRI, ROOM_WALL, assert_equals_fresh,
                        assert_queries_equal_fresh, desc_tris, each_scan, frame, guard_tris, moved, on_a_busy_stream, room_scene, staircase, with_objects)
from tests.topology_support import NEW_SPHERE, NEW_TRIANGLE, NEW_WALL, add_described, appended, fresh_handle, mesh_object, one_mesh_room, without
from tests.util import parse

pytestmark = pytest.mark.gpu

f32 = np.float32
N_LIGHTS = 2


def used(gpu, sc):
    """a handle of the description with history: buffers, tile costs"""
    ds = gpu.DeviceScene(parse(gpu, sc))
    ds.render(bounces=BOUNCES)
    return ds


def spawned(seed=7, k=5, n_other=65, shift=(0.0, 1.5, 0.0)):
    """a mesh of 70 triangles beside room_scene's own, its first k in the plane z = 0.5"""
    return (guard_tris(k, n_other=n_other, seed=seed, zero_area=False) + f32(shift)).astype(f32)


# ---------------------------------------------------------------- 1. removes

REMOVES = {"the sphere": [ROOM_SPHERE], "the triangle": [ROOM_TRI], "a wall": [ROOM_WALL], "the small mesh": [ROOM_SMALL], "the big mesh": [ROOM_MESH],
           # (each index as the list stands when its turn comes)
           "all five in a row": [ROOM_SPHERE, ROOM_TRI - 1, ROOM_WALL - 2, ROOM_SMALL - 1, ROOM_MESH]}


@pytest.mark.parametrize("which", list(REMOVES))
def test_a_removed_object_leaves_the_scene_a_fresh_handle_has(gpu, tmp_path, which):
    sc = room_scene(tmp_path, "rm")
    upd = used(gpu, sc)
    for step, i in enumerate(REMOVES[which]):
        upd.remove_object(i)
        sc = without(sc, i)
        fresh, _ = fresh_handle(gpu, sc)
        what = f"remove {which}, step {step}"
        assert upd.object_count() == len(sc["objects"]), what
        assert_equals_fresh(gpu, upd, fresh, what, same_trees=True)
        assert_queries_equal_fresh(upd, fresh, N_LIGHTS, what)             # (the `object` output: the fresh handle's shifted indices)


# ---------------------------------------------------------------- 2. adds

@pytest.mark.parametrize("obj", [NEW_SPHERE, NEW_WALL, NEW_TRIANGLE], ids=lambda o: o["type"])
def test_an_added_analytic_object_is_the_last_of_a_fresh_description(gpu, tmp_path, obj):
    sc = room_scene(tmp_path, "add")
    upd = used(gpu, sc)
    assert add_described(upd, obj) == len(sc["objects"])
    fresh, _ = fresh_handle(gpu, appended(sc, obj))
    what = f"add a {obj['type']}"
    assert_equals_fresh(gpu, upd, fresh, what, same_trees=True)
    assert_queries_equal_fresh(upd, fresh, N_LIGHTS, what)


@pytest.mark.parametrize("source", ["numpy", "tensor"])
@pytest.mark.parametrize("builder", ["host", "device"])
def test_an_added_mesh_is_the_last_of_a_fresh_description(gpu, tmp_path, builder, source):
    sc = room_scene(tmp_path, "addm")
    upd = used(gpu, sc)
    room = upd.room()
    stream = None
    tris = spawned()
    if source == "tensor":
        given, stream = on_a_busy_stream(tris)                            # (produced on a stream of its own, handed over without a wait)
        tris = given.cpu().numpy()
    fresh, hs = fresh_handle(gpu, appended(sc, mesh_object(tmp_path, "spawned", tris, MIRROR)))
    index = len(sc["objects"])
    assert np.array_equal(desc_tris(hs, index).view(np.uint32), tris.view(np.uint32))
    info = upd.add_mesh(given if source == "tensor" else tris, material=MIRROR, builder=builder, stream=stream)
    assert (info["index"], info["builder"], info["fell_back"], info["tris_reused"], info["nodes_reused"], info["tri_cap"]) == (index, int(builder == "host"), 0, 0, 0, 70), info
    after = upd.room()
    assert after["tris_total"] == room["tris_total"] + 70 + 64 and after["tris_live"] == room["tris_live"] + 70 + 64, (room, after)
    assert after["nodes4_total"] == room["nodes4_total"] + info["node_count"] + 1, (room, after, info)
    what = f"add a mesh of 70 from a {source}, {builder} builder"
    assert_equals_fresh(gpu, upd, fresh, what, same_trees=builder == "host")
    assert_queries_equal_fresh(upd, fresh, N_LIGHTS, what)


def test_an_added_mesh_whose_device_tree_is_refused_gets_the_host_builders(gpu, tmp_path):
    sc = room_scene(tmp_path, "stair")
    upd = used(gpu, sc)
    tris = (staircase() + f32([0.5, 0.5, 2.0])).astype(f32)
    fresh, hs = fresh_handle(gpu, appended(sc, mesh_object(tmp_path, "staircase", tris, OPAQUE)))
    info = upd.add_mesh(desc_tris(hs, len(sc["objects"])), material=OPAQUE)
    assert info["fell_back"] == 1 and info["builder"] == 1 and info["tri_cap"] == 63, info
    assert_equals_fresh(gpu, upd, fresh, "a staircase of 63 added", same_trees=True)


def test_the_other_render_forms_see_the_edited_list(gpu, tmp_path):
    """supersampled, uv and display images read the same host copy per launch: a remove, an added mesh and an added triangle (whose
    uv needs its own vertices in its object record)"""
    sc = room_scene(tmp_path, "forms")
    upd = used(gpu, sc)
    upd.remove_object(ROOM_SPHERE)
    tris = spawned(seed=16)
    upd.add_mesh(tris, material=OTHER, builder="host")
    add_described(upd, NEW_TRIANGLE)
    fresh, _ = fresh_handle(gpu, appended(appended(without(sc, ROOM_SPHERE), mesh_object(tmp_path, "forms_spawned", tris, OTHER)), NEW_TRIANGLE))
    assert_same_frame(upd.render(bounces=BOUNCES, samples=2), fresh.render(bounces=BOUNCES, samples=2), "supersampled")
    same_tensors(upd.render_uv(bounces=BOUNCES), fresh.render_uv(bounces=BOUNCES), "uv")
    same_tensors(upd.render_images(bounces=BOUNCES), fresh.render_images(bounces=BOUNCES), "images")
    same_tensors(upd.render_images(bounces=BOUNCES, samples=2), fresh.render_images(bounces=BOUNCES, samples=2), "supersampled images")


@pytest.mark.parametrize("edit", ["remove the sphere", "add a sphere", "add a mesh"])
def test_the_merged_tree_is_retired_once_the_list_has_changed(gpu, tmp_path, edit):
    sc = room_scene(tmp_path, "merge")
    upd = gpu.DeviceScene(parse(gpu, sc))
    upd.set_variant(gpu.VAR_MERGE)
    upd.render(bounces=BOUNCES)
    assert upd.last_kernel() & KV_MERGE, "the room of two meshes walks its merged tree before the edit"
    if edit == "remove the sphere":
        upd.remove_object(ROOM_SPHERE)
        sc = without(sc, ROOM_SPHERE)
    elif edit == "add a sphere":
        add_described(upd, NEW_SPHERE)
        sc = appended(sc, NEW_SPHERE)
    else:
        tris = spawned(seed=17)
        upd.add_mesh(tris, material=OPAQUE, builder="host")
        sc = appended(sc, mesh_object(tmp_path, "merge_spawned", tris, OPAQUE))
    upd.set_variant(gpu.VAR_MERGE)                                   # (accepted, and builds nothing)
    r = upd.render(bounces=BOUNCES)
    assert not upd.last_kernel() & KV_MERGE, hex(upd.last_kernel())
    fresh, _ = fresh_handle(gpu, sc)
    assert_same_frame(r, frame(fresh, gpu.VAR_AUTO), f"VAR_MERGE after {edit}: the two-level walk")
    assert_equals_fresh(gpu, upd, fresh, f"{edit}, the merged tree retired", same_trees=True)


# ---------------------------------------------------------------- 3. launch shape and mesh presence

def test_launch_shape_and_room_facts_follow_the_mesh_count(gpu, tmp_path):
    first, second = spawned(seed=11, k=0, n_other=70, shift=(0.0, 0.0, 0.0)), spawned(seed=12, k=0, n_other=12, shift=(2.5, 0.0, 0.0))
    sc = one_mesh_room(tmp_path, "shape", first)
    upd = used(gpu, sc)
    assert upd.last_shape() == 1, "one mesh in a plane room takes the one-mesh launch shape"
    second_obj, first_obj = mesh_object(tmp_path, "shape_second", second, 1), mesh_object(tmp_path, "shape_again", first, 0)
    steps = (("a second mesh added", lambda: upd.add_mesh(second, material=1, builder="host"), lambda s: appended(s, second_obj), 0),
             ("the second mesh removed", lambda: upd.remove_object(6), lambda s: without(s, 6), 1),
             ("the first mesh removed: none left", lambda: upd.remove_object(0), lambda s: without(s, 0), 0),
             ("a mesh added back", lambda: upd.add_mesh(first, material=0, builder="host"), lambda s: appended(s, first_obj), 1))
    for what, call, describe, shape in steps:
        info = call()
        sc = describe(sc)
        fresh, _ = fresh_handle(gpu, sc)
        assert_equals_fresh(gpu, upd, fresh, what, same_trees=True)
        a, b = frame(upd, gpu.VAR_AUTO), frame(fresh, gpu.VAR_AUTO)
        assert_same_frame(a, b, what)
        assert upd.last_shape() == fresh.last_shape() == shape, f"{what}: launch shape {upd.last_shape()} against the fresh handle's {fresh.last_shape()}"
        assert upd.last_kernel() == fresh.last_kernel(), f"{what}: kernel {upd.last_kernel():#x} against {fresh.last_kernel():#x}"
        fa, fb = upd.room_facts(), fresh.room_facts()
        assert json.dumps({k: np.asarray(v).tolist() for k, v in fa.items()}) == json.dumps({k: np.asarray(v).tolist() for k, v in fb.items()}), (what, fa, fb)
        assert (fa["lights"] != 0) == (shape == 1), f"{what}: the one-mesh shape carries the facts of the room of five opaque walls: {fa}"
        assert_queries_equal_fresh(upd, fresh, N_LIGHTS, what)
    assert info["tris_reused"] == 1 and info["nodes_reused"] == 1, info    # the mesh that came back lives where it lived


# ---------------------------------------------------------------- 4. the guard

def test_the_guard_follows_a_mesh_that_comes_and_a_mirror_that_goes(gpu, tmp_path, monkeypatch):
    """the far wall reflects and stands at z = 0: the eye's image lies in z = 0.5, the plane of five triangles of the added mesh"""
    sc = with_objects(room_scene(tmp_path, "guard"), {ROOM_WALL: dict(point=[0, 0, 0], material=MIRROR)})
    tris = spawned(seed=9)
    added = appended(sc, mesh_object(tmp_path, "guard_spawned", tris, OPAQUE))
    index = len(sc["objects"])

    def body():
        upd = used(gpu, sc)
        assert upd.add_mesh(tris, material=OPAQUE, builder="host")["index"] == index
        seen = [assert_equals_fresh(gpu, upd, fresh_handle(gpu, added)[0], "a mesh added in front of a mirror wall", same_trees=True)]
        assert upd.guard_state(index) == ([0, 1, 2, 3, 4], False), upd.guard_state(index)
        upd.remove_object(ROOM_WALL)
        seen.append(assert_equals_fresh(gpu, upd, fresh_handle(gpu, without(added, ROOM_WALL))[0], "the mirror wall removed", same_trees=True))
        assert upd.guard_state(index - 1) == ([], False), upd.guard_state(index - 1)
        return seen
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 5. indices that shifted

def test_mesh_calls_find_a_mesh_at_its_new_index(gpu, tmp_path):
    sc = room_scene(tmp_path, "shift")
    upd = used(gpu, sc)
    big, small = desc_tris(parse(gpu, sc), ROOM_MESH), desc_tris(parse(gpu, sc), ROOM_SMALL)

    def now(sc, changes, name):
        """the description with the meshes at the indices of `changes` holding those triangles"""
        return with_objects(sc, {i: dict(file=mesh_object(tmp_path, f"{name}_{i}", t, 0)["file"]) for i, t in changes.items()})

    # both meshes get a refit schedule, then a wall in front of them goes: the schedules must travel with their meshes
    big1, small1 = moved(big, 0.1, 0.02, seed=1), moved(small, 0.2, 0.02, seed=2)
    upd.update_mesh(ROOM_MESH, big1)
    upd.update_mesh(ROOM_SMALL, small1)
    upd.remove_object(0)
    sc = now(without(sc, 0), {ROOM_MESH - 1: big1, ROOM_SMALL - 1: small1}, "s0")
    assert_equals_fresh(gpu, upd, fresh_handle(gpu, sc)[0], "two updates, then a wall in front removed")
    big2 = moved(big, 0.3, 0.02, seed=3)
    upd.update_mesh(ROOM_MESH - 1, big2)
    sc = now(sc, {ROOM_MESH - 1: big2}, "s1")
    assert_equals_fresh(gpu, upd, fresh_handle(gpu, sc)[0], "update_mesh at the new index")
    small2 = moved(small, 0.5, 0.05, seed=4)
    assert upd.rebuild_mesh(ROOM_SMALL - 1, small2)["fell_back"] == 0
    sc = now(sc, {ROOM_SMALL - 1: small2}, "s2")
    assert_equals_fresh(gpu, upd, fresh_handle(gpu, sc)[0], "rebuild_mesh at the new index")
    big3 = spawned(seed=13, k=0, n_other=90, shift=(0.0, 0.0, 0.0))
    assert upd.replace_mesh(ROOM_MESH - 1, big3)["tris_moved"] == 1
    sc = now(sc, {ROOM_MESH - 1: big3}, "s3")
    assert_equals_fresh(gpu, upd, fresh_handle(gpu, sc)[0], "replace_mesh at the new index")
    # the first mesh goes: the second mesh's schedule moves down a slot
    upd.remove_object(ROOM_MESH - 1)
    sc = without(sc, ROOM_MESH - 1)
    small3 = moved(small, 0.7, 0.02, seed=5)
    upd.update_mesh(ROOM_SMALL - 2, small3)
    sc = now(sc, {ROOM_SMALL - 2: small3}, "s4")
    assert_equals_fresh(gpu, upd, fresh_handle(gpu, sc)[0], "update_mesh of the second mesh once the first is gone")
    # a mesh that add_mesh made takes an update like any other
    tris = spawned(seed=14)
    index = upd.add_mesh(tris, material=OTHER)["index"]
    tris2 = moved(tris, 0.2, 0.02, seed=6)
    upd.update_mesh(index, tris2)
    sc = appended(sc, mesh_object(tmp_path, "s5", tris2, OTHER))
    fresh = fresh_handle(gpu, sc)[0]
    assert_equals_fresh(gpu, upd, fresh, "update_mesh of an added mesh")
    assert_queries_equal_fresh(upd, fresh, N_LIGHTS, "update_mesh of an added mesh")


# ---------------------------------------------------------------- 6. refusals

def test_refused_calls_leave_the_handle_as_it_was(gpu, tmp_path):
    import torch
    sc = room_scene(tmp_path, "bad")
    ds = used(gpu, sc)
    before, count, room = frame(ds, gpu.VAR_AUTO), ds.object_count(), ds.room()
    good = spawned()
    nan_host = good.copy()
    nan_host[69, 2, 1] = np.nan
    nan_dev = torch.from_numpy(good).to(torch.device("cuda", 0))
    nan_dev[3, 0, 0] = float("nan")
    L = _lib.hip_lib()

    def untouched(what):
        assert_same_frame(frame(ds, gpu.VAR_AUTO), before, f"after the refused call ({what})")
        assert ds.object_count() == count and ds.room() == room, (what, ds.object_count(), ds.room())

    assert L.ctr_scene_remove_object(ds._h, count) == 1 and b"out of range" in L.ctr_last_error(), L.ctr_last_error()
    untouched("remove_object past the end")
    with pytest.raises(ValueError, match="bad object index"):
        ds.remove_object(count)
    o = ds.get_object(ROOM_SMALL)
    assert L.ctr_scene_add_object(ds._h, C.byref(o), None) == 1 and b"ctr_scene_add_mesh" in L.ctr_last_error(), L.ctr_last_error()
    untouched("a mesh through add_object")
    o = ds.get_object(ROOM_SPHERE)
    o.type = 4
    assert L.ctr_scene_add_object(ds._h, C.byref(o), None) == 1 and b"bad type" in L.ctr_last_error(), L.ctr_last_error()
    untouched("a type above CTR_OBJ_SPHERE")
    with pytest.raises(RuntimeError, match=r"ctr_scene_add_object failed \(1\).*material index"):
        ds.add_object("sphere", material=4, center=(0, 0, 3), radius=1.0)
    untouched("add_object with material 4 of 4")
    for what, tris, material in (("material 4 of 4", good, 4), ("no triangles", good[:0], 0), ("a NaN vertex in a host array", nan_host, 0),
                                 ("a NaN vertex in a device tensor", nan_dev, 0)):
        for builder in ("device", "host"):
            with pytest.raises(RuntimeError, match=r"ctr_scene_add_mesh failed \(1\)"):
                ds.add_mesh(tris, material=material, builder=builder)
            untouched(f"add_mesh: {what}, {builder}")
    good_c = np.ascontiguousarray(good)
    assert L.ctr_scene_add_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), 0, 0, None, None) == 1 and b"0 triangles" in L.ctr_last_error(), L.ctr_last_error()
    assert L.ctr_scene_add_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), 0x1000000, 0, None, None) == 1 and b"16777216 triangles" in L.ctr_last_error()
    assert L.ctr_scene_add_mesh(ds._h, 0, C.c_void_p(good_c.ctypes.data), len(good_c), 2, None, None) == 1 and b"unknown flag bits" in L.ctr_last_error()
    untouched("add_mesh: counts and flags")
    info = ds.add_mesh(good, material=MIRROR)                              # and the handle still takes a good one
    assert info["index"] == count and info["fell_back"] == 0, info
    fresh = fresh_handle(gpu, appended(sc, mesh_object(tmp_path, "good", good, MIRROR)))[0]
    assert_equals_fresh(gpu, ds, fresh, "a good add after the refused ones")


# ---------------------------------------------------------------- 7. steady state

def test_a_steady_spawn_and_despawn_stops_growing_the_arrays(gpu, tmp_path):
    sc = room_scene(tmp_path, "steady")
    upd = used(gpu, sc)
    start = upd.room()
    tris = spawned(seed=15)                                               # (the same triangles every round: the same tree, the same room)
    index = len(sc["objects"])
    with_mesh = appended(sc, mesh_object(tmp_path, "steady_spawned", tris, OTHER))
    rooms = []
    for k in range(8):
        info = upd.add_mesh(tris, material=OTHER)
        assert (info["index"], info["tris_reused"], info["nodes_reused"], info["tri_cap"]) == (index, int(k > 0), int(k > 0), 70), (k, info)
        rooms.append(upd.room())
        if k == 7:
            assert_equals_fresh(gpu, upd, fresh_handle(gpu, with_mesh)[0], "the eighth spawn")
        upd.remove_object(index)
        assert upd.room() == dict(rooms[-1], tris_live=start["tris_live"], nodes4_live=start["nodes4_live"]), (k, upd.room())
    assert all(r == rooms[0] for r in rooms), rooms
    assert rooms[0]["tris_total"] == start["tris_total"] + 70 + 64 and rooms[0]["tris_live"] == start["tris_live"] + 70 + 64, (start, rooms[0])
    fresh = fresh_handle(gpu, sc)[0]
    assert_equals_fresh(gpu, upd, fresh, "after the eighth despawn", same_trees=True)
    assert_queries_equal_fresh(upd, fresh, N_LIGHTS, "after the eighth despawn")
