"""Live objects on the GPU (include/cutrace_objects.h): a handle whose spheres, planes and stand-alone triangles
were moved or whose objects were given other materials through set_objects / set_object, against a handle freshly created from
the edited description — depth, normal, colour and ray count BITWISE under the default build and under VAR_EXACT_POW, the handle's
own VAR_NO_CLUSTER walk, the kernel build, the work counters under VAR_STATS and the guard state.  Every case runs with the guard's
plane scan on the device and again on the host (CUTRACE_GUARD_SCAN), and the guard states of the two runs are compared.  The
helpers are those of tests/live.py.  Every frame is 96 x 54 or smaller."""
import json

import numpy as np
import pytest

from cutrace_amd import _lib, lenses, scenes
from tests.gpu_support import FRAME, assert_same_frame, camera_of, gpu, same_tensors  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, EYE, GLASS, KV_MERGE, LIGHTS, MATERIALS, MIRROR, OPAQUE, OTHER, ROOM_MESH, ROOM_PLANES, ROOM_SMALL, ROOM_SPHERE, ROOM_TRI,
                        ROOM_WALL, assert_equals_fresh, assert_queries_equal_fresh, camera, desc_lights, desc_objects, each_scan, frame, guard_tris,
                        mesh_objects, room_scene, with_objects)
from tests.util import parse, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32


def plain_scene(w=96, h=54):
    """(a) of scripts/object_edit_check.cpp, sphere_plane-like: planes, spheres and stand-alone triangles, no mesh"""
    objs = [{"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": OTHER},
            {"type": "sphere", "center": [0.0, 0.0, 3.0], "radius": 0.8, "material": OPAQUE},
            {"type": "plane", "point": [0, 0, 9], "normal": [0.2, 0.1, -1.0], "material": OPAQUE},
            {"type": "triangle", "p1": [-1, 0, 4], "p2": [1, 0.5, 4.5], "p3": [0, 2, 4], "material": OTHER},
            {"type": "plane", "point": [-4, 0, 0], "normal": [1, 0, 0], "material": OPAQUE},
            {"type": "sphere", "center": [1.5, 0.5, 2.0], "radius": 0.4, "material": OTHER},
            {"type": "triangle", "p1": [2, -1, 5], "p2": [3, 1, 5], "p3": [2.5, 1.5, 6], "material": OPAQUE},
            {"type": "plane", "point": [4, 0, 0], "normal": [-1, 0, 0], "material": OTHER}]
    return {"camera": camera([0.3, 0.2, -0.5], [0.1, 0.0, 1.0], w, h), "lights": LIGHTS, "materials": MATERIALS, "objects": objs}


def two_mesh_scene(tmp_path, name, w=48, h=27):
    """(c): two meshes (the merged tree has its room), a floor and a sphere"""
    paths = [str(tmp_path / f"{name}_{k}.stl") for k in range(2)]
    scenes.write_stl(paths[0], guard_tris(4, n_other=40, seed=1))
    scenes.write_stl(paths[1], guard_tris(3, n_other=40, seed=2, zero_area=False) + f32([0.4, 0.3, 0.0]))
    objs = [{"type": "mesh", "file": paths[0], "material": OPAQUE}, {"type": "plane", "point": [0, -1.5, 0], "normal": [0, 1, 0], "material": OTHER},
            {"type": "mesh", "file": paths[1], "material": OTHER}, {"type": "sphere", "center": [1.0, 0.0, 1.0], "radius": 0.5, "material": OPAQUE}]
    return {"camera": camera(EYE, [0.0, 0.0, 0.0], w, h), "lights": LIGHTS, "materials": MATERIALS, "objects": objs}


def follow(gpu, upd, sc, what, **kw):
    """`upd` takes the objects of the description `sc`; then everything of assert_equals_fresh.  Returns (guard states, fresh handle)."""
    fresh_scene = parse(gpu, sc)
    upd.set_objects(desc_objects(fresh_scene))
    fresh = gpu.DeviceScene(fresh_scene)
    return assert_equals_fresh(gpu, upd, fresh, what, same_trees=True, **kw), fresh


def counters_and_frame(gpu, ds, variant=0):
    f = frame(ds, variant | gpu.VAR_STATS)
    c = ds.last_counters().copy()
    ds.set_variant(variant)
    return f, c


# ---------------------------------------------------------------- 1. no mesh: the guard refresh has nothing to do

def test_a_scene_without_a_mesh(gpu, monkeypatch):
    sc = plain_scene()
    steps = [("the sphere moved and resized", {1: dict(center=[0.4, 0.3, 2.6], radius=1.1)}),
             ("the floor tilted", {1: dict(center=[0.4, 0.3, 2.6], radius=1.1), 0: dict(normal=[0.1, 1.0, -0.05])}),
             ("a wall tilted too: two axis-aligned planes left", {0: dict(normal=[0.1, 1.0, -0.05]), 4: dict(normal=[1.0, 0.0, 0.2])}),
             ("every plane general: two records", {i: dict(normal=[0.25, 1.0, 0.125]) for i in (0, 2, 4, 7)}),
             ("three planes normal to y beside a general one: seven records, the most four planes can need",
              {0: dict(normal=[0, 1, 0]), 2: dict(normal=[0, 1, 0]), 4: dict(normal=[0, 1, 0]), 7: dict(normal=[0.25, 1.0, 0.0])}),
             ("all four normal to y: six", {i: dict(normal=[0, 1, 0]) for i in (0, 2, 4, 7)}),
             ("as it was", {})]

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)
        seen = []
        for what, changes in steps:
            states, _ = follow(gpu, upd, with_objects(sc, changes), what)
            assert states == []
            seen.append(what)
        return seen
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 2. the plane packing

def test_the_room_planes_are_packed_again(gpu, tmp_path, monkeypatch):
    """3 records (one axis triple) -> 4 (a general pair behind it) -> 3 general pairs and no triple -> 7 -> 9 records, three triples:
    more than the device array was created with -> 3 general pairs -> 9 in one edit -> 3"""
    sc = room_scene(tmp_path, "pack")
    tilted = lambda ids: {i: dict(normal=[0.25 if sc["objects"][i]["normal"][0] == 0 else sc["objects"][i]["normal"][0],
                                          0.25 if sc["objects"][i]["normal"][0] != 0 else sc["objects"][i]["normal"][1],
                                          sc["objects"][i]["normal"][2]]) for i in ids}
    steps = [("a wall tilted off its axis", tilted(ROOM_PLANES[:1])), ("back on its axis", {}),
             ("all but two planes tilted: general pairs", tilted(ROOM_PLANES[2:])), ("the planes back on their axes", {}),
             ("three planes normal to y, one general, one normal to x: seven records",
              {1: dict(normal=[0, 1, 0]), 3: dict(normal=[0, 1, 0]), 5: dict(normal=[0, 1, 0]), 8: dict(normal=[0.25, 0, 1])}),
             ("every plane normal to y: nine records", {i: dict(normal=[0, 1, 0]) for i in ROOM_PLANES}),
             ("every plane general: three records", {i: dict(normal=[0.25, 1.0, 0.125]) for i in ROOM_PLANES}),
             ("from general pairs to nine records", {i: dict(normal=[0, 1, 0]) for i in ROOM_PLANES}),
             ("a wall's point beyond 1e37", {0: dict(point=[-5, 2e37, 0])}), ("the planes as they were", {})]

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)
        states = []
        for what, changes in steps:
            states += follow(gpu, upd, with_objects(sc, changes), what)[0]
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 3. a stand-alone triangle: its DObj carries p1 / p3, its normal lives in gn

def test_a_triangle_moved_uv_and_normal(gpu, monkeypatch):
    import torch
    sc = plain_scene()
    moved = with_objects(sc, {3: dict(p1=[-0.7, 0.1, 3.8], p2=[0.9, 0.75, 4.65], p3=[0.2, 1.7, 4.4]), 6: dict(p1=[1.2, -0.8, 3.0], p2=[2.4, 0.6, 3.2], p3=[1.7, 1.2, 3.6])})
    rng = np.random.default_rng(3)
    n = 1024
    o = (np.array(sc["camera"]["eye"]) + rng.uniform(-0.2, 0.2, (n, 3))).astype(f32)
    target = np.array([[-0.7, 0.1, 3.8], [0.9, 0.75, 4.65], [0.2, 1.7, 4.4], [1.2, -0.8, 3.0], [2.4, 0.6, 3.2], [1.7, 1.2, 3.6]])
    w = rng.dirichlet([1, 1, 1], n)
    aim = np.where(np.arange(n)[:, None] % 2 == 0, w @ target[:3], w @ target[3:])
    d = (aim - o).astype(f32)

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render_uv(bounces=BOUNCES)
        states, fresh = follow(gpu, upd, moved, "two triangles moved")
        u, f = upd.render_uv(bounces=BOUNCES), fresh.render_uv(bounces=BOUNCES)
        for k in ("uv",) + FRAME:
            assert same_bits(u[k], f[k]), f"render_uv: {k}"
        cu, cf = upd.cast_rays(o, d), fresh.cast_rays(o, d)
        for k in ("uv", "normal", "prim", "object", "t"):
            assert torch.equal(cu[k].view(torch.int32), cf[k].view(torch.int32)), f"cast_rays: {k}"
        hit = cf["object"].cpu().numpy()
        assert (hit == 3).sum() > 100 and (hit == 6).sum() > 100, "the rays must meet the moved triangles"
        return ["two triangles moved", states]
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 4. material reassignment

def test_objects_take_other_materials(gpu, tmp_path, monkeypatch):
    """No object uses the transparent material at first, so all_opaque is false from the start and stays: the kernel build
    does not change, and what the casts skip or stop at comes from the objects' bits alone."""
    import torch
    sc = room_scene(tmp_path, "mats")
    steps = [("the sphere and a wall take the transparent material", {ROOM_SPHERE: dict(material=GLASS), 3: dict(material=GLASS)}),
             ("opaque again", {}),
             ("the triangle takes the transparent material", {ROOM_TRI: dict(material=GLASS)}),
             ("the 70-triangle mesh takes another material", {ROOM_MESH: dict(material=OTHER)}),
             ("the 70-triangle mesh transparent, the small one no mirror any more", {ROOM_MESH: dict(material=GLASS), ROOM_SMALL: dict(material=OPAQUE)}),
             ("the triangle reflects: a new mirror", {ROOM_TRI: dict(material=MIRROR)}),
             ("as it was", {})]
    rng = np.random.default_rng(4)
    o = (np.array(sc["camera"]["eye"]) + rng.uniform(-0.3, 0.3, (1024, 3))).astype(f32)
    d = (rng.uniform(-1, 1, (1024, 3)) * [3, 3, 0] + [-1.0, -1.0, 4.0] - o).astype(f32)

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        frame(upd, gpu.VAR_AUTO)
        kernel0 = upd.last_kernel()
        states = []
        for what, changes in steps:
            st, fresh = follow(gpu, upd, with_objects(sc, changes), what)
            states += st
            frame(upd, gpu.VAR_AUTO)
            assert upd.last_kernel() == kernel0, f"{what}: the materials did not change, the kernel build must not"
            cu, cf = upd.cast_rays(o, d, ignore_transparent=True), fresh.cast_rays(o, d, ignore_transparent=True)
            for k in cf:
                assert torch.equal(cu[k].view(torch.int32), cf[k].view(torch.int32)), f"{what}: cast_rays(ignore_transparent): {k}"
            u, f = frame(upd, gpu.VAR_IGNORE_TRANSPARENT), frame(fresh, gpu.VAR_IGNORE_TRANSPARENT)
            assert_same_frame(u, f, f"{what}: VAR_IGNORE_TRANSPARENT")
            upd.set_variant(0)
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 5. the moving mirror

def test_a_mirror_moves_the_eyes_image_into_the_plane_of_triangles_and_out_again(gpu, tmp_path, monkeypatch):
    sc = room_scene(tmp_path, "mirror")
    reflecting = {ROOM_WALL: dict(material=MIRROR)}
    moved = {ROOM_WALL: dict(material=MIRROR, point=[0, 0, 0])}

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)
        assert upd.guard_state(ROOM_MESH) == ([], False)
        states = []
        for what, changes, want in (("the wall reflects", reflecting, []), ("the mirror at z = 0: the eye's image in z = 0.5", moved, [0, 1, 2, 3, 4]),
                                    ("the mirror back at z = -6", reflecting, []), ("the wall reflects no more", {}, [])):
            states += follow(gpu, upd, with_objects(sc, changes), what)[0]
            assert upd.guard_state(ROOM_MESH) == (want, False), (what, upd.guard_state(ROOM_MESH))
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 6., 11. the identity edit and the round trip

@pytest.mark.parametrize("which", ["plain", "room", "two meshes"])
def test_identity_edit_and_round_trip(gpu, tmp_path, monkeypatch, which):
    """the description's own objects, then get_object of every object fed back: frames AND counters are the untouched handle's"""
    sc = plain_scene(48, 27) if which == "plain" else room_scene(tmp_path, "same") if which == "room" else two_mesh_scene(tmp_path, "same")

    def body():
        hs = parse(gpu, sc)
        upd, untouched = gpu.DeviceScene(hs), gpu.DeviceScene(hs)
        want_frame, want_counters = counters_and_frame(gpu, untouched)
        kernel = untouched.last_kernel()
        assert upd.object_count() == len(sc["objects"])
        seen = []
        for what in ("identity", "round trip"):
            objs = desc_objects(hs) if what == "identity" else [upd.get_object(i) for i in range(upd.object_count())]
            for i, o in enumerate(objs):
                assert (int(o.type), int(o.mat_idx)) == (int(hs.desc.contents.objects[i].type), sc["objects"][i]["material"])
                assert what == "identity" or int(o.tri_begin) == 0
            upd.set_objects(objs)
            got_frame, got_counters = counters_and_frame(gpu, upd)
            assert_same_frame(got_frame, want_frame, f"{which}: {what}")
            assert np.array_equal(got_counters, want_counters) and upd.last_kernel() == kernel, (which, what)
            seen.append([upd.guard_state(m) for m in mesh_objects(hs)])
            assert seen[-1] == [untouched.guard_state(m) for m in mesh_objects(hs)]
        for m in mesh_objects(hs):                               # a mesh comes back with its box and its count
            o, (lo, hi) = upd.get_object(m), upd.mesh_box(m)
            assert o.v0.tup() == tuple(lo) and o.v1.tup() == tuple(hi) and int(o.tri_count) == int(hs.desc.contents.objects[m].tri_count)
        return [which, seen]
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 7. with the other edits

def test_update_mesh_then_set_objects_then_set_lights(gpu, tmp_path, monkeypatch):
    sc = room_scene(tmp_path, "order")
    final = with_objects(sc, {ROOM_SPHERE: dict(center=[-1.5, -0.5, 2.5]), ROOM_WALL: dict(material=MIRROR, point=[0, 0, 0]), ROOM_MESH: dict(material=OTHER)})
    final["lights"] = [{"type": "point", "point": [2.0, 1.0, -0.2], "color": [0.7, 0.7, 0.7]}]
    tris = guard_tris(5, n_other=65, seed=5, zero_area=False)
    tris[:, :, 0] += f32(0.125)                                        # every triangle slides within its plane
    tris[:, :, 1] -= f32(0.0625)
    path = str(tmp_path / "order_moved.stl")
    scenes.write_stl(path, tris)
    final["objects"][ROOM_MESH]["file"] = path

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)
        fresh_scene = parse(gpu, final)
        upd.update_mesh(ROOM_MESH, tris)
        lo, hi = upd.mesh_box(ROOM_MESH)
        upd.set_objects(desc_objects(fresh_scene))
        lo2, hi2 = upd.mesh_box(ROOM_MESH)
        o = upd.get_object(ROOM_MESH)
        assert same_bits(lo, lo2) and same_bits(hi, hi2), "set_objects must leave the refitted box"
        assert o.v0.tup() == tuple(lo) and o.v1.tup() == tuple(hi) and int(o.mat_idx) == OTHER
        upd.set_lights(desc_lights(fresh_scene))
        # the counters: of a handle created with the final objects and lights whose mesh then got the same vertices (the same refitted tree)
        start = json.loads(json.dumps(final))
        start["objects"][ROOM_MESH]["file"] = sc["objects"][ROOM_MESH]["file"]
        ref = gpu.DeviceScene(parse(gpu, start))
        ref.update_mesh(ROOM_MESH, tris)
        states = assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "update_mesh, set_objects, set_lights", counters_of=ref)
        assert states[0] == ([0, 1, 2, 3, 4], False), states
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 8. queries and the other renders

def test_queries_and_the_other_renders_on_an_edited_handle(gpu, tmp_path, monkeypatch):
    import torch
    sc = room_scene(tmp_path, "queries")
    final = with_objects(sc, {ROOM_SPHERE: dict(center=[-1.0, 0.0, 2.5], radius=0.9, material=GLASS), ROOM_WALL: dict(material=MIRROR, point=[0, 0, 0]),
                              ROOM_TRI: dict(p1=[-2, 0, 4], p2=[-1, 0.5, 4.5], p3=[-1.5, 2, 4], material=MIRROR), 0: dict(normal=[1, 0.25, 0]), ROOM_MESH: dict(material=OTHER)})
    w, h = sc["camera"]["width"], sc["camera"]["height"]
    dev = torch.device("cuda:0")

    def batch(ds, cams):
        ds.set_cameras(cams)
        depth = torch.zeros(2 * h * w, dtype=torch.float32, device=dev)
        color, normal = torch.zeros(2 * h * w * 3, dtype=torch.float32, device=dev), torch.zeros(2 * h * w * 3, dtype=torch.float32, device=dev)
        counters = torch.zeros(16, dtype=torch.int64, device=dev)
        ds.render_device_batch(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), n_frames=2, frame_stride_px=h * w, d_counters=counters.data_ptr(), bounces=BOUNCES)
        torch.cuda.synchronize()
        return dict(depth=depth, color=color, normal=normal, rays=counters[:1])

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)
        fresh_scene = parse(gpu, final)
        upd.set_objects(desc_objects(fresh_scene))
        fresh = gpu.DeviceScene(fresh_scene)
        assert_queries_equal_fresh(upd, fresh, len(LIGHTS), "edited room")
        same_tensors(upd.render(bounces=BOUNCES, samples=2), fresh.render(bounces=BOUNCES, samples=2), "render(samples=2)")
        o, d = lenses.pinhole(fresh_scene.desc.contents.cam, w, h)
        lu, lf = upd.render_lens(o, d, bounces=BOUNCES), fresh.render_lens(o, d, bounces=BOUNCES)
        same_tensors(lu, lf, "render_lens")
        plain = fresh.render(bounces=BOUNCES)
        assert same_bits(lf["color"].cpu().numpy().reshape(plain["color"].shape), plain["color"]), "the camera's own rays give the plain frame"
        same_tensors(upd.render_images(bounces=BOUNCES), fresh.render_images(bounces=BOUNCES), "render_images")
        cam, other = camera_of(gpu, fresh_scene), camera_of(gpu, fresh_scene)
        other.pos = _lib.Vec3(-0.6, 0.5, -0.9)
        same_tensors(batch(upd, [cam, other]), batch(fresh, [cam, other]), "render_device_batch")
        return [upd.guard_state(m) for m in mesh_objects(fresh_scene)] + [fresh.guard_state(m) for m in mesh_objects(fresh_scene)]
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 9. the merged tree

def test_the_merged_tree_stays_in_use_across_an_object_edit(gpu, tmp_path, monkeypatch):
    sc = two_mesh_scene(tmp_path, "merged")
    steps = [("a mesh takes another material", {0: dict(material=MIRROR)}), ("the sphere moved, the other mesh transparent", {3: dict(center=[0.2, 0.4, 1.4]), 2: dict(material=GLASS)}),
             ("as it was", {})]

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.set_variant(gpu.VAR_MERGE)
        upd.render(bounces=2)
        assert upd.last_kernel() & KV_MERGE, "the scene of two meshes walks its merged tree"
        states = []
        for what, changes in steps:
            fresh_scene = parse(gpu, with_objects(sc, changes))
            fresh = gpu.DeviceScene(fresh_scene)
            fresh.set_variant(gpu.VAR_MERGE)
            upd.set_objects(desc_objects(fresh_scene))
            states += assert_equals_fresh(gpu, upd, fresh, f"merged tree, {what}", bounces=2, base=gpu.VAR_MERGE, same_trees=True)
            upd.render(bounces=2)
            assert upd.last_kernel() & KV_MERGE, f"{what}: {upd.last_kernel():#x}"
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- 10. every rejection

def test_every_rejection_raises_and_leaves_the_handle_as_it_was(gpu, tmp_path, monkeypatch):
    sc = room_scene(tmp_path, "reject")

    def body():
        hs = parse(gpu, sc)
        upd = gpu.DeviceScene(hs)
        upd.set_object(ROOM_SPHERE, center=(-1.5, -0.5, 2.5))          # (a handle that has been edited before)
        before, counters = counters_and_frame(gpu, upd)
        good = [upd.get_object(i) for i in range(upd.object_count())]

        def changed(i, **kw):
            objs = [upd.get_object(k) for k in range(upd.object_count())]
            objs[0].v0 = _lib.Vec3(9, 9, 9)                           # valid, and BEFORE the bad record: every check runs before the first write
            for k, v in kw.items():
                setattr(objs[i], k, v)
            return objs
        cases = [("the count is fixed", good[:-1]), ("the count is fixed", good + good[:1]), ("bad type", changed(ROOM_WALL, type=4)),
                 ("the type is fixed", changed(ROOM_SPHERE, type=2)), ("the type is fixed", changed(ROOM_MESH, type=0)),
                 ("the count is fixed", changed(ROOM_MESH, tri_count=71)), ("the count is fixed", changed(ROOM_SMALL, tri_count=0)),
                 ("material index out of range", changed(ROOM_TRI, mat_idx=len(MATERIALS))), ("material index out of range", changed(ROOM_MESH, mat_idx=2 ** 32 + 1))]
        for text, objs in cases:
            with pytest.raises(RuntimeError, match=rf"ctr_scene_set_objects failed \(1\).*{text}"):
                upd.set_objects(objs)
        L = _lib.hip_lib()
        assert L.ctr_scene_set_objects(upd._h, None, len(good)) == 1 and b"null argument" in L.ctr_last_error()
        with pytest.raises(RuntimeError, match=r"ctr_scene_get_object failed \(1\).*out of range"):
            upd.get_object(len(good))
        with pytest.raises(RuntimeError, match="material index out of range"):
            upd.set_object(ROOM_PLANES[0], material=len(MATERIALS))
        got, got_counters = counters_and_frame(gpu, upd)
        assert_same_frame(got, before, "after the rejected edits")
        assert np.array_equal(got_counters, counters)
        moved = with_objects(sc, {ROOM_SPHERE: dict(center=[-1.5, -0.5, 2.5])})
        return assert_equals_fresh(gpu, upd, gpu.DeviceScene(parse(gpu, moved)), "after the rejected edits", same_trees=True)
    each_scan(monkeypatch, body)
