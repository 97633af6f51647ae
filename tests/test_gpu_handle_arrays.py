"""The scene handle's device arrays through every way they grow (cutrace_amd/csrc/ctr_internal.h GrowBuf / SceneBuf; DESIGN.md §19 .. §21):
ONE handle whose light, material, plane, node and camera arrays each outgrow what ctr_scene_create allocated, one after the other,
against a handle freshly created from the edited description after every step — depth, colour and normal bit for bit, with
everything else tests/test_gpu_scene_edit.py's assert_equals_fresh looks at; and a node array that moves while another mesh's
device nodes are the unbounded payload the host copy does not hold.  The existing edit tests grow each array on a handle of its
own; none takes one handle through all of them, and none moves the node array next to a linear mesh.  The helpers are those of
tests/test_gpu_scene_edit.py, test_gpu_object_edit.py and test_gpu_mesh_rebuild.py.  Every frame is 48 x 27, bounces 3."""
import ctypes as C
import json

import numpy as np
import pytest

from cutrace_amd import _lib, scenes
from tests import test_gpu_mesh_rebuild as rebuild
from tests import test_gpu_object_edit as objects
from tests import test_gpu_scene_edit as base
from tests.util import same_bits

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 48, 27, 3
f32 = np.float32
SMALL_AT = f32([2.5, 0.0, 2.5])       # where the 12-triangle mesh's new set goes: beside the 70-triangle mesh, in front of the eye


@pytest.fixture(scope="module")
def gpu(ca):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return ca


def outgrowing_set():
    """12 triangles over ten octaves (test_gpu_mesh_rebuild.py's cluster): the device's tree over them has four nodes, where the
    12-triangle meshes of the scenes here were created with one (scripts/mesh_rebuild_check.cpp's text says so for both), so the tree
    leaves its range and the node array grows"""
    return (rebuild.cluster(12, seed=3) + SMALL_AT).astype(f32)


def camera_of(gpu, hs):
    c = gpu.Camera()
    C.memmove(C.byref(c), C.byref(hs.desc.contents.cam), C.sizeof(gpu.Camera))
    return c


def with_file(sc, obj, path, tris):
    scenes.write_stl(path, tris)
    out = json.loads(json.dumps(sc))
    out["objects"][obj]["file"] = path
    return out


def batch_frames(ds, n):
    """frames 0 .. n-1 of the handle's camera path in one launch, as numpy"""
    import torch
    dev = torch.device("cuda:0")
    depth = torch.zeros(n * H * W, dtype=torch.float32, device=dev)
    color, normal = torch.zeros(n * H * W * 3, dtype=torch.float32, device=dev), torch.zeros(n * H * W * 3, dtype=torch.float32, device=dev)
    ds.render_device_batch(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), n_frames=n, frame_stride_px=H * W, bounces=BOUNCES)
    torch.cuda.synchronize()
    return [dict(depth=depth.cpu().numpy().reshape(n, H, W)[k], color=color.cpu().numpy().reshape(n, H, W, 3)[k],
                 normal=normal.cpu().numpy().reshape(n, H, W, 3)[k]) for k in range(n)]


def equals_fresh(gpu, upd, fresh_scene, fresh, what, same_trees):
    """the frames bit for bit and the guard state of every mesh; same_trees: every tree of `upd` is the builder's own, so the kernel
    build and the work counters are compared too (a rebuilt mesh is walked through another tree: same frame, other work)"""
    if same_trees:
        return base.assert_equals_fresh(gpu, upd, fresh_scene, what, bounces=BOUNCES, fresh=fresh)
    rebuild.assert_equals_fresh(gpu, upd, fresh, what, bounces=BOUNCES)
    state = [upd.guard_state(m) for m in base.mesh_objects(fresh_scene)]
    assert state == [fresh.guard_state(m) for m in base.mesh_objects(fresh_scene)], what
    return state


def test_one_handle_through_every_grow_path(gpu, tmp_path):
    """lights 1 -> 5 -> 0 -> 2, materials 2 -> 4, three plane records -> four, a tree that leaves its node range, cameras 1 -> 3 -> 1;
    then one rejected call of each kind, after each of which the frame is still the fresh handle's"""
    sc = objects.room_scene(tmp_path, "grow", W, H)
    sc["lights"], sc["materials"] = objects.LIGHTS[:1], objects.MATERIALS[:2]
    sc["objects"][objects.ROOM_SMALL]["material"] = objects.OTHER
    upd = gpu.DeviceScene(base.parse(gpu, sc))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    cur = {"sc": sc}

    def step(what, apply, **changes):
        cur["sc"] = base.edited(cur["sc"], **changes)
        fresh_scene = base.parse(gpu, cur["sc"])
        out = apply(fresh_scene)
        fresh = gpu.DeviceScene(fresh_scene)
        equals_fresh(gpu, upd, fresh_scene, fresh, what, same_trees=not cur.get("rebuilt"))
        return out, fresh_scene, fresh

    rng = np.random.default_rng(4)
    five = [{"type": "point", "point": [float(x) for x in rng.uniform(-3, 3, 3) + (0, 2, 0)], "color": [0.3, 0.3, 0.3]} for _ in range(5)]
    for what, lights in (("1 -> 5 lights", five), ("5 -> 0 lights", []), ("0 -> 2 lights", objects.LIGHTS)):
        step(what, lambda fs: upd.set_lights(base.desc_lights(fs)), lights=lights)
        assert upd.n_lights == len(lights)
    step("2 -> 4 materials", lambda fs: upd.set_materials(base.desc_materials(fs)), materials=objects.MATERIALS)

    tilted = objects.with_objects(cur["sc"], {0: dict(normal=[1, 0.25, 0]), 1: dict(normal=[-1, 0.25, 0]), objects.ROOM_SMALL: dict(material=objects.MIRROR)})
    step("two walls tilted off their axis: a general pair behind the axis triple", lambda fs: upd.set_objects(objects.desc_objects(fs)), objects=tilted["objects"])

    moved_scene = with_file(cur["sc"], objects.ROOM_SMALL, str(tmp_path / "grow_cluster.stl"), outgrowing_set())
    cur["rebuilt"] = True
    info, _, _ = step("the 12-triangle mesh rebuilt from a cluster", lambda fs: upd.rebuild_mesh(objects.ROOM_SMALL, base.desc_tris(fs, objects.ROOM_SMALL)),
                      objects=moved_scene["objects"])
    assert info["moved"] == 1 and info["fell_back"] == 0 and info["builder"] == 0, info

    # ---- a camera path of 3 cameras: frame k is the frame of a handle created with camera k; then 1 camera again ----
    eyes = [cur["sc"]["camera"]["eye"], [-0.6, 0.5, -0.9], [0.9, -0.4, -1.3]]
    per_eye = [base.parse(gpu, base.edited(cur["sc"], camera=dict(cur["sc"]["camera"], eye=e))) for e in eyes]
    upd.set_cameras([camera_of(gpu, hs) for hs in per_eye])
    upd.set_variant(gpu.VAR_AUTO)
    for k, (got, hs) in enumerate(zip(batch_frames(upd, 3), per_eye)):
        want = gpu.DeviceScene(hs).render(bounces=BOUNCES)
        for plane in base.FRAME:
            assert same_bits(got[plane], want[plane]), f"camera {k} of 3: {plane}"
    _, fresh_scene, fresh = step("1 camera again", lambda fs: upd.set_cameras([camera_of(gpu, fs)]))

    # ---- one rejected call of each kind ----
    want = base.frame(fresh, gpu.VAR_AUTO)
    bad_light = base.desc_lights(fresh_scene)
    bad_light[0] = _lib.Light(type=7)
    other_size = camera_of(gpu, fresh_scene)
    other_size.w += 1
    small = base.desc_tris(fresh_scene, objects.ROOM_SMALL)
    rejected = [("a light of no type", lambda: upd.set_lights(bad_light)),
                ("one material for objects that use four", lambda: upd.set_materials(base.desc_materials(fresh_scene)[:1])),
                ("one object fewer", lambda: upd.set_objects(objects.desc_objects(fresh_scene)[:-1])),
                ("a rebuild with one triangle fewer", lambda: upd.rebuild_mesh(objects.ROOM_SMALL, small[:-1])),
                ("an update with a vertex that is not finite", lambda: upd.update_mesh(objects.ROOM_SMALL, np.where(np.arange(small.size).reshape(small.shape) == 5, f32(np.inf), small))),
                ("cameras of two sizes", lambda: upd.set_cameras([camera_of(gpu, fresh_scene), other_size]))]
    for what, call in rejected:
        with pytest.raises(RuntimeError):
            call()
        base.assert_same_frame(base.frame(upd, gpu.VAR_AUTO), want, f"after the rejected call: {what}")
    assert [upd.guard_state(m) for m in base.mesh_objects(fresh_scene)] == [fresh.guard_state(m) for m in base.mesh_objects(fresh_scene)]


def test_a_linear_mesh_keeps_its_device_nodes_when_the_node_array_moves(gpu, tmp_path):
    """Mesh A: 70 triangles, 65 of them in the eye's plane z = 0.5, more than the guard has records for, so A is walked linearly and its
    nodes on the device carry unbounded boxes that the host copy does not hold.  Mesh B's new tree leaves its range: the node array
    grows, and what it held must arrive in the new one from the DEVICE."""
    a = base._guard_tris(65, n_other=5, seed=8, zero_area=False)
    b = base._guard_tris(0, n_other=12, seed=6, zero_area=False) + f32([2.5, 0.0, 0.0])
    sc = base._guard_scene(tmp_path, "linear", [a, b], base.OFF, eye=[0.3, 3.0, 0.5], w=W, h=H)
    upd = gpu.DeviceScene(base.parse(gpu, sc))
    assert upd.guard_state(0) == ([], True), upd.guard_state(0)
    upd.render(bounces=BOUNCES)
    fresh_scene = base.parse(gpu, with_file(sc, 1, str(tmp_path / "linear_cluster.stl"), outgrowing_set()))
    info = upd.rebuild_mesh(1, base.desc_tris(fresh_scene, 1))
    assert info["moved"] == 1 and info["fell_back"] == 0 and info["builder"] == 0, info
    state = equals_fresh(gpu, upd, fresh_scene, gpu.DeviceScene(fresh_scene), "B rebuilt into a new node range beside the linear A", same_trees=False)
    assert state[0] == ([], True), state
