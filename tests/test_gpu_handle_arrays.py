"""The scene handle's device arrays through every way they grow (cutrace_amd/csrc/ctr_internal.h GrowBuf / SceneBuf; DESIGN.md §19 .. §21):
ONE handle whose light, material, plane, node and camera arrays each outgrow what ctr_scene_create allocated, one after the other,
against a handle freshly created from the edited description after every step — depth, colour and normal bit for bit, with
everything else tests/live.py's assert_equals_fresh looks at; and a node array that moves while another mesh's
device nodes are the unbounded payload the host copy does not hold.  The existing edit tests grow each array on a handle of its
own; none takes one handle through all of them, and none moves the node array next to a linear mesh.  The helpers are those of
tests/live.py.  Every frame is 48 x 27, bounces 3."""
import json

import numpy as np
import pytest

from cutrace_amd import _lib, scenes
from tests.gpu_support import FRAME, assert_same_frame, camera_of, gpu  # noqa: F401  (gpu: the fixture)
from tests.live import (LIGHTS, MATERIALS, MIRROR, OFF, OTHER, ROOM_SMALL, assert_equals_fresh, desc_lights, desc_materials, desc_objects, desc_tris,
                        edited, frame, guard_scene, guard_tris, mesh_objects, outgrowing_set, room_scene, with_objects)
from tests.util import parse, same_bits

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 48, 27, 3
f32 = np.float32


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


def test_one_handle_through_every_grow_path(gpu, tmp_path):
    """lights 1 -> 5 -> 0 -> 2, materials 2 -> 4, three plane records -> four, a tree that leaves its node range, cameras 1 -> 3 -> 1;
    then one rejected call of each kind, after each of which the frame is still the fresh handle's"""
    sc = room_scene(tmp_path, "grow", W, H)
    sc["lights"], sc["materials"] = LIGHTS[:1], MATERIALS[:2]
    sc["objects"][ROOM_SMALL]["material"] = OTHER
    upd = gpu.DeviceScene(parse(gpu, sc))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    cur = {"sc": sc}

    def step(what, apply, **changes):
        cur["sc"] = edited(cur["sc"], **changes)
        fresh_scene = parse(gpu, cur["sc"])
        out = apply(fresh_scene)
        fresh = gpu.DeviceScene(fresh_scene)
        # once a mesh is rebuilt it is walked through another tree than the fresh handle's: same frame, other work
        assert_equals_fresh(gpu, upd, fresh, what, bounces=BOUNCES, same_trees=not cur.get("rebuilt"))
        return out, fresh_scene, fresh

    rng = np.random.default_rng(4)
    five = [{"type": "point", "point": [float(x) for x in rng.uniform(-3, 3, 3) + (0, 2, 0)], "color": [0.3, 0.3, 0.3]} for _ in range(5)]
    for what, lights in (("1 -> 5 lights", five), ("5 -> 0 lights", []), ("0 -> 2 lights", LIGHTS)):
        step(what, lambda fs: upd.set_lights(desc_lights(fs)), lights=lights)
        assert upd.n_lights == len(lights)
    step("2 -> 4 materials", lambda fs: upd.set_materials(desc_materials(fs)), materials=MATERIALS)

    tilted = with_objects(cur["sc"], {0: dict(normal=[1, 0.25, 0]), 1: dict(normal=[-1, 0.25, 0]), ROOM_SMALL: dict(material=MIRROR)})
    step("two walls tilted off their axis: a general pair behind the axis triple", lambda fs: upd.set_objects(desc_objects(fs)), objects=tilted["objects"])

    moved_scene = with_file(cur["sc"], ROOM_SMALL, str(tmp_path / "grow_cluster.stl"), outgrowing_set())
    cur["rebuilt"] = True
    info, _, _ = step("the 12-triangle mesh rebuilt from a cluster", lambda fs: upd.rebuild_mesh(ROOM_SMALL, desc_tris(fs, ROOM_SMALL)),
                      objects=moved_scene["objects"])
    assert info["moved"] == 1 and info["fell_back"] == 0 and info["builder"] == 0, info

    # ---- a camera path of 3 cameras: frame k is the frame of a handle created with camera k; then 1 camera again ----
    eyes = [cur["sc"]["camera"]["eye"], [-0.6, 0.5, -0.9], [0.9, -0.4, -1.3]]
    per_eye = [parse(gpu, edited(cur["sc"], camera=dict(cur["sc"]["camera"], eye=e))) for e in eyes]
    upd.set_cameras([camera_of(gpu, hs) for hs in per_eye])
    upd.set_variant(gpu.VAR_AUTO)
    for k, (got, hs) in enumerate(zip(batch_frames(upd, 3), per_eye)):
        want = gpu.DeviceScene(hs).render(bounces=BOUNCES)
        for plane in FRAME:
            assert same_bits(got[plane], want[plane]), f"camera {k} of 3: {plane}"
    _, fresh_scene, fresh = step("1 camera again", lambda fs: upd.set_cameras([camera_of(gpu, fs)]))

    # ---- one rejected call of each kind ----
    want = frame(fresh, gpu.VAR_AUTO)
    bad_light = desc_lights(fresh_scene)
    bad_light[0] = _lib.Light(type=7)
    other_size = camera_of(gpu, fresh_scene)
    other_size.w += 1
    small = desc_tris(fresh_scene, ROOM_SMALL)
    rejected = [("a light of no type", lambda: upd.set_lights(bad_light)),
                ("one material for objects that use four", lambda: upd.set_materials(desc_materials(fresh_scene)[:1])),
                ("one object fewer", lambda: upd.set_objects(desc_objects(fresh_scene)[:-1])),
                ("a rebuild with one triangle fewer", lambda: upd.rebuild_mesh(ROOM_SMALL, small[:-1])),
                ("an update with a vertex that is not finite", lambda: upd.update_mesh(ROOM_SMALL, np.where(np.arange(small.size).reshape(small.shape) == 5, f32(np.inf), small))),
                ("cameras of two sizes", lambda: upd.set_cameras([camera_of(gpu, fresh_scene), other_size]))]
    for what, call in rejected:
        with pytest.raises(RuntimeError):
            call()
        assert_same_frame(frame(upd, gpu.VAR_AUTO), want, f"after the rejected call: {what}")
    assert [upd.guard_state(m) for m in mesh_objects(fresh_scene)] == [fresh.guard_state(m) for m in mesh_objects(fresh_scene)]


def test_a_linear_mesh_keeps_its_device_nodes_when_the_node_array_moves(gpu, tmp_path):
    """Mesh A: 70 triangles, 65 of them in the eye's plane z = 0.5, more than the guard has records for, so A is walked linearly and its
    nodes on the device carry unbounded boxes that the host copy does not hold.  Mesh B's new tree leaves its range: the node array
    grows, and what it held must arrive in the new one from the DEVICE."""
    a = guard_tris(65, n_other=5, seed=8, zero_area=False)
    b = guard_tris(0, n_other=12, seed=6, zero_area=False) + f32([2.5, 0.0, 0.0])
    sc = guard_scene(tmp_path, "linear", [a, b], OFF, eye=[0.3, 3.0, 0.5], w=W, h=H)
    upd = gpu.DeviceScene(parse(gpu, sc))
    assert upd.guard_state(0) == ([], True), upd.guard_state(0)
    upd.render(bounces=BOUNCES)
    fresh_scene = parse(gpu, with_file(sc, 1, str(tmp_path / "linear_cluster.stl"), outgrowing_set()))
    info = upd.rebuild_mesh(1, desc_tris(fresh_scene, 1))
    assert info["moved"] == 1 and info["fell_back"] == 0 and info["builder"] == 0, info
    state = assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "B rebuilt into a new node range beside the linear A", bounces=BOUNCES)
    assert state[0] == ([], True), state
