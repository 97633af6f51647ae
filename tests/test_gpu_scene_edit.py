"""Live lights and materials on the GPU (include/cutrace_edit.h): a handle whose lights or materials were replaced
through set_lights / set_materials against a handle freshly created from the edited description — depth, normal, colour and ray
count BITWISE under the default build and under VAR_EXACT_POW, the handle's own VAR_NO_CLUSTER walk, the kernel build, the work
counters under VAR_STATS and the guard state.  Every case runs with the guard's plane scan on the device and again on the host
(CUTRACE_GUARD_SCAN), and the guard states of the two runs are compared.  Every frame is 96 x 54 or smaller."""
import ctypes as C

import numpy as np
import pytest

from cutrace_amd import _lib
from tests.gpu_support import assert_same_frame, gpu  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, KV_MERGE, OFF, assert_equals_fresh, assert_queries_equal_fresh, base_scene, desc_lights, desc_materials, desc_tris,
                        each_scan, edited, frame, guard_scene, guard_tris, random_mesh)
from tests.util import parse

pytestmark = pytest.mark.gpu

f32 = np.float32
POINT, SUN = 1, 0                 # CTR_LIGHT_POINT, CTR_LIGHT_SUN


# ---------------------------------------------------------------- lights

def _light_steps():
    point = {"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]}
    sun = {"type": "sun", "direction": [-0.3, -1.0, -0.2], "color": [0.4, 0.4, 0.4]}
    rng = np.random.default_rng(7)

    def some(n):
        out = []
        for k in range(n):
            c = [float(x) for x in rng.uniform(0.0, 2.0 / n, 3)]
            if k % 3 == 2:
                out.append({"type": "sun", "direction": [float(x) for x in rng.uniform(-1, 1, 3) - (0, 1.5, 0)], "color": c})
            else:
                out.append({"type": "point", "point": [float(x) for x in rng.uniform(-3, 3, 3) + (0, 4, 0)], "color": c})
        return out
    return [("the point light moved", [dict(point, point=[-0.7, 1.9, 3.0]), sun]),
            ("colours 0 and negative", [dict(point, color=[0.0, 0.0, 0.0]), dict(sun, color=[-0.2, 0.4, 0.1])]),
            ("point and sun swapped", [dict(sun, direction=[0.4, -1.0, 0.3]), dict(point, point=[0.2, 3.0, 1.0])]),
            ("2 -> 0 lights", []),
            ("0 -> 5 lights", some(5)),
            ("5 -> 33 lights", some(33))]


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_edited_lights_equal_a_fresh_handle(gpu, tmp_path, monkeypatch, n):
    sc = base_scene(tmp_path, "lights", random_mesh(n, seed=n))

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.render(bounces=BOUNCES)                                  # (a handle with history: buffers, tile costs)
        states = []
        for what, lights in _light_steps():
            fresh_scene = parse(gpu, edited(sc, lights=lights))
            upd.set_lights(desc_lights(fresh_scene))
            assert upd.n_lights == len(lights)
            fresh = gpu.DeviceScene(fresh_scene)
            states.append(assert_equals_fresh(gpu, upd, fresh, f"{n} triangles, {what}", same_trees=True))
            assert_queries_equal_fresh(upd, fresh, len(lights), f"{n} triangles, {what}")
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- materials

def _mirror_mesh(n, k, seed):
    """random_mesh with its first k triangles in the plane y = -2.8: the plane that holds the image of EYE in the floor y = -1"""
    tris = random_mesh(n, seed)
    rng = np.random.default_rng(seed + 1)
    for i in range(k):
        c = rng.uniform(-1, 1, 2)
        tris[i] = [[c[0] + dx, -2.8, c[1] + dz] for dx, dz in ((0, 0), (0.3, 0.05), (0.1, 0.35))]
    return tris


def test_edited_materials_equal_a_fresh_handle(gpu, tmp_path, monkeypatch):
    sc = base_scene(tmp_path, "mats", _mirror_mesh(65, 3, seed=21))
    sc["camera"]["eye"] = [0.3, 0.8, 4.0]
    MESH, FLOOR = 0, 1
    steps = [("floor transmits", FLOOR, dict(transparency=0.4)), ("floor opaque again", FLOOR, dict(transparency=0.0)),
             ("floor reflects: a mirror", FLOOR, dict(reflexivity=0.3)), ("floor reflects no more", FLOOR, dict(reflexivity=0.0)),
             ("mesh reflects and transmits", MESH, dict(transparency=0.5)), ("mesh opaque again", MESH, dict(transparency=0.0)),
             ("phong exponent 5000", MESH, dict(phong_exp=5000.0)), ("phong exponent 40 again", MESH, dict(phong_exp=40.0))]

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        fresh_scene = parse(gpu, sc)                                 # follows the edits through HostScene.set_material
        frame(upd, gpu.VAR_AUTO)
        kernel0 = upd.last_kernel()
        states, kernels = [], {}
        for what, idx, kw in steps:
            fresh_scene.set_material(idx, **kw)
            upd.set_material(idx, **kw)
            states.append(assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), what, same_trees=True))
            frame(upd, gpu.VAR_AUTO)
            kernels[what] = upd.last_kernel()
        assert kernels["floor transmits"] != kernel0, "a transmitting material: the any-hit shadow build must go"
        assert kernels["floor opaque again"] == kernel0, "... and come back"
        assert states[2] == [([0, 1, 2], False)] and states[1] == states[3] == [([], False)], "the mirror's virtual eye lies in the plane of 3 triangles"
        assert kernels["mesh reflects and transmits"] != kernel0 and kernels["mesh opaque again"] == kernel0
        assert kernels["phong exponent 5000"] != kernel0, "the fast specular path is outside the colour tolerance at 5000"
        assert kernels["phong exponent 40 again"] == kernel0
        # the count 2 -> 3 -> 2, then 1: rejected while the floor uses index 1
        two = desc_materials(fresh_scene)
        upd.set_materials(two + [two[0]])
        states.append(assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "three materials, the third unused", same_trees=True))
        upd.set_materials(two)
        states.append(assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "two materials again", same_trees=True))
        before = frame(upd, gpu.VAR_AUTO)
        with pytest.raises(RuntimeError, match=r"ctr_scene_set_materials failed \(1\).*material index out of range"):
            upd.set_materials(two[:1])
        bad = _lib.Material()
        C.memmove(C.byref(bad), C.byref(two[0]), C.sizeof(bad))
        bad.type = 7
        with pytest.raises(RuntimeError, match=r"ctr_scene_set_materials failed \(1\).*bad type"):
            upd.set_materials([two[0], bad])
        with pytest.raises(RuntimeError, match=r"ctr_scene_set_lights failed \(1\).*bad type"):
            upd.set_lights([_lib.Light(2, _lib.Vec3(0, 1, 0), _lib.Vec3(1, 1, 1))])
        assert_same_frame(frame(upd, gpu.VAR_AUTO), before, "after the rejected edits")
        states.append(assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "after the rejected edits", same_trees=True))
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- the guard, through a light

IN_POINT = [{"type": "point", "point": [3.0, -1.0, 0.5], "color": [0.9, 0.9, 0.9]}]
OFF_SUN = [{"type": "sun", "direction": [0.3, -0.8, 0.5], "color": [0.9, 0.9, 0.9]}]
IN_SUN = [{"type": "sun", "direction": [0.3, -0.8, 0.0], "color": [0.9, 0.9, 0.9]}]      # parallel to z = 0.5, to no filler


@pytest.mark.parametrize("k", [3, 70])
def test_a_light_moved_into_the_plane_of_triangles_and_out_again(gpu, tmp_path, monkeypatch, k):
    """guard records (3), the linear fallback (70 > CTR_GUARD_SLOTS) and back to plain culling, through a point light and a sun"""
    sc = guard_scene(tmp_path, f"through_{k}", [guard_tris(k)], OFF)
    want_in = ([], True) if k > 64 else (list(range(k)), False)

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        assert upd.guard_state(0) == ([], False)
        states = []
        for what, lights, want in (("point light in the plane", IN_POINT, want_in), ("out again", OFF, ([], False)),
                                   ("a sun off the plane", OFF_SUN, ([], False)), ("the sun parallel to the plane", IN_SUN, want_in),
                                   ("a point light off the plane", OFF, ([], False))):
            fresh_scene = parse(gpu, edited(sc, lights=lights))
            upd.set_lights(desc_lights(fresh_scene))
            assert upd.guard_state(0) == want, f"{k} triangles in the plane, {what}: {upd.guard_state(0)}"
            states += assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"{k} triangles in the plane, {what}", bounces=2, same_trees=True)
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- the device scan's edges

def _stack(n, first=0, seed=0):
    """n triangles, file triangle i alone in the plane z = level(first + i)"""
    rng = np.random.RandomState(seed + n)
    tris = []
    for i in range(n):
        c = rng.uniform(-1, 1, 2)
        tris.append([[c[0] + dx, c[1] + dy, _level(first + i)] for dx, dy in ((0, 0), (0.3, 0.05), (0.1, 0.35))])
    return np.asarray(tris, f32)


def _level(i):
    return float(f32(0.5 + 0.05 * i))     # 0.05 apart: three orders of magnitude above the guard's tolerance at this scene's size


def _point_at(z):
    return [_lib.Light(POINT, _lib.Vec3(3.0, -1.0, z), _lib.Vec3(0.9, 0.9, 0.9))]


@pytest.mark.parametrize("sizes", [(1,), (63,), (64,), (65,), (257,), (65, 64)])
def test_every_leaf_position_answers_for_itself(gpu, tmp_path, monkeypatch, sizes):
    """Every triangle lies alone in a plane of its own, and the light visits every plane in turn: whichever leaf position a
    triangle has — 0, 63, 64, n - 1, the last of the first mesh, the first of the second (whose range starts in the middle of
    a word) — exactly that triangle is guarded, in its own mesh.  The first, a middle and the last visit also render."""
    meshes, first = [], 0
    for n in sizes:
        meshes.append(_stack(n, first))
        first += n
    sc = guard_scene(tmp_path, "stack_" + "_".join(map(str, sizes)), meshes, OFF)

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        states, first = [], 0
        for m, n in enumerate(sizes):
            for i in range(n):
                upd.set_lights(_point_at(_level(first + i)))
                got = [upd.guard_state(q) for q in range(len(sizes))]
                assert got == [([i], False) if q == m else ([], False) for q in range(len(sizes))], (m, i, got)
                states.append(got)
                if i in (0, n // 2, n - 1):
                    fresh_scene = parse(gpu, edited(sc, lights=[{"type": "point", "point": [3.0, -1.0, _level(first + i)], "color": [0.9, 0.9, 0.9]}]))
                    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"meshes {sizes}: mesh {m}, triangle {i}", bounces=1, same_trees=True)
            first += n
        return states
    each_scan(monkeypatch, body)


def test_sixty_four_stay_guarded_sixty_five_go_linear_and_no_light_at_all(gpu, tmp_path, monkeypatch):
    """64 triangles in z = 0.5, 65 in z = 0.8 (and zero-area ones in both, which never count), one elsewhere; then no light at
    all, with the eye in the first plane: the eye is the only probe"""
    a, b = guard_tris(64, n_other=1, seed=3), guard_tris(65, n_other=0, seed=4)
    b[:, :, 2] = f32(0.8)
    mesh = np.concatenate([a, b])
    n_a = len(a)
    sc = guard_scene(tmp_path, "slots", [mesh], OFF)
    sc_eye = guard_scene(tmp_path, "slots_eye", [mesh], OFF, eye=[0.3, 0.8, 0.5])

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        states = []
        for what, z, want in (("64 in the plane", 0.5, (list(range(64)), False)), ("65 in the plane", 0.8, ([], True)),
                              ("64 again", 0.5, (list(range(64)), False))):
            fresh_scene = parse(gpu, edited(sc, lights=[dict(OFF[0], point=[3.0, -1.0, z])]))
            upd.set_lights(desc_lights(fresh_scene))
            assert upd.guard_state(0) == want, (what, upd.guard_state(0))
            states += assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), what, bounces=2, same_trees=True)
        assert n_a == 64 + 1 + 2
        eye = gpu.DeviceScene(parse(gpu, sc_eye))
        eye.set_lights([])
        assert eye.guard_state(0) == (list(range(64)), False), eye.guard_state(0)
        states += assert_equals_fresh(gpu, eye, gpu.DeviceScene(parse(gpu, edited(sc_eye, lights=[]))), "no light, the eye in the plane", bounces=2, same_trees=True)
        return states
    each_scan(monkeypatch, body)


# ---------------------------------------------------------------- with the other edits

def test_mesh_updates_and_light_edits_in_turn(gpu, tmp_path, monkeypatch):
    """update_mesh, set_lights, update_mesh, set_lights: the scan's planes on the device follow the mesh (the second update finds
    them there already and replaces the mesh's range), and a light in the plane of the moved triangles guards them.  The
    triangle count is fixed by contract: the mesh has 9 candidates, of which the first k lie in z = 0.5."""
    other = random_mesh(64, seed=31, spread=0.5) + f32([1.5, 0.5, -1.0])

    def tris(step, k):
        t = guard_tris(9, n_other=60, seed=30, zero_area=False)             # (shifted below: three points of a line would not stay one)
        t[k:9, :, 2] += f32(0.21)                                     # the others: z = 0.71, in nobody's plane
        t[:, :, 0] += f32(0.1 * step)                                 # (every triangle moves within its plane)
        return t

    def scene(step, k, lights):
        return guard_scene(tmp_path, f"mixed_{step}_{k}", [tris(step, k), other], lights)

    def body():
        upd = gpu.DeviceScene(parse(gpu, scene(0, 0, OFF)))
        upd.render(bounces=2)
        states = []
        for what, step, k, lights, want in (("update_mesh: 5 triangles into z = 0.5", 1, 5, OFF, []),
                                            ("set_lights: into that plane", 1, 5, IN_POINT, [0, 1, 2, 3, 4]),
                                            ("update_mesh: 9 triangles in the plane", 2, 9, IN_POINT, list(range(9))),
                                            ("set_lights: out of the plane", 2, 9, OFF, [])):
            fresh_scene = parse(gpu, scene(step, k, lights))
            if what.startswith("update_mesh"):
                upd.update_mesh(0, desc_tris(fresh_scene, 0))
            else:
                upd.set_lights(desc_lights(fresh_scene))
            assert upd.guard_state(0) == (want, False), (what, upd.guard_state(0))
            # the counters: of a handle CREATED with these lights (its guard is the host's, made at creation) whose mesh then got
            # the same vertices, so that both walk the same refitted tree
            ref = gpu.DeviceScene(parse(gpu, scene(0, 0, lights)))
            ref.update_mesh(0, desc_tris(fresh_scene, 0))
            states += assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), what, bounces=2, counters_of=ref)
        return states
    each_scan(monkeypatch, body)


def test_the_merged_tree_stays_in_use_across_a_light_edit(gpu, tmp_path, monkeypatch):
    a, b = guard_tris(4, n_other=40, seed=1), guard_tris(3, n_other=40, seed=2, zero_area=False) + f32([0.4, 0.3, 0.0])
    sc = guard_scene(tmp_path, "merged", [a, b], OFF)

    def body():
        upd = gpu.DeviceScene(parse(gpu, sc))
        upd.set_variant(gpu.VAR_MERGE)
        upd.render(bounces=2)
        assert upd.last_kernel() & KV_MERGE, "the scene of two meshes walks its merged tree"
        states = []
        for what, lights, want in (("into the plane", IN_POINT, [([0, 1, 2, 3], False), ([0, 1, 2], False)]), ("out again", OFF, [([], False)] * 2)):
            fresh_scene = parse(gpu, edited(sc, lights=lights))
            upd.set_lights(desc_lights(fresh_scene))
            fresh = gpu.DeviceScene(fresh_scene)
            fresh.set_variant(gpu.VAR_MERGE)
            states += assert_equals_fresh(gpu, upd, fresh, f"merged tree, light {what}", bounces=2, base=gpu.VAR_MERGE, same_trees=True)
            assert states[-2:] == want, (what, states[-2:])
            upd.render(bounces=2)
            assert upd.last_kernel() & KV_MERGE, f"light {what}: {upd.last_kernel():#x}"
        return states
    each_scan(monkeypatch, body)
