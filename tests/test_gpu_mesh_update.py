"""Mesh updates on the GPU (include/cutrace_update.h): a handle whose mesh got new vertices through update_mesh
against a handle freshly created from the replaced description — depth, normal and colour BITWISE, under the default build and
under VAR_EXACT_POW — and against its own VAR_NO_CLUSTER walk, which is what catches a box that no longer contains its
triangles.  Every frame is 96 x 54 or smaller; the shapes are the smallest at which each part can go wrong."""
import numpy as np
import pytest

from cutrace_amd import scenes
from tests.gpu_support import assert_same_frame, gpu, same_tensors  # noqa: F401  (gpu: the fixture)
from tests.live import (BOUNCES, H, KV_MERGE, W, assert_box, assert_equals_fresh, desc_tris, frame, in_plane_scene, mesh_objects, moved,
                        on_a_busy_stream, random_mesh, scene_with, with_in_plane)
from tests.util import mesh_scene, parse

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65, 1000])
def test_moved_mesh_equals_a_fresh_handle(gpu, tmp_path, n):
    """one child; one leaf; two leaves; the wave boundary of update_tris; several levels"""
    base = random_mesh(n, seed=n)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "base", [base]))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    fresh_scene = scene_with(gpu, tmp_path, "moved", [moved(base, 0.6, 0.05, seed=n)])
    upd.update_mesh(0, desc_tris(fresh_scene, 0))
    assert_box(upd, 0, fresh_scene, f"{n} triangles")
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"{n} triangles")


def test_identity_update_changes_nothing_at_all(gpu, tmp_path):
    """tests/test_mesh_update_cpu.py shows the identity refit reproduces the builder's boxes byte for byte: the frames AND the work
    counters of the walk are those of the untouched handle"""
    s = scene_with(gpu, tmp_path, "identity", [random_mesh(1000, seed=3)])
    untouched, upd = gpu.DeviceScene(s), gpu.DeviceScene(s)
    upd.update_mesh(0, desc_tris(s, 0))
    for bits in (gpu.VAR_AUTO, gpu.VAR_STATS):
        a, b = frame(untouched, bits), frame(upd, bits)
        assert_same_frame(b, a, f"identity, variant {bits}")
        assert np.array_equal(upd.last_counters(), untouched.last_counters()), (bits, upd.last_counters(), untouched.last_counters())


def test_one_mesh_of_two_moves_through_past_and_away(gpu, tmp_path):
    """top-level refit, tl_mn / tl_mx, the scene head's copy of a mesh record"""
    still, mover = random_mesh(64, seed=5, spread=0.5), random_mesh(65, seed=6, spread=0.5)
    s = scene_with(gpu, tmp_path, "two", [still, moved(mover, 0.0, 0.0, shift=(-2.0, 0.0, 0.0))])
    upd = gpu.DeviceScene(s)
    obj = mesh_objects(s)[1]
    upd.render(bounces=BOUNCES)
    for name, shift in (("through", (0.1, 0.0, 0.0)), ("past", (2.2, 0.3, 0.0)), ("far away", (900.0, 50.0, -3000.0))):
        fresh_scene = scene_with(gpu, tmp_path, "two_" + name.replace(" ", "_"), [still, moved(mover, 0.3, 0.02, shift=shift)])
        upd.update_mesh(obj, desc_tris(fresh_scene, obj))
        assert_box(upd, obj, fresh_scene, name)
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"second mesh {name}")


def test_three_updates_in_a_row_carry_nothing_over(gpu, tmp_path):
    base = random_mesh(65, seed=8)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "row", [base]))
    for k, (angle, wobble) in enumerate(((2.0, 0.3), (-1.0, 0.0), (0.2, 0.6))):
        fresh_scene = scene_with(gpu, tmp_path, f"row_{k}", [moved(base, angle, wobble, seed=k)])
        upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_box(upd, 0, fresh_scene, f"update {k}")
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"update {k}")


def test_triangles_moved_into_the_eyes_plane_and_out_again(gpu, tmp_path):
    """guard records (3), the linear fallback (70 > CTR_GUARD_SLOTS), a linear mesh updated to another linear state — its device
    nodes must get the unbounded payload again after the refit wrote real boxes — and back to culling (0)"""
    w, h = 96, 24
    base = moved(random_mesh(100, seed=9, spread=0.8, size=0.25), 0.0, 0.0, shift=(0.0, 1.2, 0.0))   # above the rows' plane
    upd = gpu.DeviceScene(in_plane_scene(gpu, tmp_path, "plane_base", base, w, h))
    upd.render(bounces=2)
    for step, (k, seed) in enumerate(((3, 1), (70, 2), (70, 3), (0, 4))):
        fresh_scene = in_plane_scene(gpu, tmp_path, f"plane_{step}", with_in_plane(moved(base, 0.05 * step, 0.0), k, h, seed), w, h)
        upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {step}: {k} triangles in the eye's plane", bounces=2)


def test_reflective_small_mesh_moved(gpu, tmp_path):
    """a mesh of 12 reflecting triangles is 12 flat mirrors to the guard: the virtual eyes follow it"""
    mirror = random_mesh(12, seed=10, spread=0.6, size=0.5)
    other = moved(random_mesh(200, seed=11, spread=0.7), 0.0, 0.0, shift=(0.3, 0.4, -1.0))
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "mirror", [mirror, other]))
    fresh_scene = scene_with(gpu, tmp_path, "mirror_moved", [moved(mirror, 0.8, 0.0, shift=(0.2, 0.1, 0.3)), other])
    upd.update_mesh(0, desc_tris(fresh_scene, 0))
    assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "reflective mesh of 12")


def test_merged_tree_is_retired_by_an_update(gpu, tmp_path):
    a, b = random_mesh(64, seed=12, spread=0.5), moved(random_mesh(65, seed=13, spread=0.5), 0.0, 0.0, shift=(0.8, 0.2, 0.0))
    s = scene_with(gpu, tmp_path, "merge", [a, b])
    upd = gpu.DeviceScene(s)
    upd.set_variant(gpu.VAR_MERGE)
    upd.render(bounces=BOUNCES)
    assert upd.last_kernel() & KV_MERGE, "the scene of two meshes walks its merged tree before the update"
    obj = mesh_objects(s)[1]
    fresh_scene = scene_with(gpu, tmp_path, "merge_moved", [a, moved(b, 0.5, 0.05, shift=(-0.6, 0.0, 0.2))])
    upd.update_mesh(obj, desc_tris(fresh_scene, obj))
    upd.set_variant(gpu.VAR_MERGE)                                   # (accepted, and builds nothing)
    r = upd.render(bounces=BOUNCES)
    assert not upd.last_kernel() & KV_MERGE, hex(upd.last_kernel())
    fresh = gpu.DeviceScene(fresh_scene)
    assert_same_frame(r, frame(fresh, gpu.VAR_AUTO), "VAR_MERGE after an update: the two-level walk")
    assert_equals_fresh(gpu, upd, fresh, "after the merged tree retired")


def test_queries_see_the_update(gpu, tmp_path):
    import torch
    base = random_mesh(1000, seed=14)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "q", [base]))
    fresh_scene = scene_with(gpu, tmp_path, "q_moved", [moved(base, 0.9, 0.05)])
    upd.update_mesh(0, desc_tris(fresh_scene, 0))
    fresh = gpu.DeviceScene(fresh_scene)
    rng = np.random.default_rng(15)
    n = 4096
    o = (np.array([0.3, 0.8, 4.0]) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
    d = (rng.uniform(-1.2, 1.2, (n, 3)) - o).astype(f32)
    cu, cf = upd.cast_rays(o, d), fresh.cast_rays(o, d)
    same_tensors(cu, cf, "cast_rays")
    assert int((cu["object"] == 0).sum()) > n // 10, "the rays are aimed at the mesh"
    same_tensors(upd.shade_rays(o, d, bounces=2, outputs=("color", "t", "object", "normal")),
                 fresh.shade_rays(o, d, bounces=2, outputs=("color", "t", "object", "normal")), "shade_rays")
    args = dict(normals=cf["normal"], view_dirs=torch.from_numpy(d), objects=cf["object"], outputs=("color", "light_shadow"))
    same_tensors(upd.shade_points(cf["point"], **args), fresh.shade_points(cf["point"], **args), "shade_points")


def test_numpy_input_and_tensor_on_its_producing_stream(gpu, tmp_path):
    """both input paths; the tensor is produced on a non-default stream and handed over without a wait in between"""
    base = random_mesh(1000, seed=16)
    s = scene_with(gpu, tmp_path, "in", [base])
    from_tensor, from_numpy = gpu.DeviceScene(s), gpu.DeviceScene(s)
    t, stream = on_a_busy_stream(base)
    from_tensor.update_mesh(0, t, stream=stream)
    new = t.cpu().numpy()
    from_numpy.update_mesh(0, new)
    fresh_scene = scene_with(gpu, tmp_path, "in_new", [new])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), new.view(np.uint32))
    fresh = gpu.DeviceScene(fresh_scene)
    assert_equals_fresh(gpu, from_tensor, fresh, "device tensor on its own stream")
    assert_equals_fresh(gpu, from_numpy, fresh, "numpy array")


def test_rejected_updates_leave_the_handle_untouched(gpu, tmp_path):
    import torch
    base = random_mesh(65, seed=17)
    s = scene_with(gpu, tmp_path, "bad", [base])
    ds = gpu.DeviceScene(s)
    before, box = frame(ds, gpu.VAR_AUTO), ds.mesh_box(0)
    bad = torch.from_numpy(moved(base, 0.4, 0.0)).to(torch.device("cuda", 0))
    bad[40, 1, 2] = float("nan")
    inf = moved(base, 0.4, 0.0)
    inf[64, 2, 0] = np.inf
    for what, obj, tris in (("wrong count", 0, moved(base, 0.4, 0.0)[:64]), ("not a mesh", 1, base), ("object out of range", 99, base),
                            ("NaN vertex in a device tensor", 0, bad), ("infinite vertex in a host array", 0, inf)):
        with pytest.raises(RuntimeError, match=r"ctr_scene_update_mesh failed \(1\)"):
            ds.update_mesh(obj, tris)
        assert_same_frame(frame(ds, gpu.VAR_AUTO), before, f"after the rejected update ({what})")
        assert all(np.array_equal(x, y) for x, y in zip(ds.mesh_box(0), box)), what
    with pytest.raises(RuntimeError, match=r"ctr_scene_mesh_box failed \(1\)"):
        ds.mesh_box(1)
    empty = str(tmp_path / "empty.stl")
    scenes.write_stl(empty, np.zeros((0, 3, 3), f32))
    es = parse(gpu, mesh_scene(str(tmp_path / "one.stl"), W, H, base, extra_objects=[{"type": "mesh", "file": empty, "material": 1}]))
    with pytest.raises(RuntimeError, match="empty mesh"):
        gpu.DeviceScene(es).update_mesh(2, base[:1])


def test_degenerate_meshes_update_like_any_other(gpu, tmp_path):
    """zero-area triangles among the others, then the whole mesh collapsed to one point: finite input, equals the fresh handle"""
    base = random_mesh(65, seed=18)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "deg", [base]))
    some = moved(base, 0.3, 0.0)
    some[::4, 1] = some[::4, 0]                                      # two vertices coincide
    some[1::8, 2] = (some[1::8, 0] + some[1::8, 1]) * f32(0.5)       # three points of a line
    some[7] = some[7, 0]                                             # a point
    point = np.broadcast_to(f32([0.1, 0.2, 0.3]), base.shape).copy()
    for name, tris in (("zero-area triangles", some), ("collapsed to a point", point), ("and back", moved(base, 1.0, 0.1))):
        fresh_scene = scene_with(gpu, tmp_path, "deg_" + name.replace(" ", "_"), [tris])
        upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_box(upd, 0, fresh_scene, name)
        assert_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), name)
