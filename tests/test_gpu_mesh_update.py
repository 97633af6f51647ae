"""Mesh updates on the GPU (include/cutrace_update.h): a handle whose mesh got new vertices through update_mesh
against a handle freshly created from the replaced description — depth, normal and colour BITWISE, under the default build and
under VAR_EXACT_POW — and against its own VAR_NO_CLUSTER walk, which is what catches a box that no longer contains its
triangles.  Every frame is 96 x 54 or smaller; the shapes are the smallest at which each part can go wrong."""
import ctypes as C
import json

import numpy as np
import pytest

from cutrace_amd import _lib, scenes
from tests.util import mesh_scene, same_bits

pytestmark = pytest.mark.gpu

W, H = 96, 54
BOUNCES = 3
KV_MERGE = 512
FRAME = ("depth", "normal", "color")
f32 = np.float32


@pytest.fixture(scope="module")
def gpu(ca):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return ca


def random_mesh(n, seed, spread=0.9, size=0.3):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-spread, spread, (n, 1, 3))
    return (centre + rng.uniform(-size, size, (n, 3, 3))).astype(f32)


def moved(tris, angle, wobble, seed=0, shift=(0.0, 0.0, 0.0)):
    """a rotation about (1, 2, 3) by `angle`, a translation and a per-vertex wobble"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    rng = np.random.default_rng(seed)
    return (tris.astype(np.float64) @ R.T + np.asarray(shift) + rng.uniform(-wobble, wobble, tris.shape)).astype(f32)


def parse(ca, text):
    s = ca.HostScene.parse(text)
    assert s.ok
    return s


def scene_with(ca, tmp_path, name, meshes, w=W, h=H):
    """util.mesh_scene: meshes[0] (reflecting material), a floor, two lights — and the other meshes behind them"""
    paths = []
    for k, t in enumerate(meshes):
        paths.append(str(tmp_path / f"{name}_{k}.stl"))
        scenes.write_stl(paths[-1], t)
    extra = [{"type": "mesh", "file": p, "material": 1} for p in paths[1:]]
    return parse(ca, mesh_scene(paths[0], w, h, meshes[0], extra_objects=extra))


def mesh_objects(hs):
    d = hs.desc.contents
    return [i for i in range(d.n_objects) if d.objects[i].type == 1]


def desc_tris(hs, obj):
    """the triangles of mesh `obj` as the description holds them, (n, 3, 3) float32: exactly what a fresh handle is built from"""
    d = hs.desc.contents
    o = d.objects[obj]
    n = int(o.tri_count)
    raw = C.string_at(C.addressof(d.triangles[int(o.tri_begin)]), n * C.sizeof(_lib.Triangle))
    return np.frombuffer(raw, f32).reshape(n, 3, 3).copy()


def desc_box(hs, obj):
    o = hs.desc.contents.objects[obj]
    return np.array(o.v0.tup(), f32), np.array(o.v1.tup(), f32)


def frame(ds, bits, bounces=BOUNCES):
    ds.set_variant(bits)
    return ds.render(bounces=bounces)


def assert_same_frame(got, want, what):
    for k in FRAME:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words"
    assert got["ray_count"] == want["ray_count"], what


def assert_updated_equals_fresh(ca, upd, fresh, what, bounces=BOUNCES):
    for bits in (ca.VAR_AUTO, ca.VAR_EXACT_POW):
        u = frame(upd, bits, bounces)
        assert_same_frame(u, frame(fresh, bits, bounces), f"{what}, variant {bits}: updated vs fresh")
        assert_same_frame(u, frame(upd, bits | ca.VAR_NO_CLUSTER, bounces), f"{what}, variant {bits}: updated vs its own linear walk")
    upd.set_variant(ca.VAR_AUTO)
    fresh.set_variant(ca.VAR_AUTO)


def assert_box(upd, obj, fresh_scene, what):
    lo, hi = upd.mesh_box(obj)
    want_lo, want_hi = desc_box(fresh_scene, obj)                    # the loader's ctr_mesh_bounds
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), f"{what}: box {lo} {hi}, ctr_mesh_bounds {want_lo} {want_hi}"


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65, 1000])
def test_moved_mesh_equals_a_fresh_handle(gpu, tmp_path, n):
    """one child; one leaf; two leaves; the wave boundary of update_tris; several levels"""
    base = random_mesh(n, seed=n)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "base", [base]))
    upd.render(bounces=BOUNCES)                                      # (a handle with history: buffers, tile costs)
    fresh_scene = scene_with(gpu, tmp_path, "moved", [moved(base, 0.6, 0.05, seed=n)])
    upd.update_mesh(0, desc_tris(fresh_scene, 0))
    assert_box(upd, 0, fresh_scene, f"{n} triangles")
    assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"{n} triangles")


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
        assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"second mesh {name}")


def test_three_updates_in_a_row_carry_nothing_over(gpu, tmp_path):
    base = random_mesh(65, seed=8)
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "row", [base]))
    for k, (angle, wobble) in enumerate(((2.0, 0.3), (-1.0, 0.0), (0.2, 0.6))):
        fresh_scene = scene_with(gpu, tmp_path, f"row_{k}", [moved(base, angle, wobble, seed=k)])
        upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_box(upd, 0, fresh_scene, f"update {k}")
        assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"update {k}")


def _in_plane_scene(ca, tmp_path, name, tris, w, h):
    """the scene of util._coplanar_scene around a mesh of our own: one of its lights lies in the plane of image row `ROW` too"""
    eye, up, look = (0.3, 0.8, 4.0), (0.0, 1.0, 0.0), (-0.05, -0.15, -1.0)
    E, R, v = _row_plane(h)
    stl = str(tmp_path / f"{name}.stl")
    scenes.write_stl(stl, tris)
    sc = {"camera": {"eye": list(eye), "up": list(up), "look": list(look), "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1},
          "lights": [{"type": "point", "point": [1.5, 2.5, 2.0], "color": [0.8, 0.8, 0.8]},
                     {"type": "point", "point": [float(x) for x in (E + f32(0.5) * R + f32(1.0) * v)], "color": [0.5, 0.5, 0.5]}],
          "materials": [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
                        {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.2, "phong": 10}],
          "objects": [{"type": "mesh", "file": stl, "material": 0},
                      {"type": "plane", "point": [0, -1.0, 0], "normal": [0, 1, 0], "material": 1},
                      {"type": "plane", "point": [0, 0, -6.0], "normal": [0, 0, 1], "material": 1}]}
    return parse(ca, json.dumps(sc))


ROW = 12


def _row_plane(h):
    """eye, right and the in-plane direction of image row ROW, as util._coplanar_scene (test_rays_coplanar_with_triangles) builds them"""
    cam = _lib.Camera()
    _lib.host_lib().ctr_camera_look_at(C.byref(cam), _lib.Vec3(0.3, 0.8, 4.0), _lib.Vec3(0.0, 1.0, 0.0), _lib.Vec3(-0.05, -0.15, -1.0))
    E, R, U, F = (np.array(x.tup(), f32) for x in (cam.pos, cam.right, cam.up, cam.forward))
    return E, R, (f32(0.5) - f32(ROW) / f32(h)) * U + F


def _with_in_plane(base, k, h, seed):
    """`base` with its first k triangles put into the plane that holds every primary ray of row ROW"""
    rng = np.random.default_rng(seed)
    E, R, v = _row_plane(h)
    out = base.copy()
    for i in range(k):
        s0, t0 = f32(rng.uniform(-1.2, 1.2)), f32(rng.uniform(2.0, 5.0))
        for p in range(3):
            s, t = s0 + f32(rng.uniform(-0.25, 0.25)), t0 + f32(rng.uniform(-0.4, 0.4))
            out[i, p] = (E + s * R + t * v).astype(f32)
    return out


def test_triangles_moved_into_the_eyes_plane_and_out_again(gpu, tmp_path):
    """guard records (3), the linear fallback (70 > CTR_GUARD_SLOTS), a linear mesh updated to another linear state — its device
    nodes must get the unbounded payload again after the refit wrote real boxes — and back to culling (0)"""
    w, h = 96, 24
    base = moved(random_mesh(100, seed=9, spread=0.8, size=0.25), 0.0, 0.0, shift=(0.0, 1.2, 0.0))   # above the rows' plane
    upd = gpu.DeviceScene(_in_plane_scene(gpu, tmp_path, "plane_base", base, w, h))
    upd.render(bounces=2)
    for step, (k, seed) in enumerate(((3, 1), (70, 2), (70, 3), (0, 4))):
        fresh_scene = _in_plane_scene(gpu, tmp_path, f"plane_{step}", _with_in_plane(moved(base, 0.05 * step, 0.0), k, h, seed), w, h)
        upd.update_mesh(0, desc_tris(fresh_scene, 0))
        assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), f"step {step}: {k} triangles in the eye's plane", bounces=2)


def test_reflective_small_mesh_moved(gpu, tmp_path):
    """a mesh of 12 reflecting triangles is 12 flat mirrors to the guard: the virtual eyes follow it"""
    mirror = random_mesh(12, seed=10, spread=0.6, size=0.5)
    other = moved(random_mesh(200, seed=11, spread=0.7), 0.0, 0.0, shift=(0.3, 0.4, -1.0))
    upd = gpu.DeviceScene(scene_with(gpu, tmp_path, "mirror", [mirror, other]))
    fresh_scene = scene_with(gpu, tmp_path, "mirror_moved", [moved(mirror, 0.8, 0.0, shift=(0.2, 0.1, 0.3)), other])
    upd.update_mesh(0, desc_tris(fresh_scene, 0))
    assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), "reflective mesh of 12")


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
    assert_updated_equals_fresh(gpu, upd, fresh, "after the merged tree retired")


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

    def same(got, want, what):
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), f"{what}: {k}"
    cu, cf = upd.cast_rays(o, d), fresh.cast_rays(o, d)
    same(cu, cf, "cast_rays")
    assert int((cu["object"] == 0).sum()) > n // 10, "the rays are aimed at the mesh"
    same(upd.shade_rays(o, d, bounces=2, outputs=("color", "t", "object", "normal")),
         fresh.shade_rays(o, d, bounces=2, outputs=("color", "t", "object", "normal")), "shade_rays")
    args = dict(normals=cf["normal"], view_dirs=torch.from_numpy(d), objects=cf["object"], outputs=("color", "light_shadow"))
    same(upd.shade_points(cf["point"], **args), fresh.shade_points(cf["point"], **args), "shade_points")


def test_numpy_input_and_tensor_on_its_producing_stream(gpu, tmp_path):
    """both input paths; the tensor is produced on a non-default stream and handed over without a wait in between"""
    import torch
    base = random_mesh(1000, seed=16)
    s = scene_with(gpu, tmp_path, "in", [base])
    from_tensor, from_numpy = gpu.DeviceScene(s), gpu.DeviceScene(s)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    src = torch.from_numpy(base).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        t = src
        for _ in range(20):                                           # (some work for the stream to be busy with)
            t = t * f32(1.01) + f32(0.001)
        t = t.contiguous()
    from_tensor.update_mesh(0, t, stream=stream)
    new = t.cpu().numpy()
    from_numpy.update_mesh(0, new)
    fresh_scene = scene_with(gpu, tmp_path, "in_new", [new])
    assert np.array_equal(desc_tris(fresh_scene, 0).view(np.uint32), new.view(np.uint32))
    fresh = gpu.DeviceScene(fresh_scene)
    assert_updated_equals_fresh(gpu, from_tensor, fresh, "device tensor on its own stream")
    assert_updated_equals_fresh(gpu, from_numpy, fresh, "numpy array")


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
        assert_updated_equals_fresh(gpu, upd, gpu.DeviceScene(fresh_scene), name)
