"""What any GPU test module uses: the `gpu` fixture (imported by name: tests/conftest.py stays as it is), the bitwise frame and
tensor comparisons, the creation-time environment switches, the fixture row of a kernel choice, and the plane room around meshes of
small octahedra.  pytest rewrites `assert` in test modules only, so every assert here says what it compared."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

from cutrace_amd import scenes
from tests.util import fast_pow_kept, same_bits

f32 = np.float32
FRAME = ("depth", "normal", "color")


@pytest.fixture(scope="module")
def gpu(ca):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return ca


def assert_same_frame(got, want, what):
    for k in FRAME:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words"
    assert got["ray_count"] == want["ray_count"], f"{what}: ray count {got['ray_count']} against {want['ray_count']}"


def held(r):
    """a frame that outlives the handle's next render (a pinned render returns views of the handle's block)"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def same_tensors(got, want, what):
    """two results of one call — dicts of tensors, arrays and plain values — hold the same keys, shapes and bits (the times of a
    render aside)"""
    import torch
    assert set(got) == set(want), f"{what}: outputs {sorted(got)} against {sorted(want)}"
    for k in want:
        a, b = got[k], want[k]
        if isinstance(b, torch.Tensor):
            if b.dtype == torch.float32:
                a, b = a.view(torch.int32), b.view(torch.int32)
            assert a.shape == b.shape, f"{what}: {k}: shape {tuple(a.shape)} against {tuple(b.shape)}"
            assert torch.equal(a, b), f"{what}: {k} differs in {int((a != b).sum())} words"
        elif isinstance(b, np.ndarray):
            assert a.shape == b.shape, f"{what}: {k}: shape {a.shape} against {b.shape}"
            assert a.tobytes() == b.tobytes(), f"{what}: {k} differs in {sum(x != y for x, y in zip(a.tobytes(), b.tobytes()))} bytes"
        elif k not in ("kernel_ms", "total_ms"):
            assert a == b, f"{what}: {k}: {a!r} against {b!r}"


def camera_of(ca, hs):
    """a copy of the camera of a parsed description"""
    c = ca.Camera()
    C.memmove(C.byref(c), C.byref(hs.desc.contents.cam), C.sizeof(ca.Camera))
    return c


@contextlib.contextmanager
def env(name):
    """handles created inside see `name`=1 (CUTRACE_NO_SHAPE_BUILD, CUTRACE_NO_WALL_SKIP and CUTRACE_NO_SCENE_HEAD are read when
    a handle is created)"""
    old = os.environ.get(name)
    os.environ[name] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ---- the kernel choice: tests/golden/kernel_choice.npz ----
# the fixture's entry axis (KernelEntry) and whether the caller's buffers qualify for delivery by the kernel
FIXTURE_ENTRY = {"render": (0, 0), "render_pinned": (0, 1), "algorithmic_bytes": (1, 0), "render_uv": (2, 0), "render_ss": (3, 0),
                 "device": (4, 0), "device_ss": (5, 0)}


def expected_kernel(ca, golden, host_scene, mask, entry, bounces):
    """The fixture row of this call: scene flags by the rules of scene_flatten.cpp lights_and_materials, stack shape from bounces.
    The fixture's rows have fast_pow_ok true; a scene whose exponents and colours put the fast specular path outside the
    colour tolerance (tests/util.py fast_pow_kept) gets the row of the same call with VAR_EXACT_POW."""
    d = host_scene.desc.contents
    mats = [d.materials[i] for i in range(d.n_materials)]
    meshes = [d.objects[i].tri_count for i in range(d.n_objects) if d.objects[i].type == 1 and d.objects[i].tri_count]
    all_opaque = all(m.transparency == 0.0 for m in mats)
    need_cold = any(m.transparency >= 1e-6 and m.reflexivity >= 1e-6 for m in mats)
    any_bounce = any(m.transparency >= 1e-6 or m.reflexivity >= 1e-6 for m in mats)
    flags = (1 if all_opaque else 0) | (2 if sum(meshes) >= 1000 else 0) | (4 if len(meshes) >= 2 else 0)
    # the stack shape matters only through "the 6-wave build fits" (the fixture's rows of the cold shapes equal those of the
    # plain ones): stacks of 24 waves plus one parking granule each in granules of 1280 bytes, five per wave at most
    frames, nf = (bounces if bounces > 0 and any_bounce else 1), (10 if need_cold else 4)
    fits = (frames * nf * 64 * 4 + 1280 + 1279) // 1280 <= 5
    bits = (ca.VAR_NO_PREFILTER, ca.VAR_NO_ANYHIT, ca.VAR_NO_CLUSTER, ca.VAR_STATS, ca.VAR_EXACT_POW, ca.VAR_NO_OCC6, ca.VAR_NO_DIRECT,
            ca.VAR_MERGE, ca.VAR_IGNORE_TRANSPARENT)
    if not fast_pow_kept(host_scene):   # KernelFacts::fast_pow_ok false: the row of the same call with VAR_EXACT_POW
        mask |= ca.VAR_EXACT_POW
    m = sum(1 << k for k, b in enumerate(bits) if mask & b)
    e, deliverable = FIXTURE_ENTRY[entry]
    return int(golden[e, m, flags, deliverable, 0 if fits else 1])


# ---- scenes: the flagship's room (five axis-aligned walls, open towards the camera) around meshes of small octahedra ----
def octahedra(centres, r=0.12):
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * r
    tris = [[c + ax[i], c + ax[j], c + ax[k]] for c in np.asarray(centres, np.float64) for i in (0, 1) for j in (2, 3) for k in (4, 5)]
    return np.asarray(tris, f32)


RIGHT = [[0.5, -0.5, -0.3], [0.75, -0.2, 0.1], [0.6, 0.3, -0.5], [0.8, 0.5, 0.2], [0.55, 0.0, 0.3], [0.7, -0.7, -0.6]]   # x >= 0.38: the right half
LIGHTS_IN = [{"type": "point", "point": [0.5, 0.8, 1.5], "color": [0.6, 0.6, 0.6]},
             {"type": "point", "point": [-0.6, 0.7, 1.0], "color": [0.4, 0.4, 0.5]}]
FLOOR = 4   # index of the floor among the walls


def room(tmp_path, name, meshes, w=64, h=48, lights=LIGHTS_IN, sphere=False, transparent=False, floor_y=-1.0, eye=(0.0, 0.0, 2.8)):
    """(scene JSON, index of the first mesh, index of the floor): the meshes, then the five walls, then — `sphere` — a sphere"""
    objs = []
    for k, t in enumerate(meshes):
        path = str(tmp_path / f"{name}_{k}.stl")
        scenes.write_stl(path, np.asarray(t, f32))
        objs.append({"type": "mesh", "file": path, "material": 0})
    walls = [([-1, 0, 0], [1, 0, 0]), ([0, 0, -1], [0, 0, 1]), ([0, 1, 0], [0, -1, 0]), ([1, 0, 0], [-1, 0, 0]), ([0, floor_y, 0], [0, 1, 0])]
    objs += [{"type": "plane", "point": p, "normal": n, "material": 1 + i % 2} for i, (p, n) in enumerate(walls)]
    if sphere:
        objs.append({"type": "sphere", "center": [-0.5, -0.6, 0.0], "radius": 0.3, "material": 2})
    mats = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.3, "phong": 40},
            {"type": "solid", "color": [0.3, 0.5, 0.9], "specular": 0.2, "reflect": 0.1, "phong": 10},
            {"type": "solid", "color": [0.9, 0.9, 0.9], "specular": 0.5, "reflect": 0.2, "phong": 80, "transparency": 0.5 if transparent else 0.0}]
    cam = {"eye": list(eye), "up": [0, 1, 0], "look": [0.0, 0.0, -1.0], "near_plane": 0.1, "far_plane": 100.0, "width": w, "height": h, "ambient": 0.1}
    return json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs}), 0, len(meshes) + FLOOR
