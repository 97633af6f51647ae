"""The ray-query C-ABI (include/cutrace_rays.h) without a GPU, and the NumPy checker of its GPU tests (tests/ray_ref.py)
pinned against the C oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from cutrace_amd import _lib
from tests import ray_ref
from tests.conftest import load_scene

ROOT = _lib.ROOT


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", txt)))


def test_ray_header_declares_exactly_the_ray_symbols_and_the_library_exports_them():
    names = _declared("cutrace_rays.h")
    assert set(names) == set(_lib.RAY_SYMBOLS), (names, _lib.RAY_SYMBOLS)
    assert not set(names) & set(_lib.HIP_SYMBOLS)
    L = _lib.hip_lib()
    for n in names:
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"


def test_ray_query_mirror_has_the_header_layout(tmp_path):
    """sizeof / offsetof of ctr_ray_query as the C compiler lays it out, against the ctypes mirror"""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    fields = [f for f, _ in _lib.RayQuery._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_rays.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ctr_ray_query));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(ctr_ray_query, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.RayQuery) == 112
    assert got[1:] == [getattr(_lib.RayQuery, f).offset for f in fields]


def test_cast_rays_rejects_a_null_scene_and_unknown_flags():
    L = _lib.hip_lib()
    q = _lib.RayQuery()
    q.n_rays = 4
    q.d_t = 0x1000  # (never dereferenced: the call fails first)
    assert L.ctr_cast_rays(None, C.byref(q), None) == 1
    assert b"null scene" in L.ctr_last_error()
    assert L.ctr_cast_rays(None, None, None) == 1
    assert b"null query" in L.ctr_last_error()
    q.flags = 8
    assert L.ctr_cast_rays(None, C.byref(q), None) == 1
    assert b"unknown flag" in L.ctr_last_error()
    q.flags = 4 | 1  # SHADOW with IGNORE_TRANSPARENT
    assert L.ctr_cast_rays(None, C.byref(q), None) == 1
    assert b"exclude each other" in L.ctr_last_error()


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_primary(scene, what):
    """ray_ref fed the camera's primary rays against the oracle's primary cast (fudge = min_t = 1e-3)"""
    w, h = scene.size
    rs = ray_ref.RefScene(scene)
    o, d = ray_ref.camera_rays(rs.cam)
    r = ray_ref.ray_cast(rs, o, d, np.float32(1e-3))
    g = oracle.oracle_render(scene, fudge=1e-3, bounces=0, threads=os.cpu_count() or 4, hit_ids=True, uv=True)
    assert _same(r["t"], g["depth"].reshape(-1)), what
    assert _same(r["normal"], g["normal"].reshape(-1, 3)), what
    assert np.array_equal(r["object"], g["hit_id"].reshape(-1)), what
    uv, guv = r["uv"], g["uv"].reshape(-1, 2)
    sphere = np.isin(r["object"], [i for i, ob in enumerate(rs.objects) if ob["type"] == ray_ref.OBJ_SPHERE])
    assert np.array_equal(np.isnan(uv), np.isnan(guv)), what
    assert _same(np.nan_to_num(uv[~sphere]), np.nan_to_num(guv[~sphere])), what
    if sphere.any():
        assert np.abs(uv[sphere].astype(np.float64) - guv[sphere]).max() <= 1e-4, what
    # prim: a mesh hit names one of the mesh's triangles, and that triangle gives the reported normal
    mesh = np.isin(r["object"], [i for i, ob in enumerate(rs.objects) if ob["type"] == ray_ref.OBJ_MESH])
    assert (r["prim"][mesh] >= 0).all() and (r["prim"][~mesh] == -1).all(), what
    return int(np.isfinite(r["t"]).sum())


@pytest.mark.parametrize("name,w,h", [("triangle", 24, 18), ("sphere_plane", 48, 27), ("mirror", 40, 24), ("bunny", 40, 24)])
def test_ray_ref_reproduces_the_oracle_primary_cast(ca, name, w, h):
    s = load_scene(ca, name, w, h)
    assert _check_primary(s, name) > 0


@pytest.mark.parametrize("seed", [0, 3, 7])
def test_ray_ref_reproduces_the_oracle_on_random_scenes(ca, seed):
    from tests.util import _random_scene
    s = ca.HostScene.parse(_random_scene(seed, w=40, h=28))
    assert s.ok
    _check_primary(s, f"random scene {seed}")


def test_ray_ref_shadow_loop_and_ignore_transparent_by_hand():
    """Known answers: two transparent quads and an opaque one along +z; the loop adds 1 - transparency per hit in hit
    order, stops at 1, and ignores what lies beyond max_t; ignore_transparent sees only the opaque one."""
    class S:  # a description-free scene for ray_ref (objects in scene order)
        pass
    sc = S()
    quad = lambda z: np.array([[[-1, -1, z], [1, -1, z], [0, 1, z]]], np.float32)
    sc.tris = np.concatenate([quad(2.0), quad(4.0), quad(6.0)])
    sc.objects = [dict(type=ray_ref.OBJ_MESH, mat=m, v0=np.float32([-1, -1, z]), v1=np.float32([1, 1, z]),
                       v2=np.zeros(3, np.float32), f0=np.float32(0), tri_begin=k, tri_count=1)
                  for k, (m, z) in enumerate(((0, 2.0), (0, 4.0), (1, 6.0)))]
    sc.transparency = np.float32([0.375, 0.0])
    sc.transparent = lambda i: float(sc.transparency[sc.objects[i]["mat"]]) >= 1e-6
    o = np.zeros((4, 3), np.float32)
    d = np.tile(np.float32([0, 0, 1]), (4, 1))
    got = ray_ref.shadow_intensity(sc, o, d, np.float32([1.0, 3.0, 5.0, 9.0]))
    assert got.tolist() == [0.0, 0.625, 1.0, 1.0]
    r = ray_ref.ray_cast(sc, o, d, np.float32(1e-3), ignore_transparent=True)
    assert r["object"].tolist() == [2] * 4 and r["t"].tolist() == [6.0] * 4
