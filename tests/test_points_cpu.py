"""The surface-shading C-ABI (ctr_shade_points, include/cutrace_rays.h) without a GPU, and the NumPy checker of its GPU
tests (tests/points_ref.py) pinned against the C oracle."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from cutrace_amd import _lib
from tests import points_ref, shade_ref
from tests.conftest import load_scene
from tests.util import TOL

ROOT = _lib.ROOT


def test_shade_points_is_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "cutrace_rays.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ctr_shade_points" in re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", txt)
    assert "ctr_shade_points" in _lib.RAY_SYMBOLS and "ctr_shade_points" not in _lib.HIP_SYMBOLS
    L = _lib.hip_lib()
    assert hasattr(L, "ctr_shade_points"), "libcutrace_amd.so does not export ctr_shade_points"
    assert L.ctr_abi_version() == 3


def test_point_query_mirror_has_the_header_layout(tmp_path):
    """sizeof / offsetof of ctr_point_query as the C compiler lays it out, against the ctypes mirror"""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    fields = [f for f, _ in _lib.PointQuery._fields_]
    assert fields == ["n_points", "flags", "material", "ambient", "reserved", "d_point", "d_normal", "d_view", "d_material",
                      "d_object", "d_color", "d_light_shadow"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_rays.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ctr_point_query));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(ctr_point_query, {f}));\n' for f in fields) +
                   '  printf("%u %u\\n", CTR_POINTS_LINEAR, CTR_POINTS_EXACT_POW);\n'
                   '  printf("%zu %zu\\n", sizeof(ctr_shade_query), sizeof(ctr_ray_query));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.PointQuery) == 80
    assert got[1:-4] == [getattr(_lib.PointQuery, f).offset for f in fields]
    import cutrace_amd as ca
    assert got[-4:-2] == [ca.POINTS_LINEAR, ca.POINTS_EXACT_POW] == [1, 2]
    assert got[-2:] == [C.sizeof(_lib.ShadeQuery), C.sizeof(_lib.RayQuery)] == [72, 112]  # the other two queries are untouched


def test_shade_points_validates_before_the_gpu_is_touched():
    L = _lib.hip_lib()
    P = 0x1000  # (never dereferenced: every call fails first)

    def q(**kw):
        x = _lib.PointQuery()
        x.n_points = 4
        x.d_point, x.d_normal, x.d_view, x.d_color = P, P, P, P
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def bad(x, text):
        assert L.ctr_shade_points(None, C.byref(x) if x is not None else None, None) == 1, text
        assert text.encode() in L.ctr_last_error(), (text, L.ctr_last_error())

    bad(q(), "null scene")
    bad(q(d_color=None, d_light_shadow=P, d_normal=None, d_view=None), "null scene")  # a valid shadow-only query
    bad(None, "null query")
    bad(q(flags=4), "unknown flag")
    bad(q(flags=8), "unknown flag")
    bad(q(d_color=None), "no output")
    bad(q(d_normal=None), "d_color needs d_normal and d_view")
    bad(q(d_view=None), "d_color needs d_normal and d_view")
    bad(q(d_material=P, d_object=P), "exclude each other")
    # what needs the scene's arrays (the scalar material's range, the pointers' device, the walk stack's size) comes
    # after the scene check; tests/test_gpu_points.py::test_bad_arguments covers it on a live scene


def test_device_scene_has_shade_points():
    import cutrace_amd as ca
    sig = inspect.signature(ca.DeviceScene.shade_points)
    assert list(sig.parameters) == ["self", "points", "normals", "view_dirs", "materials", "objects", "ambient", "exact_pow",
                                    "linear", "outputs", "stream"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["normals"] is None and d["view_dirs"] is None and d["materials"] is None and d["objects"] is None
    assert d["ambient"] is None and d["exact_pow"] is False and d["linear"] is False and d["stream"] is None
    assert d["outputs"] == ("color",)
    assert (ca.POINTS_LINEAR, ca.POINTS_EXACT_POW) == (1, 2)
    assert set(ca._RAY_OUT) == {"t", "object", "prim", "point", "normal", "uv", "color"}  # no key was added


def test_shade_points_raises_before_a_device_is_needed(ca):
    """every ValueError / TypeError of the Python method, on a handle that was never created"""
    ds = object.__new__(ca.DeviceScene)
    ds.device, ds.n_lights, ds._ambient, ds._h = 0, 2, 0.1, None
    n = 5
    p = np.zeros((n, 3), np.float32)
    idx = np.zeros(n, np.int32)
    ok = dict(normals=p, view_dirs=p, materials=0)
    for kw in (dict(ok, outputs=()), dict(ok, outputs=("depth",)), dict(ok, outputs=("color", "color")),
               dict(ok, objects=idx),                                           # both materials and objects
               dict(normals=p, view_dirs=p),                                    # neither, with colour
               dict(view_dirs=p, materials=0), dict(normals=p, materials=0),    # colour without normals / view_dirs
               dict(ok, normals=p[:3]), dict(ok, view_dirs=p.astype(np.float64)), dict(ok, normals=np.zeros((n, 2), np.float32)),
               dict(normals=p, view_dirs=p, materials=idx[:3]), dict(normals=p, view_dirs=p, objects=idx[:3]),
               dict(normals=p, view_dirs=p, materials=idx.astype(np.int64)), dict(normals=p, view_dirs=p, objects=idx.reshape(n, 1))):
        with pytest.raises(ValueError):
            ds.shade_points(p, **kw)
    with pytest.raises(ValueError):
        ds.shade_points(np.zeros((n, 4), np.float32), **ok)
    with pytest.raises(ValueError):
        ds.shade_points(p.astype(np.float64), outputs=("light_shadow",))
    with pytest.raises(TypeError):
        ds.shade_points([[0.0, 0.0, 0.0]], **ok)
    with pytest.raises(TypeError):
        ds.shade_points(p, normals=p, view_dirs=p, materials=[0] * n)


@pytest.mark.parametrize("name", ["bunny", "mirror", "sphere_plane"])
def test_points_ref_reproduces_the_oracle(ca, name):
    """points_ref fed the primary hits of the camera's rays (point, normal, the hit object's material, the ray direction)
    against the oracle's frame at bounces = 0: hit pixels within TOL (the bar shade_ref is held to), NaN positions equal"""
    w, h = 48, 27
    s = load_scene(ca, name, w, h)
    sc = shade_ref.ShadeScene(s)
    _, d, r, hit = points_ref.primary_hits(sc)
    assert hit.any()
    got = points_ref.shade_points(sc, r["point"][hit], r["normal"][hit], d[hit], sc.obj_mat[r["object"][hit]])
    g = oracle.oracle_render(s, fudge=1e-3, bounces=0, threads=os.cpu_count() or 4, hit_ids=True)
    assert np.array_equal(r["object"], g["hit_id"].reshape(-1))
    # the cheaper way to the same points that tests/test_gpu_points.py takes at 96x54: the oracle's hits
    _, d2, r2, hit2 = points_ref.oracle_hits(sc, g)
    assert np.array_equal(hit2, hit) and np.array_equal(d2, d)
    for k in ("t", "point", "normal"):
        assert np.array_equal(r2[k][hit].view(np.uint32), r[k][hit].view(np.uint32)), k
    want = g["color"].reshape(-1, 3)[hit]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    diff = np.abs(np.nan_to_num(got).astype(np.float64) - np.nan_to_num(want))
    print(f"{name}: colour max|diff| {diff.max():.3e}, {int(hit.sum())} hits")
    assert diff.max() <= TOL, f"{name}: {diff.max()}"
    # the shadow matrix is phong's: where it says a light is fully blocked for every light, only the ambient term is left
    ls = points_ref.light_shadow(sc, r["point"][hit])
    assert ls.shape == (int(hit.sum()), len(sc.lights)) and ((ls >= 0) & (ls <= 1)).all()
    dark = (ls >= 1).all(1)
    amb = (sc.mat_color[sc.obj_mat[r["object"][hit]]] * sc.ambient).astype(np.float32)
    assert np.array_equal(got[dark], amb[dark])
