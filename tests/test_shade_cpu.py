"""The radiance-query C-ABI (ctr_shade_rays, include/cutrace_rays.h) without a GPU, and the NumPy checker of its GPU
tests (tests/shade_ref.py) pinned against the C oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from cutrace_amd import _lib
from tests import ray_ref, shade_ref
from tests.conftest import load_scene
from tests.util import TOL

ROOT = _lib.ROOT


def test_shade_rays_is_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "cutrace_rays.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ctr_shade_rays" in re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", txt)
    assert "ctr_shade_rays" in _lib.RAY_SYMBOLS and "ctr_shade_rays" not in _lib.HIP_SYMBOLS
    L = _lib.hip_lib()
    assert hasattr(L, "ctr_shade_rays"), "libcutrace_amd.so does not export ctr_shade_rays"
    assert L.ctr_abi_version() == 3


def test_shade_query_mirror_has_the_header_layout(tmp_path):
    """sizeof / offsetof of ctr_shade_query as the C compiler lays it out, against the ctypes mirror"""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    fields = [f for f, _ in _lib.ShadeQuery._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_rays.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ctr_shade_query));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(ctr_shade_query, {f}));\n' for f in fields) +
                   '  printf("%u %u\\n", CTR_SHADE_LINEAR, CTR_SHADE_EXACT_POW);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.ShadeQuery) == 72
    assert got[1:-2] == [getattr(_lib.ShadeQuery, f).offset for f in fields]
    import cutrace_amd as ca
    assert got[-2:] == [ca.SHADE_LINEAR, ca.SHADE_EXACT_POW] == [1, 2]
    assert C.sizeof(_lib.RayQuery) == 112  # the cast query is untouched


def test_shade_rays_validates_before_the_gpu_is_touched():
    L = _lib.hip_lib()

    def q(**kw):
        x = _lib.ShadeQuery()
        x.n_rays = 4
        x.bounces = 5
        x.d_color = 0x1000  # (never dereferenced: the call fails first)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def bad(scene, x, text):
        assert L.ctr_shade_rays(scene, C.byref(x) if x is not None else None, None) == 1, text
        assert text.encode() in L.ctr_last_error(), (text, L.ctr_last_error())

    bad(None, q(), "null scene")
    bad(None, None, "null query")
    bad(None, q(flags=4), "unknown flag")
    bad(None, q(flags=8), "unknown flag")
    bad(None, q(bounces=-1), "bounces -1")
    bad(None, q(bounces=16), "bounces 16")
    bad(None, q(d_color=None), "d_color")


def test_device_scene_has_shade_rays():
    import inspect
    import cutrace_amd as ca
    sig = inspect.signature(ca.DeviceScene.shade_rays)
    assert list(sig.parameters) == ["self", "origins", "dirs", "bounces", "min_t", "ambient", "exact_pow", "linear", "outputs", "stream"]
    assert sig.parameters["bounces"].default == 5 and sig.parameters["ambient"].default is None
    assert ca.SHADE_OUTPUTS == ("color", "t", "object", "normal")


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("bounces", [0, 1, 5])
@pytest.mark.parametrize("name", ["bunny", "mirror", "sphere_plane"])
def test_shade_ref_reproduces_the_oracle(ca, name, bounces):
    """shade_ref fed the camera's rays against the oracle's frame: every ray, colour within TOL, the first hit bitwise"""
    w, h = 48, 27
    s = load_scene(ca, name, w, h)
    sc = shade_ref.ShadeScene(s)
    o, d = ray_ref.camera_rays(sc.cam)
    r = shade_ref.ray_color(sc, o, d, min_t=1e-3, bounces=bounces)
    g = oracle.oracle_render(s, fudge=1e-3, bounces=bounces, threads=os.cpu_count() or 4, hit_ids=True)
    assert r["color"].shape == (w * h, 3)
    want = g["color"].reshape(-1, 3)
    assert np.array_equal(np.isnan(r["color"]), np.isnan(want))
    diff = np.abs(np.nan_to_num(r["color"]).astype(np.float64) - np.nan_to_num(want))
    print(f"{name} bounces {bounces}: colour max|diff| {diff.max():.3e}, {int((r['object'] >= 0).sum())} hits")
    assert diff.max() <= TOL, f"{name} bounces {bounces}: {diff.max()}"
    assert _same(r["t"], g["depth"].reshape(-1))
    assert np.array_equal(r["object"], g["hit_id"].reshape(-1))
    assert _same(r["normal"], g["normal"].reshape(-1, 3))
    assert (r["object"] >= 0).any() and (r["color"][r["object"] < 0] == 0).all()
