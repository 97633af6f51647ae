"""What ctr_cast_rays, ctr_shade_rays and ctr_shade_points check once they have a scene (csrc/ctr_rays.cpp): the count, the
input arrays, where every pointer lives and, for ctr_shade_points, the material.  The checks before the scene need no GPU:
tests/test_query_checks_cpu.py.  Every case: status CTR_E_INVALID and the whole text of ctr_last_error()."""
import numpy as np
import pytest

from tests.conftest import load_scene
from tests.util import refusal

pytestmark = pytest.mark.gpu
N = 2
NOT_DEVICE = " is not device memory of the scene's device"


@pytest.fixture(scope="module")
def live(ca):
    """(library, DeviceScene of scene/triangle.json at 16x16, the address of an (N, 3) float tensor on the device, that of a host array)"""
    import torch
    from cutrace_amd import _lib
    ds = ca.DeviceScene(load_scene(ca, "triangle", 16, 16))
    f3 = torch.ones(N, 3, device="cuda")
    host = np.zeros((N, 3), np.float32)
    yield _lib.hip_lib(), ds, f3.data_ptr(), host.ctypes.data
    torch.cuda.synchronize()
    ds.close()


def refused(entry, ds, make, cases):
    for fields, text in cases:
        q = make()
        for k, v in fields.items():
            setattr(q, k, v)
        assert refusal(entry, ds._h, q, text) == text, fields


def test_cast_rays_checks_behind_the_scene(live):
    from cutrace_amd import _lib
    L, ds, f3, host = live
    who = "ctr_cast_rays: "
    refused(L.ctr_cast_rays, ds, lambda: _lib.RayQuery(n_rays=N, min_t=1e-3, d_origin=f3, d_dir=f3, d_t=f3), [
        (dict(n_rays=1 << 31), who + "n_rays must be below 2^31"),
        (dict(n_rays=1 << 31, d_origin=None, d_t=host), who + "n_rays must be below 2^31"),  # the count comes first
        (dict(d_origin=None), who + "null rays"),
        (dict(d_dir=None, d_t=host), who + "null rays"),
        (dict(d_t=host), who + "d_t" + NOT_DEVICE),
        (dict(d_uv=host), who + "d_uv" + NOT_DEVICE),
        (dict(d_dir=host, d_t=host), who + "d_dir" + NOT_DEVICE),                            # in the order of the header
        (dict(flags=4, d_t=None, d_shadow=host), who + "d_shadow" + NOT_DEVICE),
    ])


def test_shade_rays_checks_behind_the_scene(live):
    from cutrace_amd import _lib
    L, ds, f3, host = live
    who = "ctr_shade_rays: "
    refused(L.ctr_shade_rays, ds, lambda: _lib.ShadeQuery(n_rays=N, bounces=5, min_t=1e-3, d_origin=f3, d_dir=f3, d_color=f3), [
        (dict(n_rays=1 << 31), who + "n_rays must be below 2^31"),
        (dict(n_rays=1 << 31, d_dir=None), who + "n_rays must be below 2^31"),
        (dict(d_origin=None), who + "null rays"),
        (dict(d_dir=None, d_color=host), who + "null rays"),
        (dict(d_color=host), who + "d_color" + NOT_DEVICE),
        (dict(d_origin=host, d_color=host), who + "d_origin" + NOT_DEVICE),
        (dict(d_normal=host), who + "d_normal" + NOT_DEVICE),
    ])


def test_shade_points_checks_behind_the_scene(live):
    from cutrace_amd import _lib
    L, ds, f3, host = live
    who = "ctr_shade_points: "
    n_mat = 1  # scene/triangle.json has one material
    refused(L.ctr_shade_points, ds, lambda: _lib.PointQuery(n_points=N, d_point=f3, d_normal=f3, d_view=f3, d_color=f3), [
        (dict(n_points=1 << 31), who + "n_points must be below 2^31"),
        (dict(n_points=1 << 31, d_point=None, material=-1), who + "n_points must be below 2^31"),
        (dict(d_point=None), who + "null d_point"),
        (dict(d_point=None, material=-1), who + "null d_point"),                             # before the material
        (dict(material=-1), who + "material -1 outside [0, 1)"),
        (dict(material=n_mat), who + "material 1 outside [0, 1)"),
        (dict(material=n_mat, d_color=host), who + "material 1 outside [0, 1)"),             # before the pointers
        (dict(material=n_mat, n_points=0), who + "material 1 outside [0, 1)"),               # and before the empty query returns
        (dict(d_color=host), who + "d_color" + NOT_DEVICE),
        (dict(d_point=host, d_color=host), who + "d_point" + NOT_DEVICE),
        (dict(d_object=host), who + "d_object" + NOT_DEVICE),
        (dict(d_color=None, d_normal=None, d_view=None, d_light_shadow=host), who + "d_light_shadow" + NOT_DEVICE),
        (dict(d_material=host), who + "d_material" + NOT_DEVICE),                            # (the scalar is not in use then)
    ])
