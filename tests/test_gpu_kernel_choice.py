"""The wiring of the kernel choice on the GPU (-m gpu): ctr_render.cpp must hand choose_kernel (csrc/kernel_choice.h) the right
facts.  16x16 frames through every entry point under the variant masks that steer the choice; the build each launch ran
(ctr_debug_last_kernel) against the row of tests/golden/kernel_choice.npz that the test works out itself from the scene's
materials and triangle count, the entry and `bounces`; where the row says "rejected", the call fails with the message it
always failed with.  Every rendered frame is also compared bit for bit with the same call under VAR_NO_REORDER (a scene
head or top-level root left stale by the launch set-up would show there)."""
import os

import numpy as np
import pytest

from tests.conftest import load_scene
from tests.gpu_support import expected_kernel
from tests.util import _multi_mesh_scene, corner_meshes, mesh_scene, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
REJECTIONS = {0xF001: "supersampling: no build for", 0xF002: "not with the counting / statistics variants",
              0xF003: "CTR_VAR_IGNORE_TRANSPARENT: host-buffer calls only"}
ENTRIES = ("render", "render_pinned", "render_uv", "render_ss", "device", "device_ss", "algorithmic_bytes")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kernel_choice.npz"))["choice"].reshape(6, 512, 8, 2, 4)


def _masks(ca):
    return (0, ca.VAR_NO_OCC6, ca.VAR_EXACT_POW, ca.VAR_NO_PREFILTER | ca.VAR_NO_CLUSTER, ca.VAR_NO_ANYHIT, ca.VAR_STATS, ca.VAR_MERGE,
            ca.VAR_IGNORE_TRANSPARENT, ca.VAR_NO_DIRECT)


def _call(ds, entry, bounces, dev):
    """One call through `entry`; what it produced, as a dict of numpy arrays"""
    import torch
    if entry == "algorithmic_bytes":
        return {"bytes_rays": np.array(ds.algorithmic_bytes(bounces=bounces), np.uint64)}
    if entry in ("device", "device_ss"):
        for t in dev:
            t.fill_(-1.0)
        ds.render_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), bounces=bounces, samples=2 if entry == "device_ss" else 1)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(("depth", "color", "normal"), dev)}
    if entry == "render_uv":
        r = ds.render_uv(bounces=bounces)
    else:
        r = ds.render(bounces=bounces, pinned=entry == "render_pinned", samples=2 if entry == "render_ss" else 1)
    return {k: np.array(r[k]) for k in ("depth", "color", "normal", "uv") if k in r}


def _scene(ca, tmp_path, name):
    if name == "small_opaque_mesh":  # 9 triangles, no transparency, a reflecting material
        return ca.HostScene.parse(mesh_scene(str(tmp_path / "fan.stl"), W, H, corner_meshes()[3]))
    if name == "two_meshes":
        return ca.HostScene.parse(_multi_mesh_scene(tmp_path, 0, w=W, h=H, opaque=True, n_mesh=2))
    return load_scene(ca, name, W, H)  # bunny: 1000 triangles, the 6-wave threshold exactly; sphere_plane: a transparent material


@pytest.mark.parametrize("name", ["small_opaque_mesh", "bunny", "sphere_plane", "two_meshes"])
def test_every_entry_launches_the_build_the_fixture_names(ca, golden, tmp_path, name):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    s = _scene(ca, tmp_path, name)
    assert s.ok
    ds = ca.DeviceScene(s)
    dev = [torch.empty(shape, device="cuda:0") for shape in ((H, W), (H, W, 3), (H, W, 3))]
    builds = set()
    for mask in _masks(ca):
        for bounces in (5, 6):  # the 6-wave build's stacks fit up to 5 frames of a bouncing scene
            for entry in ENTRIES:
                what = (name, hex(mask), bounces, entry)
                want = expected_kernel(ca, golden, s, mask, entry, bounces)
                ds.set_variant(mask)
                if want in REJECTIONS:
                    with pytest.raises(RuntimeError, match=REJECTIONS[want]):
                        _call(ds, entry, bounces, dev)
                    continue
                got = _call(ds, entry, bounces, dev)
                assert ds.last_kernel() == want, (what, hex(ds.last_kernel()), hex(want))
                builds.add(want)
                ds.set_variant(mask | ca.VAR_NO_REORDER)
                again = _call(ds, entry, bounces, dev)
                assert ds.last_kernel() == want, what
                for k in got:
                    assert same_bits(got[k], again[k]), (what, k)
    ds.close()
    # the scenes are chosen to reach the 6-wave, delivering and merged builds
    if name == "bunny":
        assert {0x06B, 0x02B, 0x0EB, 0x86B, 0x82B} <= builds, sorted(hex(b) for b in builds)
    if name == "two_meshes":
        assert any(b & 0x200 for b in builds), sorted(hex(b) for b in builds)
