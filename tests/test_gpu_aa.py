"""Supersampled render on the GPU (-m gpu): DeviceScene.render(samples=s) / render_device(samples=s), ctr_render_aa and the
CLI's CUTRACE_SAMPLES against the definition of include/cutrace_aa.h — the oracle's render of the same scene at
s*w x s*h, reduced by tests/aa_ref.py.  Every pixel is compared.

Bar: depth and normal bit-exact; colour within util.TOL by default, bit-exact under VAR_EXACT_POW (which also pins the
order of the sum: tests/test_aa_cpu.py shows that another order changes bits)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

from tests import aa_ref
from tests.conftest import load_scene
from tests.gpu_support import gpu  # noqa: F401  (the fixture)
from tests.util import _random_scene, assert_parity, hall_of_mirrors_json, same_bits

pytestmark = pytest.mark.gpu

NT = min(os.cpu_count() or 4, 16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (w, h, bounces)
SCENES = {"random3": (21, 13, 5), "random5": (21, 13, 5), "random11_b0": (21, 13, 0), "hall": (24, 16, 15), "bunny": (40, 24, 5)}


def host_scene(ca, name):
    w, h, _ = SCENES[name]
    if name.startswith("random"):
        s = ca.HostScene.parse(_random_scene(int(name[6:].split("_")[0]), w, h))
    elif name == "hall":
        s = ca.HostScene.parse(hall_of_mirrors_json(w, h))
    else:
        s = load_scene(ca, "bunny", w, h)
    assert s.ok
    return s


_want = {}


def wanted(ca, name, ss, rows=None):
    """the definition: the oracle at s*w x s*h (rows scaled likewise), reduced; computed once per (scene, s, rows)"""
    key = (name, ss, rows)
    if key not in _want:
        w, h, b = SCENES[name]
        s = host_scene(ca, name)
        s.set_size(ss * w, ss * h)
        big_rows = None if rows is None else (rows[0] * ss, rows[1] * ss, rows[2] * ss, rows[3], rows[4])
        big = oracle.oracle_render(s, bounces=b, rows=big_rows, threads=NT)
        for k in ("depth", "normal", "color"):
            assert not np.isnan(big[k]).any(), (name, ss, k)
        r = aa_ref.reduce_frame(big, ss)
        r["ray_count"] = big["ray_count"]
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = r
    return _want[key]


@pytest.mark.parametrize("ss", [2, 4, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_parity(gpu, name, ss):
    w, h, b = SCENES[name]
    want = wanted(gpu, name, ss)
    ds = gpu.DeviceScene(host_scene(gpu, name))
    r = ds.render(bounces=b, samples=ss)
    assert r["depth"].shape == (h, w) and r["color"].shape == (h, w, 3) and r["rows"] == h
    assert_parity(r, want, what=f"{name} s={ss}")
    assert r["ray_count"] == want["ray_count"]
    ds.set_variant(gpu.VAR_EXACT_POW)
    e = ds.render(bounces=b, samples=ss)
    for k in ("depth", "normal", "color"):
        assert same_bits(e[k], want[k]), f"{name} s={ss} EXACT_POW: {k} differs in {int((e[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words"
    ds.close()


@pytest.mark.parametrize("name", ["random3", "bunny"])
def test_depth_and_normal_are_the_plain_render(gpu, name):
    w, h, b = SCENES[name]
    ds = gpu.DeviceScene(host_scene(gpu, name))
    plain = ds.render(bounces=b)
    for ss in (2, 4, 8):
        r = ds.render(bounces=b, samples=ss)
        assert same_bits(r["depth"], plain["depth"]) and same_bits(r["normal"], plain["normal"]), ss
        assert r["max_depth"] == plain["max_depth"], ss
    one = ds.render(bounces=b, samples=1)
    for k in ("depth", "normal", "color"):
        assert same_bits(one[k], plain[k]), k
    assert one["ray_count"] == plain["ray_count"]
    ds.close()


@pytest.mark.parametrize("ss", [2, 4])
def test_rows(gpu, ss):
    w, h, b = SCENES["random3"]
    rows = (0, h, 2, 1, 3)
    want = wanted(gpu, "random3", ss, rows)
    ds = gpu.DeviceScene(host_scene(gpu, "random3"))
    n = gpu.rows_count(h, rows)
    r = ds.render(bounces=b, rows=rows, samples=ss)
    assert r["depth"].shape == (n, w) and want["depth"].shape == (n, w)
    assert r["rows"] == n
    assert_parity(r, want, what=f"rows s={ss}")
    ds.set_variant(gpu.VAR_EXACT_POW)
    e = ds.render(bounces=b, rows=rows, samples=ss)
    for k in ("depth", "normal", "color"):
        assert same_bits(e[k], want[k]), k
    ds.close()


def test_device_form(gpu):
    import torch
    w, h, b = SCENES["random3"]
    ds = gpu.DeviceScene(host_scene(gpu, "random3"))
    host = ds.render(bounces=b, samples=2)
    dev = torch.device("cuda", 0)
    depth = torch.full((h, w), -1.0, device=dev)
    color = torch.full((h, w, 3), -1.0, device=dev)
    normal = torch.full((h, w, 3), -1.0, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), d_counters=counters.data_ptr(), stream=st.cuda_stream,
                         bounces=b, samples=2)
    st.synchronize()
    for k, t in (("depth", depth), ("color", color), ("normal", normal)):
        assert same_bits(t.cpu().numpy(), host[k]), k
    assert int(counters[0]) == host["ray_count"]
    # captured under VAR_NO_REORDER (no tile-order buffers, nothing allocated) and replayed twice
    ds.set_variant(gpu.VAR_NO_REORDER)
    with torch.cuda.stream(st):
        ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=st.cuda_stream, bounces=b, samples=2)
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream,
                         bounces=b, samples=2)
    for _ in range(2):
        for t in (depth, color, normal):
            t.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k, t in (("depth", depth), ("color", color), ("normal", normal)):
            assert same_bits(t.cpu().numpy(), host[k]), k
    del g
    ds.close()


def test_plain_aa_plain_on_one_handle(gpu):
    w, h, b = SCENES["bunny"]
    ds = gpu.DeviceScene(host_scene(gpu, "bunny"))

    def tiles(ww, hh):
        return ((ww + 7) // 8) * ((hh + 7) // 8)

    a = ds.render(bounces=b)
    assert len(ds.tile_costs()) == tiles(w, h)
    aa = ds.render(bounces=b, samples=4)
    assert len(ds.tile_costs()) == tiles(4 * w, 4 * h)
    assert_parity(aa, wanted(gpu, "bunny", 4), what="bunny s=4 between plain renders")
    c = ds.render(bounces=b)
    assert len(ds.tile_costs()) == tiles(w, h)
    for k in ("depth", "normal", "color"):
        assert same_bits(a[k], c[k]), k
    assert a["ray_count"] == c["ray_count"]
    ds.close()


def test_rejections(gpu):
    from cutrace_amd import _lib
    w, h, b = SCENES["random3"]
    ds = gpu.DeviceScene(host_scene(gpu, "random3"))
    for bad in (3, 16, 0, -2, 2.0, True):
        with pytest.raises(ValueError):
            ds.render(bounces=b, samples=bad)
        with pytest.raises(ValueError):
            ds.render_device(0, 0, 0, bounces=b, samples=bad)
    L = _lib.hip_lib()
    depth, color, normal = np.empty((h, w), np.float32), np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32)

    def call(samples):
        return L.ctr_render_aa(ds._h, C.c_float(1e-3), b, samples, None, depth.ctypes.data, color.ctypes.data, normal.ctypes.data, None)

    assert call(3) == 1 and b"samples" in L.ctr_last_error()  # CTR_E_INVALID
    good = ds.render(bounces=b, samples=2)
    plain = ds.render(bounces=b)
    for var in (gpu.VAR_STATS, gpu.VAR_IGNORE_TRANSPARENT, gpu.VAR_NO_PREFILTER, gpu.VAR_NO_CLUSTER):
        ds.set_variant(var)
        assert call(2) == 1 and L.ctr_last_error(), var
        with pytest.raises(RuntimeError):
            ds.render(bounces=b, samples=2)
    ds.set_variant(gpu.VAR_STATS)
    assert call(1) == 0  # samples = 1 is ctr_render, whatever the variant
    ds.set_variant(0)
    # the handle renders normally afterwards
    again, plain2 = ds.render(bounces=b, samples=2), ds.render(bounces=b)
    for k in ("depth", "normal", "color"):
        assert same_bits(again[k], good[k]) and same_bits(plain2[k], plain[k]), k
    # variant bits with nothing to act on are ignored, the ones that pick a build honoured: same bits as the default
    for var in (gpu.VAR_MERGE, gpu.VAR_NO_DIRECT, gpu.VAR_NO_ANYHIT, gpu.VAR_NO_REORDER, gpu.VAR_IMAGE_ORDER_FIRST, gpu.VAR_NO_OCC6):
        ds.set_variant(var)
        r = ds.render(bounces=b, samples=2)
        for k in ("depth", "normal", "color"):
            assert same_bits(r[k], good[k]), (var, k)
    ds.close()


def test_cli_samples(gpu, tmp_path):
    """cutrace with CUTRACE_SAMPLES=2: the same depth and normal maps, byte for byte, another frame.jpg — the oracle's"""
    from PIL import Image
    from cutrace_amd import build
    exe = build.build_cli()
    os.symlink(os.path.join(ROOT, "scene"), tmp_path / "scene")
    env = dict(os.environ, CUTRACE_WIDTH="160", CUTRACE_HEIGHT="90")
    env.pop("CUTRACE_SAMPLES", None)
    env.pop("CUTRACE_DEVICES", None)
    env.pop("CUTRACE_DEVICE_LIST", None)
    files = {}
    for tag, extra in (("plain", {}), ("aa", {"CUTRACE_SAMPLES": "2"})):
        p = subprocess.run([exe, "scene/bunny.json"], cwd=tmp_path, env=dict(env, **extra), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert "Render time was " in p.stdout
        files[tag] = {n: (tmp_path / n).read_bytes() for n in ("frame.jpg", "depth_map.jpg", "normal_map.jpg")}
        if tag == "aa":
            frame = np.asarray(Image.open(tmp_path / "frame.jpg").convert("RGB")).astype(np.int32)
    assert files["plain"]["depth_map.jpg"] == files["aa"]["depth_map.jpg"]
    assert files["plain"]["normal_map.jpg"] == files["aa"]["normal_map.jpg"]
    assert files["plain"]["frame.jpg"] != files["aa"]["frame.jpg"]
    s = gpu.HostScene.load("scene/bunny.json")
    s.set_size(320, 180)
    want = aa_ref.reduce_color(oracle.oracle_render(s, bounces=5, threads=NT)["color"], 2)
    q = np.zeros((90, 160, 3), np.uint8)
    oracle.oracle_lib().orc_quantise_color(want.ctypes.data, 160 * 90, q.ctypes.data)
    assert frame.shape == (90, 160, 3)
    assert np.abs(frame - q.astype(np.int32)).mean() < 4.0  # test_cli_drop_in's bound: JPEG q=90 loss only
    for extra in ({"CUTRACE_SAMPLES": "3"}, {"CUTRACE_SAMPLES": "2", "CUTRACE_DEVICES": "2"}):
        p = subprocess.run([exe, "scene/bunny.json"], cwd=tmp_path, env=dict(env, **extra), capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "CUTRACE_SAMPLES" in p.stderr, (extra, p.returncode, p.stderr)
