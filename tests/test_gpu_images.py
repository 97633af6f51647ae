"""Display frames on the GPU (-m gpu): ctr_quantise_device / DeviceScene.quantise and ctr_render_images / DeviceScene.render_images
against the definition of include/cutrace_images.h.

Bar: every byte equal.  References: the host quantisers ctr_quantise_* and the oracle's orc_quantise_* on the same inputs, and
tests/images_ref.py — which tests/test_images_cpu.py pins to both — where the host's C++ has no defined answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cutrace_amd
import oracle
from cutrace_amd import _lib, lenses
from tests import images_ref as ir
from tests.conftest import load_scene

pytestmark = pytest.mark.gpu

ROOT = _lib.ROOT
f32 = np.float32
GUARD = 0xA5
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)
PLANE_SETS = (("depth",), ("color",), ("normal",), ("depth", "color"), ("depth", "normal"), ("color", "normal"),
              ("depth", "color", "normal"))


@pytest.fixture(scope="module")
def ds(ca):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d = ca.DeviceScene(load_scene(ca, "sphere_plane", 160, 90))
    yield d
    d.close()


def dev_of(ds):
    import torch
    return torch.device("cuda", ds.device)


def gq(ds, depth=None, color=None, normal=None, max_depth=None):
    """DeviceScene.quantise of numpy planes, as numpy (n, 3) byte planes"""
    import torch
    dev = dev_of(ds)
    t = {k: torch.from_numpy(np.ascontiguousarray(v, f32)).to(dev) for k, v in (("depth", depth), ("color", color), ("normal", normal))
         if v is not None}
    r = ds.quantise(max_depth=max_depth, **t)
    return {k: v.cpu().numpy().reshape(-1, 3) for k, v in r.items()}


def host_bytes(kind, data, *extra):
    """(ctr_quantise_<kind>, orc_quantise_<kind>) of the same floats"""
    data = np.ascontiguousarray(data, f32)
    n = data.size // (1 if kind == "depth" else 3)
    outs = []
    for lib, pre in ((_lib.host_lib(), "ctr"), (oracle.oracle_lib(), "orc")):
        out = np.zeros((n, 3), np.uint8)
        getattr(lib, f"{pre}_quantise_{kind}")(data.ctypes.data, n, *extra, out.ctypes.data)
        outs.append(out)
    return outs


def assert_bytes(got, want, what):
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def frame_bytes(r):
    """the host quantisers on what DeviceScene.render returned, with the call's own max depth: {plane: (rows, w, 3)}"""
    shape = r["color"].shape
    return {"depth": host_bytes("depth", r["depth"], C.c_float(r["max_depth"]))[0].reshape(shape),
            "color": host_bytes("color", r["color"])[0].reshape(shape),
            "normal": host_bytes("normal", r["normal"])[0].reshape(shape)}


# ---- ctr_quantise_device against the host quantisers ----
def test_colour_cases(ds):
    c = ir.color_cases()
    got = gq(ds, color=c)["color"]
    for want in host_bytes("color", c) + [ir.quantise_color(c)]:
        assert_bytes(got, want, "colour cases")
    one = gq(ds, color=np.array([[np.nan, np.inf, -np.inf], [0.0, 1.0, -0.0]], f32))["color"]
    assert one.tolist() == [[0, 255, 0], [0, 255, 0]]


@pytest.mark.parametrize("case", range(len(ir.depth_cases())))
def test_depth_cases(ds, case):
    m, d = ir.depth_cases()[case]
    got = gq(ds, depth=d, max_depth=m)["depth"]
    for want in host_bytes("depth", d, C.c_float(m)) + [ir.quantise_depth(d, m)]:
        assert_bytes(got, want, f"depth cases, max {m}")
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    reached = set(np.unique(got[:, 0]).tolist())
    assert len(reached) >= 250 and {0, 255} <= reached   # (the cases do walk the whole byte range)


def test_normal_cases_and_the_contraction_fixture(ds):
    for what, n in (("normal cases", ir.normal_cases()), ("contraction fixture", ir.contraction_fixture())):
        got = gq(ds, normal=n)["normal"]
        for want in host_bytes("normal", n) + [ir.quantise_normal(n)]:
            assert_bytes(got, want, what)
    # a kernel that fused a product into the sum of len^2 would differ on every pixel of the fixture
    n = ir.contraction_fixture()
    assert (gq(ds, normal=n)["normal"] != ir.quantise_normal(n, fused=True)).any(1).all()


def test_random_pixels(ds):
    depth, color, normal, m = ir.random_pixels(1 << 20)
    got = gq(ds, depth=depth, color=color, normal=normal, max_depth=float(m))
    for kind, data, extra in (("depth", depth, (C.c_float(m),)), ("color", color, ()), ("normal", normal, ())):
        for want in host_bytes(kind, data, *extra):
            assert_bytes(got[kind], want, f"2^20 random pixels, {kind}")


def test_inputs_the_host_leaves_undefined(ds):
    """NaN and infinite normals, negative depth, depth above max, max = 0 with a finite depth: the saturated bytes of the
    header (tests/test_images_cpu.py spells them out for images_ref); the pixels around them stay correct"""
    depth, color, normal, m = ir.random_pixels(4099, seed=9)
    bad_n = np.array([[np.nan, 0, 1], [np.inf, 1, 0], [-np.inf, 0, 0], [3e38, 3e38, 0], [1, 0, np.nan], [np.inf, np.inf, np.inf]], f32)
    bad_d = np.array([-1.0, -1e-30, -3e38, 2 * m, 3e38, np.nextafter(m, f32(np.inf)), -np.inf, np.nan], f32)
    at_n = np.array([0, 3, 64, 257, 4095, 4098])
    at_d = np.array([1, 2, 63, 65, 255, 256, 4097, 4098])
    clean_n, clean_d = ir.quantise_normal(normal), ir.quantise_depth(depth, m)
    normal[at_n], depth[at_d] = bad_n, bad_d
    got = gq(ds, depth=depth, color=color, normal=normal, max_depth=float(m))
    assert_bytes(got["normal"], ir.quantise_normal(normal), "undefined normals")
    assert_bytes(got["depth"], ir.quantise_depth(depth, m), "undefined depths")
    assert got["normal"][at_n].tolist() == [[0, 0, 0], [0, 127, 127], [0, 127, 127], [127, 127, 127], [0, 0, 0], [0, 0, 0]]
    assert got["depth"][at_d, 0].tolist() == [255, 255, 255, 0, 0, 0, 0, 0]
    keep_n, keep_d = np.setdiff1d(np.arange(4099), at_n), np.setdiff1d(np.arange(4099), at_d)
    assert_bytes(got["normal"][keep_n], clean_n[keep_n], "neighbours of undefined normals")
    assert_bytes(got["depth"][keep_d], clean_d[keep_d], "neighbours of undefined depths")
    assert_bytes(got["color"], host_bytes("color", color)[0], "colour beside them")
    zero = gq(ds, depth=np.array([0.0, -1.0, 1.0, np.inf, 0.0], f32), max_depth=0.0)["depth"]
    assert zero[:, 0].tolist() == [0, 255, 0, 0, 0]


@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_alignment(ds, n):
    """inputs 0..3 floats and outputs 0..3 bytes off an aligned allocation, every plane singly and in pairs: the bytes are
    right and the bytes before and after each output plane are untouched"""
    import torch
    dev = dev_of(ds)
    depth, color, normal, m = ir.random_pixels(n, seed=n)
    want = {"depth": ir.quantise_depth(depth, m), "color": ir.quantise_color(color), "normal": ir.quantise_normal(normal)}
    src = {"depth": depth.reshape(-1), "color": color.reshape(-1), "normal": normal.reshape(-1)}
    pad = 16
    for in_off in range(4):
        fin = {}
        for k, v in src.items():
            buf = torch.zeros(v.size + 8, dtype=torch.float32, device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[in_off:in_off + v.size] = torch.from_numpy(v).to(dev)
            fin[k] = buf[in_off:in_off + v.size] if k == "depth" else buf[in_off:in_off + v.size].view(n, 3)
        for out_off in range(4):
            for planes in PLANE_SETS:
                outs, expect = {}, {}
                for j, k in enumerate(planes):
                    off = pad + (out_off + j) % 4   # (the planes of one call differ in alignment)
                    buf = torch.full((2 * pad + 3 * n + 4,), GUARD, dtype=torch.uint8, device=dev)
                    assert buf.data_ptr() % 16 == 0
                    outs[k] = buf
                    e = np.full(buf.numel(), GUARD, np.uint8)
                    e[off:off + 3 * n] = want[k].reshape(-1)
                    expect[k] = (off, torch.from_numpy(e).to(dev))
                r = ds.quantise(max_depth=float(m) if "depth" in planes else None, **{k: fin[k] for k in planes},
                                out={k: outs[k][expect[k][0]:expect[k][0] + 3 * n] for k in planes})
                assert set(r) == set(planes)
                for k in planes:
                    assert torch.equal(outs[k], expect[k][1]), f"n {n}, input +{in_off} floats, {k} at +{expect[k][0] - pad} bytes, planes {planes}"


# ---- the d_counters path ----
def device_frame(ds, rows=None, bounces=5, stream=None, counters=None):
    """render_device into fresh tensors on `stream`, no synchronisation: (depth, color, normal, counters)"""
    import torch
    dev = dev_of(ds)
    n = cutrace_amd.rows_count(ds.h, rows)
    depth = torch.full((n, ds.w), -1.0, device=dev)
    color = torch.full((n, ds.w, 3), -1.0, device=dev)
    normal = torch.full((n, ds.w, 3), -1.0, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev) if counters is None else counters
    ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), d_counters=counters.data_ptr(),
                     stream=(stream or torch.cuda.current_stream(dev)).cuda_stream, bounces=bounces, rows=rows)
    return depth, color, normal, counters


def test_counters_path_and_rows(ds):
    import torch
    dev = dev_of(ds)
    host = ds.render()
    want = frame_bytes(host)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        depth, color, normal, counters = device_frame(ds, stream=st)
        chained = ds.quantise(depth=depth, color=color, normal=normal, counters=counters, stream=st)   # no synchronisation in between
    st.synchronize()
    explicit = ds.quantise(depth=depth, color=color, normal=normal, max_depth=host["max_depth"])
    for k in ("depth", "color", "normal"):
        assert chained[k].shape == (ds.h, ds.w, 3) and chained[k].dtype == torch.uint8
        assert torch.equal(chained[k], explicit[k]), k
        assert np.array_equal(chained[k].cpu().numpy(), want[k]), k
    # a rows part, quantised with the WHOLE frame's max passed explicitly, is those rows of the whole frame's images
    rows = (0, ds.h, 8, 1, 3)
    sel = np.array([y for y in range(ds.h) if (y // 8) % 3 == 1])
    pd, pc, pn, _ = device_frame(ds, rows=rows)
    part = ds.quantise(depth=pd, color=pc, normal=pn, max_depth=host["max_depth"])
    for k in ("depth", "color", "normal"):
        assert np.array_equal(part[k].cpu().numpy(), want[k][sel]), k
    with pytest.raises(ValueError):
        ds.quantise(depth=depth)
    with pytest.raises(ValueError):
        ds.quantise(depth=depth, counters=counters, max_depth=1.0)
    with pytest.raises(ValueError):
        ds.quantise()
    with pytest.raises(ValueError):
        ds.quantise(color=color, normal=normal[:4])


def test_graph_capture(ds):
    """render_device -> quantise(counters) as one linear chain on one stream, captured after a warm-up launch under
    VAR_NO_REORDER (no tile-order buffers, nothing allocated), replayed twice"""
    import torch
    dev = dev_of(ds)
    want = frame_bytes(ds.render())
    ds.set_variant(cutrace_amd.VAR_NO_REORDER)
    try:
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        out = {k: torch.zeros(ds.h, ds.w, 3, dtype=torch.uint8, device=dev) for k in ("depth", "color", "normal")}
        with torch.cuda.stream(st):
            depth, color, normal, counters = device_frame(ds, stream=st)
            ds.quantise(depth=depth, color=color, normal=normal, counters=counters, out=out, stream=st)
        st.synchronize()
        for k in out:
            assert np.array_equal(out[k].cpu().numpy(), want[k]), ("eager", k)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            cur = torch.cuda.current_stream(dev)
            counters.zero_()
            ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), d_counters=counters.data_ptr(), stream=cur.cuda_stream)
            ds.quantise(depth=depth, color=color, normal=normal, counters=counters, out=out, stream=cur)
        for _ in range(2):
            for t in out.values():
                t.zero_()
            depth.fill_(-1.0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for k in out:
                assert np.array_equal(out[k].cpu().numpy(), want[k]), ("replay", k)
        del g
    finally:
        ds.set_variant(0)


# ---- ctr_render_images ----
STAT_KEYS = ("ray_count", "max_depth", "rows")


@pytest.mark.parametrize("name", ["sphere_plane", "bunny", "mirror"])
def test_render_images(ca, name):
    d = ca.DeviceScene(load_scene(ca, name, 160, 90))
    rows = (0, 90, 8, 1, 3)
    for what, kw, planes, pinned in (("plain", {}, cutrace_amd.IMAGE_PLANES, False),
                                     ("samples 2", {"samples": 2}, cutrace_amd.IMAGE_PLANES, False),
                                     ("rows part 1 of 3", {"rows": rows}, cutrace_amd.IMAGE_PLANES, False),
                                     ("rows, samples 2, page-locked", {"rows": rows, "samples": 2}, cutrace_amd.IMAGE_PLANES, True),
                                     ("depth only", {}, ("depth",), False),
                                     ("normal only, page-locked", {}, ("normal",), True),
                                     ("colour only", {"samples": 2}, ("color",), False),
                                     ("page-locked", {}, cutrace_amd.IMAGE_PLANES, True)):
        ref = d.render(**kw)
        want = frame_bytes(ref)
        got = d.render_images(planes=planes, pinned=pinned, **kw)
        assert set(got) == set(planes) | {"ray_count", "kernel_ms", "total_ms", "max_depth", "rows"}, what
        for k in planes:
            assert got[k].dtype == np.uint8 and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(got[k], want[k]), f"{name}, {what}: {k} differs in {int((got[k] != want[k]).sum())} bytes"
        for k in STAT_KEYS:
            assert got[k] == ref[k], (what, k)
    d.close()


def test_render_images_rejections_and_variants(ca):
    d = ca.DeviceScene(load_scene(ca, "sphere_plane", 96, 54))
    L = _lib.hip_lib()
    out = np.zeros((54, 96, 3), np.uint8)
    flt = [np.empty((54, 96), f32), np.empty((54, 96, 3), f32), np.empty((54, 96, 3), f32)]

    def images(samples):
        st = L.ctr_render_images(d._h, C.c_float(1e-3), 5, samples, None, None, out.ctypes.data, None, None)
        return st, L.ctr_last_error()

    def aa(samples):
        st = L.ctr_render_aa(d._h, C.c_float(1e-3), 5, samples, None, flt[0].ctypes.data, flt[1].ctypes.data, flt[2].ctypes.data, None)
        return st, L.ctr_last_error()

    assert images(3) == aa(3) and images(3)[0] == 1 and b"samples" in images(3)[1]
    assert L.ctr_render_images(d._h, C.c_float(1e-3), 5, 1, None, None, None, None, None) == 1
    for bad in (3, 0, True):
        with pytest.raises(ValueError):
            d.render_images(samples=bad)
    for bad in ((), ("color", "color"), ("uv",)):
        with pytest.raises(ValueError):
            d.render_images(planes=bad)
    for var in (ca.VAR_STATS, ca.VAR_IGNORE_TRANSPARENT, ca.VAR_NO_PREFILTER, ca.VAR_NO_CLUSTER):
        d.set_variant(var)
        assert images(2) == aa(2) and images(2)[0] == 1 and images(2)[1], var   # the same message as ctr_render_aa
    # CTR_VAR_IGNORE_TRANSPARENT with samples == 1 is honoured as in ctr_render
    d.set_variant(ca.VAR_IGNORE_TRANSPARENT)
    ref = d.render()
    got = d.render_images()
    d.set_variant(0)
    plain = d.render()
    want = frame_bytes(ref)
    for k in cutrace_amd.IMAGE_PLANES:
        assert np.array_equal(got[k], want[k]), k
    assert any(not np.array_equal(ref[k], plain[k]) for k in cutrace_amd.IMAGE_PLANES)   # (the variant does change this scene's frame)
    again = d.render_images()
    for k in cutrace_amd.IMAGE_PLANES:
        assert np.array_equal(again[k], frame_bytes(plain)[k]), k
    d.close()


def test_lens_then_quantise(ca):
    s = load_scene(ca, "bunny", 96, 54)
    d = ca.DeviceScene(s)
    o, dr = lenses.pinhole(s.desc.contents.cam, 96, 54)
    r = d.render_lens(o, dr)
    q = d.quantise(depth=r["depth"], color=r["color"], normal=r["normal"], max_depth=r["max_depth"])
    want = d.render_images()
    assert r["max_depth"] == want["max_depth"]
    for k in cutrace_amd.IMAGE_PLANES:
        assert np.array_equal(q[k].cpu().numpy(), want[k]), k
    d.close()


def test_cli_gpu_images(ca, tmp_path):
    """cutrace with and without CUTRACE_GPU_IMAGES=1, in two working directories: the three files byte for byte"""
    from cutrace_amd import build
    exe = build.build_cli()
    env = dict(os.environ, CUTRACE_WIDTH="160", CUTRACE_HEIGHT="90")
    for k in ("CUTRACE_SAMPLES", "CUTRACE_DEVICES", "CUTRACE_DEVICE_LIST", "CUTRACE_GPU_IMAGES"):
        env.pop(k, None)
    files = {}
    for tag, extra in (("host", {}), ("gpu", {"CUTRACE_GPU_IMAGES": "1"})):
        cwd = tmp_path / tag
        cwd.mkdir()
        os.symlink(os.path.join(ROOT, "scene"), cwd / "scene")
        p = subprocess.run([exe, "scene/sphere_plane.json"], cwd=cwd, env=dict(env, **extra), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert "Render time was " in p.stdout and " ms; kernel time with setup/teardown was " in p.stdout
        files[tag] = {n: (cwd / n).read_bytes() for n in ("frame.jpg", "depth_map.jpg", "normal_map.jpg")}
    for n in files["host"]:
        assert len(files["host"][n]) > 1000 and files["host"][n] == files["gpu"][n], n
    p = subprocess.run([exe, "scene/sphere_plane.json"], cwd=tmp_path / "gpu", env=dict(env, CUTRACE_GPU_IMAGES="1", CUTRACE_DEVICES="2"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "CUTRACE_GPU_IMAGES" in p.stderr
