"""The lens render on the GPU (-m gpu): DeviceScene.render_lens / ctr_render_device_lens against the definition of
include/cutrace_lens.h.  Every pixel is compared.

Bar: depth, normal and the masked positions bit-exact; colour within util.TOL by default and bit-exact where both sides
compute the specular pow exactly.  References: the plain render of the same handle (pinhole rays), tests/shade_ref.py and
tests/ray_ref.py on the CPU (random scenes), ctr_shade_rays with the linear walk of the same build (bunny, hall of mirrors),
and tests/aa_ref.py's reduction of the samples=1 lens render (samples)."""
import ctypes as C

import numpy as np
import pytest

from cutrace_amd import _lib, lenses
from tests import aa_ref, ray_ref, shade_ref
from tests.gpu_support import gpu  # noqa: F401  (the fixture)
from tests.lens_rays import CastCounter, assert_frames, cam_of, frame_from_rays, host_scene, lens, normalised, plain_device
from tests.util import same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
KV_OCC6, KV_SS, KV_RAYS = 64, 2048, 4096
# name -> (w, h, bounces) of the pinhole test; the other tests say their own sizes
SCENES = {"random3": (21, 13, 5), "random5": (21, 13, 5), "bunny": (40, 24, 5), "mirror": (32, 24, 8)}


# ---- 1. the camera through the lens is the render ----
@pytest.mark.parametrize("name", list(SCENES))
def test_pinhole_rays_give_the_plain_render(gpu, name):
    w, h, b = SCENES[name]
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.pinhole(cam_of(s), w, h)
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        want = plain_device(ds, b)
        kv_plain = ds.last_kernel()
        got = lens(ds, o, d, bounces=b)
        kv = ds.last_kernel()
        assert got["depth"].shape == (h, w) and got["color"].shape == (h, w, 3) and got["rows"] == h
        assert_frames(got, want, f"{name} var={var}")
        assert got["ray_count"] == want["ray_count"] and got["max_depth"] == want["max_depth"], (name, var)
        assert kv & KV_RAYS and not kv & KV_SS
        assert kv == kv_plain | KV_RAYS, (hex(kv), hex(kv_plain))  # the same walk, pow and occupancy as the plain launch
        if name == "bunny" and var == 0:
            assert kv & KV_OCC6  # the large mesh: the 6-wave build
        # (n, 3) rays are the same call
        flat = lens(ds, o.reshape(-1, 3), d.reshape(-1, 3), bounces=b)
        assert_frames(flat, want, f"{name} var={var} flat")
    ds.close()


# ---- 2. other lenses against the reference ----
def other_lenses(cam, w, h):
    """a fisheye with a masked rim, a stereo pair (two origins in one frame), a thin lens (an origin per pixel)"""
    return {"fisheye": lenses.fisheye(cam, w, h, 150.0), "stereo": lenses.stereo(cam, w, h, 0.4),
            "thin": lenses.thin_lens(cam, w, h, 1, 0.15, 4.0, seed=11)}


@pytest.mark.parametrize("name", ["random3", "random5"])
def test_other_lenses_against_shade_ref(gpu, name):
    w, h, b = 24, 16, 5
    s = host_scene(gpu, name, w, h)
    sc = shade_ref.ShadeScene(s)
    ds = gpu.DeviceScene(s)
    for lname, (o, d) in other_lenses(cam_of(s), w, h).items():
        keep = ~lenses.is_masked(o, d).reshape(-1)
        assert (lname == "fisheye") == (not keep.all()) and keep.sum() > h * w // 3
        of, df = o.reshape(-1, 3)[keep], normalised(d.reshape(-1, 3)[keep])
        ref = shade_ref.ray_color(sc, of, df, min_t=1e-3, bounces=b)
        cast = ray_ref.ray_cast(sc, of, df, f32(1e-3))
        assert same_bits(cast["t"], ref["t"]) and same_bits(cast["normal"], ref["normal"])
        assert not np.isnan(ref["color"]).any()
        want = frame_from_rays(h, w, keep, cast["t"], cast["normal"], ref["color"])
        # the reference side does not depend on the walk for these rays: the BVH walk of the radiance query gives the linear one's bits
        lin = ds.shade_rays(of, df, bounces=b, exact_pow=True, linear=True, outputs=("color", "t", "normal"))
        bvh = ds.shade_rays(of, df, bounces=b, exact_pow=True, linear=False, outputs=("color", "t", "normal"))
        for k in ("color", "t", "normal"):
            assert same_bits(lin[k].cpu().numpy(), bvh[k].cpu().numpy()), (lname, k)
        ds.set_variant(0)
        assert_frames(lens(ds, o, d, bounces=b), want, f"{name} {lname}", color="tol")
        ds.set_variant(gpu.VAR_EXACT_POW)
        got = lens(ds, o, d, bounces=b)
        assert_frames(got, want, f"{name} {lname} exact pow")
        assert (got["depth"].reshape(-1)[~keep] == np.inf).all() and (got["color"].reshape(-1, 3)[~keep] == 0).all()
        fin = got["depth"][np.isfinite(got["depth"]) & (got["depth"] > 0)]
        assert got["max_depth"] == (float(fin.max()) if fin.size else 0.0)
    ds.close()


@pytest.mark.parametrize("name,w,h,b", [("bunny", 40, 24, 5), ("hall", 24, 16, 15)])
def test_other_lenses_against_the_linear_radiance_query(gpu, name, w, h, b):
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    for lname, (o, d) in other_lenses(cam_of(s), w, h).items():
        keep = ~lenses.is_masked(o, d).reshape(-1)
        of, df = o.reshape(-1, 3)[keep], normalised(d.reshape(-1, 3)[keep])
        for exact in (False, True):
            ref = {k: v.cpu().numpy() for k, v in ds.shade_rays(of, df, bounces=b, exact_pow=exact, linear=True, outputs=("color", "t", "normal")).items()}
            bvh = {k: v.cpu().numpy() for k, v in ds.shade_rays(of, df, bounces=b, exact_pow=exact, linear=False, outputs=("color", "t", "normal")).items()}
            for k in ("t", "normal"):  # the chosen rays: the default walk is the linear walk on the reference side
                assert same_bits(ref[k], bvh[k]), (lname, k)
            want = frame_from_rays(h, w, keep, ref["t"], ref["normal"], ref["color"])
            ds.set_variant(gpu.VAR_EXACT_POW if exact else 0)
            got = lens(ds, o, d, bounces=b)
            assert_frames(got, want, f"{name} {lname} exact={exact}", color="bits" if exact else "tol")
            assert (ds.last_kernel() & KV_RAYS) != 0
    ds.close()


# ---- 3. masking ----
def test_masked_pixels(gpu, monkeypatch):
    """ray_count: the drop equals the cast count of tests/shade_ref.py's ray_color for the masked pixels' camera rays, plus the
    duplicated primary cast of each (the reference's count, not a plain render of those pixels alone: `rows` selects rows,
    and the masked pixels are columns)."""
    name = "random3"
    w, h, b = SCENES[name]
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    want = plain_device(ds, b)
    o, d = lenses.pinhole(cam_of(s), w, h)
    o, d = o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    idx = np.arange(0, h * w, 7)
    kinds = ["nan", "+inf", "-inf", "zero", "long", "nan origin"]
    for j, k in enumerate(idx):
        kind = kinds[j % len(kinds)]
        if kind == "nan":
            d[k, j % 3] = np.nan
        elif kind == "+inf":
            d[k, j % 3] = np.inf
        elif kind == "-inf":
            d[k] = -np.inf
        elif kind == "zero":
            d[k] = [0.0, -0.0, 0.0]
        elif kind == "long":
            d[k] = normalised(d[k:k + 1])[0] * f32(1e30)
        else:
            o[k, j % 3] = np.nan
    masked = np.zeros(h * w, bool)
    masked[idx] = True
    assert np.array_equal(lenses.is_masked(o, d), masked)
    got = lens(ds, o, d, bounces=b)
    dep, nrm, col = got["depth"].reshape(-1), got["normal"].reshape(-1, 3), got["color"].reshape(-1, 3)
    assert (dep[masked] == np.inf).all() and same_bits(nrm[masked], np.zeros((len(idx), 3), f32)) and same_bits(col[masked], np.zeros((len(idx), 3), f32))
    for k in ("depth", "normal", "color"):
        g, p = got[k].reshape(h * w, -1), want[k].reshape(h * w, -1)
        assert same_bits(g[~masked], p[~masked]), k
    fin = want["depth"].reshape(-1)[~masked]
    fin = fin[np.isfinite(fin) & (fin > 0)]
    assert got["max_depth"] == float(fin.max())
    # the casts the reference makes for the masked pixels' camera rays
    po, pd = ray_ref.camera_rays(ray_ref.RefScene(s).cam)
    counter = CastCounter(monkeypatch)
    shade_ref.ray_color(shade_ref.ShadeScene(s), po[masked], pd[masked], min_t=1e-3, bounces=b)
    print(f"plain {want['ray_count']} masked {got['ray_count']} reference casts of the masked pixels {counter.n} + {len(idx)}")
    assert want["ray_count"] - got["ray_count"] == counter.n + len(idx)
    ds.close()


# ---- 4. samples ----
def big_lens_reduced(ds, o, d, w, h, ss, b):
    """the definition: the samples=1 lens render of the s*w x s*h rays, reduced by tests/aa_ref.py"""
    ds.set_size(ss * w, ss * h)
    big = lens(ds, o, d, bounces=b)
    ds.set_size(w, h)
    r = aa_ref.reduce_frame(big, ss)
    fin = r["depth"][np.isfinite(r["depth"]) & (r["depth"] > 0)]
    r.update(ray_count=big["ray_count"], max_depth=float(fin.max()) if fin.size else 0.0)
    return r


@pytest.mark.parametrize("ss", [2, 4, 8])
@pytest.mark.parametrize("name,w,h,b", [("random5", 21, 13, 5), ("hall", 16, 12, 15)])
def test_samples(gpu, name, w, h, b, ss):
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.thin_lens(cam_of(s), w, h, ss, 0.15, 4.0, seed=5)
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        want = big_lens_reduced(ds, o, d, w, h, ss, b)
        got = lens(ds, o, d, bounces=b, samples=ss)
        kv = ds.last_kernel()
        assert kv & KV_RAYS and kv & KV_SS
        assert got["depth"].shape == (h, w)
        assert_frames(got, want, f"{name} s={ss} var={var}", color="bits" if var else "tol")
        assert got["ray_count"] == want["ray_count"] and got["max_depth"] == want["max_depth"]
    ds.close()


def test_samples_with_a_masked_rim_through_blocks(gpu):
    name, w, h, b, ss = "random5", 21, 13, 5, 2
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.fisheye(cam_of(s), ss * w, ss * h, 150.0)
    m = lenses.is_masked(o, d).reshape(h, ss, w, ss)
    per_block = m.sum((1, 3))
    assert ((per_block > 0) & (per_block < ss * ss)).any() and (per_block == ss * ss).any() and (per_block == 0).any()
    assert (m[:, 0, :, 0] & (per_block < ss * ss)).any()  # a block whose sample (0, 0) is masked and another is not
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        want = big_lens_reduced(ds, o, d, w, h, ss, b)
        got = lens(ds, o, d, bounces=b, samples=ss)
        assert_frames(got, want, f"fisheye s=2 var={var}", color="bits" if var else "tol")
        assert got["ray_count"] == want["ray_count"] and got["max_depth"] == want["max_depth"]
        assert (got["depth"][m[:, 0, :, 0]] == np.inf).all() and (got["color"][per_block == ss * ss] == 0).all()
    ds.close()


# ---- 5. plumbing ----
def test_rows_parts_reassemble(gpu):
    name = "random3"
    w, h, b = SCENES[name]
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    cam = cam_of(s)
    for ss, (o, d) in ((1, lenses.fisheye(cam, w, h, 150.0)), (2, lenses.thin_lens(cam, w, h, 2, 0.15, 4.0, seed=3))):
        whole = lens(ds, o, d, bounces=b, samples=ss)
        out = {k: np.full_like(whole[k], -1.0) for k in ("depth", "normal", "color")}
        total = 0
        for part in range(3):
            rows = (0, h, 2, part, 3)
            r = lens(ds, o, d, bounces=b, samples=ss, rows=rows)
            ys = [y for y in range(h) if (y // 2) % 3 == part]
            assert r["depth"].shape == (len(ys), w) and r["rows"] == len(ys)
            for k in out:
                out[k][ys] = r[k]
            total += r["ray_count"]
        for k in out:
            assert same_bits(out[k], whole[k]), (ss, k)
        assert total == whole["ray_count"]
        r = lens(ds, o, d, bounces=b, samples=ss, rows=(3, 8))
        for k in out:
            assert same_bits(r[k], whole[k][3:8]), (ss, k)
    ds.close()


def lens_abi(ds, o, d, depth, color, normal, stream, b, samples=1, counters=None, ambient=None):
    """ctr_render_device_lens itself, on torch tensors that live on"""
    q = _lib.Lens(o.shape[0], samples, float(ds._ambient if ambient is None else ambient), o.data_ptr(), d.data_ptr())
    st = _lib.hip_lib().ctr_render_device_lens(ds._h, C.c_float(1e-3), b, C.byref(q), None, depth.data_ptr(), color.data_ptr(),
                                               normal.data_ptr(), counters.data_ptr() if counters is not None else None, C.c_void_p(stream))
    assert st == 0, _lib.hip_lib().ctr_last_error()


def test_side_stream_and_graph_replay(gpu):
    import torch
    name = "random3"
    w, h, b = SCENES[name]
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.stereo(cam_of(s), w, h, 0.4)
    want = lens(ds, o, d, bounces=b)
    dev = torch.device("cuda", 0)
    ot, dt = torch.from_numpy(o.reshape(-1, 3)).to(dev), torch.from_numpy(d.reshape(-1, 3)).to(dev)
    depth, color, normal = torch.full((h, w), -1.0, device=dev), torch.full((h, w, 3), -1.0, device=dev), torch.full((h, w, 3), -1.0, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        lens_abi(ds, ot, dt, depth, color, normal, st.cuda_stream, b, counters=counters)
        lens_abi(ds, ot, dt, depth, color, normal, st.cuda_stream, b, counters=counters)
    st.synchronize()
    for k, t in (("depth", depth), ("color", color), ("normal", normal)):
        assert same_bits(t.cpu().numpy(), want[k]), k
    assert int(counters[0]) == 2 * want["ray_count"]  # counters accumulate
    # through render_lens on a side stream
    with torch.cuda.stream(st):
        r = ds.render_lens(ot, dt, bounces=b, stream=st)
    for k in ("depth", "color", "normal"):
        assert same_bits(r[k].cpu().numpy(), want[k]), k
    # captured under VAR_NO_REORDER (no tile-order buffers, nothing allocated) and replayed twice
    ds.set_variant(gpu.VAR_NO_REORDER)
    with torch.cuda.stream(st):
        lens_abi(ds, ot, dt, depth, color, normal, st.cuda_stream, b)
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        lens_abi(ds, ot, dt, depth, color, normal, torch.cuda.current_stream(dev).cuda_stream, b)
    for _ in range(2):
        for t in (depth, color, normal):
            t.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k, t in (("depth", depth), ("color", color), ("normal", normal)):
            assert same_bits(t.cpu().numpy(), want[k]), k
    del g
    ds.close()


def test_plain_lens_plain_and_repeated_launches(gpu):
    w, h, b = SCENES["bunny"]
    s = host_scene(gpu, "bunny", w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.fisheye(cam_of(s), w, h, 120.0)
    a = plain_device(ds, b)
    l1 = lens(ds, o, d, bounces=b)
    assert len(ds.tile_costs()) == ((w + 7) // 8) * ((h + 7) // 8)
    l2 = lens(ds, o, d, bounces=b)  # on the order the first one learned
    l3 = lens(ds, o, d, bounces=b)
    c = plain_device(ds, b)
    for k in ("depth", "normal", "color"):
        assert same_bits(a[k], c[k]), k
        assert same_bits(l1[k], l2[k]) and same_bits(l1[k], l3[k]), k
    assert a["ray_count"] == c["ray_count"] and l1["ray_count"] == l2["ray_count"] == l3["ray_count"]
    # another ambient factor changes the colour of a lit pixel and nothing else
    l4 = lens(ds, o, d, bounces=b, ambient=0.5)
    assert same_bits(l4["depth"], l1["depth"]) and same_bits(l4["normal"], l1["normal"]) and not same_bits(l4["color"], l1["color"])
    ds.close()


def test_a_9_by_9_frame(gpu):
    s = host_scene(gpu, "random5", 9, 9)
    ds = gpu.DeviceScene(s)
    o, d = lenses.pinhole(cam_of(s), 9, 9)
    want = plain_device(ds, 5)
    got = lens(ds, o, d, bounces=5)
    assert_frames(got, want, "9x9")
    assert got["ray_count"] == want["ray_count"]
    o2, d2 = lenses.thin_lens(cam_of(s), 9, 9, 2, 0.1, 4.0, seed=2)
    want2 = big_lens_reduced(ds, o2, d2, 9, 9, 2, 5)
    assert_frames(lens(ds, o2, d2, bounces=5, samples=2), want2, "9x9 s=2", color="tol")
    ds.close()


# ---- 6. rejections ----
def test_rejections(gpu):
    import torch
    name = "random3"
    w, h, b = SCENES[name]
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.pinhole(cam_of(s), w, h)
    good = lens(ds, o, d, bounces=b)
    dev = torch.device("cuda", 0)
    ot, dt = torch.from_numpy(o.reshape(-1, 3)).to(dev), torch.from_numpy(d.reshape(-1, 3)).to(dev)
    depth, color, normal = torch.empty((h, w), device=dev), torch.empty((h, w, 3), device=dev), torch.empty((h, w, 3), device=dev)
    L = _lib.hip_lib()
    n = h * w

    def call(q, outs=(depth, color, normal), bounces=b):
        ptrs = [t.data_ptr() if t is not None else None for t in outs]
        return L.ctr_render_device_lens(ds._h, C.c_float(1e-3), bounces, C.byref(q) if q is not None else None, None, *ptrs, None, None)

    def refused(q, word, **kw):
        assert call(q, **kw) == 1, word  # CTR_E_INVALID
        assert word.encode() in L.ctr_last_error(), (word, L.ctr_last_error())

    amb = ds._ambient
    refused(None, "null lens")
    refused(_lib.Lens(n, 1, amb, None, dt.data_ptr()), "null rays")
    refused(_lib.Lens(n, 1, amb, ot.data_ptr(), None), "null rays")
    refused(_lib.Lens(n, 1, amb, ot.data_ptr(), dt.data_ptr()), "null output", outs=(depth, None, normal))
    refused(_lib.Lens(n, 1, amb, ot.data_ptr(), dt.data_ptr()), "bounces", bounces=16)
    refused(_lib.Lens(n - 1, 1, amb, ot.data_ptr(), dt.data_ptr()), "n_rays")
    refused(_lib.Lens(n, 2, amb, ot.data_ptr(), dt.data_ptr()), "n_rays")
    for bad in (0, 3, 16):
        refused(_lib.Lens(n, bad, amb, ot.data_ptr(), dt.data_ptr()), "samples")
    # rays in host memory
    refused(_lib.Lens(n, 1, amb, o.ctypes.data, dt.data_ptr()), "d_origin is not device memory")
    refused(_lib.Lens(n, 1, amb, ot.data_ptr(), d.ctypes.data), "d_dir is not device memory")
    # the sample frame's size limits
    ds.set_size(0x7FFFFFFF, 1)
    refused(_lib.Lens(16 * 0x7FFFFFFF, 4, amb, ot.data_ptr(), dt.data_ptr()), "exceeds 32 bits")
    ds.set_size(w, h)
    # variant bits without a lens build
    for var in (gpu.VAR_STATS, gpu.VAR_IGNORE_TRANSPARENT, gpu.VAR_NO_PREFILTER, gpu.VAR_NO_CLUSTER):
        ds.set_variant(var)
        refused(_lib.Lens(n, 1, amb, ot.data_ptr(), dt.data_ptr()), "no build for")
        with pytest.raises(RuntimeError):
            ds.render_lens(o, d, bounces=b)
    ds.set_variant(0)
    # the Python layer's own checks
    with pytest.raises(ValueError):
        ds.render_lens(o[:-1], d[:-1], bounces=b)
    with pytest.raises(ValueError):
        ds.render_lens(o.astype(np.float64), d, bounces=b)
    with pytest.raises(ValueError):
        ds.render_lens(o, d, bounces=b, samples=3)
    with pytest.raises(TypeError):
        ds.render_lens(o.tolist(), d, bounces=b)
    # the handle renders normally afterwards; bits that pick no other result are honoured or ignored
    again = lens(ds, o, d, bounces=b)
    for k in ("depth", "normal", "color"):
        assert same_bits(again[k], good[k]), k
    for var in (gpu.VAR_MERGE, gpu.VAR_NO_DIRECT, gpu.VAR_NO_ANYHIT, gpu.VAR_NO_REORDER, gpu.VAR_IMAGE_ORDER_FIRST, gpu.VAR_NO_OCC6):
        ds.set_variant(var)
        r = lens(ds, o, d, bounces=b)
        for k in ("depth", "normal", "color"):
            assert same_bits(r[k], good[k]), (var, k)
        assert r["ray_count"] == good["ray_count"]
    ds.close()
