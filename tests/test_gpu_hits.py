"""Hit lists on the GPU (ctr_list_hits, DeviceScene.list_hits) against three independent sources: tests/hits_ref.py (the chain over
the NumPy ray_cast of tests/ray_ref.py), a loop of cast_rays calls, and shadow().  "Same bits": bitwise, except against the NumPy
checker the sphere's texture coordinates (atan2f / asinf on the device, 1e-4)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import hits_ref, ray_ref, util
from tests.conftest import load_scene
from tests.gpu_support import same_tensors
from tests.topology_support import appended, fresh_handle, mesh_object, without
from tests.util import assert_same, f32_bits, random_rays, to_np

pytestmark = pytest.mark.gpu
f32 = np.float32
OUT = hits_ref.OUTPUTS


def _flat(h):
    """slot-major (K, n, ...) outputs as one batch of K * n"""
    return {k: h[k].reshape((-1,) + h[k].shape[2:]) for k in OUT if k in h}


def _same_lists(rs, got, want, what):
    """count and every per-slot output of `want` in `got`: the bits of tests/util.py assert_same; returns the slots filled"""
    assert np.array_equal(got["count"], want["count"]), f"{what}: count differs in {int((got['count'] != want['count']).sum())} rays"
    return assert_same(rs, _flat(got), _flat(want), what)


def _nonempty(count, K, what):
    """the reference's lists are what the test means to check: empty ones, long ones, full ones at K = 4, none full at K = 16.
    (15 % of empty lists is asked of the layered scene, which was built for it: 923 of its 4000 rays hit nothing.  scene/bunny.json
    is a closed room but for the side of the camera, and the reference alone leaves 175 of these 3000 rays without a hit; there
    the condition is that such rays exist.)"""
    n = len(count)
    assert (count == 0).sum() >= (0.15 * n if what == "layered" else 1) and (count >= 3).sum() >= 0.05 * n, (what, np.bincount(count))
    if K == 4:
        assert (count == 4).sum() >= 0.02 * n, (what, np.bincount(count))
    if K == 16:
        assert not (count == 16).any(), (what, np.bincount(count))


class Case:
    """one scene on the device with its rays and the reference's lists, computed once and left unchanged"""
    def __init__(self, ca, host_scene, o, d):
        self.rs = ray_ref.RefScene(host_scene)
        self.ds = ca.DeviceScene(host_scene)
        self.o, self.d = o, d
        self.ref = {}

    def want(self, K):
        if K not in self.ref:
            self.ref[K] = hits_ref.list_hits(self.rs, self.o, self.d, K)
        return self.ref[K]


@pytest.fixture(scope="module")
def layered(ca, tmp_path_factory):
    o, d = hits_ref.layered_rays()
    c = Case(ca, hits_ref.layered_scene(ca, tmp_path_factory.mktemp("layers")), o, d)
    yield c
    c.ds.close()


@pytest.fixture(scope="module")
def bunny(ca):
    s = load_scene(ca, "bunny", 32, 32)
    o, d, _ = random_rays(np.random.RandomState(3), 3000, ray_ref.RefScene(s), -3.0, 3.0)
    c = Case(ca, s, o, d)
    yield c
    c.ds.close()


# ---- 1. against hits_ref ----
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("which", ["layered", "bunny"])
def test_lists_equal_the_reference_chain(request, which, K):
    c = request.getfixturevalue(which)
    want = c.want(K)
    _nonempty(want["count"], K, which)
    for linear in (False, True):
        got = to_np(c.ds.list_hits(c.o, c.d, K, linear=linear))
        assert got["t"].shape == (K, len(c.o)) and got["point"].shape == (K, len(c.o), 3) and got["uv"].shape == (K, len(c.o), 2)
        assert _same_lists(c.rs, got, want, f"{which} K={K} linear={linear}") == int(want["count"].sum())


# ---- 2. against a loop of cast_rays ----
def _loop_of_casts(ds, o, d, K, min_t=1e-3, max_t=float("inf"), step=1e-3, **kw):
    """the same lists made by K calls of cast_rays with a per-ray min_t tensor, on the device"""
    import torch
    n = o.shape[0]
    m = torch.full((n,), float(min_t), dtype=torch.float32, device=o.device)
    live = torch.ones(n, dtype=torch.bool, device=o.device)
    count = torch.zeros(n, dtype=torch.int32, device=o.device)
    slots = {k: [] for k in OUT}
    miss = {"t": float("inf"), "object": -1, "prim": -1, "point": 0.0, "normal": 0.0, "uv": 0.0}
    for _ in range(K):
        r = ds.cast_rays(o, d, min_t=m, **kw)
        live = live & (r["object"] >= 0) & (r["t"] < max_t)
        for k in OUT:
            keep = live if r[k].dim() == 1 else live[:, None]
            slots[k].append(torch.where(keep, r[k], torch.full_like(r[k], miss[k])))
        count += live.to(torch.int32)
        m = torch.where(live, (r["t"].double() + step).float(), torch.full_like(m, float("inf")))
    out = {k: torch.stack(v) for k, v in slots.items()}
    out["count"] = count
    return out


@pytest.mark.parametrize("linear", [False, True])
def test_lists_equal_a_loop_of_cast_rays_bit_for_bit(layered, linear):
    import torch
    c = layered
    o, d = torch.from_numpy(c.o).cuda(), torch.from_numpy(c.d).cuda()
    full = c.ds.list_hits(o, d, 16, linear=linear)
    same_tensors(full, _loop_of_casts(c.ds, o, d, 16, linear=linear), f"K=16 linear={linear}")
    four = c.ds.list_hits(o, d, 4, linear=linear)
    same_tensors(four, _loop_of_casts(c.ds, o, d, 4, linear=linear), f"K=4 linear={linear}")
    assert torch.equal(four["count"], full["count"].clamp(max=4))
    for k in OUT:   # the first four slots of the K = 16 list are the K = 4 list
        same_tensors({k: four[k]}, {k: full[k][:4]}, f"prefix linear={linear}")
    assert int((full["count"] >= 3).sum()) > len(c.o) // 20
    mx = torch.from_numpy(np.random.RandomState(4).choice([0.5, 2.0, 100.0, np.inf], len(c.o)).astype(f32)).cuda()
    same_tensors(c.ds.list_hits(o, d, 16, max_t=mx, linear=linear), _loop_of_casts(c.ds, o, d, 16, max_t=mx, linear=linear), "per-ray max_t")


# ---- 3. against shadow ----
@pytest.mark.parametrize("which", ["layered", "random1", "random7"])
def test_a_lists_running_sum_is_shadow(ca, layered, which):
    import torch
    K = 24
    if which == "layered":
        rs, ds, o, d = layered.rs, layered.ds, layered.o, layered.d
    else:
        s = util.parse(ca, util._random_scene(int(which[6:]), w=32, h=32))
        rs, ds = ray_ref.RefScene(s), ca.DeviceScene(s)
        assert (rs.transparency > 0).any(), "a scene with transmitting materials is meant"
        o, d, _ = random_rays(np.random.RandomState(int(which[6:])), 3000, rs, -2.5, 2.5)
    max_t = np.random.RandomState(6).choice([0.5, 2.0, 100.0, np.inf], len(o)).astype(f32)
    want = hits_ref.list_hits(rs, o, d, K, min_t=f32(0.0 + 1e-3), max_t=max_t, step=1e-3)
    assert want["count"].max() < K, "the reference fills some ray's slots: its list may go on"
    for linear in (False, True):
        h = to_np(ds.list_hits(o, d, K, min_t=1e-3, max_t=torch.from_numpy(max_t), outputs=("object",), linear=linear))
        assert np.array_equal(h["count"], want["count"]) and np.array_equal(h["object"], want["object"]), f"{which} linear={linear}"
        got = hits_ref.shadow_from_lists(rs, h["count"], h["object"])
        sh = ds.shadow(o, d, max_t=torch.from_numpy(max_t), linear=linear).cpu().numpy()
        assert np.array_equal(f32_bits(got), f32_bits(sh)), f"{which} linear={linear}: {int((f32_bits(got) != f32_bits(sh)).sum())} rays"
    assert ((sh > 0) & (sh < 1)).any() and (sh == 1).any() and (sh == 0).any()
    if which != "layered":
        ds.close()


# ---- 4. parameters ----
def test_step_min_t_max_t_and_ignore_transparent_against_the_reference(layered):
    import torch
    c, K = layered, 16
    rng = np.random.RandomState(12)
    n = len(c.o)
    longest = {}
    for step in (2.0 ** -12, 0.0):
        want = hits_ref.list_hits(c.rs, c.o, c.d, K, step=step)
        for linear in (False, True):
            _same_lists(c.rs, to_np(c.ds.list_hits(c.o, c.d, K, step=step, linear=linear)), want, f"step {step} linear={linear}")
        longest[step] = int(want["count"].max())
    # the mesh rule: with step 0 a mesh hit at t is rejected whole by the next cast, and its farther layers vanish
    assert longest[0.0] < int(c.want(16)["count"].max())
    mn = rng.choice([1e-3, 0.0, -0.5, 0.25], n).astype(f32)
    mx = rng.choice([0.5, 2.0, 100.0, np.inf], n).astype(f32)
    want = hits_ref.list_hits(c.rs, c.o, c.d, K, min_t=mn, max_t=mx)
    assert (want["count"] == 0).sum() > (c.want(16)["count"] == 0).sum() and (want["count"] >= 3).any()
    for linear in (False, True):
        got = to_np(c.ds.list_hits(c.o, c.d, K, min_t=torch.from_numpy(mn), max_t=torch.from_numpy(mx), linear=linear))
        _same_lists(c.rs, got, want, f"per-ray min_t and max_t linear={linear}")
    want = hits_ref.list_hits(c.rs, c.o, c.d, K, ignore_transparent=True)
    opaque = [i for i in range(len(c.rs.objects)) if not c.rs.transparent(i)]
    assert set(np.unique(want["object"])) == set(opaque) | {-1}
    for linear in (False, True):
        _same_lists(c.rs, to_np(c.ds.list_hits(c.o, c.d, K, ignore_transparent=True, linear=linear)), want, f"ignore_transparent linear={linear}")


@pytest.mark.parametrize("j", [24, -24])
def test_directions_of_another_length_with_the_step_to_match(layered, j):
    """dir * 2^j: every t but a sphere's scales by 2^-j, and min_t and step with it"""
    c, K = layered, 16
    s, inv = util.pow2(j), float(util.pow2(-j))
    d = (c.d * s).astype(f32)
    want = hits_ref.list_hits(c.rs, c.o, d, K, min_t=f32(1e-3) * util.pow2(-j), step=1e-3 * inv)
    assert (want["count"] >= 3).sum() > len(c.o) // 20 and (want["count"] == 0).any()
    for linear in (False, True):
        got = to_np(c.ds.list_hits(c.o, d, K, min_t=float(f32(1e-3) * util.pow2(-j)), step=1e-3 * inv, linear=linear))
        _same_lists(c.rs, got, want, f"dir * 2^{j} linear={linear}")


# ---- 5. shapes ----
def test_sizes_output_subsets_counts_and_graph_capture(ca, layered):
    import torch
    c, K = layered, 4
    o, d = torch.from_numpy(c.o[:1000]).cuda(), torch.from_numpy(c.d[:1000]).cuda()
    full = c.ds.list_hits(o, d, K)
    _same_lists(c.rs, to_np(full), {k: v[..., :1000] if k == "count" else v[:, :1000] for k, v in c.want(K).items()}, "1000 rays")
    for m in (0, 1, 63, 64, 65, 129):
        part = c.ds.list_hits(o[:m], d[:m], K)
        assert part["count"].shape == (m,) and part["t"].shape == (K, m) and part["normal"].shape == (K, m, 3)
        same_tensors(part, {k: (v[:m] if k == "count" else v[:, :m]) for k, v in full.items()}, f"{m} rays")
    # K = 1 is cast_rays wherever t < max_t
    one = c.ds.list_hits(o, d, 1, max_t=2.0)
    cast = c.ds.cast_rays(o, d)
    near = cast["t"] < 2.0
    assert torch.equal(one["count"], near.to(torch.int32)) and 100 < int(near.sum()) < int((cast["object"] >= 0).sum())
    for k in OUT:
        same_tensors({k: one[k][0][near]}, {k: cast[k][near]}, "K = 1")
    # every single output, a pair, and none
    for names in [(k,) for k in OUT] + [("uv", "prim")]:
        sub = c.ds.list_hits(o, d, K, outputs=names)
        assert list(sub) == ["count"] + list(names)
        same_tensors(sub, {k: full[k] for k in sub}, str(names))
    deep = c.ds.list_hits(o, d, 16)["count"]
    for k_max in (K, 16, 65535):
        alone = c.ds.list_hits(o, d, k_max, outputs=())
        assert list(alone) == ["count"] and torch.equal(alone["count"], deep.clamp(max=k_max)), k_max
    # unfilled slots hold cast_rays' miss values
    f = to_np(full)
    for j in range(K):
        off = j >= f["count"]
        assert off.any() and np.isposinf(f["t"][j, off]).all() and (f["object"][j, off] == -1).all() and (f["prim"][j, off] == -1).all()
        assert not f["point"][j, off].any() and not f["normal"][j, off].any() and not f["uv"][j, off].any()
        assert np.isfinite(f["t"][j, ~off]).all() and (f["object"][j, ~off] >= 0).all()
    # a single-stream graph capture, replayed once
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.ds.list_hits(o, d, K)   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = c.ds.list_hits(o, d, K)
    graph.replay()
    torch.cuda.synchronize()
    same_tensors(cap, full, "graph replay")


# ---- 6. rays that must not disturb others ----
def test_nan_zero_and_infinite_rays_among_ordinary_ones(layered):
    c, K = layered, 16
    o, d = c.o[:256].copy(), c.d[:256].copy()
    o[10, 1] = np.nan
    d[70] = 0.0
    d[130, 0] = np.inf
    d[200] = [np.inf, -np.inf, np.nan]
    odd = [10, 70, 130, 200]
    want = hits_ref.list_hits(c.rs, o, d, K)
    base = c.want(K)
    for linear in (False, True):
        got = to_np(c.ds.list_hits(o, d, K, linear=linear))
        assert np.array_equal(got["count"][odd], want["count"][odd]), (got["count"][odd], want["count"][odd])
        rest = np.setdiff1d(np.arange(256), odd)
        _same_lists(c.rs, {k: (v[rest] if k == "count" else v[:, rest]) for k, v in got.items()},
                    {k: (v[rest] if k == "count" else v[:, rest]) for k, v in base.items()}, f"neighbours linear={linear}")


# ---- 7. bad arguments on the device ----
def test_bad_arguments(ca, layered):
    import torch
    from cutrace_amd import _lib
    L = _lib.hip_lib()
    ds = layered.ds
    n, K = 100, 4
    o = torch.zeros(n, 3, device="cuda")
    d = torch.ones(n, 3, device="cuda")
    t = torch.empty(K * n, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    host = np.zeros((K * n, 3), f32)

    def q(**kw):
        x = _lib.HitQuery()
        x.n_rays, x.max_hits, x.step = n, K, 1e-3
        x.d_origin, x.d_dir = o.data_ptr(), d.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = functools.partial(util.bad, L.ctr_list_hits, ds._h)
    assert L.ctr_list_hits(ds._h, C.byref(q(d_t=t.data_ptr(), d_count=cnt.data_ptr())), None) == 0
    bad(q(d_t=t.data_ptr(), d_origin=None), "null rays")
    bad(q(d_t=t.data_ptr(), flags=4), "unknown flag bits 4")
    bad(q(d_t=t.data_ptr(), max_hits=0), "max_hits 0 outside")
    bad(q(d_t=t.data_ptr(), step=-1e-3), "step must be finite")
    bad(q(), "no output")
    bad(q(d_point=host.ctypes.data), "d_point is not device memory")
    bad(q(d_count=host.ctypes.data), "d_count is not device memory")
    bad(q(d_t=t.data_ptr(), d_origin=host.ctypes.data), "d_origin is not device memory")
    bad(q(d_t=t.data_ptr(), n_rays=1 << 31), "n_rays must be below 2^31")
    bad(q(d_t=t.data_ptr(), n_rays=1 << 20, max_hits=1 << 11), "n_rays * max_hits must be below 2^31")
    bad(q(d_t=t.data_ptr(), d_count=cnt.data_ptr(), n_rays=(1 << 31) // 65535 + 1, max_hits=65535), "n_rays * max_hits must be below 2^31")
    assert L.ctr_list_hits(ds._h, C.byref(q(d_t=t.data_ptr(), n_rays=0)), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ds.list_hits(o.double(), d, K)
    with pytest.raises(ValueError):
        ds.list_hits(o, d[:10], K)
    with pytest.raises(ValueError):
        ds.list_hits(o, d, K, max_t=torch.ones(7, device="cuda"))
    with pytest.raises(ValueError):
        ds.list_hits(o, d, K, outputs=("depth",))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ds.list_hits(o.to("cuda:1"), d, K)


# ---- 8. larger scenes ----
def test_slot_zero_of_the_camera_rays_is_the_render(ca):
    s = load_scene(ca, "bunny", 96, 54)
    ds = ca.DeviceScene(s)
    o, d = ray_ref.camera_rays(ray_ref.RefScene(s).cam)
    h = ds.list_hits(o, d, 4)
    cast = ds.cast_rays(o, d, min_t=1e-3)
    for k in OUT:
        same_tensors({k: h[k][0]}, {k: cast[k]}, "slot 0")
    r = ds.render_uv(bounces=0, fudge=1e-3)
    got = to_np(h)
    assert np.array_equal(f32_bits(got["t"][0]), f32_bits(r["depth"].reshape(-1)))
    assert np.array_equal(f32_bits(got["normal"][0]), f32_bits(r["normal"].reshape(-1, 3)))
    assert (got["count"] >= 2).sum() > len(o) // 20
    ds.close()


def test_linear_and_default_walk_agree_on_the_dense_bunny(ca, tmp_path):
    import torch
    from cutrace_amd import scenes
    s = ca.HostScene.load(scenes.make_dense_bunny(str(tmp_path), rounds=3, width=64, height=36))
    assert s.ok
    ds = ca.DeviceScene(s)
    g = torch.Generator().manual_seed(8)
    n = 100000
    o = (torch.rand(n, 3, generator=g) * 2.4 - 1.2).cuda()
    o[:, 1] += 0.5
    d = torch.randn(n, 3, generator=g).cuda()
    a = ds.list_hits(o, d, 8)
    b = ds.list_hits(o, d, 8, linear=True)
    same_tensors(a, b, "dense bunny")
    assert int((a["count"] >= 2).sum()) > n // 20
    ds.close()


# ---- 9. the handle is undisturbed and stays current ----
def test_renders_before_and_after_hit_lists_are_identical(ca):
    s = load_scene(ca, "bunny", 128, 72)
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=5)
    ca_ = ds.last_counters()
    o, d, _ = random_rays(np.random.RandomState(10), 50000, rs, -3.0, 3.0)
    ds.list_hits(o, d, 8)
    ds.list_hits(o, d, 3, linear=True, outputs=("t",))
    ds.list_hits(o, d, 65535, outputs=())
    b = ds.render(bounces=5)
    cb = ds.last_counters()
    for k in ("depth", "color", "normal"):
        assert np.array_equal(f32_bits(a[k]), f32_bits(b[k])), k
    assert a["ray_count"] == b["ray_count"] and np.array_equal(ca_[:2], cb[:2])
    ds.close()


def test_lists_follow_an_added_mesh_and_a_removed_object(ca, tmp_path):
    sc = hits_ref.layered_description(tmp_path)
    tris = np.asarray([[[-2, -1, z], [2, -1, z + 0.3], [0, 2, z]] for z in (-1.5, -0.8, 0.7, 1.6)], f32)
    upd = ca.DeviceScene(util.parse(ca, sc))
    o, d = hits_ref.layered_rays(2000, seed=5)
    before = upd.list_hits(o, d, 16)
    upd.add_mesh(tris, material=1, builder="host")
    upd.remove_object(0)
    fresh, hs = fresh_handle(ca, without(appended(sc, mesh_object(tmp_path, "added", tris, 1)), 0))
    for linear in (False, True):
        got = upd.list_hits(o, d, 16, linear=linear)
        same_tensors(got, fresh.list_hits(o, d, 16, linear=linear), f"edited handle linear={linear}")
    g = to_np(got)
    assert (g["object"] == 6).any() and not np.array_equal(g["count"], before["count"].cpu().numpy())   # the new mesh is object 6 now
    _same_lists(ray_ref.RefScene(hs), g, hits_ref.list_hits(ray_ref.RefScene(hs), o, d, 16), "edited handle against the reference")
    upd.close()
    fresh.close()
