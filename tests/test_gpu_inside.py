"""Inside queries on the GPU (ctr_count_crossings, ctr_inside_points; DeviceScene.count_crossings, inside, signed_distance) against
tests/cross_ref.py, the NumPy restatement of include/cutrace_inside.h (held against the float64 winding number by
tests/test_inside_cpu.py), against the kernels' own linear walk, against the winding number itself, and against fresh handles after
every kind of edit.  The answers are integers and signs: "equal" is exact everywhere."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import cross_ref, hits_ref, ray_ref, util
from tests.conftest import load_scene
from tests.gpu_support import same_tensors
from tests.live import OFF, guard_scene, guard_tris, moved, room_scene, scene_with, staircase
from tests.topology_support import appended, fresh_handle, mesh_object, without
from tests.util import f32_bits, pow2, random_rays, range_offset, render_range_scene_json, scaled_scene_json, to_np

pytestmark = pytest.mark.gpu
f32 = np.float32
BOTH = ("count", "signed")
SIZES = (1, 63, 64, 65, 127, 128, 129, 4099)
KINDS = {ray_ref.OBJ_TRIANGLE: "triangle", ray_ref.OBJ_MESH: "mesh", ray_ref.OBJ_PLANE: "plane", ray_ref.OBJ_SPHERE: "sphere"}


def _same(got, want, what):
    for k in BOTH:
        g, w = got[k], np.asarray(want[k]).astype(np.int32)
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{what}: {k} differs in {int((g != w).sum())} of {len(w)} rays, first {np.flatnonzero(g != w)[:5]}"


def _walks(ds, o, d, what, **kw):
    """the default walk's answer, which is also the linear walk's"""
    a = ds.count_crossings(o, d, outputs=BOTH, **kw)
    same_tensors(a, ds.count_crossings(o, d, outputs=BOTH, linear=True, **kw), f"{what}: tree against linear")
    return to_np(a)


def _check(ds, rs, o, d, what, **kw):
    got = _walks(ds, o, d, what, **kw)
    ref_kw = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in kw.items()}
    want = cross_ref.count_crossings(rs, o, d, **ref_kw)
    _same(got, want, what)
    return got


def _mesh_vertices(rs):
    return np.concatenate([rs.tris[ob["tri_begin"]:ob["tri_begin"] + ob["tri_count"]].reshape(-1, 3)
                           for ob in rs.objects if ob["type"] == ray_ref.OBJ_MESH and ob["tri_count"]])


def _rays(rs, n, seed, lo=-3.0, hi=3.0, aimed=0.25):
    """random_rays, the last `aimed` of them pointed EXACTLY at vertices of the scene's meshes (the counts there are whatever the
    inclusive edge rule gives each triangle — and the same on every walk)"""
    rng = np.random.RandomState(seed)
    o, d, _ = random_rays(rng, n, rs, lo, hi)
    m = int(n * aimed)
    v = _mesh_vertices(rs)
    d[n - m:] = (v[rng.randint(0, len(v), m)] - o[n - m:]).astype(f32)
    return o, d


# ---- 1. ray counts and shapes ----
@pytest.fixture(scope="module")
def bunny(ca):
    hs = load_scene(ca, "bunny", 32, 32)
    rs = ray_ref.RefScene(hs)
    ds = ca.DeviceScene(hs)
    o, d = _rays(rs, 4099, 3)
    yield ds, rs, o, d, cross_ref.count_crossings(rs, o, d)
    ds.close()


def test_counts_equal_the_reference_on_the_bunny_at_every_batch_size(bunny):
    ds, rs, o, d, want = bunny
    assert int(want["count"].max()) >= 4 and (want["count"] == 0).any() and (want["signed"] != 0).any()
    full = _walks(ds, o, d, "bunny.json")
    _same(full, want, "bunny.json")
    for m in SIZES:
        for linear in (False, True):
            part = to_np(ds.count_crossings(o[:m], d[:m], outputs=BOTH, linear=linear))
            assert part["count"].shape == (m,) and part["signed"].shape == (m,)
            _same(part, {k: want[k][:m] for k in BOTH}, f"{m} rays linear={linear}")
    assert list(ds.count_crossings(o[:5], d[:5])) == ["count"] and list(ds.count_crossings(o[:5], d[:5], outputs=("signed",))) == ["signed"]
    empty = ds.count_crossings(np.zeros((0, 3), f32), np.zeros((0, 3), f32), outputs=BOTH)
    assert empty["count"].shape == (0,) and empty["signed"].shape == (0,)


def test_counts_equal_the_reference_on_the_smallest_and_the_deepest_trees(ca, tmp_path):
    """a mesh of one triangle and one of two (a tree of a single node), and live.staircase(), the deepest tree the suite can make"""
    one = f32([[[-1.0, -0.8, 0.3], [1.2, -0.7, 0.1], [0.1, 1.1, 0.5]]])
    two = f32([[[-1, -1, -0.6], [1, -1, -0.6], [1, 1, -0.4]], [[-1, -1, -0.6], [1, 1, -0.4], [-1, 1, -0.4]]])
    hs = scene_with(ca, tmp_path, "deep", [staircase(), one, two], w=32, h=32)
    rs, ds = ray_ref.RefScene(hs), ca.DeviceScene(hs)
    o, d = _rays(rs, 3000, 4, -1.5, 1.5, aimed=0.5)
    got = _check(ds, rs, o, d, "staircase, one triangle, two triangles")
    per = [_check(ds, rs, o, d, f"object {i}", object=i)["count"] for i in range(3)]
    assert all(int(p.sum()) > 20 for p in per), [int(p.sum()) for p in per]
    assert int(got["count"].max()) >= 2
    ds.close()


# ---- 2. a guarded mesh: the walk starts at node 0 ----
def test_a_mesh_with_guard_records_is_counted_once(ca, tmp_path):
    """three triangles in the eye's plane get guard records: the RAY walk starts at the spare node, whose guard leaf holds copies of
    them.  A count that started there would count every crossing of those three twice."""
    tris = guard_tris(3, n_other=40, seed=6, zero_area=False)
    big = guard_tris(65, n_other=5, seed=8, zero_area=False) + f32([2.5, 0.0, 0.0])   # more than the guard holds: walked linearly by rays
    hs = util.parse(ca, guard_scene(tmp_path, "inside_guard", [tris, big], OFF, eye=[0.3, 3.0, 0.5], w=32, h=32))
    ds = ca.DeviceScene(hs)
    assert ds.guard_state(0) == ([0, 1, 2], False) and ds.guard_state(1)[1] is True, (ds.guard_state(0), ds.guard_state(1))
    rs = ray_ref.RefScene(hs)
    rng = np.random.RandomState(5)
    o, d = _rays(rs, 2000, 5, -3.0, 5.0)
    # ... and rays through the inside of the guarded triangles
    w = rng.dirichlet([1, 1, 1], 600)
    target = np.einsum("nk,nkc->nc", w, tris[rng.randint(0, 3, 600)].astype(np.float64))
    o2 = rng.uniform(-3, 3, (600, 3)).astype(f32)
    o, d = np.concatenate([o, o2]), np.concatenate([d, (target - o2).astype(f32)])
    got = _check(ds, rs, o, d, "guarded mesh and linear mesh")
    only = cross_ref.count_crossings(rs, o[2000:], d[2000:], object=0)["count"]
    assert int((only > 0).sum()) > 500, "the rays meant for the guarded triangles miss them"
    _check(ds, rs, o, d, "guarded mesh alone", object=0)
    assert {0, 1, 2} <= set(np.unique(got["count"]))
    ds.close()


# ---- 3. scenes of several objects; selection ----
def test_counts_on_three_meshes_and_planes(ca):
    hs = load_scene(ca, "mirror", 32, 32)
    rs, ds = ray_ref.RefScene(hs), ca.DeviceScene(hs)
    assert sum(o["type"] == ray_ref.OBJ_MESH for o in rs.objects) >= 3 and any(o["type"] == ray_ref.OBJ_PLANE for o in rs.objects)
    o, d = _rays(rs, 1500, 6)
    _check(ds, rs, o, d, "mirror.json")
    _check(ds, rs, o, d, "mirror.json without planes", skip_planes=True)
    ds.close()


@pytest.fixture(scope="module")
def room(ca, tmp_path_factory):
    hs = util.parse(ca, room_scene(tmp_path_factory.mktemp("inside_room"), "room", w=32, h=32))
    rs, ds = ray_ref.RefScene(hs), ca.DeviceScene(hs)
    o, d = _rays(rs, 2000, 7, -4.0, 7.0)
    tri = next(ob for ob in rs.objects if ob["type"] == ray_ref.OBJ_TRIANGLE)     # small: some rays are sent through it
    w = np.random.RandomState(17).dirichlet([1, 1, 1], 100)
    d[500:600] = (w @ np.stack([tri["v0"], tri["v1"], tri["v2"]]).astype(np.float64) - o[500:600]).astype(f32)
    yield ds, rs, (o, d)
    ds.close()


def test_object_and_the_skip_flags_select_the_terms(room):
    ds, rs, (o, d) = room
    by_kind = {}
    for i, ob in enumerate(rs.objects):
        by_kind.setdefault(KINDS[ob["type"]], i)
    assert set(by_kind) == {"mesh", "sphere", "plane", "triangle"}
    everything = _check(ds, rs, o, d, "room")
    for kind, i in by_kind.items():
        got = _check(ds, rs, o, d, f"object={i} ({kind})", object=i)
        assert int(got["count"].sum()) > 0, kind
    no_planes = _check(ds, rs, o, d, "skip_planes", skip_planes=True)
    no_tris = _check(ds, rs, o, d, "skip_triangles", skip_triangles=True)
    solids = _check(ds, rs, o, d, "both", skip_planes=True, skip_triangles=True)
    want = cross_ref.count_crossings(rs, o, d, solids=True)
    _same(solids, want, "both flags are what inside counts")
    assert (everything["count"] >= no_planes["count"]).all() and (no_planes["count"] >= solids["count"]).all()
    assert (everything["count"] != no_tris["count"]).any() and (no_planes["count"] != everything["count"]).any()
    # a plane alone with planes skipped: nothing
    got = to_np(ds.count_crossings(o, d, object=by_kind["plane"], skip_planes=True, outputs=BOTH))
    assert not got["count"].any() and not got["signed"].any()
    for kind in ("plane", "triangle"):
        with pytest.raises(RuntimeError, match=("plane" if kind == "plane" else "stand-alone triangle")):
            ds.inside(o[:10], object=by_kind[kind])
    for kind in ("mesh", "sphere"):
        r = to_np(ds.inside(o, object=by_kind[kind], outputs=("inside", "votes")))
        want = cross_ref.inside(rs, o, ca_dirs(), object=by_kind[kind])
        assert np.array_equal(r["votes"], want["votes"]) and np.array_equal(r["inside"], want["inside"]), kind
    assert to_np(ds.inside(o, object=by_kind["sphere"]))["inside"].sum() > 0


def ca_dirs():
    import cutrace_amd
    return cutrace_amd.inside_default_dirs()


# ---- 4. per-ray intervals, rays that are none ----
def test_per_ray_intervals_and_degenerate_rays(room):
    import torch
    ds, rs, (o, d) = room
    o, d = o.copy(), d.copy()
    n = len(o)
    rng = np.random.RandomState(8)
    mn = rng.choice([0.0, 1e-3, -0.5, 0.25, 2.0, -np.inf], n).astype(f32)
    mx = rng.choice([np.inf, 0.5, 3.0, 10.0, 1e-3, np.nan], n).astype(f32)
    odd = np.arange(3, n, 41)
    bad = [(0, [np.nan, 0, 0]), (0, [0, np.inf, 0]), (0, [0, 0, -np.inf]), (1, [0, 0, 0]), (1, [-0.0, 0.0, -0.0]), (1, [np.nan, 1, 0]),
           (1, [1, np.inf, 0]), (1, [0, 1, -np.inf])]
    for j, i in enumerate(odd):
        which, v = bad[j % len(bad)]
        (o if which == 0 else d)[i] = v
    for kw in (dict(min_t=torch.from_numpy(mn), max_t=torch.from_numpy(mx)), dict(min_t=torch.from_numpy(mn)), dict(max_t=torch.from_numpy(mx)),
               dict(min_t=0.25, max_t=3.0)):
        got = _check(ds, rs, o, d, f"per-ray {sorted(kw)}", **kw)
        assert not got["count"][odd].any() and not got["signed"][odd].any()
        assert got["count"].any()
    got = _check(ds, rs, o, d, "NaN ends", min_t=0.0, max_t=torch.from_numpy(mx))
    assert not got["count"][np.isnan(mx)].any()
    with pytest.raises(ValueError):
        ds.count_crossings(o, d, max_t=torch.ones(7))


# ---- 5. scale and offset ----
@pytest.mark.parametrize("case", [(-20, None), (0, None), (24, None), (0, 18)], ids=lambda c: f"k={c[0]},e={c[1]}")
def test_counts_across_scale_and_offset(ca, tmp_path, case):
    k, e = case
    hs = util.parse(ca, scaled_scene_json(tmp_path, k) if e is None else render_range_scene_json(tmp_path, k, e, w=32, h=32))
    rs, ds = ray_ref.RefScene(hs), ca.DeviceScene(hs)
    base, d, _ = util.sweep_rays(9, 2000, ray_ref.RefScene(util.parse(ca, scaled_scene_json(tmp_path, 0))))   # the rays of the scene at scale 1
    o = (base * pow2(k) + range_offset(k, e)).astype(f32)
    v = _mesh_vertices(rs)
    rng = np.random.RandomState(10)
    d[1500:] = (v[rng.randint(0, len(v), 500)] - o[1500:]).astype(f32)   # aimed at this scene's own vertices
    got = _check(ds, rs, o, d, f"k={k} e={e}")
    assert int((got["count"] > 0).sum()) > 500 and int(got["count"].max()) >= 3
    p = o[:1000]
    r = ds.inside(p, outputs=("inside", "votes"))
    same_tensors(r, ds.inside(p, outputs=("inside", "votes"), linear=True), f"k={k} e={e}: inside, tree against linear")
    want = cross_ref.inside(rs, p, ca_dirs())
    assert np.array_equal(to_np(r)["votes"], want["votes"]), f"k={k} e={e}: votes"
    ds.close()


# ---- 6. inside, votes, signed distance against the winding number ----
@pytest.mark.parametrize("name", ["bunny", "skull", "mirror"])
def test_inside_votes_and_signed_distance_equal_the_winding_truth(ca, tmp_path, name):
    import torch
    tris = np.asarray(ca.scenes.read_stl(os.path.join(util.ROOT, "scene", name + ".stl")), f32)
    hs = scene_with(ca, tmp_path, name, [tris], w=32, h=32)          # the mesh (object 0) over a floor
    ds = ca.DeviceScene(hs)
    p = cross_ref.box_points(tris, 4099, 7)
    if name == "bunny":
        p = np.concatenate([p, cross_ref.centroid_points(tris)])
    truth = cross_ref.winding_number(tris, p) != 0
    assert 20 < int(truth.sum()) < len(p) - 20
    r = ds.inside(p, outputs=("inside", "votes"))
    same_tensors(r, ds.inside(p, outputs=("inside", "votes"), linear=True), f"{name}: tree against linear")
    got = to_np(r)
    assert got["inside"].dtype == np.bool_ and got["votes"].dtype == np.uint8
    assert np.array_equal(got["inside"], truth), f"{name}: inside differs from the winding number at {np.flatnonzero(got['inside'] != truth)[:5]}"
    assert set(np.unique(got["votes"])) == {0, 3}                     # every ray alone is right on these points
    # without votes a wave may stop early: the same answer
    assert np.array_equal(to_np(ds.inside(p))["inside"], truth) and np.array_equal(to_np(ds.inside(p, object=0))["inside"], truth)
    # the votes are three count_crossings launches' parities
    dirs = ca_dirs()
    pt = torch.from_numpy(p).cuda()
    votes = sum((ds.count_crossings(pt, torch.from_numpy(np.broadcast_to(dv, p.shape).copy()).cuda(), skip_planes=True,
                                    skip_triangles=True)["count"] & 1) for dv in dirs)
    assert torch.equal(votes.to(torch.uint8), r["votes"])
    # signed distance: nearest_points' bits with the truth's sign
    dist = to_np(ds.nearest_points(p, skip_planes=True, outputs=("distance",)))["distance"]
    want = np.where(truth, -dist, dist).astype(f32)
    for linear in (False, True):
        sd = to_np({"d": ds.signed_distance(pt, linear=linear)})["d"]
        assert np.array_equal(f32_bits(sd), f32_bits(want)), f"{name}: signed distance, linear={linear}"
    assert (want < 0).any() and (want > 0).any()
    # max_dist: half of the INSIDE points are farther than it and keep +inf (points within 1e-5 of the limit are not looked at)
    md = float(np.median(dist[truth]))
    sd = to_np({"d": ds.signed_distance(p, max_dist=md, object=0)})["d"]
    far, near = dist > f32(md * (1 + 1e-5)), dist < f32(md * (1 - 1e-5))
    assert np.isposinf(sd[far]).all() and truth[far].any() and np.array_equal(f32_bits(sd[near]), f32_bits(want[near])) and truth[near].any()
    # caller-supplied directions: one (each default direction alone is right here), and five
    for k in range(3):
        one = to_np(ds.inside(p, dirs=dirs[k:k + 1], outputs=("inside", "votes")))
        assert np.array_equal(one["inside"], truth) and np.array_equal(one["votes"], truth.astype(np.uint8)), k
    five = np.random.RandomState(11).normal(size=(5, 3)).astype(f32)
    sub = slice(0, len(p), 8)
    r5 = to_np(ds.inside(p[sub], dirs=five, outputs=("inside", "votes")))
    w5 = cross_ref.inside(ray_ref.RefScene(hs), p[sub], five)
    assert np.array_equal(r5["votes"], w5["votes"]) and np.array_equal(r5["inside"], w5["inside"]) and int(r5["votes"].max()) == 5
    assert np.array_equal(to_np(ds.inside(p[sub], dirs=torch.from_numpy(five)))["inside"], w5["inside"])
    # points that are none: outside, no votes, and their distance keeps its sign
    q = p[:200].copy()
    q[::7, 1] = np.nan
    q[3::7, 2] = np.inf
    rq = to_np(ds.inside(q, outputs=("inside", "votes")))
    dead = ~np.isfinite(q).all(1)
    assert not rq["inside"][dead].any() and not rq["votes"][dead].any() and np.array_equal(rq["inside"][~dead], truth[:200][~dead])
    assert np.isposinf(to_np({"d": ds.signed_distance(q)})["d"][dead]).all()
    ds.close()


def test_nothing_is_inside_the_frame(ca, tmp_path):
    """scene/frame.stl holds every triangle twice: every count is even"""
    tris = np.asarray(ca.scenes.read_stl(os.path.join(util.ROOT, "scene", "frame.stl")), f32)
    hs = scene_with(ca, tmp_path, "frame", [tris], w=32, h=32)
    ds = ca.DeviceScene(hs)
    p = cross_ref.box_points(tris, 1024, 7)
    r = to_np(ds.inside(p, outputs=("inside", "votes")))
    assert not r["inside"].any() and not r["votes"].any()
    d = np.broadcast_to(ca_dirs()[0], p.shape).copy()
    c = to_np(ds.count_crossings(p, d, object=0, outputs=BOTH))
    assert (c["count"] % 2 == 0).all() and int(c["count"].max()) >= 2
    sd = to_np({"d": ds.signed_distance(p)})["d"]
    assert (sd >= 0).all()
    ds.close()


# ---- 7. live handles ----
def _three_calls(ds, o, d, p, linear):
    out = dict(ds.count_crossings(o, d, outputs=BOTH, linear=linear))
    out.update(ds.inside(p, outputs=("inside", "votes"), linear=linear))
    out["sd"] = ds.signed_distance(p, linear=linear)
    return out


def _equals_fresh(upd, fresh, o, d, p, what):
    for linear in (False, True):
        got = _three_calls(upd, o, d, p, linear)
        same_tensors(got, _three_calls(fresh, o, d, p, linear), f"{what} linear={linear}")
    return to_np(got)


def test_the_queries_follow_every_edit_of_the_handle(ca, tmp_path):
    sc = hits_ref.layered_description(tmp_path)
    bunny_tris = np.asarray(ca.scenes.read_stl(os.path.join(util.ROOT, "scene", "bunny.stl")), f32)
    sc["objects"][0] = mesh_object(tmp_path, "live", bunny_tris, 0)
    upd, hs = fresh_handle(ca, sc)
    rs = ray_ref.RefScene(hs)
    o, d = _rays(rs, 1500, 12)
    p = np.random.RandomState(13).uniform(-2.0, 2.0, (1500, 3)).astype(f32)
    state = {"sc": sc, "n": 0}

    def check(what):
        fresh, fhs = fresh_handle(ca, state["sc"])
        got = _equals_fresh(upd, fresh, o, d, p, what)
        want = cross_ref.count_crossings(ray_ref.RefScene(fhs), o[::4], d[::4])
        _same({k: got[k][::4] for k in BOTH}, want, f"{what}: reference")
        fresh.close()
        return got

    def with_mesh(tris):
        state["n"] += 1
        objs = list(state["sc"]["objects"])
        objs[0] = mesh_object(tmp_path, f"live_{state['n']}", tris, 0)
        state["sc"] = dict(state["sc"], objects=objs)

    before = check("as created")
    assert before["inside"].sum() > 20 and (before["sd"] < 0).any()
    turned = moved(bunny_tris, 0.7, 0.0)
    upd.update_mesh(0, turned)
    with_mesh(turned)
    after = check("update_mesh (a rotation)")
    assert not np.array_equal(after["inside"], before["inside"])
    skull = np.asarray(ca.scenes.read_stl(os.path.join(util.ROOT, "scene", "skull.stl")), f32)
    assert len(skull) != len(bunny_tris)
    upd.replace_mesh(0, skull, builder="host")
    with_mesh(skull)
    check("replace_mesh to another count")
    # a moved sphere
    upd.set_object(1, center=[0.2, 0.1, 1.5])
    objs = list(state["sc"]["objects"])
    objs[1] = dict(objs[1], center=[0.2, 0.1, 1.5])
    state["sc"] = dict(state["sc"], objects=objs)
    check("a moved sphere")
    # an added mesh, a removed object
    mirror = np.asarray(ca.scenes.read_stl(os.path.join(util.ROOT, "scene", "mirror.stl")), f32)
    upd.add_mesh(mirror, material=1, builder="host")
    state["sc"] = appended(state["sc"], mesh_object(tmp_path, "added", mirror, 1))
    check("add_mesh")
    upd.remove_object(2)
    state["sc"] = without(state["sc"], 2)
    check("remove_object")
    upd.close()


# ---- 8. streams; refusals that need a scene ----
def test_a_stream_of_the_callers(bunny):
    import torch
    ds, rs, o, d, want = bunny
    s = torch.cuda.Stream()
    ot, dt = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    a = ds.count_crossings(ot, dt, outputs=BOTH, stream=s)
    b = ds.inside(ot, outputs=("inside", "votes"), stream=s)
    c = ds.signed_distance(ot, stream=s)
    s.synchronize()
    _same(to_np(a), want, "on a stream")
    same_tensors(b, ds.inside(ot, outputs=("inside", "votes")), "inside on a stream")
    same_tensors({"d": c}, {"d": ds.signed_distance(ot)}, "signed_distance on a stream")


def test_bad_arguments(ca, bunny):
    import torch
    from cutrace_amd import _lib
    L = _lib.hip_lib()
    ds, rs, o, d, _ = bunny
    n = 100
    pts = torch.zeros(n, 3, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    flag = torch.empty(n, dtype=torch.uint8, device="cuda")
    host = np.zeros((n, 3), f32)
    n_obj = len(rs.objects)
    plane = next(i for i, ob in enumerate(rs.objects) if ob["type"] == ray_ref.OBJ_PLANE)

    def cq(**kw):
        x = _lib.CrossingQuery()
        x.n_rays, x.object, x.max_t = n, -1, float("inf")
        x.d_origin, x.d_dir, x.d_count = pts.data_ptr(), pts.data_ptr(), cnt.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def iq(**kw):
        x = _lib.InsideQuery()
        x.n_points, x.object = n, -1
        x.d_point, x.d_inside = pts.data_ptr(), flag.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = functools.partial(util.bad, L.ctr_count_crossings, ds._h)
    assert L.ctr_count_crossings(ds._h, C.byref(cq()), None) == 0
    bad(cq(object=n_obj), f"object {n_obj} outside [-1, {n_obj})")
    bad(cq(object=-2), "outside [-1")
    bad(cq(d_dir=None), "null rays")
    bad(cq(n_rays=1 << 31), "n_rays must be below 2^31")
    bad(cq(flags=8), "unknown flag bits 8")
    bad(cq(d_count=None), "no output")
    bad(cq(d_signed=host.ctypes.data), "d_signed is not device memory")
    bad(cq(d_origin=host.ctypes.data), "d_origin is not device memory")
    bad(cq(d_max_t=host.ctypes.data), "d_max_t is not device memory")
    assert L.ctr_count_crossings(ds._h, C.byref(cq(n_rays=0, d_origin=None, d_dir=None)), None) == 0
    bad = functools.partial(util.bad, L.ctr_inside_points, ds._h)
    table = (C.c_float * 48)(*([0.5] * 48))
    assert L.ctr_inside_points(ds._h, C.byref(iq()), None) == 0
    assert L.ctr_inside_points(ds._h, C.byref(iq(n_dirs=15, dirs=table)), None) == 0
    bad(iq(n_dirs=2, dirs=table), "n_dirs 2 is not 0 or an odd number up to 15")
    bad(iq(n_dirs=16, dirs=table), "n_dirs 16 is not 0 or an odd number up to 15")
    bad(iq(n_dirs=3), "null dirs")
    bad(iq(d_inside=None), "no output")
    bad(iq(flags=2), "unknown flag bits 2")
    bad(iq(object=plane), f"object {plane} is a plane")
    bad(iq(object=n_obj), "outside [-1")
    bad(iq(d_point=None), "null d_point")
    bad(iq(d_votes=host.ctypes.data), "d_votes is not device memory")
    bad(iq(d_distance=host.ctypes.data), "d_distance is not device memory")
    bad(iq(d_inside=host.ctypes.data), "d_inside is not device memory")
    torch.cuda.synchronize()
    for call in (lambda: ds.count_crossings(pts, pts, outputs=()), lambda: ds.count_crossings(pts, pts, outputs=("t",)),
                 lambda: ds.inside(pts, outputs=()), lambda: ds.inside(pts, dirs=np.ones((2, 3), f32)),
                 lambda: ds.inside(pts, dirs=np.ones((16, 3), f32)), lambda: ds.inside(pts.double()),
                 lambda: ds.count_crossings(pts, pts[:7]), lambda: ds.inside(pts, object=-1)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="outside"):
        ds.count_crossings(pts, pts, object=n_obj)
    with pytest.raises(RuntimeError, match="not finite or is all zero"):
        ds.inside(pts, dirs=np.zeros((1, 3), f32))
    if torch.cuda.device_count() > 1:
        other = torch.empty(n, dtype=torch.int32, device="cuda:1")
        functools.partial(util.bad, L.ctr_count_crossings, ds._h)(cq(d_count=other.data_ptr()), "d_count is not device memory")
        with pytest.raises(ValueError):
            ds.inside(pts.to("cuda:1"))
