"""Nearest-point queries on the GPU (ctr_nearest_points, DeviceScene.nearest_points) against tests/nearest_ref.py, the NumPy
restatement of cutrace_amd/csrc/nearest_point.h (pinned on the CPU by tests/test_nearest_cpu.py), against the kernel's own linear
walk, and against fresh handles after every kind of edit.  "Same bits": bitwise, every output."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import hits_ref, nearest_ref, ray_ref, util
from tests.conftest import load_scene
from tests.gpu_support import same_tensors
from tests.live import OFF, guard_scene, guard_tris, moved
from tests.topology_support import appended, fresh_handle, mesh_object, without
from tests.util import OFFSET_CASES, SCALE_EXPONENTS, f32_bits, pow2, range_offset, render_range_scene_json, to_np

pytestmark = pytest.mark.gpu
f32 = np.float32
OUT = nearest_ref.OUTPUTS
KINDS = {ray_ref.OBJ_TRIANGLE: "triangle", ray_ref.OBJ_MESH: "mesh", ray_ref.OBJ_PLANE: "plane", ray_ref.OBJ_SPHERE: "sphere"}


def _same(got, want, what, rows=None):
    """every output of the reference in the kernel's answer, bit for bit (rows: only those points)"""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    for k in ("object", "prim"):
        g, w = pick(got[k]), pick(np.asarray(want[k])).astype(np.int32)
        assert np.array_equal(g, w), f"{what}: {k} differs in {int((g != w).sum())} of {len(w)} points, first {np.flatnonzero(g != w)[:5]}"
    for k in ("distance", "point", "normal"):
        g, w = f32_bits(pick(got[k])), f32_bits(pick(want[k]))
        bad = (g != w).reshape(len(g), -1).any(1)
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {len(g)} points, first {np.flatnonzero(bad)[:5]}"


def _miss(r, rows, what):
    assert np.isposinf(r["distance"][rows]).all() and (r["object"][rows] == -1).all() and (r["prim"][rows] == -1).all(), what
    assert not r["point"][rows].any() and not r["normal"][rows].any(), what


def _kinds_that_win(rs, objects):
    return {KINDS[rs.objects[i]["type"]] for i in np.unique(objects) if i >= 0}


def _points(rs, n, seed, lo=-3.0, hi=3.0):
    """uniform points in [lo, hi]^3, and for every sphere a few points about its surface and its centre (inside and outside)"""
    rng = np.random.RandomState(seed)
    p = [rng.uniform(lo, hi, (n, 3))]
    for o in rs.objects:
        if o["type"] == ray_ref.OBJ_SPHERE:
            d = rng.normal(size=(24, 3))
            p.append(o["v0"] + d / np.linalg.norm(d, axis=1)[:, None] * float(o["f0"]) * rng.uniform(0.0, 1.6, (24, 1)))
            p.append(o["v0"][None])
        if o["type"] == ray_ref.OBJ_TRIANGLE:
            c = (o["v0"] + o["v1"] + o["v2"]) / f32(3)
            p.append(c + rng.normal(0, 0.05, (24, 3)))
    return np.concatenate(p).astype(f32)


class Case:
    """one scene on the device with its points and the reference's answer, computed once and left unchanged"""
    def __init__(self, ca, host_scene, n=1500, seed=1):
        self.rs = ray_ref.RefScene(host_scene)
        self.ds = ca.DeviceScene(host_scene)
        self.p = _points(self.rs, n, seed)
        self.ref = {}

    def want(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self.ref:
            self.ref[key] = nearest_ref.nearest_points(self.rs, self.p, **kw)
        return self.ref[key]


@pytest.fixture(scope="module")
def bunny(ca):
    c = Case(ca, load_scene(ca, "bunny", 32, 32), seed=2)
    yield c
    c.ds.close()


@pytest.fixture(scope="module")
def sphere_plane(ca):
    c = Case(ca, load_scene(ca, "sphere_plane", 32, 32), seed=3)
    yield c
    c.ds.close()


@pytest.fixture(scope="module")
def layered(ca, tmp_path_factory):
    c = Case(ca, hits_ref.layered_scene(ca, tmp_path_factory.mktemp("layers")), seed=4)
    yield c
    c.ds.close()


@pytest.fixture(scope="module")
def multi(ca, tmp_path_factory):
    c = Case(ca, util.parse(ca, util._multi_mesh_scene(tmp_path_factory.mktemp("multi"), 5, w=32, h=32, n_mesh=3)), n=1200, seed=5)
    yield c
    c.ds.close()


# ---- 1. against nearest_ref ----
@pytest.mark.parametrize("which", ["bunny", "sphere_plane", "layered", "multi"])
def test_answers_equal_the_reference_bit_for_bit(request, which):
    c = request.getfixturevalue(which)
    want = c.want()
    present = {KINDS[o["type"]] for o in c.rs.objects if o["type"] != ray_ref.OBJ_MESH or o["tri_count"]}
    assert _kinds_that_win(c.rs, want["object"]) == present, (which, _kinds_that_win(c.rs, want["object"]), present)
    assert (want["object"] >= 0).all() and len(c.p) <= 4000
    if which == "multi":
        assert {"mesh", "triangle", "sphere", "plane"} <= present and sum(o["type"] == ray_ref.OBJ_MESH for o in c.rs.objects) >= 3
    for linear in (False, True):
        got = to_np(c.ds.nearest_points(c.p, linear=linear))
        assert got["distance"].shape == (len(c.p),) and got["point"].shape == (len(c.p), 3) and got["object"].dtype == np.int32
        _same(got, want, f"{which} linear={linear}")


# ---- 2. the default walk equals the linear walk ----
def _both_walks(ds, p, what, **kw):
    a = ds.nearest_points(p, skip_planes=True, **kw)
    same_tensors(a, ds.nearest_points(p, skip_planes=True, linear=True, **kw), what)
    return a


def test_default_walk_equals_linear_on_random_surface_and_far_points(bunny):
    c = bunny
    rng = np.random.RandomState(21)
    a = _both_walks(c.ds, rng.uniform(-3, 3, (4000, 3)).astype(f32), "random points")
    assert (a["object"] >= 0).all() and int((a["prim"] >= 0).sum()) > 1000
    # points ON the surface: cast_rays' hit points
    o, d = ray_ref.camera_rays(dict(c.rs.cam, w=64, h=48))
    hit = c.ds.cast_rays(o, d, outputs=("point", "object"))
    mesh = next(i for i, ob in enumerate(c.rs.objects) if ob["type"] == ray_ref.OBJ_MESH)
    on = hit["point"][hit["object"] == mesh]
    near = _both_walks(c.ds, on, "hit points")
    assert len(on) > 100 and bool((near["object"] == mesh).all()) and float(near["distance"].max()) < 1e-5
    # points 10^6 away: the whole mesh is one direction, candidates differ in the last bits
    far = (rng.normal(size=(1000, 3)) * 1e6).astype(f32)
    a = _both_walks(c.ds, far, "far points")
    assert (a["object"] >= 0).all() and float(a["distance"].min()) > 1e5


def test_default_walk_equals_linear_on_every_vertex_and_edge_midpoint(bunny):
    """the ties: several triangles at one d2, the lowest file index wins on both walks — and it is the reference's"""
    c = bunny
    mesh = next(o for o in c.rs.objects if o["type"] == ray_ref.OBJ_MESH)
    tr = c.rs.tris[mesh["tri_begin"]:mesh["tri_begin"] + mesh["tri_count"]]
    a, b, A = nearest_ref.records(tr)
    B, Cc = A - a, A - b                                   # the RECORDS' corners
    verts = np.concatenate([A, B, Cc])
    mids = np.concatenate([(A + B) * f32(0.5), (B + Cc) * f32(0.5), (Cc + A) * f32(0.5)])
    for what, p in (("vertices", verts), ("edge midpoints", mids)):
        p = p[:4000].astype(f32)
        got = to_np(_both_walks(c.ds, p, what))
        want = nearest_ref.nearest_points(c.rs, p, skip_planes=True)
        _same(got, want, what)
        if what == "vertices":
            # corner A of a record is a file vertex, exactly: its own triangle is at d2 = 0, so the answer is at 0 too and is never
            # a later triangle; and the bunny's vertices ARE shared, so these are ties between several triangles
            m = len(tr)
            assert (got["distance"][:m] == 0).all() and (got["prim"][:m] <= np.arange(m)).all()
            assert (got["prim"][:m] < np.arange(m)).sum() > m // 2


CASES = tuple((k, None) for k in SCALE_EXPONENTS) + OFFSET_CASES


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"k={c[0]},e={c[1]}")
def test_default_walk_equals_linear_across_scale_and_offset(ca, tmp_path, case):
    k, e = case
    s = util.parse(ca, render_range_scene_json(tmp_path, k, e, w=32, h=32))
    rs = ray_ref.RefScene(s)
    ds = ca.DeviceScene(s)
    rng = np.random.RandomState(31)
    base = np.concatenate([rng.uniform(-3, 3, (1500, 3)), rng.normal(0, 0.6, (1500, 3))]).astype(f32)
    verts = rs.tris.reshape(-1, 3)[rng.randint(0, 3 * len(rs.tris), 500)]
    p = np.concatenate([(base * pow2(k) + range_offset(k, e)).astype(f32), verts]).astype(f32)
    for skip in (True, False):
        a = ds.nearest_points(p, skip_planes=skip)
        same_tensors(a, ds.nearest_points(p, skip_planes=skip, linear=True), f"k={k} e={e} skip_planes={skip}")
    a = to_np(ds.nearest_points(p, skip_planes=True))
    assert _kinds_that_win(rs, a["object"]) == {"mesh", "triangle", "sphere"}
    some = slice(0, 3500, 10)
    _same({x: v[some] for x, v in a.items()}, nearest_ref.nearest_points(rs, p[some], skip_planes=True), f"k={k} e={e} against the reference")
    ds.close()


# ---- 3. one object, no planes, nothing ----
def test_object_and_skip_planes_restrict_the_candidates(multi, layered):
    c = multi
    by_kind = {}
    for i, o in enumerate(c.rs.objects):
        by_kind.setdefault(KINDS[o["type"]], i)
    assert set(by_kind) == {"mesh", "sphere", "plane", "triangle"}
    p = c.p[:600]
    for kind, i in by_kind.items():
        want = nearest_ref.nearest_points(c.rs, p, object=i)
        assert (want["object"] == i).all()
        for linear in (False, True):
            _same(to_np(c.ds.nearest_points(p, object=i, linear=linear)), want, f"object={i} ({kind}) linear={linear}")
    want = c.want(skip_planes=True)
    assert "plane" not in _kinds_that_win(c.rs, want["object"]) and "plane" in _kinds_that_win(c.rs, c.want()["object"])
    for linear in (False, True):
        _same(to_np(c.ds.nearest_points(c.p, skip_planes=True, linear=linear)), want, f"skip_planes linear={linear}")
    # an empty admitted set: a plane alone, with planes skipped
    for linear in (False, True):
        r = to_np(c.ds.nearest_points(p, object=by_kind["plane"], skip_planes=True, linear=linear))
        _miss(r, slice(None), "a plane alone with skip_planes")
    r = to_np(layered.ds.nearest_points(layered.p[:100], object=hits_ref.COINCIDENT_PLANE))
    assert (r["object"] == hits_ref.COINCIDENT_PLANE).all()   # the tie with object 4 is not in play: 4 is not admitted


# ---- 4. max_dist ----
@pytest.mark.parametrize("which", ["bunny", "multi"])
def test_max_dist_scalar_and_per_point(request, which):
    import torch
    c = request.getfixturevalue(which)
    full = c.want(skip_planes=True)
    md = f32(np.median(full["distance"]))
    within = full["distance"] <= md
    assert 0.3 * len(c.p) < within.sum() < 0.7 * len(c.p)
    want = nearest_ref.nearest_points(c.rs, c.p, max_dist=md, skip_planes=True)
    for linear in (False, True):
        got = to_np(c.ds.nearest_points(c.p, max_dist=float(md), skip_planes=True, linear=linear))
        _same(got, want, f"{which} max_dist linear={linear}")
        hit = got["object"] >= 0
        assert hit.sum() > 0.3 * len(c.p) and (~hit).sum() > 0.3 * len(c.p)
        _same(got, full, f"{which} within max_dist linear={linear}", rows=hit)
        _miss(got, ~hit, "beyond max_dist")
        assert (full["distance"][hit] <= md).all() and (full["distance"][~hit] >= md).all()
    # per point: the scalar's answer where the entry is the scalar, everything for +inf, a miss for NaN, 0 and a negative entry
    rng = np.random.RandomState(41)
    sel = rng.randint(0, 5, len(c.p))
    per = np.choose(sel, [md, f32(np.inf), f32(np.nan), f32(0.0), f32(-1.0)]).astype(f32)
    want = nearest_ref.nearest_points(c.rs, c.p, max_dist=per, skip_planes=True)
    for linear in (False, True):
        got = to_np(c.ds.nearest_points(c.p, max_dist=torch.from_numpy(per), skip_planes=True, linear=linear))
        _same(got, want, f"{which} per-point max_dist linear={linear}")
        _same(got, full, "+inf entries", rows=sel == 1)
        _miss(got, sel == 2, "NaN entries")
        _miss(got, sel == 4, "negative entries")
        _miss(got, (sel == 3) & (full["distance"] > 0), "zero entries off the surface")


# ---- 5. points that must not disturb others; sizes ----
def test_non_finite_points_among_ordinary_ones_and_batch_sizes(bunny):
    import torch
    c = bunny
    p = c.p[:700].copy()
    odd = np.arange(5, 700, 37)
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(odd):
        p[i, j % 3] = vals[(j // 3) % 3]
    p[odd[0]] = np.nan
    p[odd[1]] = [np.inf, -np.inf, np.nan]
    rest = np.setdiff1d(np.arange(700), odd)
    base = {k: v[:700] for k, v in c.want().items()}
    for linear in (False, True):
        for skip in (False, True):
            got = to_np(c.ds.nearest_points(p, linear=linear, skip_planes=skip))
            _miss(got, odd, f"non-finite points linear={linear}")
            want = base if not skip else {k: v[:700] for k, v in c.want(skip_planes=True).items()}
            _same(got, want, f"neighbours linear={linear} skip_planes={skip}", rows=rest)
    full = c.ds.nearest_points(c.p[:700])
    for m in (0, 1, 63, 64, 65, 127, 128, 129):
        part = c.ds.nearest_points(c.p[:m])
        assert part["distance"].shape == (m,) and part["point"].shape == (m, 3) and part["normal"].shape == (m, 3)
        same_tensors(part, {k: v[:m] for k, v in full.items()}, f"{m} points")
    empty = c.ds.nearest_points(np.zeros((0, 3), f32), linear=True, outputs=("object", "point"))
    assert list(empty) == ["object", "point"] and empty["object"].shape == (0,) and empty["point"].shape == (0, 3)
    for names in [(k,) for k in OUT] + [("normal", "prim")]:
        sub = c.ds.nearest_points(c.p[:700], outputs=names)
        assert list(sub) == list(names)
        same_tensors(sub, {k: full[k] for k in names}, str(names))
    # a tensor already on the device is used in place and left alone
    t = torch.from_numpy(c.p[:700]).cuda()
    keep = t.clone()
    same_tensors(c.ds.nearest_points(t), full, "device tensor")
    assert torch.equal(t, keep)


# ---- 6. live handles ----
def _equals_fresh(upd, fresh, p, what):
    for linear in (False, True):
        for skip in (False, True):
            got = upd.nearest_points(p, linear=linear, skip_planes=skip)
            same_tensors(got, fresh.nearest_points(p, linear=linear, skip_planes=skip), f"{what} linear={linear} skip_planes={skip}")
    return to_np(got)


def test_the_query_follows_every_edit_of_the_handle(ca, tmp_path):
    sc = hits_ref.layered_description(tmp_path)
    rng = np.random.RandomState(51)
    base = np.asarray(ca.scenes.read_stl(util.os.path.join(util.ROOT, "scene", "bunny.stl")), f32)
    sc["objects"][0] = mesh_object(tmp_path, "live", base[:400], 0)
    upd, hs = fresh_handle(ca, sc)
    p = rng.uniform(-2.5, 2.5, (2000, 3)).astype(f32)
    before = to_np(upd.nearest_points(p, skip_planes=True))

    def described(tris):
        return dict(sc, objects=[mesh_object(tmp_path, f"live_{described.n}", tris, 0)] + sc["objects"][1:])
    described.n = 0

    def check(tris, what):
        described.n += 1
        fresh, fhs = fresh_handle(ca, described(tris))
        got = _equals_fresh(upd, fresh, p, what)
        _same({k: v[::8] for k, v in got.items()}, nearest_ref.nearest_points(ray_ref.RefScene(fhs), p[::8], skip_planes=True), f"{what}: reference")
        fresh.close()
        return got

    turned = moved(base[:400], 0.7, 0.0)
    upd.update_mesh(0, turned)
    after = check(turned, "update_mesh (a rotation)")
    assert not np.array_equal(after["distance"], before["distance"])
    for builder in ("device", "host"):
        turned = moved(base[:400], -0.4 if builder == "host" else 1.3, 0.01, seed=3)
        upd.rebuild_mesh(0, turned, builder=builder)
        check(turned, f"rebuild_mesh builder={builder}")
    other = base[400:1000]
    upd.replace_mesh(0, other, builder="host")
    got = check(other, "replace_mesh to 600 triangles")
    assert int(got["prim"].max()) >= 400
    upd.close()


def test_the_query_follows_an_added_mesh_and_a_removed_object(ca, tmp_path):
    sc = hits_ref.layered_description(tmp_path)
    tris = np.asarray([[[-2, -1, z], [2, -1, z + 0.3], [0, 2, z]] for z in (-1.5, -0.8, 0.7, 1.6)], f32)
    upd = ca.DeviceScene(util.parse(ca, sc))
    p = np.random.RandomState(52).uniform(-3, 3, (2000, 3)).astype(f32)
    upd.add_mesh(tris, material=1, builder="host")
    upd.remove_object(0)
    fresh, hs = fresh_handle(ca, without(appended(sc, mesh_object(tmp_path, "added", tris, 1)), 0))
    got = _equals_fresh(upd, fresh, p, "add_mesh and remove_object")
    assert (got["object"] == 6).any()   # the new mesh is object 6 now
    _same({k: v[::4] for k, v in got.items()}, nearest_ref.nearest_points(ray_ref.RefScene(hs), p[::4], skip_planes=True), "edited handle against the reference")
    upd.close()
    fresh.close()


def test_a_mesh_the_ray_walk_takes_linearly_answers_as_its_linear_query(ca, tmp_path):
    """65 triangles in the eye's plane: more than the guard has records for, so the ray walk takes the mesh linearly and its nodes
    on the device carry unbounded boxes.  The nearest-point walk starts at node 0 all the same and finds every triangle once."""
    a = guard_tris(65, n_other=5, seed=8, zero_area=False)
    b = guard_tris(3, n_other=40, seed=6, zero_area=False) + f32([2.5, 0.0, 0.0])
    hs = util.parse(ca, guard_scene(tmp_path, "nearest_linear", [a, b], OFF, eye=[0.3, 3.0, 0.5], w=32, h=32))
    ds = ca.DeviceScene(hs)
    assert ds.guard_state(0)[1] is True and ds.guard_state(1) == ([0, 1, 2], False), (ds.guard_state(0), ds.guard_state(1))
    p = np.random.RandomState(53).uniform(-3, 5, (3000, 3)).astype(f32)
    for skip in (True, False):
        got = ds.nearest_points(p, skip_planes=skip)
        same_tensors(got, ds.nearest_points(p, skip_planes=skip, linear=True), f"linear mesh, guarded mesh, skip_planes={skip}")
    got = to_np(got)
    _same({k: v[::4] for k, v in got.items()}, nearest_ref.nearest_points(ray_ref.RefScene(hs), p[::4]), "against the reference")
    assert {0, 1} <= set(np.unique(got["object"]))
    ds.close()


# ---- 7. refusals that need a scene ----
def test_bad_arguments(ca, multi):
    import torch
    from cutrace_amd import _lib
    L = _lib.hip_lib()
    ds = multi.ds
    n = 100
    pts = torch.zeros(n, 3, device="cuda")
    dist = torch.empty(n, device="cuda")
    host = np.zeros((n, 3), f32)
    n_obj = len(multi.rs.objects)

    def q(**kw):
        x = _lib.NearestQuery()
        x.n_points, x.object, x.max_dist = n, -1, float("inf")
        x.d_point, x.d_distance = pts.data_ptr(), dist.data_ptr()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = functools.partial(util.bad, L.ctr_nearest_points, ds._h)
    assert L.ctr_nearest_points(ds._h, C.byref(q()), None) == 0
    assert L.ctr_nearest_points(ds._h, C.byref(q(object=n_obj - 1)), None) == 0
    bad(q(object=n_obj), f"object {n_obj} outside [-1, {n_obj})")
    bad(q(object=-2), f"object -2 outside [-1, {n_obj})")
    bad(q(d_point=None), "null d_point")
    bad(q(n_points=1 << 31), "n_points must be below 2^31")
    bad(q(flags=4), "unknown flag bits 4")
    bad(q(d_distance=None), "no output")
    bad(q(max_dist=-1.0), "max_dist must not be negative or NaN")
    bad(q(d_nearest=host.ctypes.data), "d_nearest is not device memory")
    bad(q(d_normal=host.ctypes.data), "d_normal is not device memory")
    bad(q(d_point=host.ctypes.data), "d_point is not device memory")
    bad(q(d_max_dist=host.ctypes.data), "d_max_dist is not device memory")
    assert L.ctr_nearest_points(ds._h, C.byref(q(n_points=0, d_point=None)), None) == 0
    bad(q(n_points=0, object=n_obj), "outside [-1")       # the object is checked before an empty batch returns
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ds.nearest_points(pts.double())
    with pytest.raises(ValueError):
        ds.nearest_points(pts, max_dist=torch.ones(7, device="cuda"))
    with pytest.raises(RuntimeError, match="outside"):
        ds.nearest_points(pts, object=n_obj)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ds.nearest_points(pts.to("cuda:1"))
        other = torch.empty(n, device="cuda:1")
        bad(q(d_distance=other.data_ptr()), "d_distance is not device memory")


# ---- 8. the handle is undisturbed ----
def test_renders_before_and_after_nearest_point_queries_are_identical(ca):
    s = load_scene(ca, "bunny", 64, 36)
    ds = ca.DeviceScene(s)
    a = ds.render(bounces=3)
    ca_ = ds.last_counters()
    p = np.random.RandomState(61).uniform(-3, 3, (4000, 3)).astype(f32)
    ds.nearest_points(p)
    ds.nearest_points(p, linear=True, outputs=("distance",))
    b = ds.render(bounces=3)
    cb = ds.last_counters()
    for k in ("depth", "color", "normal"):
        assert np.array_equal(f32_bits(a[k]), f32_bits(b[k])), k
    assert a["ray_count"] == b["ray_count"] and np.array_equal(ca_[:2], cb[:2])
    ds.close()
