"""Nearest-point queries (include/cutrace_nearest.h, DeviceScene.nearest_points) as far as they need no device: the header, the
prototype table, the struct layout, the refusals in front of the scene, the Python argument checks, the host half of the
definition (scripts/nearest_check.cpp) — and the NumPy checker of the GPU tests (tests/nearest_ref.py) pinned twice: bit for bit
against the header compiled for the host, and against a float64 brute force of another algorithm."""
import contextlib
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cutrace_amd
from cutrace_amd import _lib
from tests import nearest_ref, ray_ref
from tests.checkers import HOST_FLAGS, ROOT, check_output, check_program, declared
from tests.conftest import load_scene

f32, f64 = np.float32, np.float64
NAMES = {"ctr_nearest_points"}
K_BAR = 8.0   # scripts/nearest_check.cpp NP_K_BAR: four times the largest k its part (a) sees


def test_nearest_entry_point_is_declared_exported_and_laid_out_as_the_header_says(tmp_path):
    assert set(declared("cutrace_nearest.h")) == set(_lib.NEAREST_SYMBOLS) == NAMES
    others = [_lib.HOST_SYMBOLS, _lib.HIP_SYMBOLS, _lib.RAY_SYMBOLS, _lib.AA_SYMBOLS, _lib.LENS_SYMBOLS, _lib.IMAGES_SYMBOLS, _lib.UPDATE_SYMBOLS,
              _lib.EDIT_SYMBOLS, _lib.OBJECT_SYMBOLS, _lib.REBUILD_SYMBOLS, _lib.REPLACE_SYMBOLS, _lib.TOPOLOGY_SYMBOLS, _lib.HITS_SYMBOLS]
    assert not any(NAMES & set(symbols) for symbols in others)
    assert not any(NAMES & set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_nearest.h")
    assert not any(NAMES & set(t) for t in _lib.HIP_PROTOS.values())
    assert set(declared("cutrace_hits.h")) == {"ctr_list_hits"}   # the neighbours' lists are as they were
    assert set(declared("cutrace_rays.h")) == {"ctr_cast_rays", "ctr_shade_rays", "ctr_shade_points"}
    L = _lib.hip_lib()
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_nearest.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert L.ctr_abi_version() == 3
    # sizeof / offsetof of ctr_nearest_query as the C compiler lays it out, against the ctypes mirror
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    fields = [f for f, _ in _lib.NearestQuery._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_nearest.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ctr_nearest_query));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(ctr_nearest_query, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.NearestQuery) == 80
    assert got[1:] == [getattr(_lib.NearestQuery, f).offset for f in fields]
    header = open(os.path.join(ROOT, "include", "cutrace_nearest.h")).read()
    for name, value in (("CTR_NEAREST_LINEAR", cutrace_amd.NEAREST_LINEAR), ("CTR_NEAREST_SKIP_PLANES", cutrace_amd.NEAREST_SKIP_PLANES)):
        assert re.search(rf"#define\s+{name}\s+{value}u\b", header), name
    assert cutrace_amd.NEAREST_OUTPUTS == ("distance", "object", "prim", "point", "normal") == nearest_ref.OUTPUTS


def _query(**kw):
    q = _lib.NearestQuery()
    q.n_points, q.object, q.max_dist = 4, -1, float("inf")
    q.d_distance = 0x1000   # (never dereferenced: every call here fails first)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_nearest_points_refuses_a_bad_query_before_it_looks_at_the_scene():
    L = _lib.hip_lib()

    def refused(q, text):
        assert L.ctr_nearest_points(None, C.byref(q) if q is not None else None, None) == 1, text
        assert L.ctr_last_error().decode() == "ctr_nearest_points: " + text

    refused(None, "null query")
    for flags in (4, 8, 0x80000000, 0xFFFFFFFC):
        refused(_query(flags=flags), f"unknown flag bits {flags}")
    refused(_query(flags=7), "unknown flag bits 4")
    refused(_query(d_distance=None), "no output: one of d_distance, d_object, d_prim, d_nearest and d_normal is required")
    for md in (-1.0, -0.0 - 1e-30, float("nan"), -float("inf")):
        refused(_query(max_dist=md), "max_dist must not be negative or NaN")
    refused(_query(flags=4, d_distance=None, max_dist=-1.0), "unknown flag bits 4")   # check_query's order: flags, then the entry point's rules
    refused(_query(d_distance=None, max_dist=-1.0), "no output: one of d_distance, d_object, d_prim, d_nearest and d_normal is required")
    # what is allowed gets as far as the scene: every flag, a zero limit, an infinite one, a per-point array in place of a bad scalar,
    # a single output of any kind, a count that the scene's checks would refuse
    refused(_query(), "null scene")
    refused(_query(flags=3, max_dist=0.0), "null scene")
    refused(_query(max_dist=-1.0, d_max_dist=0x2000), "null scene")
    for only in ("d_object", "d_prim", "d_nearest", "d_normal"):
        refused(_query(d_distance=None, **{only: 0x1000}), "null scene")
    refused(_query(n_points=1 << 31, d_point=None, object=-7), "null scene")


class _NoHandle(cutrace_amd.DeviceScene):
    """a scene that reaches no library: whatever gets past the method's own checks fails on the missing device"""
    def __init__(self, device=None):
        self._h = None
        self._dev = device

    def _torch_device(self):
        if self._dev is None:
            raise AssertionError("the arguments were not checked before the device was asked for")
        return self._dev


def test_nearest_points_names_what_is_wrong_before_the_library_is_called(monkeypatch):
    import torch
    ok = np.zeros((4, 3), f32)
    ds = _NoHandle()
    for outputs in (("t",), ("distance", "distance"), "point", (), ("uv",), (None,)):
        with pytest.raises(ValueError, match="outputs"):
            ds.nearest_points(ok, outputs=outputs)
    for obj in (1.0, "1", True, [1]):
        with pytest.raises(TypeError, match="object"):
            ds.nearest_points(ok, object=obj)
    with pytest.raises(ValueError, match="object"):
        ds.nearest_points(ok, object=-1)
    for md in (-1e-3, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            ds.nearest_points(ok, max_dist=md)

    # what is wrong with the arrays is said once the device is known, before anything is copied to it
    @contextlib.contextmanager
    def no_stream(dev, stream):
        yield None
    monkeypatch.setattr(cutrace_amd, "_on_stream", no_stream)
    ds = _NoHandle(torch.device("cpu"))
    with pytest.raises(ValueError, match="points: expected float32"):
        ds.nearest_points(ok.astype(f64))
    with pytest.raises(ValueError, match="points: expected float32"):
        ds.nearest_points(np.zeros((4, 2), f32))
    with pytest.raises(ValueError, match="points: expected float32"):
        ds.nearest_points(np.zeros(12, f32))
    with pytest.raises(TypeError, match="points"):
        ds.nearest_points([[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="max_dist: 3 values for 4"):
        ds.nearest_points(ok, max_dist=np.zeros(3, f32))
    with pytest.raises(ValueError, match="max_dist: expected float32"):
        ds.nearest_points(ok, max_dist=np.zeros(4, f64))
    with pytest.raises(TypeError, match="max_dist"):
        ds.nearest_points(ok, max_dist=[1.0] * 4)


# ---- the host half of the definition ----
@pytest.fixture(scope="module")
def nearest_check(tmp_path_factory):
    return check_program(tmp_path_factory, "nearest_check", HOST_FLAGS)


def test_candidates_hold_their_bar_and_the_cull_is_conservative(nearest_check):
    out = check_output(nearest_check)
    assert out.rstrip().endswith("all checks hold"), out
    a = re.search(r"a: cases (\d+) nan (\d+) k_max ([0-9.]+) bar ([0-9.]+)", out)
    assert a and int(a.group(1)) >= 1000000 and int(a.group(2)) == 0, out
    k_max, bar = float(a.group(3)), float(a.group(4))
    assert bar == K_BAR and k_max <= bar <= 4.0 * k_max + 0.1, out     # the bar is four times what the search sees, not more
    assert len(re.findall(r"a: .* k_max [0-9.]+\n", out)) == 6, out  # the six classes
    b = re.search(r"b: boxes (\d+) pairs (\d+) violations (\d+)\n", out)
    assert b and int(b.group(1)) > 100000 and int(b.group(2)) > 5000000 and int(b.group(3)) == 0, out
    c = re.search(r"c: boxes (\d+) pairs (\d+) violations (\d+) ", out)
    assert c and int(c.group(3)) > 0, out                              # the search can see a violation


def _random_records(rng, n):
    """triangle records and points at many scales: ordinary, thin, and points on the triangle's own features"""
    s = np.ldexp(1.0, rng.randint(-20, 21, n))[:, None]
    t = rng.uniform(-1, 1, (n, 3, 3)) * s[:, None]
    thin = rng.rand(n) < 0.3
    f = rng.uniform(-0.5, 1.5, (n, 1))
    t[thin, 2] = (t[:, 0] + f * (t[:, 1] - t[:, 0]) + rng.uniform(-1, 1, (n, 3)) * s * np.ldexp(1.0, -rng.randint(4, 21, n))[:, None])[thin]
    t = t.astype(f32)
    p = (rng.uniform(-2, 2, (n, 3)) * s).astype(f32)
    kind = rng.randint(0, 5, n)
    u = rng.rand(n, 1)
    p = np.where((kind == 1)[:, None], t[np.arange(n), rng.randint(0, 3, n)], p)
    p = np.where((kind == 2)[:, None], (t[:, 0].astype(f64) + u * (t[:, 1].astype(f64) - t[:, 0])).astype(f32), p)
    p = np.where((kind == 3)[:, None], (p.astype(f64) * np.ldexp(1.0, rng.randint(3, 20, n))[:, None]).astype(f32), p)
    return t, p.astype(f32)


def test_the_numpy_restatement_is_the_header_bit_for_bit(nearest_check, tmp_path):
    n = 60000
    t, p = _random_records(np.random.RandomState(7), n)
    t[:50, 2] = t[:50, 1]                     # zero edges and zero areas: NaNs must agree too
    t[50:100, 0] = t[50:100, 1] = t[50:100, 2]
    p[100:110] = np.nan
    p[110:120, 1] = np.inf
    a, b, A = nearest_ref.records(t)
    rows = np.concatenate([a, b, A, p], axis=1).astype(f32)
    rows.tofile(str(tmp_path / "in.bin"))
    check_output(nearest_check, ["eval", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    want = np.fromfile(str(tmp_path / "out.bin"), f32).reshape(n, 4)
    with np.errstate(all="ignore"):
        d2 = np.empty(n, f32)
        q = np.empty((n, 3), f32)
        for r0 in range(0, n, 500):   # one record against its own point: the diagonal, in chunks
            dd, qq = nearest_ref.triangle(a[r0:r0 + 500], b[r0:r0 + 500], A[r0:r0 + 500], p[r0:r0 + 500])
            i = np.arange(len(dd))
            d2[r0:r0 + 500], q[r0:r0 + 500] = dd[i, i], qq[i, i]
    got = np.concatenate([d2[:, None], q], axis=1)
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{int(diff.any(1).sum())} of {n} records differ, first {np.flatnonzero(diff.any(1))[:5]}"
    assert np.isnan(want[:, 0]).sum() >= 10 and (~np.isfinite(want[:, 0])).sum() >= 20 and np.isfinite(want[:, 0]).sum() > 0.95 * n


# ---- nearest_ref against an independent float64 brute force ----
def _seg(p, a, b):
    e = b - a
    ee = (e * e).sum(-1)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, ((p - a) * e).sum(-1) / ee, 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(p - (a + e * t[..., None]), axis=-1)


def _brute_triangles(p, A, B, Cc):
    """float64 distances (n, m) of points to triangles by ANOTHER algorithm: the foot on the plane where it lies inside all three
    edges, else the nearest of the three segments"""
    p = p[:, None, :]
    n = np.cross(B - A, Cc - A)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        h = ((p - A) * n).sum(-1) / nn
        foot = p - n * h[..., None]
        inside = ((np.cross(B - A, foot - A) * n).sum(-1) >= 0) & ((np.cross(Cc - B, foot - B) * n).sum(-1) >= 0) & \
                 ((np.cross(A - Cc, foot - Cc) * n).sum(-1) >= 0) & (nn > 0)
        plane = np.abs(((p - A) * n).sum(-1)) / np.sqrt(nn)
    edges = np.minimum(np.minimum(_seg(p, A, B), _seg(p, B, Cc)), _seg(p, Cc, A))
    return np.where(inside, plane, edges)


def _brute_scene(rs, p):
    """per candidate (every plane, sphere, stand-alone triangle and mesh triangle): float64 distance (n, c), the bar's scale
    (n, c) = distance + largest edge + |p - A|, and the candidate's (object, prim)"""
    p = p.astype(f64)
    dist, scale, who = [], [], []
    for i, o in enumerate(rs.objects):
        if o["type"] == ray_ref.OBJ_PLANE:
            n = o["v1"].astype(f64)
            d = np.abs((p - o["v0"].astype(f64)) @ (n / np.linalg.norm(n)))[:, None]
            ext = np.linalg.norm(p - o["v0"].astype(f64), axis=1)[:, None]
            ids = [(i, -1)]
        elif o["type"] == ray_ref.OBJ_SPHERE:
            ln = np.linalg.norm(p - o["v0"].astype(f64), axis=1)[:, None]
            d, ext, ids = np.abs(ln - abs(float(o["f0"]))), ln + abs(float(o["f0"])), [(i, -1)]
        else:
            tr = np.stack([o["v0"], o["v1"], o["v2"]])[None] if o["type"] == ray_ref.OBJ_TRIANGLE else \
                rs.tris[o["tri_begin"]:o["tri_begin"] + o["tri_count"]]
            a, b, A = (x.astype(f64) for x in nearest_ref.records(tr))   # the record's triangle, exactly: A, A - a, A - b
            B, Cc = A - a, A - b
            d = _brute_triangles(p, A, B, Cc)
            edge = np.maximum(np.maximum(np.linalg.norm(B - A, axis=1), np.linalg.norm(Cc - A, axis=1)), np.linalg.norm(Cc - B, axis=1))
            ext = edge[None] + np.linalg.norm(p[:, None] - A[None], axis=2)
            ids = [(i, k if o["type"] == ray_ref.OBJ_MESH else -1) for k in range(len(A))]
        dist.append(d)
        scale.append(d + ext)
        who += ids
    return np.concatenate(dist, 1), np.concatenate(scale, 1), np.array(who)


@pytest.mark.parametrize("name", ["bunny", "sphere_plane"])
def test_the_numpy_restatement_against_a_float64_brute_force(ca, name):
    rs = ray_ref.RefScene(load_scene(ca, name, 32, 32))
    rng = np.random.RandomState(11)
    p = rng.uniform(-3, 3, (240, 3)).astype(f32)
    if len(rs.tris):   # points on and next to the surface
        v = rs.tris.reshape(-1, 3)[rng.randint(0, 3 * len(rs.tris), 120)]
        p = np.concatenate([p, v[:40], v[40:] + rng.normal(0, 0.02, (80, 3)).astype(f32)]).astype(f32)
    for skip in (False, True):
        got = nearest_ref.nearest_points(rs, p, skip_planes=skip)
        dist, scale, who = _brute_scene(rs, p)
        if skip:
            keep = np.array([rs.objects[i]["type"] != ray_ref.OBJ_PLANE for i, _ in who])
            dist, scale, who = dist[:, keep], scale[:, keep], who[keep]
        order = np.argsort(dist, axis=1, kind="stable")
        rows = np.arange(len(p))
        best, second = order[:, 0], order[:, 1]
        bar = K_BAR * 2.0 ** -24 * scale[rows, best]
        err = np.abs(got["distance"].astype(f64) - dist[rows, best])
        assert (err <= bar).all(), f"{name} skip_planes={skip}: worst {np.max(err / bar) * K_BAR:.2f} x 2^-24 x scale"
        clear = dist[rows, second] - dist[rows, best] > 2.0 * bar
        # (far from a mesh the nearest point is as a rule a vertex or an edge that several triangles share at one distance: no gap)
        assert clear.sum() >= 40, int(clear.sum())
        assert np.array_equal(got["object"][clear], who[best, 0][clear]) and np.array_equal(got["prim"][clear], who[best, 1][clear])
        kinds = {rs.objects[i]["type"] for i in np.unique(got["object"])}
        assert kinds == {rs.objects[i]["type"] for i in range(len(rs.objects)) if not (skip and rs.objects[i]["type"] == ray_ref.OBJ_PLANE)}
        # the point is on the object it names, the normal is that object's, to the accuracy of float
        off = np.abs(np.linalg.norm(p.astype(f64) - got["point"], axis=1) - got["distance"])
        assert (off <= 4e-6 * (1.0 + got["distance"])).all()
        flat = np.array([rs.objects[i]["type"] == ray_ref.OBJ_PLANE for i in got["object"]])
        assert np.allclose(np.linalg.norm(got["normal"][~flat].astype(f64), axis=1), 1.0, atol=1e-5)
        assert all(np.array_equal(got["normal"][j], rs.objects[got["object"][j]]["v1"]) for j in np.flatnonzero(flat))


def test_limits_restrictions_and_odd_points_on_the_reference(ca):
    """the tie rules and the miss values, on the reference alone: what the GPU tests' conditions rest on"""
    rs = ray_ref.RefScene(load_scene(ca, "bunny", 32, 32))
    rng = np.random.RandomState(12)
    p = rng.uniform(-1.5, 1.5, (200, 3)).astype(f32)
    full = nearest_ref.nearest_points(rs, p, skip_planes=True)
    md = f32(np.median(full["distance"]))
    lim = nearest_ref.nearest_points(rs, p, max_dist=md, skip_planes=True)
    near = full["distance"] <= md
    assert 50 < near.sum() < 150
    for k in nearest_ref.OUTPUTS:
        assert np.array_equal(lim[k][near], full[k][near]), k
    assert np.isposinf(lim["distance"][~near]).all() and (lim["object"][~near] == -1).all() and (lim["prim"][~near] == -1).all()
    assert not lim["point"][~near].any() and not lim["normal"][~near].any()
    # every vertex of the mesh: distance 0, and the lowest file index among the triangles that share it
    mesh = next(o for o in rs.objects if o["type"] == ray_ref.OBJ_MESH)
    tr = rs.tris[mesh["tri_begin"]:mesh["tri_begin"] + mesh["tri_count"]]
    v = tr[:80].reshape(-1, 3)
    at = nearest_ref.nearest_points(rs, v, skip_planes=True)
    first = np.array([np.flatnonzero((tr == x).all(-1).any(-1))[0] for x in v])
    assert (at["distance"] == 0).all() and np.array_equal(at["prim"], first)
    odd = p[:8].copy()
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3] = np.nan, np.inf, -np.inf, np.nan
    r = nearest_ref.nearest_points(rs, odd, max_dist=np.array([np.inf] * 4 + [np.nan, -1.0, 0.0, np.inf], f32))
    assert (r["object"][:7] == -1).all() and np.isposinf(r["distance"][:7]).all() and r["object"][7] >= 0
