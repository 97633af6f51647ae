"""The definition of the inside queries (include/cutrace_inside.h) on the CPU: tests/cross_ref.py, its NumPy restatement, against the
float64 winding number on the shipped closed meshes, on scene/frame.stl (every triangle twice: every count even), and on closed
forms; the bindings' table and layout; and scripts/query_check.cpp, the host half of the two entry points.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import cutrace_amd
from cutrace_amd import _lib, build, scenes
from tests import cross_ref
from tests.checkers import ROOT, declared
from tests.ray_ref import OBJ_MESH, OBJ_PLANE, OBJ_SPHERE, OBJ_TRIANGLE

f32 = np.float32
CSRC = os.path.join(ROOT, "cutrace_amd", "csrc")
NAMES = {"ctr_count_crossings", "ctr_inside_points", "ctr_inside_default_dirs"}
TABLE = f32([[0.3713907, 0.5570860, 0.7427814], [-0.6396021, 0.7462025, -0.1842720], [0.8017837, -0.2672612, -0.5345225]])


def soup(tris):
    """one mesh of `tris` as cross_ref takes a scene"""
    tris = np.asarray(tris, f32)
    return types.SimpleNamespace(objects=[dict(type=OBJ_MESH, tri_begin=0, tri_count=len(tris))], tris=tris)


def stl(name):
    return np.asarray(scenes.read_stl(os.path.join(ROOT, "scene", name + ".stl")), f32)


# ---- the bindings ----
def test_the_header_the_table_and_the_library_name_the_same_symbols():
    assert set(declared("cutrace_inside.h")) == set(_lib.INSIDE_SYMBOLS) == NAMES
    assert not any(NAMES & set(t) for t in _lib.HIP_PROTOS.values())
    assert not any(NAMES & set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_inside.h")
    L = _lib.hip_lib()
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_inside.h"].items():
        fn = getattr(L, n)
        assert (list(fn.argtypes), fn.restype) == (proto[0], proto[1]), n
    assert L.ctr_abi_version() == 3
    assert np.array_equal(cutrace_amd.inside_default_dirs(), TABLE)          # the header's literals, bit for bit
    assert (TABLE != 0).all()
    unit = TABLE / np.linalg.norm(TABLE, axis=1, keepdims=True)
    assert np.abs(unit @ unit.T - np.eye(3)).max() < 0.9                     # no two parallel or opposite


def test_query_records_have_the_headers_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler here")
    for struct, rec in (("ctr_crossing_query", _lib.CrossingQuery), ("ctr_inside_query", _lib.InsideQuery)):
        fields = [f for f, _ in rec._fields_]
        src = tmp_path / f"{struct}.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_inside.h"\nint main(void) {\n'
                       f'  printf("%zu\\n", sizeof({struct}));\n' +
                       "".join(f'  printf("%zu\\n", offsetof({struct}, {f}));\n' for f in fields) + "  return 0;\n}\n")
        exe = tmp_path / struct
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
        got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
        assert got[0] == C.sizeof(rec), struct
        assert got[1:] == [getattr(rec, f).offset for f in fields], struct
    assert (cutrace_amd.CROSS_LINEAR, cutrace_amd.CROSS_SKIP_PLANES, cutrace_amd.CROSS_SKIP_TRIANGLES) == (1, 2, 4)
    assert (cutrace_amd.INSIDE_LINEAR, cutrace_amd.INSIDE_MAX_DIRS) == (1, 15)


# ---- 1. against the winding number ----
def _check_against_winding(tris, points, what):
    """signed == winding and parity == (winding != 0), for each default direction alone and for the vote; NO point is left out"""
    w = cross_ref.winding_number(tris, points)
    got = cross_ref.inside(soup(tris), points, TABLE)
    for r in range(3):
        bad = np.flatnonzero(got["signed"][r] != w)
        assert not len(bad), f"{what}: direction {r}: signed differs from the winding number at {len(bad)} points, first {bad[:5]}"
        bad = np.flatnonzero((got["count"][r] & 1).astype(bool) != (w != 0))
        assert not len(bad), f"{what}: direction {r}: parity differs from containment at {len(bad)} points, first {bad[:5]}"
    assert np.array_equal(got["inside"], w != 0), what
    assert set(np.unique(got["votes"])) <= {0, 3}, what
    return w


@pytest.mark.parametrize("name", ["bunny", "skull", "mirror"])
def test_counts_equal_the_winding_number_on_uniform_points(name):
    tris = stl(name)
    w = _check_against_winding(tris, cross_ref.box_points(tris, 4099, 7), name)
    assert set(np.unique(w)) == {0, 1} and 20 < int(w.sum()) < 4000, (name, np.unique(w, return_counts=True))


def test_counts_equal_the_winding_number_beside_every_face_of_the_bunny():
    tris = stl("bunny")
    p = cross_ref.centroid_points(tris)
    w = _check_against_winding(tris, p, "bunny centroids")
    # outward normals: the smallest push along the normal is outside, against it inside (a larger one may cross a thin part)
    m = len(tris)
    for j, e in enumerate(cross_ref.OFFSETS):
        if abs(e) == 1e-5:
            assert (w[j * m:(j + 1) * m] == (0 if e > 0 else 1)).all(), e


# ---- 2. frame.stl: every triangle twice ----
def test_every_count_on_the_frame_is_even_and_nothing_is_inside_it():
    tris = stl("frame")
    rows = {}
    for t in tris:
        k = tuple(sorted(map(tuple, t.tolist())))
        rows[k] = rows.get(k, 0) + 1
    assert all(v % 2 == 0 for v in rows.values()), "frame.stl no longer holds every triangle twice"
    p = cross_ref.box_points(tris, 1024, 7)
    got = cross_ref.inside(soup(tris), p, TABLE)
    assert (got["count"] % 2 == 0).all() and int(got["count"].max()) >= 2
    assert not got["inside"].any() and not got["votes"].any()


# ---- 3. closed forms ----
SPHERE = dict(type=OBJ_SPHERE, v0=f32([0, 0, 0]), f0=f32(1.0))
PLANE = dict(type=OBJ_PLANE, v0=f32([0, 0, 5]), v1=f32([0, 0, -1]))
SHEETS = [dict(type=OBJ_TRIANGLE, v0=f32([-4, -4, z]), v1=f32([4, -4, z]), v2=f32([0, 6, z])) for z in (1.0, 2.0, 3.0, 4.0)]


def _count(objects, o, d, **kw):
    sc = types.SimpleNamespace(objects=objects, tris=np.zeros((0, 3, 3), f32))
    r = cross_ref.count_crossings(sc, f32([o]), f32([d]), **kw)
    return int(r["count"][0]), int(r["signed"][0])


def test_a_sphere_from_inside_outside_beside_and_tangent():
    assert _count([SPHERE], [0, 0, 0], [0, 0, 2]) == (1, 1)              # from inside: the way out
    assert _count([SPHERE], [0, 0, -3], [0, 0, 0.5]) == (2, 0)           # from outside: in and out
    assert _count([SPHERE], [0, 0, 3], [0, 0, 1]) == (0, 0)              # behind the origin
    assert _count([SPHERE], [2, 0, -3], [0, 0, 1]) == (0, 0)             # missed: the roots are NaN
    assert _count([SPHERE], [1, 0, -3], [0, 0, 1]) in ((0, 0), (2, 0))   # tangent: no root or a double root, never one
    assert _count([SPHERE], [0, 0, -3], [0, 0, 1], max_t=3.0) == (1, -1)  # t along d/|d|: the way in at 2, the way out at 4
    assert _count([SPHERE], [0, 0, -3], [0, 0, 4], max_t=3.0) == (1, -1)  # ... whatever the direction's length


def test_a_plane_and_a_chain_that_max_t_cuts_and_an_open_interval():
    assert _count([PLANE], [0, 0, 0], [0, 0, 1]) == (1, -1)              # d . n < 0
    assert _count([PLANE], [0, 0, 9], [0, 0, -1]) == (1, 1)              # d . n > 0
    assert _count([PLANE], [0, 0, 0], [1, 0, 0]) == (0, 0)               # parallel: t0 is not finite
    assert _count([PLANE], [0, 0, 0], [0, 0, -1]) == (0, 0)              # behind
    objs = SHEETS + [PLANE, SPHERE]
    o, d = [0.5, 0.25, -2], [0, 0, 1]                                    # sphere at t ~ 1.1 and 2.9, sheets at 3, 4, 5, 6, plane at 7
    assert _count(objs, o, d)[0] == 7
    assert _count(objs, o, d, skip_planes=True)[0] == 6
    assert _count(objs, o, d, skip_triangles=True)[0] == 3
    assert _count(objs, o, d, solids=True) == (2, 0)
    assert _count(objs, o, d, max_t=4.5)[0] == 4                         # the chain is cut: two roots, two sheets
    assert _count(objs, o, d, object=4) == (1, -1)
    # min_t EXACTLY on a crossing: excluded, the interval is open — and so is max_t
    assert _count(SHEETS, o, d, min_t=3.0)[0] == 3
    assert _count(SHEETS, o, d, min_t=3.0, max_t=6.0)[0] == 2
    assert _count(SHEETS, o, d, min_t=np.nextafter(f32(3.0), f32(0)))[0] == 4
    s = _count(SHEETS[:1], o, d)[1]
    assert s in (1, -1) and _count(SHEETS[:1], [0.5, 0.25, 9], [0, 0, -1])[1] == -s   # the other side: the other sign


def test_rays_that_are_none_count_nothing():
    for o, d in (([np.nan, 0, 0], [0, 0, 1]), ([0, np.inf, 0], [0, 0, 1]), ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [0, np.nan, 1]),
                 ([0, 0, 0], [np.inf, 0, 1]), ([0, 0, 0], [-0.0, 0.0, -0.0])):
        assert _count([SPHERE, PLANE] + SHEETS, o, d, min_t=-np.inf) == (0, 0), (o, d)
    sc = types.SimpleNamespace(objects=[SPHERE], tris=np.zeros((0, 3, 3), f32))
    r = cross_ref.inside(sc, f32([[0, 0, 0], [np.nan, 0, 0], [0, 0, np.inf], [3, 0, 0]]), TABLE)
    assert r["inside"].tolist() == [True, False, False, False] and r["votes"].tolist() == [3, 0, 0, 0]


# ---- 4. the host half of the entry points ----
def test_query_check_builds_and_prints_ok(tmp_path):
    exe = str(tmp_path / "query_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-pthread", "-Wno-unused-function",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "scripts", "query_check.cpp"),
                           *(os.path.join(CSRC, f) for f in ("ctr_scene.cpp", "ctr_rays.cpp", "ray_query.hip", "ray_shade.hip", "ray_points.hip",
                                                             "ray_hits.hip", "ray_nearest.hip", "ray_cross.hip", "guard_scan.hip",
                                                             "scene_flatten.cpp", "guard.cpp", "bvh.cpp"))],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "query_check: ok", out.stdout[-2000:] + out.stderr[-4000:]
    assert "query_check:" not in out.stderr, out.stderr[-4000:]
    for text in ("ctr_count_crossings: no output", "ctr_inside_points: n_dirs 2 is not 0 or an odd number up to 15",
                 "ctr_inside_points: direction 14 is not finite or is all zero"):
        assert text in out.stderr, text
