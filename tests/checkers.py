"""What the CPU tests of the host code share: the entry points a header declares, ONE way to build and run a scripts/*_check.cpp
program — each at most once per session, whichever modules ask for it — and scripts/flatten_check.cpp's harness with the record
layouts of its dump.  pytest rewrites `assert` in test modules only, so every assert here says what it compared."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutrace_amd import _lib

ROOT = _lib.ROOT
CSRC = os.path.join(ROOT, "cutrace_amd", "csrc")
I_CSRC, I_INCLUDE = "-I" + CSRC, "-I" + os.path.join(ROOT, "include")
HOST_FLAGS = ("-O2", "-ffp-contract=off", "-pthread", I_CSRC, I_INCLUDE)   # the host library's own arithmetic: no contraction
FLATTEN_SOURCES = tuple(os.path.join(CSRC, f) for f in ("scene_flatten.cpp", "guard.cpp", "bvh.cpp"))
SCENE_HOST = os.path.join(ROOT, "cutrace_amd", "host", "scene_host.cpp")
CHOICE_SOURCES = (os.path.join(CSRC, "kernel_choice.cpp"),)


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", txt)))


_built = {}


def check_program(tmp_path_factory, name, flags, sources=()):
    """The path of scripts/<name>.cpp compiled by g++ -std=c++17 with exactly `flags` and the further `sources`; the first call of a
    session builds it, every later one gets the same program.  Skips where there is no g++."""
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    key = (name, tuple(flags), tuple(sources))
    if key not in _built:
        exe = str(tmp_path_factory.mktemp(name) / name)
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(ROOT, "scripts", name + ".cpp"), *sources])
        _built[key] = exe
    return _built[key]


def check_output(exe, args=(), timeout=600, **kw):
    """what the program prints; it must end with status 0 inside `timeout` seconds"""
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, **kw)
    assert out.returncode == 0, f"{os.path.basename(exe)} ended with status {out.returncode}: " + out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def check_report(tmp_path_factory, name, args=(), **kw):
    """the lines of a program that flattens scenes through the host library's own sources and ends with "all checks hold" """
    exe = check_program(tmp_path_factory, name, HOST_FLAGS, FLATTEN_SOURCES + (SCENE_HOST,))
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, **kw)
    assert out.returncode == 0 and "all checks hold" in out.stdout, f"{name} ended with status {out.returncode}: " + out.stdout[-4000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


# ---------------------------------------------------------------- scripts/flatten_check.cpp

DOBJ = np.dtype([("type", "u4"), ("mat", "u4"), ("tri_begin", "u4"), ("tri_count", "u4"), ("node_begin", "u4"), ("node_count", "u4"),
                 ("bvh_root", "u4"), ("index", "u4"), ("f", "f4", 8)])
DTRI = np.dtype([("ab", "f4", (3, 2)), ("p", "f4", 3), ("orig", "u4"), ("n", "f4", 3), ("ke", "f4"), ("ke2", "f4"), ("pad1", "f4")])
DNODE4 = np.dtype([("lo", "f4", (3, 4)), ("hi", "f4", (3, 4)), ("child", "u4", 4), ("axis", "u4"), ("pad", "u4", 3)])
DPLANE = np.dtype([("p", "f4", (3, 2)), ("n", "f4", (3, 2)), ("index", "u4", 2), ("transparent", "u4", 2)])
DMAT = np.dtype([("color", "f4", 3), ("specular", "f4"), ("reflexivity", "f4"), ("phong_exp", "f4"), ("transparency", "f4"), ("pad", "f4")])
ARRAYS = {"objs": DOBJ, "oloop": DOBJ, "meshes": DOBJ, "planes": DPLANE, "tris": DTRI, "nodes4": DNODE4, "gn": np.dtype("f4"), "mats": DMAT}
SCALARS = ["n_mesh", "tlas_root", "tlas_begin", "n_axis_recs", "has_mesh", "all_opaque", "need_cold", "any_bounce", "mesh_tris",
           "mesh_bytes", "ray_slots", "merged_reserved", "merged_tri_begin", "merged_tri_count", "merged_node_begin", "merged_node_cap", "fast_pow_ok"]
GUARD = ["node_begin", "node_count", "tri_begin", "tri_count", "obj_index", "mesh_pos"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return check_program(tmp_path_factory, "flatten_check", HOST_FLAGS, FLATTEN_SOURCES)


def _typed(name, raw):
    if name in ARRAYS:
        return np.frombuffer(raw, ARRAYS[name])
    if name in ("scalars", "plan"):
        return np.frombuffer(raw, "u8")
    if name in ("dirty", "merged_built"):
        return np.frombuffer(raw, "u8").reshape(-1, 4)
    if name in ("guards", "guarded", "linear", "merged", "merged_guarded"):
        return np.frombuffer(raw, "u4")
    return raw


def write_scene(path, scene, camera_sets=()):
    """scripts/flatten_check.cpp's scene file of a HostScene, followed by the camera arrays of `camera_sets`"""
    d = scene.desc.contents
    with open(path, "wb") as f:
        f.write(np.array([d.n_objects, d.n_triangles, d.n_lights, d.n_materials, len(camera_sets)], "u8").tobytes())
        for ptr, n, T in ((d.objects, d.n_objects, _lib.Object), (d.triangles, d.n_triangles, _lib.Triangle),
                          (d.lights, d.n_lights, _lib.Light), (d.materials, d.n_materials, _lib.Material)):
            f.write(C.string_at(ptr, n * C.sizeof(T)) if n else b"")
        f.write(bytes(d.cam))
        for arr in camera_sets:
            f.write(np.array([len(arr)], "u8").tobytes() + bytes(arr))


def run(harness, tmp_path, scene, eyes=None, merge=False):
    """Flattens `scene` (a HostScene) and runs the guard once per camera set of `eyes` (a list of lists of eye positions;
    default: the scene's own camera).  Returns (flat, stages): the sections after flatten_scene as a dict, and per
    plan + apply a dict with its plan, dirty ranges, per-mesh guarded / linear lists and the arrays afterwards."""
    d = scene.desc.contents
    sets = []
    for eye_list in ([None] if eyes is None else eyes):
        arr = (_lib.Camera * len(eye_list or [0]))()
        for k in range(len(arr)):
            C.memmove(C.byref(arr[k]), C.byref(d.cam), C.sizeof(_lib.Camera))
            if eye_list:
                arr[k].pos = _lib.Vec3(*eye_list[k])
        sets.append(arr)
    path = str(tmp_path / "scene.bin")
    write_scene(path, scene, sets)
    dump = str(tmp_path / "scene.dump")
    out = check_output(harness, [path, dump] + (["merge"] if merge else []))
    assert out.strip() == "ok", f"flatten_check printed {out[-2000:]!r}"
    raw = open(dump, "rb").read()
    stages, i = [dict(what="flat", guarded=[], linear=[])], 0
    while i < len(raw):
        j = raw.index(b"\n", i)
        name, n = raw[i:j].split()
        name, n = name.decode(), int(n)
        if name in ("refresh", "again"):
            stages.append(dict(what=name, guarded=[], linear=[]))
        elif name in ("guarded", "linear"):
            stages[-1][name].append(_typed(name, raw[j + 1:j + 1 + n]))
        else:
            stages[-1][name] = _typed(name, raw[j + 1:j + 1 + n])
        i = j + 1 + n + 1
    flat = stages[0]
    flat["scalars"] = dict(zip(SCALARS, (int(x) for x in flat["scalars"])))
    flat["guards"] = [dict(zip(GUARD, (int(x) for x in g))) for g in flat["guards"].reshape(-1, 6)]
    return flat, stages[1:]
