"""The entry points of a live object count (include/cutrace_topology.h) and their Python methods as far as they need no device: the
header, the prototype table, the struct sizes, the NULL checks of the library, and the TypeError / ValueError paths of add_object,
add_mesh and remove_object."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cutrace_amd
from cutrace_amd import _lib
from tests.checkers import ROOT, declared

NAMES = {"ctr_scene_add_object", "ctr_scene_add_mesh", "ctr_scene_remove_object", "ctr_scene_room"}


def test_topology_entry_points_are_declared_and_check_their_arguments_without_a_device():
    names = declared("cutrace_topology.h")
    assert set(names) == set(_lib.TOPOLOGY_SYMBOLS) == NAMES
    others = [_lib.HOST_SYMBOLS, _lib.HIP_SYMBOLS, _lib.RAY_SYMBOLS, _lib.AA_SYMBOLS, _lib.LENS_SYMBOLS, _lib.IMAGES_SYMBOLS, _lib.UPDATE_SYMBOLS,
              _lib.EDIT_SYMBOLS, _lib.OBJECT_SYMBOLS, _lib.REBUILD_SYMBOLS, _lib.REPLACE_SYMBOLS]
    assert not any(NAMES & set(symbols) for symbols in others)
    assert not any(NAMES & set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_topology.h")
    assert not any(NAMES & set(t) for t in _lib.HIP_PROTOS.values())
    assert set(declared("cutrace_replace.h")) == {"ctr_scene_replace_mesh"}                       # the neighbours' lists are as they were
    assert set(declared("cutrace_objects.h")) == {"ctr_scene_set_objects", "ctr_scene_object_count", "ctr_scene_get_object"}
    L = _lib.hip_lib()
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_topology.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert L.ctr_abi_version() == 3
    assert C.sizeof(_lib.AddInfo) == 32 and C.sizeof(_lib.SceneRoom) == 32
    assert re.search(r"#define\s+CTR_ADD_HOST\s+1u", open(os.path.join(ROOT, "include", "cutrace_topology.h")).read()) and _lib.ADD_HOST == 1
    one, index, tri, info, room = _lib.Object(), C.c_uint64(), (_lib.Triangle * 1)(), _lib.AddInfo(), _lib.SceneRoom()
    fake = C.c_void_p(8)                                                   # never dereferenced: the other argument is NULL
    assert L.ctr_scene_add_object(None, C.byref(one), C.byref(index)) == 1 and b"ctr_scene_add_object: null argument" in L.ctr_last_error()
    assert L.ctr_scene_add_object(fake, None, None) == 1 and b"ctr_scene_add_object: null argument" in L.ctr_last_error()
    assert L.ctr_scene_add_mesh(None, 0, C.cast(tri, C.c_void_p), 1, 0, C.byref(info), None) == 1 and b"ctr_scene_add_mesh: null argument" in L.ctr_last_error()
    assert L.ctr_scene_add_mesh(fake, 0, None, 1, 0, None, None) == 1 and b"ctr_scene_add_mesh: null argument" in L.ctr_last_error()
    for flags in (2, 3, 0x80000000):
        assert L.ctr_scene_add_mesh(None, 0, C.cast(tri, C.c_void_p), 1, flags, None, None) == 1 and b"unknown flag bits" in L.ctr_last_error()
    assert L.ctr_scene_remove_object(None, 0) == 1 and b"ctr_scene_remove_object: null argument" in L.ctr_last_error()
    assert L.ctr_scene_room(None, C.byref(room)) == 1 and b"ctr_scene_room: null argument" in L.ctr_last_error()
    assert L.ctr_scene_room(fake, None) == 1 and b"ctr_scene_room: null argument" in L.ctr_last_error()


class _NoHandle(cutrace_amd.DeviceScene):
    """a scene of three objects that reaches no library: whatever gets past the methods' own checks fails on the missing handle"""
    def __init__(self):
        self._h = None

    def object_count(self):
        return 3

    def _torch_device(self):
        raise AssertionError("the arguments were not checked before the device was asked for")


def test_add_object_names_what_is_wrong_before_the_library_is_called():
    ds = _NoHandle()
    for kind in ("mesh", "cube", None, 3, b"sphere"):
        with pytest.raises(ValueError, match="kind"):
            ds.add_object(kind)
    for kind, field in (("sphere", "point"), ("sphere", "p1"), ("sphere", "v0"), ("plane", "center"), ("plane", "radius"), ("triangle", "normal"),
                        ("triangle", "radius"), ("plane", "mat_idx"), ("sphere", "type")):
        with pytest.raises(TypeError, match=rf"a {kind} has no field '{field}'"):
            ds.add_object(kind, **{field: (0.0, 0.0, 0.0)})
    with pytest.raises(TypeError):
        ds.add_object("sphere", center=1.0)                                # three floats
    for material in (-1, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="bad material index"):
            ds.add_object("sphere", material=material, center=(0, 0, 0), radius=1.0)
        with pytest.raises(ValueError, match="bad material index"):
            ds.add_mesh(np.zeros((1, 3, 3), np.float32), material=material)


def test_add_mesh_and_remove_object_check_their_arguments_first():
    ds = _NoHandle()
    with pytest.raises(ValueError, match="builder"):
        ds.add_mesh(np.zeros((1, 3, 3), np.float32), builder="sah")
    for idx in (-1, 3, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="bad object index"):
            ds.remove_object(idx)
    checked = cutrace_amd.DeviceScene._mesh_triangles
    for bad in (None, [[0.0] * 3] * 3, "triangles"):
        with pytest.raises(TypeError, match="triangles"):
            checked(bad, None)
    for bad in (np.zeros((2, 3, 3), np.float64), np.zeros((2, 9), np.float32), np.zeros((3, 3), np.float32)):
        with pytest.raises(ValueError, match="triangles"):
            checked(bad, None)
