"""The object edits' entry points (include/cutrace_objects.h) and Python methods as far as they need no device: the header, the
prototype table, the NULL checks of the library, and the TypeError / ValueError paths of set_objects / set_object."""
import ctypes as C

import numpy as np
import pytest

import cutrace_amd
from cutrace_amd import _lib

TRIANGLE, MESH, PLANE, SPHERE = 0, 1, 2, 3


def test_object_entry_points_are_declared_and_check_their_arguments_without_a_device():
    from tests.checkers import declared
    names = declared("cutrace_objects.h")
    assert set(names) == set(_lib.OBJECT_SYMBOLS) == {"ctr_scene_set_objects", "ctr_scene_object_count", "ctr_scene_get_object"}
    assert '#include "cutrace_objects.h"' in open(_lib.ROOT + "/include/cutrace_edit.h").read()   # cutrace_edit.h brings them along
    L = _lib.hip_lib()
    assert not set(names) & (set(_lib.HIP_SYMBOLS) | set(_lib.HOST_SYMBOLS) | set(_lib.UPDATE_SYMBOLS) | set(_lib.EDIT_SYMBOLS))
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_objects.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert not any(n in symbols for symbols in _lib.HIP_PROTOS.values() for n in names)
    assert L.ctr_abi_version() == 3
    objs, n, one = (_lib.Object * 1)(), C.c_uint64(), _lib.Object()
    assert L.ctr_scene_set_objects(None, objs, 1) == 1 and b"ctr_scene_set_objects: null argument" in L.ctr_last_error()
    assert L.ctr_scene_object_count(None, C.byref(n)) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_get_object(None, 0, C.byref(one)) == 1 and b"null argument" in L.ctr_last_error()


def _obj(type_, mat=0, **kw):
    o = _lib.Object()
    o.type, o.mat_idx = type_, mat
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class _NoHandle(cutrace_amd.DeviceScene):
    """set_object is get_object for every object, one record changed, then set_objects: with the three library calls replaced by
    a list, its own checks run without a handle or a device"""
    def __init__(self):
        self._h = None
        self.objects = [_obj(SPHERE, 1, v0=_lib.Vec3(0, 1, 2), f0=0.5), _obj(PLANE, 0, v0=_lib.Vec3(0, -1, 0), v1=_lib.Vec3(0, 1, 0)),
                        _obj(TRIANGLE, 0, v0=_lib.Vec3(0, 0, 0), v1=_lib.Vec3(1, 0, 0), v2=_lib.Vec3(0, 1, 0)), _obj(MESH, 1, tri_count=12)]
        self.calls = 0

    def object_count(self):
        return len(self.objects)

    def get_object(self, i):
        return cutrace_amd._records(_lib.Object, [self.objects[i]])[0]

    def set_objects(self, objects):
        arr = cutrace_amd._records(_lib.Object, objects, "objects")
        self.objects = [arr[k] for k in range(len(arr))]
        self.calls += 1


def test_set_objects_rejects_wrong_types_before_the_library_is_called():
    ds = cutrace_amd.DeviceScene.__new__(cutrace_amd.DeviceScene)
    ds._h = None
    for bad in (None, 5, "objects", b"objects", [1.0, 2.0], [_lib.Material()], [_lib.Object(), None], [_lib.Object(), (1, 2, 3)]):
        with pytest.raises(TypeError, match="objects"):
            ds.set_objects(bad)


def test_set_object_changes_one_record_and_names_what_is_wrong():
    ds = _NoHandle()
    ds.set_object(0, center=(1.0, 2.0, 3.0), radius=0.25)
    ds.set_object(1, point=[0.0, -2.0, 0.0], normal=(0.0, 1.0, 0.5), material=1)
    ds.set_object(2, p1=(1, 1, 1), p2=(2, 1, 1), p3=(1, 2, 1))
    ds.set_object(np.int64(3), material=0)
    ds.set_object(3)                                                             # no field: every record as it is
    assert ds.calls == 5
    s, p, t, m = ds.objects
    assert (s.type, s.v0.tup(), s.f0, s.mat_idx) == (SPHERE, (1.0, 2.0, 3.0), 0.25, 1)
    assert (p.type, p.v0.tup(), p.v1.tup(), p.mat_idx) == (PLANE, (0.0, -2.0, 0.0), (0.0, 1.0, 0.5), 1)
    assert (t.type, t.v0.tup(), t.v1.tup(), t.v2.tup(), t.mat_idx) == (TRIANGLE, (1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0), 0)
    assert (m.type, m.mat_idx, m.tri_count) == (MESH, 0, 12)
    for idx in (-1, 4, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="bad object index"):
            ds.set_object(idx, material=0)
    # a field the object's type does not have
    for idx, field in ((0, "point"), (0, "normal"), (0, "p1"), (1, "center"), (1, "radius"), (2, "radius"), (2, "point"), (3, "center"),
                       (3, "point"), (3, "p1"), (0, "v0"), (1, "mat_idx"), (2, "type"), (3, "tri_count")):
        with pytest.raises(TypeError, match=rf"has no field '{field}'"):
            ds.set_object(idx, **{field: (0.0, 0.0, 0.0)})
    assert ds.calls == 5, "a rejected set_object must not reach set_objects"
    with pytest.raises(TypeError):
        ds.set_object(0, center=1.0)                                             # three floats
    assert ds.calls == 5
