"""Host logic (CPU, no GPU) of the light and material edits (include/cutrace_edit.h): light_records / material_records of
scene_flatten.cpp with the guard behind them, and the shared plane scan of cutrace_amd/csrc/guard_scan.h against the loop
guard.cpp had before — run through scripts/scene_edit_check.cpp, which states what it checks.  Plus the argument checks of the
entry points and of the Python methods that need neither a handle nor a device."""
import ctypes as C
import re

import pytest

import cutrace_amd
from cutrace_amd import _lib
from tests.checkers import ROOT, check_report, declared

SCENES = ["scene/bunny.json", "scene/mirror.json", "scene/sphere_plane.json", "scene/triangle.json"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """the lines scripts/scene_edit_check.cpp prints, once for all tests"""
    return check_report(tmp_path_factory, "scene_edit_check", SCENES, cwd=ROOT)


def _edits(report):
    """scene -> step -> the flags and guard counts of the edited scene (which equalled the freshly flattened one, or the program failed)"""
    edits = {}
    for line in report:
        m = re.match(r"edit (.+?) \| (.+?) \| all_opaque (\d) need_cold (\d) any_bounce (\d) fast_pow_ok (\d) guarded (\d+) linear (\d+) merged_keys (\d+)$", line)
        if m:
            edits.setdefault(m.group(1), {})[m.group(2)] = dict(zip(("all_opaque", "need_cold", "any_bounce", "fast_pow_ok", "guarded", "linear", "merged_keys"),
                                                                    (int(x) for x in m.groups()[2:])))
    return edits


def test_every_scene_went_through_the_row_of_edits(report):
    edits = _edits(report)
    names = SCENES + ["guard scene, 3 in the plane", "guard scene, 70 in the plane"]
    for name in names:
        for scene in (name, name + " (merged)"):
            assert scene in edits, scene
            assert {"nothing changed", "no light", "33 lights", "material 0 transmits", "one material more", "the first lights again, at the end"} <= set(edits[scene])


def test_the_edits_flip_every_flag_both_ways(report):
    """the flags are derived from the defaults at every edit: set AND cleared"""
    for scene, steps in _edits(report).items():
        flags = lambda what: tuple(steps[what][k] for k in ("all_opaque", "need_cold", "any_bounce", "fast_pow_ok"))
        assert flags("all opaque, none reflects") == (1, 0, 0, 1), scene
        assert flags("material 0 transmits") == (0, 0, 1, 1), scene
        assert flags("material 0 transmits and reflects") == (0, 1, 1, 1), scene
        assert flags("material 0 reflects") == (1, 0, 1, 1), scene
        assert flags("material 0 reflects 5e-7") == (1, 0, 0, 1), scene            # below the 1e-6 of the reference's comparison
        assert flags("material 0 transmits 1e-7") == (0, 0, 0, 1), scene           # not exactly opaque, yet no bounce
        assert flags("all opaque, none reflects again") == (1, 0, 0, 1), scene
        assert flags("phong exponent 5000")[3] == 0 and flags("phong exponent 40")[3] == 1, scene
        assert flags("light colour -300")[3] == 0 and flags("light colour 1")[3] == 1, scene
        assert flags("one material more") == (0, 1, 1, 1) and flags("one material fewer") == (1, 0, 0, 1), scene


def test_the_guard_follows_lights_and_mirrors(report):
    edits = _edits(report)
    few, many = edits["guard scene, 3 in the plane"], edits["guard scene, 70 in the plane"]
    # two meshes: k and 2 triangles in z = 0.5.  A light in the plane, a sun parallel to it, or the floor turned into a mirror
    # (the eye's image lies in the plane) select them; 70 is more than the 64 records: that mesh goes linear
    for what in ("a point light in z = 0.5", "a sun parallel to z = 0.5", "the last material reflects"):
        assert (few[what]["guarded"], few[what]["linear"]) == (5, 0), what
        assert (many[what]["guarded"], many[what]["linear"]) == (2, 1), what
    for what in ("the first lights again", "all opaque, none reflects again", "no light", "33 lights"):
        assert (few[what]["guarded"], few[what]["linear"]) == (0, 0) and (many[what]["guarded"], many[what]["linear"]) == (0, 0), what
    merged = edits["guard scene, 3 in the plane (merged)"]
    assert merged["a point light in z = 0.5"]["merged_keys"] == 5 and merged["the first lights again"]["merged_keys"] == 0


def test_shared_scan_text_equals_the_old_loop(report):
    for what in ("a point light", "a sun", "no light, the eye", "lights off the plane", "random planes"):
        assert any(re.match(rf"scan {re.escape(what)}\s+the shared text equals the old loop$", line) for line in report), what


def test_edit_entry_points_are_declared_and_check_their_arguments_without_a_device():
    names = declared("cutrace_edit.h")
    assert set(names) == set(_lib.EDIT_SYMBOLS) == {"ctr_scene_set_lights", "ctr_scene_set_materials", "ctr_scene_light_count",
                                                    "ctr_scene_material_count", "ctr_debug_guard_state"}
    L = _lib.hip_lib()
    assert not set(names) & (set(_lib.HIP_SYMBOLS) | set(_lib.HOST_SYMBOLS) | set(_lib.UPDATE_SYMBOLS))
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_edit.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert not any(n in symbols for symbols in _lib.HIP_PROTOS.values() for n in names)
    assert L.ctr_abi_version() == 3
    light, mat, n, lin = (_lib.Light * 1)(), (_lib.Material * 1)(), C.c_uint64(), C.c_int()
    assert L.ctr_scene_set_lights(None, light, 1) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_set_materials(None, mat, 1) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_light_count(None, C.byref(n)) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_scene_material_count(None, C.byref(n)) == 1 and b"null argument" in L.ctr_last_error()
    assert L.ctr_debug_guard_state(None, 0, None, 0, C.byref(n), C.byref(lin)) == 1 and b"null argument" in L.ctr_last_error()


class _NoHandle(cutrace_amd.DeviceScene):
    """the Python methods' own checks run before the library is called: no handle, no device"""
    def __init__(self, materials):
        self._h = None
        self._materials = cutrace_amd._records(_lib.Material, materials)
        self.n_lights = 2


def test_python_methods_reject_wrong_types_before_the_library_is_called():
    ds = _NoHandle([_lib.Material(), _lib.Material()])
    for bad in (None, 5, "lights", [1.0, 2.0], [_lib.Material()], [_lib.Light(), None]):
        with pytest.raises(TypeError):
            ds.set_lights(bad)
    for bad in (None, 5, b"mats", [_lib.Light()], [_lib.Material(), (1, 2, 3)]):
        with pytest.raises(TypeError):
            ds.set_materials(bad)
    assert ds.n_lights == 2 and len(ds._materials) == 2
    for idx in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match="bad material index"):
            ds.set_material(idx, reflexivity=0.5)
    with pytest.raises(TypeError, match="no material field"):
        ds.set_material(0, reflect=0.5)
