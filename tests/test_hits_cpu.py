"""Hit lists (include/cutrace_hits.h, DeviceScene.list_hits) as far as they need no device: the header, the prototype table, the
struct layout, the refusals in front of the scene, the Python argument checks — and the NumPy checker of the GPU tests
(tests/hits_ref.py) pinned against independent code: a list's running sum IS ray_ref.shadow_intensity."""
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
from tests import hits_ref, ray_ref
from tests.checkers import ROOT, declared

f32 = np.float32
NAMES = {"ctr_list_hits"}


def test_hits_entry_point_is_declared_exported_and_laid_out_as_the_header_says(tmp_path):
    assert set(declared("cutrace_hits.h")) == set(_lib.HITS_SYMBOLS) == NAMES
    others = [_lib.HOST_SYMBOLS, _lib.HIP_SYMBOLS, _lib.RAY_SYMBOLS, _lib.AA_SYMBOLS, _lib.LENS_SYMBOLS, _lib.IMAGES_SYMBOLS, _lib.UPDATE_SYMBOLS,
              _lib.EDIT_SYMBOLS, _lib.OBJECT_SYMBOLS, _lib.REBUILD_SYMBOLS, _lib.REPLACE_SYMBOLS, _lib.TOPOLOGY_SYMBOLS]
    assert not any(NAMES & set(symbols) for symbols in others)
    assert not any(NAMES & set(t) for h, t in _lib.HIP_LATER_PROTOS.items() if h != "cutrace_hits.h")
    assert not any(NAMES & set(t) for t in _lib.HIP_PROTOS.values())
    assert set(declared("cutrace_rays.h")) == {"ctr_cast_rays", "ctr_shade_rays", "ctr_shade_points"}   # the neighbour's list is as it was
    L = _lib.hip_lib()
    for n, proto in _lib.HIP_LATER_PROTOS["cutrace_hits.h"].items():
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
        assert (getattr(L, n).argtypes, getattr(L, n).restype) == proto, n
    assert L.ctr_abi_version() == 3
    # sizeof / offsetof of ctr_hit_query as the C compiler lays it out, against the ctypes mirror
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    fields = [f for f, _ in _lib.HitQuery._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_hits.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(ctr_hit_query));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(ctr_hit_query, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.HitQuery) == 120
    assert got[1:] == [getattr(_lib.HitQuery, f).offset for f in fields]
    header = open(os.path.join(ROOT, "include", "cutrace_hits.h")).read()
    for name, value in (("CTR_HITS_IGNORE_TRANSPARENT", cutrace_amd.HITS_IGNORE_TRANSPARENT), ("CTR_HITS_LINEAR", cutrace_amd.HITS_LINEAR),
                        ("CTR_HITS_MAX", cutrace_amd.HITS_MAX)):
        assert re.search(rf"#define\s+{name}\s+{value}u\b", header), name
    assert cutrace_amd.HITS_OUTPUTS == cutrace_amd.RAY_OUTPUTS == hits_ref.OUTPUTS


def _query(**kw):
    q = _lib.HitQuery()
    q.n_rays, q.max_hits, q.step = 4, 4, 1e-3
    q.d_count = 0x1000   # (never dereferenced: every call here fails first)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_list_hits_refuses_a_bad_query_before_it_looks_at_the_scene():
    L = _lib.hip_lib()

    def refused(q, text):
        assert L.ctr_list_hits(None, C.byref(q) if q is not None else None, None) == 1, text
        msg = L.ctr_last_error().decode()
        assert msg.startswith("ctr_list_hits: ") and text in msg, (text, msg)

    refused(None, "null query")
    refused(_query(), "null scene")
    for flags in (4, 8, 0x80000000):
        refused(_query(flags=flags), f"unknown flag bits {flags}")
    refused(_query(max_hits=0), "max_hits 0 outside [1, 65535]")
    refused(_query(max_hits=65536), "max_hits 65536 outside [1, 65535]")
    for step in (-1.0, float("nan"), float("inf"), -float("inf")):
        refused(_query(step=step), "step must be finite and not negative")
    refused(_query(d_count=None), "no output")
    refused(_query(step=0.0, max_hits=65535, flags=3), "null scene")   # the edges of what is allowed get as far as the scene


class _NoHandle(cutrace_amd.DeviceScene):
    """a scene that reaches no library: whatever gets past the method's own checks fails on the missing device"""
    def __init__(self, device=None):
        self._h = None
        self._dev = device

    def _torch_device(self):
        if self._dev is None:
            raise AssertionError("the arguments were not checked before the device was asked for")
        return self._dev


def test_list_hits_names_what_is_wrong_before_the_library_is_called(monkeypatch):
    import torch
    ok = np.zeros((4, 3), f32)
    ds = _NoHandle()
    for outputs in (("depth",), ("t", "t"), "uv", ("count",), (None,)):
        with pytest.raises(ValueError, match="outputs"):
            ds.list_hits(ok, ok, 4, outputs=outputs)
    for k in (4.0, "4", None, True, [4]):
        with pytest.raises(TypeError, match="max_hits"):
            ds.list_hits(ok, ok, k)
    for k in (0, -1, 65536):
        with pytest.raises(ValueError, match="max_hits"):
            ds.list_hits(ok, ok, k)
    for step in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="step"):
            ds.list_hits(ok, ok, 4, step=step)

    # what is wrong with the arrays is said once the device is known, before anything is copied to it
    @contextlib.contextmanager
    def no_stream(dev, stream):
        yield None
    monkeypatch.setattr(cutrace_amd, "_on_stream", no_stream)
    ds = _NoHandle(torch.device("cpu"))
    with pytest.raises(ValueError, match="dirs: 5 rays for 4 origins"):
        ds.list_hits(ok, np.zeros((5, 3), f32), 4)
    with pytest.raises(ValueError, match="origins: expected float32"):
        ds.list_hits(ok.astype(np.float64), ok, 4)
    with pytest.raises(ValueError, match="dirs: expected float32"):
        ds.list_hits(ok, np.zeros((4, 2), f32), 4)
    with pytest.raises(ValueError, match="min_t: 3 values for 4 rays"):
        ds.list_hits(ok, ok, 4, min_t=np.zeros(3, f32))
    with pytest.raises(ValueError, match="max_t: expected float32"):
        ds.list_hits(ok, ok, 4, max_t=np.zeros(4, np.float64))
    with pytest.raises(TypeError, match="max_t"):
        ds.list_hits(ok, ok, 4, max_t=[1.0] * 4)
    with pytest.raises(ValueError, match="below 2\\^31"):
        ds.list_hits(np.zeros((40000, 3), f32), np.zeros((40000, 3), f32), 65535)


@pytest.fixture(scope="module")
def layered(ca, tmp_path_factory):
    s = hits_ref.layered_scene(ca, tmp_path_factory.mktemp("layers"))
    o, d = hits_ref.layered_rays()
    rs = ray_ref.RefScene(s)
    return rs, o, d, hits_ref.list_hits(rs, o, d, 16)


def test_the_checker_lists_what_the_test_scene_promises(layered):
    """the facts the GPU tests' conditions rest on, on the reference alone"""
    rs, o, d, full = layered
    n, count = len(o), full["count"]
    assert (count == 0).sum() >= 0.15 * n and (count >= 3).sum() >= 0.05 * n and (count >= 4).sum() >= 0.02 * n
    assert 4 < count.max() < 16
    listed = full["object"][full["object"] >= 0]
    assert set(np.unique(listed)) == set(range(7)) - {hits_ref.COINCIDENT_PLANE}      # every other object is listed somewhere
    # t strictly increases along a list, filled slots come first, unfilled slots hold the miss values
    for j in range(16):
        on, off = j < count, j >= count
        assert np.isfinite(full["t"][j, on]).all() and (full["object"][j, on] >= 0).all()
        assert np.isinf(full["t"][j, off]).all() and (full["object"][j, off] == -1).all() and (full["prim"][j, off] == -1).all()
        assert not full["point"][j, off].any() and not full["normal"][j, off].any() and not full["uv"][j, off].any()
        if j:
            assert (full["t"][j, on] > full["t"][j - 1, on]).all()
    # K = 4 is the K = 16 list cut off
    four = hits_ref.list_hits(rs, o, d, 4)
    assert np.array_equal(four["count"], np.minimum(count, 4))
    for k in hits_ref.OUTPUTS:
        assert np.array_equal(four[k], full[k][:4], equal_nan=True), k
    # step = 0: a mesh hit at t is rejected whole by the next cast, so the stack of six quads never fills two slots in a row
    zero = hits_ref.list_hits(rs, o, d, 16, step=0.0)
    assert zero["count"].max() < count.max()
    twice = lambda h: (h["object"][1:] == 0) & (h["object"][:-1] == 0)
    assert not twice(zero).any() and twice(full).any()
    assert (hits_ref.list_hits(rs, o, d, 16, max_t=f32(2.0))["count"] == 0).sum() > (count == 0).sum()


def test_a_lists_running_sum_is_shadow_intensity(layered):
    """hits_ref against ray_ref.shadow_intensity, which has a loop of its own: with min_t = (float)(0.0 + 1e-3) and step 1e-3
    the list is what shadow_intensity visits, and the clamped float32 sum over it is its value, bit for bit"""
    rs, o, d, _ = layered
    max_t = np.random.RandomState(2).choice([0.5, 2.0, 100.0, np.inf], len(o)).astype(f32)
    h = hits_ref.list_hits(rs, o, d, 16, min_t=f32(0.0 + 1e-3), max_t=max_t, step=1e-3)
    assert h["count"].max() < 16
    got = hits_ref.shadow_from_lists(rs, h["count"], h["object"])
    want = ray_ref.shadow_intensity(rs, o, d, max_t)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} rays differ"
    assert ((want > 0) & (want < 1)).any() and (want == 1).any() and (want == 0).any()
    for m in (0.5, 2.0, 100.0, np.inf):
        assert (max_t == f32(m)).sum() > len(o) // 8
