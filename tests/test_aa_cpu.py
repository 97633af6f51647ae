"""Supersampled render (include/cutrace_aa.h), what can be checked without a GPU: the two entry points exist and
reject a NULL scene, the header is C, and the premise of the definition — the s*w x s*h frame contains the w x h frame,
bit for bit, at every s-th pixel — holds for the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle

from cutrace_amd import _lib
from tests import aa_ref
from tests.checkers import declared
from tests.util import _random_scene, same_bits

ROOT = _lib.ROOT
NT = min(os.cpu_count() or 4, 8)


def test_library_exports_the_aa_entry_points():
    names = declared("cutrace_aa.h")
    assert set(names) == set(_lib.AA_SYMBOLS) == {"ctr_render_aa", "ctr_render_device_aa"}
    assert not set(names) & set(_lib.HIP_SYMBOLS)  # cutrace_amd.h is unchanged
    L = _lib.hip_lib()
    for n in names:
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
    assert L.ctr_abi_version() == 3


def test_null_scene_is_invalid():
    L = _lib.hip_lib()
    assert L.ctr_render_aa(None, C.c_float(1e-3), 5, 2, None, None, None, None, None) == 1  # CTR_E_INVALID
    assert L.ctr_last_error()
    assert L.ctr_render_device_aa(None, C.c_float(1e-3), 5, 2, None, None, None, None, None, None) == 1


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    src = tmp_path / "aa.c"
    src.write_text('#include "cutrace_aa.h"\n'
                   "int (*host_form)(ctr_scene *, float, int, uint32_t, const ctr_rows *, float *, float *, float *, ctr_render_stats *) = ctr_render_aa;\n"
                   "int (*device_form)(ctr_scene *, float, int, uint32_t, const ctr_rows *, void *, void *, void *, void *, void *) = ctr_render_device_aa;\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o",
                           str(tmp_path / "aa.o"), str(src)])


def test_reduction_tree_by_hand():
    """2 x 2 and 4 x 4 blocks whose float32 sums depend on the order: the helper follows the tree of the definition"""
    f = np.float32
    a = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], f)   # (1 + e) + (e + e) is not ((1 + e) + e) + e in float32
    blk = np.zeros((2, 2, 3), f)
    blk[0, 0], blk[0, 1], blk[1, 0], blk[1, 1] = a[0], a[1], a[2], a[3]
    want = f(f(f(a[0] + a[1]) + f(a[2] + a[3])) * f(0.25))
    assert same_bits(aa_ref.reduce_color(blk, 2), np.full((1, 1, 3), want, f))
    rng = np.random.RandomState(0)
    v = (rng.uniform(0, 1, (4, 4)) * 10.0 ** rng.uniform(-6, 2, (4, 4))).astype(f)
    rows = [f(f(v[y, 0] + v[y, 1]) + f(v[y, 2] + v[y, 3])) for y in range(4)]
    want = f(f(f(rows[0] + rows[1]) + f(rows[2] + rows[3])) * f(1.0 / 16))
    got = aa_ref.reduce_color(np.repeat(v[:, :, None], 3, 2), 4)
    assert same_bits(got, np.full((1, 1, 3), want, f))


@pytest.fixture(scope="module")
def small_and_host(ca):
    s = ca.HostScene.parse(_random_scene(3, 21, 13))
    assert s.ok
    return s, oracle.oracle_render(s, bounces=5, threads=NT), oracle.oracle_render(s, bounces=5, rows=(0, 13, 2, 1, 3), threads=NT)


@pytest.mark.parametrize("ss", [2, 4, 8])
def test_big_frame_contains_the_small_one(small_and_host, ss):
    """guards the oracle, not the feature: (float)(s*x) / (float)(s*w) == (float)x / (float)w, so pixel (s*x, s*y) of the
    s*w x s*h render is pixel (x, y) of the w x h render — whole frame and an interleaved row part"""
    s, small, small_part = small_and_host
    w, h = 21, 13
    s.set_size(ss * w, ss * h)
    try:
        big = oracle.oracle_render(s, bounces=5, threads=NT)
        big_part = oracle.oracle_render(s, bounces=5, rows=(0, ss * h, 2 * ss, 1, 3), threads=NT)
    finally:
        s.set_size(w, h)
    for b, sm, what in ((big, small, "frame"), (big_part, small_part, "rows")):
        assert b["depth"].shape == (ss * sm["depth"].shape[0], ss * w)
        for k in ("depth", "normal", "color"):
            assert not np.isnan(b[k]).any(), (what, k)
            assert same_bits(np.ascontiguousarray(b[k][::ss, ::ss]), sm[k]), (what, k, ss)
    # the order of the sum is visible in the bits: a bitwise test of the colour pins it
    tree, raster = aa_ref.reduce_color(big["color"], ss), aa_ref.raster_color(big["color"], ss)
    assert (tree.view(np.uint32) != raster.view(np.uint32)).any()
