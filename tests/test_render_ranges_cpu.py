"""The checker of tests/test_gpu_render_ranges.py stays inside its own arithmetic (CPU, no GPU).

The render-side counterpart of tests/test_query_ranges_cpu.py.  Multiplying every position of a scene, and min_t, by 2^k
multiplies every depth by 2^k and changes neither a normal nor which object a pixel sees: the oracle must reproduce that
BIT FOR BIT at every exponent the GPU sweeps use.  Then none of its products overflowed or went denormal there.  And
every case's oracle frame must show every kind of object, recurse, and hold no NaN: a frame of misses, or one whose NaNs
make every comparison pass, would hide a kernel's failure.  The flattened scene is checked too: both meshes keep their
BVH, the merged tree is usable, so the GPU runs go through the top-level, the per-mesh and the merged walk.

A case that fails one of these leaves tests/util.py RENDER_RANGE_CASES, with a comment there that says why: it is not
tolerated here."""
import numpy as np
import pytest

import oracle
from tests.checkers import harness, run  # noqa: F401  (the fixture that builds scripts/flatten_check.cpp)
from tests import aa_ref
from tests.util import (ALL_MISS_CASE, OFFSET_CASES, RANGE_FLAVOURS, RANGE_KINDS, RANGE_POW_DEPENDENT, RENDER_RANGE_CASES, SCALE_EXPONENTS,
                        pow2, range_case_id, range_fudge, render_range_scene_json, same_bits)

W = H = 48
BOUNCES = 5
CASES = [pytest.param(c, f, id=f"{range_case_id(c)},{f}") for c in RENDER_RANGE_CASES for f in RANGE_FLAVOURS]
_frames = {}


def host_scene(ca, tmp_path, case, flavour):
    s = ca.HostScene.parse(render_range_scene_json(tmp_path, case[0], case[1], opaque=flavour == "opaque", w=W, h=H))
    assert s.ok
    return s


def oracle_frame(ca, tmp_path, case, flavour):
    """the oracle's frame of a case, rendered once and left unchanged"""
    if (case, flavour) not in _frames:
        o = oracle.oracle_render(host_scene(ca, tmp_path, case, flavour), fudge=range_fudge(case), bounces=BOUNCES)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _frames[case, flavour] = o
    return _frames[case, flavour]


def test_the_list_keeps_what_the_sweep_is_for():
    assert set(SCALE_EXPONENTS) == {-20, -12, 0, 12, 24}
    assert [c for c in RENDER_RANGE_CASES if c[1] is None and c[2]] == [(k, None, True) for k in SCALE_EXPONENTS]
    assert [(k, e) for k, e, scaled in RENDER_RANGE_CASES if e is not None and scaled] == list(OFFSET_CASES)
    assert set(OFFSET_CASES) == {(0, 10), (0, 14), (0, 18), (12, 10), (-12, 14)}
    assert [k for k, e, scaled in RENDER_RANGE_CASES if not scaled and e is None] == [-20, -12, 12, 24]
    assert len(RENDER_RANGE_CASES) == 14 and ALL_MISS_CASE in RENDER_RANGE_CASES and RANGE_FLAVOURS == ("mixed", "opaque")


@pytest.mark.parametrize("flavour", RANGE_FLAVOURS)
@pytest.mark.parametrize("k", SCALE_EXPONENTS)
def test_the_oracle_is_exact_under_a_scene_scaled_by_2_to_the_k(ca, tmp_path, k, flavour):
    base = oracle_frame(ca, tmp_path, (0, None, True), flavour)
    o = oracle_frame(ca, tmp_path, (k, None, True), flavour)
    assert np.isfinite(base["depth"]).sum() > W * H // 2
    assert same_bits(o["depth"], (base["depth"] * pow2(k)).astype(np.float32)), f"k = {k}: depth"
    assert same_bits(o["normal"], base["normal"]), f"k = {k}: normal"
    assert np.array_equal(o["hit_id"], base["hit_id"]), f"k = {k}: hit_id"


@pytest.mark.parametrize("case,flavour", CASES)
def test_the_oracle_frame_shows_enough(ca, tmp_path, case, flavour):
    o = oracle_frame(ca, tmp_path, case, flavour)
    px = W * H
    for key in ("depth", "color", "normal"):
        assert not np.isnan(o[key]).any(), key
    for key in ("color", "normal"):
        assert not np.isinf(o[key]).any(), key
    hit = o["hit_id"]
    seen = {kind: int(np.isin(hit, ids).sum()) for kind, ids in RANGE_KINDS.items()}
    print(f"{range_case_id(case)} {flavour}: primary hits {seen}, misses {int((hit < 0).sum())}, {o['ray_count'] / px:.2f} casts per pixel")
    if case == ALL_MISS_CASE:
        # every object is nearer than min_t: the primary cast and kernel.hpp's second one, nothing else
        assert (hit < 0).all() and np.isinf(o["depth"]).all() and not o["color"].any() and not o["normal"].any()
        assert o["ray_count"] == 2 * px
        return
    for kind, n in seen.items():
        assert 100 * n >= px, f"{kind} is the primary hit of {n} of {px} pixels"
    assert 2 * int((hit < 0).sum()) <= px
    assert o["ray_count"] >= 3 * px


@pytest.mark.parametrize("case,flavour", CASES)
def test_ref_render_equals_oracle_render(ca, tmp_path, case, flavour):
    """the restatement against the reference's own headers, where those have been built"""
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built here (needs the reference tree at build time)")
    s = host_scene(ca, tmp_path, case, flavour)
    o = oracle_frame(ca, tmp_path, case, flavour)
    r = oracle.ref_render(s, fudge=range_fudge(case), bounces=BOUNCES)
    for key in ("depth", "normal", "color"):
        assert same_bits(o[key], r[key]), key
    assert np.array_equal(o["hit_id"], r["hit_id"]) and o["ray_count"] == r["ray_count"]
    if hasattr(oracle.ref_lib(), "ref_render_ex"):   # the frames of the texture-coordinate tests
        kw = dict(fudge=range_fudge(case), bounces=BOUNCES, uv=True, ignore_transparent_primary=flavour == "mixed")
        o, r = oracle.oracle_render(s, **kw), oracle.ref_render(s, **kw)
        for key in ("depth", "normal", "color"):
            assert same_bits(o[key], r[key]), f"uv render: {key}"
        assert np.array_equal(np.isnan(o["uv"]), np.isnan(r["uv"])) and same_bits(np.nan_to_num(o["uv"]), np.nan_to_num(r["uv"]))


@pytest.mark.parametrize("case,flavour", CASES)
def test_which_frames_depend_on_how_the_pow_is_rounded(ca, tmp_path, case, flavour):
    """VAR_EXACT_POW computes the specular term as the f64 pow rounded once; glibc's powf, the reference's, is not correctly
    rounded and now and then gives the neighbouring float.  A bitwise colour comparison is the kernel's business only on a
    frame that does not depend on the difference.  Every 48 x 48 frame, the texture-coordinate renders included, must be
    such a frame; of the reduced supersampled frames, exactly those of util.RANGE_POW_DEPENDENT are not."""
    import os
    s = host_scene(ca, tmp_path, case, flavour)
    kw = dict(fudge=range_fudge(case), bounces=BOUNCES, threads=min(os.cpu_count() or 4, 16))
    extra = [dict(uv=True), dict(uv=True, ignore_transparent_primary=True)] if flavour == "mixed" else [dict(uv=True)]
    for opts in [dict()] + extra:
        a, b = oracle.oracle_render(s, **kw, **opts), oracle.oracle_render(s, pow_rounded_once=True, **kw, **opts)
        for key in ("depth", "normal", "color"):
            assert same_bits(a[key], b[key]), (opts, key)
    for ss in (2, 4):
        s.set_size(ss * W, ss * H)
        a, b = oracle.oracle_render(s, **kw), oracle.oracle_render(s, pow_rounded_once=True, **kw)
        assert same_bits(a["depth"], b["depth"]) and same_bits(a["normal"], b["normal"]) and a["ray_count"] == b["ray_count"]
        ra, rb = aa_ref.reduce_frame(a, ss), aa_ref.reduce_frame(b, ss)
        words = int((ra["color"].view(np.uint32) != rb["color"].view(np.uint32)).sum())
        print(f"{range_case_id(case)} {flavour} s={ss}: {words} colour words of the reduced frame depend on the pow")
        assert (words != 0) == ((case, flavour, ss) in RANGE_POW_DEPENDENT), (case, flavour, ss, words)


@pytest.mark.parametrize("case,flavour", CASES)
def test_both_meshes_keep_their_bvh_and_the_merged_tree_is_usable(ca, harness, tmp_path, case, flavour):  # noqa: F811
    flat, stages = run(harness, tmp_path, host_scene(ca, tmp_path, case, flavour), merge=True)
    assert flat["scalars"]["n_mesh"] == 2 and flat["scalars"]["mesh_tris"] == 1000 and flat["scalars"]["merged_reserved"] == 1
    assert flat["scalars"]["all_opaque"] == int(flavour == "opaque")
    for st in stages:
        assert len(st["linear"]) == 2 and not any(int(x[0]) for x in st["linear"]), f"stage {st['what']}: a mesh is walked linearly"
    last = stages[-1]
    assert list(last["merged"]) == [1, 1], "the merged tree is not usable"
    print(f"{range_case_id(case)} {flavour}: guarded triangles {[len(g) for g in last['guarded']]}, in the merged tree {len(last['merged_guarded'])}")
