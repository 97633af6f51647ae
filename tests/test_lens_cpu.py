"""The lens render's host side (CPU, no GPU): choose_kernel for the two lens entries over their whole input space
(scripts/kernel_choice_lens_check.cpp), the ray builders of cutrace_amd/lenses.py, the mask rule of include/cutrace_lens.h
restated in numpy, and the C-ABI's struct and symbol."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cutrace_amd import _lib, lenses
from tests import ray_ref
from tests.checkers import CHOICE_SOURCES, I_CSRC, I_INCLUDE, check_output, check_program
from tests.util import _random_scene, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 512, 8, 2, 4)  # entry (lens, lens + samples), user mask, scene flags, deliverable, stack shape
# bit k of the user-mask index (the checker's MASK_BITS), and the KV_* bits of scene_device.h
NO_PREFILTER, NO_ANYHIT, NO_CLUSTER, STATS, EXACT_POW, NO_OCC6, NO_DIRECT, MERGE, IGNTR = (1 << k for k in range(9))
KV_PREFILTER, KV_ANYHIT, KV_BVH, KV_FASTPOW, KV_OCC6, KV_SS, KV_RAYS = 1, 2, 8, 32, 64, 2048, 4096
REJECTING = NO_PREFILTER | NO_CLUSTER | STATS | IGNTR


@pytest.fixture(scope="module")
def lens_choices(tmp_path_factory):
    exe = check_program(tmp_path_factory, "kernel_choice_lens_check", ("-O2", I_CSRC, I_INCLUDE), CHOICE_SOURCES)
    words = check_output(exe).split()
    at = {k: words.index(k) for k in ("list", "render", "reject", "neutral")}
    got = np.array([int(x, 16) for x in words[:at["list"]]], np.uint16)
    assert got.size == int(np.prod(SHAPE))
    return dict(got=got.reshape(SHAPE), builds=[int(x, 16) for x in words[at["list"] + 1:at["render"]]],
                n_render=int(words[at["render"] + 1]), kr_lens=int(words[at["reject"] + 1], 16), moved=int(words[at["neutral"] + 1]))


def test_lens_builds_and_rejections(lens_choices):
    got, builds = lens_choices["got"], lens_choices["builds"]
    assert len(builds) == len(set(builds)) == 10 and lens_choices["n_render"] == 43  # 53 builds, the first list untouched
    assert lens_choices["moved"] == 0  # CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST
    mask = np.arange(512)
    rejected = (mask & REJECTING) != 0
    # the rejections are exactly the four listed bits, with KR_LENS
    assert (got[:, rejected] == lens_choices["kr_lens"]).all()
    ok = got[:, ~rejected]
    assert (ok < 0xF000).all()
    chosen = set(int(x) for x in np.unique(ok))
    assert chosen == set(builds), (sorted(chosen - set(builds)), sorted(set(builds) - chosen))
    # every build is the shipped walk with KV_RAYS; KV_SS exactly for the samples entry
    fixed = KV_PREFILTER | KV_BVH | KV_RAYS
    assert ((ok & fixed) == fixed).all()
    assert ((ok[0] & KV_SS) == 0).all() and ((ok[1] & KV_SS) == KV_SS).all()
    assert ((ok & ~np.uint16(fixed | KV_SS | KV_ANYHIT | KV_FASTPOW | KV_OCC6)) == 0).all()


def test_lens_optional_bits(lens_choices):
    got = lens_choices["got"]
    fits = np.array([True, False, True, False])  # the checker's SHAPES
    for m in range(512):
        if m & REJECTING:
            continue
        for flags in range(8):
            all_opaque, big = bool(flags & 1), bool(flags & 2)
            anyhit = all_opaque and not (m & NO_ANYHIT)
            pow_ = not (m & EXACT_POW)
            for e in range(2):
                g = got[e, m, flags]  # (deliverable, shape)
                assert (((g & KV_ANYHIT) != 0) == anyhit).all(), (e, m, flags)
                assert (((g & KV_FASTPOW) != 0) == pow_).all(), (e, m, flags)
                # the 6-wave build: large mesh, the stacks leave it room, CTR_VAR_NO_OCC6 clear — and the default variant
                want6 = np.broadcast_to(fits & (big and anyhit and pow_ and not (m & NO_OCC6)), (2, 4))
                assert np.array_equal((g & KV_OCC6) != 0, want6), (e, m, flags)
        # bits with nothing to act on move nothing
        if not (m & (NO_DIRECT | MERGE)):
            for extra in (NO_DIRECT, MERGE, NO_DIRECT | MERGE):
                assert np.array_equal(got[:, m], got[:, m | extra]), (m, extra)
    # the merged-tree flag and deliverable are no inputs of a lens launch
    assert np.array_equal(got[:, :, :4], got[:, :, 4:]) and np.array_equal(got[:, :, :, 0], got[:, :, :, 1])


def _cams():
    from cutrace_amd import HostScene
    out = []
    for seed, w, h in ((3, 21, 13), (5, 21, 13), (5, 40, 24)):
        s = HostScene.parse(_random_scene(seed, w, h))
        assert s.ok
        out.append((ray_ref.RefScene(s).cam, s, w, h))  # (the scene itself: its camera struct lives as long as it does)
    return out


def test_pinhole_normalised_is_get_ray_bit_for_bit():
    for cam, scene, w, h in _cams():
        want_o, want_d = ray_ref.camera_rays(cam)
        for c in (cam, scene.desc.contents.cam):  # a dict or the C-ABI's struct
            o, d = lenses.pinhole(c, w, h)
            assert o.shape == d.shape == (h, w, 3) and o.dtype == d.dtype == np.float32
            assert same_bits(o.reshape(-1, 3), want_o)
            assert same_bits(ray_ref.vnormalized(d.reshape(-1, 3)).astype(np.float32), want_d)
            assert not lenses.is_masked(o, d).any()


def mask_rule(o, d):
    """include/cutrace_lens.h restated: origin not finite, or normalized(dir) not finite or (0, 0, 0)"""
    with np.errstate(all="ignore"):
        u = ray_ref.vnormalized(np.asarray(d, np.float32))
    return ~np.isfinite(o).all(-1) | ~np.isfinite(u).all(-1) | ((u[..., 0] == 0) & (u[..., 1] == 0) & (u[..., 2] == 0))


def test_mask_rule_and_fisheye_rim():
    cam, _, w, h = _cams()[0]
    for ww, hh, fov in ((w, h, 180.0), (24, 16, 220.0), (9, 9, 90.0)):
        o, d = lenses.fisheye(cam, ww, hh, fov)
        nan = np.isnan(d).any(-1)
        assert np.array_equal(mask_rule(o, d), nan) and np.array_equal(lenses.is_masked(o, d), nan)
        # the circle inscribed in the frame: a rim is masked, the centre is not, and a kept direction has unit length
        assert nan.any() and not nan.all() and nan[0, 0] and not nan[hh // 2, ww // 2]
        assert np.allclose(np.linalg.norm(d[~nan], axis=-1), 1.0, atol=1e-6)
    # the rule's other cases, one ray each: inf, zero, too long (squared length overflows), too short (underflows), NaN origin
    f = np.float32
    d = np.array([[0, 0, 1], [np.inf, 0, 0], [-np.inf, 1, 0], [0, 0, 0], [0, -0.0, 0], [1e30, 0, 0], [1e-30, 0, 0], [0, 2, 0], [3e19, 0, 0]], f)
    o = np.zeros_like(d)
    o[7, 1] = np.nan
    assert mask_rule(o, d).tolist() == [False, True, True, True, True, True, True, True, True]
    assert lenses.is_masked(o, d).tolist() == mask_rule(o, d).tolist()
    o[7, 1] = np.inf
    assert mask_rule(o, d)[7]


def test_stereo_and_thin_lens_shapes():
    cam, _, w, h = _cams()[0]
    o, d = lenses.stereo(cam, 24, 16, 0.3)
    assert o.shape == d.shape == (16, 24, 3)
    assert len(np.unique(o.reshape(-1, 3), axis=0)) == 2 and not np.array_equal(o[0, 0], o[0, 23])
    assert np.allclose(np.linalg.norm(o[0, 23] - o[0, 0]), 0.3, atol=1e-6)
    assert same_bits(d[:, :12], lenses.pinhole(cam, 12, 16)[1]) and same_bits(d[:, 12:], d[:, :12])
    for s in (1, 2, 4):
        o, d = lenses.thin_lens(cam, 21, 13, s, 0.2, 4.0, seed=7)
        assert o.shape == d.shape == (13 * s, 21 * s, 3) and o.dtype == d.dtype == np.float32
        assert not lenses.is_masked(o, d).any()
        assert len(np.unique(o.reshape(-1, 3), axis=0)) == 13 * 21 * s * s  # an origin per sample
        assert np.linalg.norm(o - cam["pos"], axis=-1).max() <= 0.1 + 1e-6
        o2, d2 = lenses.thin_lens(cam, 21, 13, s, 0.2, 4.0, seed=7)
        assert same_bits(o, o2) and same_bits(d, d2)
    # aperture 0: every ray from the eye, through its jittered pinhole point
    o, d = lenses.thin_lens(cam, 8, 8, 2, 0.0, 4.0, seed=1)
    assert (o == cam["pos"]).all()


def test_abi_struct_and_symbol():
    assert ctypes.sizeof(_lib.Lens) == 32
    assert [f[0] for f in _lib.Lens._fields_] == ["n_rays", "samples", "ambient", "d_origin", "d_dir"]
    assert (_lib.Lens.samples.offset, _lib.Lens.ambient.offset, _lib.Lens.d_origin.offset, _lib.Lens.d_dir.offset) == (8, 12, 16, 24)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cutrace_lens.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ctr_[a-z0-9_]+)\s*\(", txt))) == _lib.LENS_SYMBOLS
    # the struct as the C compiler lays it out
    if shutil.which("gcc"):
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "cutrace_lens.h"\nint main(void){printf("%zu %zu %zu", sizeof(ctr_lens), offsetof(ctr_lens, d_origin), offsetof(ctr_lens, d_dir));return 0;}\n'
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            open(os.path.join(td, "s.c"), "w").write(src)
            subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(td, "s"), os.path.join(td, "s.c")])
            assert subprocess.run([os.path.join(td, "s")], capture_output=True, text=True, check=True).stdout.split() == ["32", "16", "24"]
    L = _lib.hip_lib()
    assert hasattr(L, "ctr_render_device_lens")
    assert L.ctr_abi_version() == 3
    # a null scene is refused before anything else (no GPU here)
    q = _lib.Lens(1, 1, 0.1, None, None)
    assert L.ctr_render_device_lens(None, ctypes.c_float(1e-3), 5, ctypes.byref(q), None, None, None, None, None, None) == 1
    assert b"null scene" in L.ctr_last_error()
