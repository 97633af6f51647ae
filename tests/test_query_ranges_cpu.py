"""The checker of tests/test_gpu_query_ranges.py stays inside its own arithmetic (CPU, no GPU).

Multiplying a ray's direction by 2^j divides every distance by 2^j and changes nothing else; multiplying a scene by 2^k
multiplies distances and points by 2^k.  tests/ray_ref.py must reproduce that BIT FOR BIT at every exponent the GPU
sweeps use: then none of its products overflowed or went denormal there, and a mismatch on the GPU is the kernel's."""
import numpy as np
import pytest

from tests import ray_ref
from tests.conftest import load_scene
from tests.util import DIR_EXPONENTS, SCALE_EXPONENTS, f32, f32_bits, pow2, scaled_scene_json, sweep_rays

N = 3000


def _same(a, b, what):
    assert np.array_equal(f32_bits(a), f32_bits(b)), f"{what}: {int((f32_bits(a) != f32_bits(b)).reshape(len(a), -1).any(-1).sum())} rays"


def test_the_sweep_keeps_what_the_issue_of_the_clamp_needs():
    assert sum(j <= -100 for j in DIR_EXPONENTS) >= 2      # every reciprocal beyond the box test's 1e30
    assert any(-99 <= j <= -94 for j in DIR_EXPONENTS)     # some components beyond it, some not
    assert 0 in SCALE_EXPONENTS


@pytest.mark.parametrize("j", DIR_EXPONENTS)
def test_ray_ref_is_exact_under_a_direction_of_length_2_to_the_j(ca, j):
    rs = ray_ref.RefScene(load_scene(ca, "bunny", 32, 32))
    assert not any(o["type"] == ray_ref.OBJ_SPHERE for o in rs.objects)   # a sphere normalises: its t does not scale
    o, d, sel = sweep_rays(1, N, rs)
    mt = np.where(sel == 0, f32(0.0), f32(1e-3)).astype(f32)
    base = ray_ref.ray_cast(rs, o, d, mt)
    mesh = [i for i, ob in enumerate(rs.objects) if ob["type"] == ray_ref.OBJ_MESH]
    assert np.isin(base["object"], mesh).sum() >= N // 20 and (base["object"] >= 0).sum() >= N // 10
    s, inv = pow2(j), pow2(-j)
    got = ray_ref.ray_cast(rs, o, d * s, mt * inv)
    assert np.array_equal(got["object"], base["object"]) and np.array_equal(got["prim"], base["prim"])
    _same(got["t"], base["t"] * inv, f"j = {j}: t")
    for k in ("point", "normal", "uv"):
        _same(got[k], base[k], f"j = {j}: {k}")


@pytest.mark.parametrize("k", SCALE_EXPONENTS)
def test_ray_ref_is_exact_under_a_scene_scaled_by_2_to_the_k(ca, tmp_path, k):
    def scene(e):
        s = ca.HostScene.parse(scaled_scene_json(tmp_path, e))
        assert s.ok
        return ray_ref.RefScene(s)
    rs0, rs = scene(0), scene(k)
    o, d, sel = sweep_rays(2, N, rs0)
    mt = np.where(sel == 0, f32(0.0), f32(1e-3)).astype(f32)
    base = ray_ref.ray_cast(rs0, o, d, mt)
    kinds = {t: np.isin(base["object"], [i for i, ob in enumerate(rs0.objects) if ob["type"] == t]) for t in range(4)}
    assert kinds[ray_ref.OBJ_MESH].sum() >= N // 20 and all(m.sum() >= 20 for m in kinds.values())
    s = pow2(k)
    got = ray_ref.ray_cast(rs, o * s, d, mt * s)
    assert np.array_equal(got["object"], base["object"]) and np.array_equal(got["prim"], base["prim"])
    _same(got["t"], base["t"] * s, f"k = {k}: t")
    _same(got["point"], base["point"] * s, f"k = {k}: point")
    _same(got["normal"], base["normal"], f"k = {k}: normal")
    pos_uv = kinds[ray_ref.OBJ_MESH] | kinds[ray_ref.OBJ_PLANE]   # a mesh's and a plane's uv are positions
    _same(got["uv"], np.where(pos_uv[:, None], base["uv"] * s, base["uv"]), f"k = {k}: uv")
