"""CPU tests: the oracle (oracle/ctr_oracle.c, plain-C restatement) is pinned
 (a) bit-for-bit against the committed golden buffers that were generated from the
     reference's own headers compiled for the host (tests/golden/make_golden.py), and
 (b) where oracle/_ref exists (the build container; the prebuilt .so also travels to the
     GPU box), bit-for-bit against a live run of that reference build.
The reference holds no render tests or golden vectors of its own."""
import os

import numpy as np
import pytest

import oracle

from tests.conftest import load_scene
from tests.util import GOLD, GOLD_SMALL, golden_case, same_bits

SMALL = GOLD_SMALL


def test_golden_fixtures_exist():
    assert len(SMALL) >= 6, "golden fixtures missing: run tests/golden/make_golden.py in the build container"


@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p) for p in SMALL])
def test_oracle_matches_golden_bit_for_bit(ca, path):
    name, w, h, b = golden_case(path)
    g = np.load(path)
    s = load_scene(ca, name, w, h)
    r = oracle.oracle_render(s, bounces=b, threads=4)
    assert same_bits(r["depth"], g["depth"])
    assert same_bits(r["normal"], g["normal"])
    assert same_bits(r["color"], g["color"])
    assert np.array_equal(r["hit_id"], g["hit_id"].astype(np.int64))
    assert r["ray_count"] == int(g["ray_count"])


def test_survey_known_answers(ca):
    """Numbers SURVEY.md §8(c) recorded from the host-compiled reference."""
    s = load_scene(ca, "triangle")  # 20x20 as shipped
    r = oracle.oracle_render(s, bounces=5)
    fin = np.isfinite(r["depth"])
    assert int(fin.sum()) == 38
    assert np.allclose(r["color"].astype(np.float64).reshape(-1, 3).sum(0), [0.266, 0.076, 0.266], atol=1e-6)
    assert abs(float(r["depth"][fin].astype(np.float64).sum()) - 192.460781) < 1e-5
    s = load_scene(ca, "triangle", 128, 128)
    r = oracle.oracle_render(s, bounces=5)
    assert int(np.isfinite(r["depth"]).sum()) == 1301
    assert r["ray_count"] == 34069


def test_full_resolution_samples_sphere_plane(ca):
    """Full-size golden (checksums + 4096 sampled pixels) for the cheapest 1080p config."""
    path = os.path.join(GOLD, "full_sphere_plane_1920x1080_b5.npz")
    if not os.path.exists(path):
        pytest.skip("full-resolution golden not generated")
    g = np.load(path)
    s = load_scene(ca, "sphere_plane")
    r = oracle.oracle_render(s, bounces=5, threads=os.cpu_count() or 4)
    idx = g["sample_idx"]
    assert same_bits(r["depth"].reshape(-1)[idx], g["depth"])
    assert same_bits(r["color"].reshape(-1, 3)[idx], g["color"])
    assert same_bits(r["normal"].reshape(-1, 3)[idx], g["normal"])
    assert r["ray_count"] == int(g["ray_count"]) == 13973091
    assert int(np.isfinite(r["depth"]).sum()) == int(g["n_finite"]) == 1053501


REF_CASES = [("triangle", 20, 20, 5), ("sphere_plane", 64, 36, 5), ("sphere_plane", 64, 36, 1), ("bunny", 48, 27, 5),
             ("mirror", 64, 36, 8), ("mirror", 64, 36, 0)]


@pytest.mark.parametrize("name,w,h,b", REF_CASES)
def test_oracle_matches_live_reference_build(ca, name, w, h, b):
    from cutrace_amd import _lib
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    s = load_scene(ca, name, w, h)
    o = oracle.oracle_render(s, bounces=b, threads=4)
    r = oracle.ref_render(s, bounces=b, threads=4)
    for k in ("depth", "normal", "color"):
        assert same_bits(o[k], r[k]), k
    assert np.array_equal(o["hit_id"], r["hit_id"])
    assert o["ray_count"] == r["ray_count"]


def test_row_selection_matches_full_frame(ca):
    """Interleaved row blocks (the multi-GPU tiling) reproduce the full frame exactly."""
    s = load_scene(ca, "sphere_plane", 64, 40)
    full = oracle.oracle_render(s, bounces=3, threads=4)
    n_parts, br = 3, 8
    total = 0
    for part in range(n_parts):
        rows = (0, 40, br, part, n_parts)
        r = oracle.oracle_render(s, bounces=3, rows=rows, threads=2)
        ys = [y for y in range(40) if (y // br) % n_parts == part]
        assert r["depth"].shape[0] == len(ys) == ca.rows_count(40, rows)
        assert same_bits(r["color"], full["color"][ys])
        assert same_bits(r["depth"], full["depth"][ys])
        total += r["ray_count"]
    assert total == full["ray_count"]


def test_look_at_matches(ca):
    """Host camera basis (libcutrace_host) == oracle restatement == reference build."""
    import ctypes as C
    from cutrace_amd import _lib
    eye, up, look = _lib.Vec3(1, 0, 2), _lib.Vec3(0, 1, 0), _lib.Vec3(-0.92388, 0, -0.38268)
    a, b = _lib.Camera(), _lib.Camera()
    _lib.host_lib().ctr_camera_look_at(C.byref(a), eye, up, look)
    oracle.oracle_lib().orc_look_at(C.byref(b), eye, up, look)
    for f in ("pos", "up", "forward", "right"):
        assert getattr(a, f).tup() == getattr(b, f).tup()
    R = oracle.ref_lib()
    if R is not None:
        c = _lib.Camera()
        R.ref_look_at(C.byref(c), eye, up, look)
        for f in ("pos", "up", "forward", "right"):
            assert getattr(a, f).tup() == getattr(c, f).tup()


def test_oracle_matches_reference_build_on_corner_meshes(ca, tmp_path):
    """The restatement against the reference's own headers (oracle/_ref) where the shortcuts of the HIP
    path are most exposed: duplicate and zero-area triangles, fudge 0 and negative."""
    import oracle
    from tests.util import mesh_scene, corner_meshes
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built (needs /root/reference at build time)")
    quad, dup, degenerate, fan, far = corner_meshes()
    for name, tris in (("dup", dup), ("degenerate", degenerate), ("fan", fan), ("far", far)):
        s = ca.HostScene.parse(mesh_scene(str(tmp_path / f"{name}.stl"), 48, 32, tris))
        assert s.ok
        for fudge in (1e-3, 0.0, -0.5):
            o = oracle.oracle_render(s, bounces=3, fudge=fudge, threads=os.cpu_count() or 2)
            r = oracle.ref_render(s, bounces=3, fudge=fudge, threads=os.cpu_count() or 2)
            for k in ("depth", "normal", "color", "hit_id"):
                assert np.array_equal(o[k].view(np.uint32) if o[k].dtype == np.float32 else o[k],
                                      r[k].view(np.uint32) if r[k].dtype == np.float32 else r[k]), (name, fudge, k)
            assert o["ray_count"] == r["ray_count"]


def test_oracle_matches_c4_rows_fixture(ca, tmp_path):
    """C4 (4x4 bunny grid @4096x4096): whole rows rendered by the reference build (tests/golden/make_golden.py)."""
    from cutrace_amd import scenes
    g = np.load(os.path.join(GOLD, "rows_bunny_grid4x4_4096x4096_b5.npz"))
    s = ca.HostScene.load(scenes.make_bunny_grid(str(tmp_path)))
    assert s.ok and s.size == (4096, 4096)
    for y in [int(v) for v in g["rows"]][::3]:   # three of the eight rows keep this CPU test to seconds
        r = oracle.oracle_render(s, bounces=5, rows=(y, y + 1), threads=os.cpu_count() or 4)
        assert same_bits(r["depth"][0], g[f"depth_{y}"]) and same_bits(r["color"][0], g[f"color_{y}"])
        assert same_bits(r["normal"][0], g[f"normal_{y}"]) and r["ray_count"] == int(g[f"rays_{y}"])


def test_oracle_matches_mirror_depth8_full_fixture(ca):
    """C3 as BASELINE.json words it: mirror.json@1920x1080, bounces 8 (identical to bounces 5: SURVEY fact 9)."""
    g8 = np.load(os.path.join(GOLD, "full_mirror_1920x1080_b8.npz"))
    g5 = np.load(os.path.join(GOLD, "full_mirror_1920x1080_b5.npz"))
    assert int(g8["ray_count"]) == int(g5["ray_count"]) == 8712144
    assert np.array_equal(g8["sum_color"], g5["sum_color"]) and float(g8["sum_depth"]) == float(g5["sum_depth"])
    s = load_scene(ca, "mirror")
    rows = (0, 1080, 8, 5, 9)    # every 9th 8-row block: 120 rows, checked against the samples that fall into them
    r = oracle.oracle_render(s, bounces=8, rows=rows, threads=os.cpu_count() or 4)
    ys = [y for y in range(1080) if (y // 8) % 9 == 5]
    pos = {y: k for k, y in enumerate(ys)}
    idx = g8["sample_idx"]
    hit = 0
    for j, i in enumerate(idx):
        y, x = divmod(int(i), 1920)
        if y in pos:
            k = pos[y]
            assert r["depth"][k, x].view(np.uint32) == g8["depth"][j].view(np.uint32)
            assert same_bits(r["color"][k, x], g8["color"][j]) and same_bits(r["normal"][k, x], g8["normal"][j])
            hit += 1
    assert hit > 300


def test_cuda_minmax_semantics_gap(ca):
    """DIAGNOSTIC: the reference build with fminf/fmaxf semantics for the device code's
    unqualified min/max (what nvcc binds) against the parity target (std::min/max selects).  The shipped configs
    must not depend on the difference; scripts/cuda_minmax_gap.py reports the full-size counts
    (profiles/r02/cuda_minmax_gap.txt)."""
    if oracle.ref_lib() is None or oracle.ref_cudaminmax_lib() is None:
        pytest.skip("oracle/_ref flavours not built here (need /root/reference)")
    for name, w, h, b in (("bunny", 96, 54, 5), ("mirror", 96, 54, 8), ("sphere_plane", 96, 54, 5), ("triangle", 64, 64, 5)):
        s = load_scene(ca, name, w, h)
        a = oracle.ref_render(s, bounces=b, threads=4)
        c = oracle.ref_cudaminmax_render(s, bounces=b, threads=4)
        for k in ("depth", "normal", "color"):
            assert same_bits(a[k], c[k]), (name, k)
        assert a["ray_count"] == c["ray_count"]


def test_fma_contraction_gap_is_small_but_not_zero(ca):
    """DIAGNOSTIC: the reference headers compiled with contraction allowed (what nvcc's default
    --fmad=true does in its own way) against the parity target.  Most pixels change in some bit, nearly none by more than
    the 1e-4 colour bar: a CUDA binary cannot be matched bit for bit by ANY host definition, and the bar holds away from
    silhouettes.  scripts/cuda_fmad_gap.py reports the larger sizes (profiles/r03/cuda_fmad_gap.txt)."""
    if oracle.ref_lib() is None or oracle.ref_fmad_lib() is None:
        pytest.skip("oracle/_ref flavours not built here (need /root/reference)")
    for name, w, h, b in (("bunny", 96, 54, 5), ("mirror", 96, 54, 8)):
        s = load_scene(ca, name, w, h)
        a = oracle.ref_render(s, bounces=b, threads=4)
        c = oracle.ref_fmad_render(s, bounces=b, threads=4)
        assert not same_bits(a["color"], c["color"]), name          # the flavour really contracts
        assert np.abs(a["color"].astype(np.float64) - c["color"]).max() < 1e-4, name
        fin = np.isfinite(a["depth"])
        assert (np.isfinite(c["depth"]) == fin).all()
        assert np.abs(a["depth"][fin].astype(np.float64) - c["depth"][fin]).max() < 1e-4


UV_FIXTURES = [("triangle", 20, 20), ("sphere_plane", 96, 54), ("bunny", 96, 54)]


@pytest.mark.parametrize("name,w,h", UV_FIXTURES)
def test_oracle_texture_coordinates_match_reference_fixture(ca, name, w, h):
    """ray_cast's tex_coords of the primary hit (triangle::uv_for, plane::uv_for, the sphere's atan2 / asin, a mesh's
    (hit.x, hit.y): default_schema.hpp:37-46,138-139,169-178,246-249): the C restatement against buffers the reference
    build wrote (tests/golden/make_golden.py --uv-only), bit for bit, NaNs included (a plane whose normal has no x and y
    normalises a zero vector, :170)."""
    g = np.load(os.path.join(GOLD, f"uv_{name}_{w}x{h}.npz"))
    s = ca.HostScene.load(f"scene/{name}.json")
    s.set_size(w, h)
    r = oracle.oracle_render(s, bounces=0, threads=4, uv=True)
    assert np.array_equal(r["uv"].view(np.uint32), g["uv"].view(np.uint32))
    assert np.array_equal(r["hit_id"], g["hit_id"])
    ref = oracle.ref_lib()
    if ref is not None and hasattr(ref, "ref_render_uv"):
        live = oracle.ref_render(s, bounces=0, threads=4, uv=True)
        assert np.array_equal(live["uv"].view(np.uint32), g["uv"].view(np.uint32))


def test_oracle_ignore_transparent_matches_reference_fixture(ca):
    """ray_cast's ninth argument (inc/ray_cast.hpp:30,39-40: objects with a transparent material are skipped) — the one
    branch of SURVEY §8(a) without a restatement until round 4, because no caller of the reference passes true.  The oracle's
    kernel.hpp:52 cast with the flag set, against a fixture the reference build produced the same way (its harness calls the
    reference's ray_cast with `true`; tests/golden/make_golden.py), and live against that build where it exists.
    sphere_plane.json holds a transparent sphere: the primary hit changes in hundreds of pixels, the colour in none
    (ray_color makes its own casts, with false: shading.hpp:32,123)."""
    g = np.load(os.path.join(GOLD, "ignore_transparent_sphere_plane_96x54_b5.npz"))
    s = load_scene(ca, "sphere_plane", 96, 54)
    r = oracle.oracle_render(s, bounces=5, threads=4, uv=True, ignore_transparent_primary=True)
    plain = oracle.oracle_render(s, bounces=5, threads=4)
    for k in ("depth", "normal", "color", "uv"):
        assert same_bits(r[k], g[k]), k
    assert np.array_equal(r["hit_id"], g["hit_id"]) and r["ray_count"] == int(g["ray_count"]) == plain["ray_count"]
    assert int((r["hit_id"] != plain["hit_id"]).sum()) > 300 and same_bits(r["color"], plain["color"])
    if oracle.ref_lib() is not None:
        live = oracle.ref_render(s, bounces=5, threads=4, uv=True, ignore_transparent_primary=True)
        for k in ("depth", "normal", "color", "uv"):
            assert same_bits(r[k], live[k]), k


def test_oracle_ignore_transparent_full_resolution_samples(ca):
    """The same branch at BASELINE's full size: sphere_plane.json @1920x1080, the kernel.hpp:52 cast with ignore_transparent = true — 4096 sampled
    pixels and the checksums of a frame the reference build rendered (its ray_cast called with `true`)."""
    g = np.load(os.path.join(GOLD, "full_ignore_transparent_sphere_plane_1920x1080_b5.npz"))
    s = load_scene(ca, "sphere_plane")
    r = oracle.oracle_render(s, bounces=5, threads=os.cpu_count() or 4, uv=True, ignore_transparent_primary=True)
    idx = g["sample_idx"]
    for k, n in (("depth", 1), ("color", 3), ("normal", 3), ("uv", 2)):
        assert same_bits(r[k].reshape(-1, n)[idx] if n > 1 else r[k].reshape(-1)[idx], g[k]), k
    assert r["ray_count"] == int(g["ray_count"]) == 13973091 and int(np.isfinite(r["depth"]).sum()) == int(g["n_finite"])
