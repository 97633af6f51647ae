"""The lens render on rays that share nothing (-m gpu): DeviceScene.render_lens on the frames of tests/lens_rays.py.

The render kernel walks a mesh one wave per 8x8 tile, together.  Node and triangle records are wave-uniform, the visiting
order comes from one lane, `have_rinv`, `axis_fast`, `skip_planes`, `first_trip` and the any-hit early exit are decided once
per wave, and everything per ray is a lane mask.  Every camera and every lens of cutrace_amd/lenses.py gives a tile 64 rays
of one octant, one origin (to within an aperture) and, mostly, one recursion depth.  Here a tile holds all eight octants,
origins inside and outside spheres and mesh boxes and up to 4096 box sizes away, rays aimed at mesh vertices, lanes at
different depths, and lanes with no ray at all.

Bar, as in tests/test_gpu_lens.py: depth and normal bit for bit; colour bit for bit under VAR_EXACT_POW and within util.TOL
under the default variant; masked pixels hold the miss values; no NaN.  Every pixel of every frame is compared.
a. frames 1 to 3 against tests/shade_ref.py and tests/ray_ref.py on the CPU (random scenes);
b. the same frames against ctr_shade_rays with the linear walk on the builds the random scenes do not reach;
c. permutation invariance: which rays share a wave changes no bit of any of them;
d. tiles with few live lanes, and tiles whose 64 lanes carry one ray.
tests/test_lens_rays_cpu.py proves on the CPU what the frames hold."""
import numpy as np
import pytest

from cutrace_amd import lenses
from tests import lens_rays, shade_ref
from tests.gpu_support import gpu  # noqa: F401  (the fixture)
from tests.lens_rays import (CastCounter, assert_frames, block_perm, cam_of, family_frames, frame_from_rays, host_scene, largest_depth, lens,
                             normalised, permuted, plain_device, repeated, shuffle, sparse, sparse_patterns, tile_transpose, unpermuted)
from tests.util import same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
KV_OCC6, KV_RAYS = 64, 4096
FRAME = ("depth", "normal", "color")


def as_numpy(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def assert_same_bits(got, want, what):
    for k in FRAME:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words of {got[k].size}"
    assert not np.isnan(got["color"]).any(), what


# ---- a. frames 1 to 3 against the CPU reference ----
@pytest.mark.parametrize("w,h", [(24, 16), (21, 13)])
@pytest.mark.parametrize("name", ["random3", "random5"])
def test_frames_against_shade_ref(gpu, name, w, h):
    b = 5
    s, _, frames = lens_rays.reference(gpu, name, w, h, b)
    ds = gpu.DeviceScene(s)
    for fam, fr in frames.items():
        what = f"{name} {w}x{h} {fam}"
        assert fr["keep"].all()
        want = frame_from_rays(h, w, fr["keep"], fr["cast"]["t"], fr["cast"]["normal"], fr["ref"]["color"])
        # the reference side does not depend on the walk for these rays: the BVH walk of the radiance query gives the linear one's bits
        kw = dict(bounces=b, exact_pow=True, outputs=("color", "t", "normal"))
        lin, bvh = as_numpy(ds.shade_rays(fr["of"], fr["df"], linear=True, **kw)), as_numpy(ds.shade_rays(fr["of"], fr["df"], linear=False, **kw))
        for k in ("color", "t", "normal"):
            assert same_bits(lin[k], bvh[k]), f"{what}: the radiance query's BVH walk differs from its linear walk in {k}"
        for var, color in ((0, "tol"), (gpu.VAR_EXACT_POW, "bits"), (gpu.VAR_NO_ANYHIT, "tol"), (gpu.VAR_NO_ANYHIT | gpu.VAR_EXACT_POW, "bits")):
            ds.set_variant(var)
            got = lens(ds, fr["o"], fr["d"], bounces=b)
            assert ds.last_kernel() & KV_RAYS
            assert_frames(got, want, f"{what} var={var}", color=color)
            assert got["max_depth"] == largest_depth(want["depth"]), (what, var)
    ds.close()


# ---- b. the same frames on the builds the random scenes do not reach ----
@pytest.mark.parametrize("name,w,h,b,families", [
    ("bunny", 40, 24, 5, ("scrambled", "far 64", "aimed")),     # the large mesh: the 6-wave build
    ("hall", 24, 16, 15, ("scrambled", "far 64")),              # lanes of one wave end at very different depths
    ("sphere_plane", 24, 16, 5, ("scrambled", "far 64"))])      # a transparent material: no any-hit, the pass-through continuation
def test_frames_against_the_linear_radiance_query(gpu, name, w, h, b, families):
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    frames = family_frames(s, w, h)
    for fam in families:
        o, d = frames[fam]
        assert not lenses.is_masked(o, d).any()
        keep = np.ones(h * w, bool)
        of, df = o.reshape(-1, 3), normalised(d.reshape(-1, 3))
        for exact in (False, True):
            what = f"{name} {fam} exact={exact}"
            ref = as_numpy(ds.shade_rays(of, df, bounces=b, exact_pow=exact, linear=True, outputs=("color", "t", "normal")))
            want = frame_from_rays(h, w, keep, ref["t"], ref["normal"], ref["color"])
            ds.set_variant(gpu.VAR_EXACT_POW if exact else 0)
            got = lens(ds, o, d, bounces=b)
            kv = ds.last_kernel()
            assert kv & KV_RAYS
            if name == "bunny" and not exact:
                assert kv & KV_OCC6
            assert_frames(got, want, what, color="bits" if exact else "tol")
            assert got["max_depth"] == largest_depth(want["depth"]), what
            assert np.isfinite(got["depth"]).sum() > h * w // 2, f"{what}: the frame sees too little"
    ds.close()


# ---- c. permutation invariance: results never depend on which rays share a wave ----
def base_rays(s, w, h, kind):
    return lenses.pinhole(cam_of(s), w, h) if kind == "pinhole" else lens_rays.scrambled(s, w, h, 1)


@pytest.mark.parametrize("name,w,h,b,kind", [
    ("bunny", 40, 24, 5, "pinhole"), ("mirror", 32, 24, 8, "pinhole"), ("hall", 24, 16, 15, "pinhole"), ("sphere_plane", 24, 16, 5, "pinhole"),
    ("random3", 24, 16, 5, "scrambled"),
    # the smallest frame with 64 tiles, where the tile transpose makes every wave of one lane from each of 64 tiles (no CPU
    # reference is computed for it: three launches of a few microseconds each)
    ("bunny", 64, 64, 5, "pinhole")])
def test_permuted_rays_give_the_permuted_frame(gpu, name, w, h, b, kind):
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = base_rays(s, w, h, kind)
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        base = lens(ds, o, d, bounces=b)
        assert ds.last_kernel() & KV_RAYS
        if kind == "pinhole":   # ... and the plain render: three launches then agree
            plain = plain_device(ds, b)
            assert_frames(base, plain, f"{name} var={var} pinhole against the plain render")
            assert base["ray_count"] == plain["ray_count"] and base["max_depth"] == plain["max_depth"], (name, var)
        assert np.isfinite(base["depth"]).sum() > h * w // 3   # (sphere_plane's camera sees sky in over half of its frame)
        for pname, perm in (("shuffle", shuffle(w, h, 11)), ("tile transpose", tile_transpose(w, h))):
            po, pd = permuted(o, d, perm)
            got = unpermuted(lens(ds, po, pd, bounces=b), perm)
            assert_same_bits(got, base, f"{name} {w}x{h} var={var} {pname}")
            assert got["ray_count"] == base["ray_count"] and got["max_depth"] == base["max_depth"], (name, var, pname)
    ds.close()


def test_permuted_pixels_of_a_sample_frame(gpu):
    """samples = 2: whole pixels are permuted, each pixel's 2x2 block of samples moving together; the reduced frame is the
    permuted reduced frame"""
    name, w, h, b, ss = "random5", 20, 12, 5, 2
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lenses.thin_lens(cam_of(s), w, h, ss, 0.15, 4.0, seed=5)
    perm = shuffle(w, h, 13)
    po, pd = permuted(o, d, block_perm(perm, w, h, ss))
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        base = lens(ds, o, d, bounces=b, samples=ss)
        assert base["depth"].shape == (h, w)
        got = unpermuted(lens(ds, po, pd, bounces=b, samples=ss), perm)
        assert_same_bits(got, base, f"samples=2 var={var}")
        assert got["ray_count"] == base["ray_count"] and got["max_depth"] == base["max_depth"], var
    ds.close()


def test_a_shuffled_frame_in_two_row_parts(gpu):
    name, w, h, b = "random3", 24, 16, 5
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = lens_rays.scrambled(s, w, h, 1)
    po, pd = permuted(o, d, shuffle(w, h, 11))
    whole = lens(ds, po, pd, bounces=b)
    out = {k: np.full_like(whole[k], -1.0) for k in FRAME}
    total = 0
    for part in range(2):
        r = lens(ds, po, pd, bounces=b, rows=(0, h, 2, part, 2))
        ys = [y for y in range(h) if (y // 2) % 2 == part]
        assert r["depth"].shape == (len(ys), w)
        for k in out:
            out[k][ys] = r[k]
        total += r["ray_count"]
    assert_same_bits(out, whole, "two row parts")
    assert total == whole["ray_count"]
    ds.close()


# ---- d. sparse and repeated tiles ----
@pytest.mark.parametrize("name,w,h,b,kind", [("random3", 24, 16, 5, "scrambled"), ("bunny", 40, 24, 5, "pinhole")])
def test_sparse_tiles(gpu, monkeypatch, name, w, h, b, kind):
    """ray_count (random3): the drop equals the cast count of tests/shade_ref.py's ray_color for the masked rays, plus the
    duplicated primary cast of each, as tests/test_gpu_lens.py test_masked_pixels counts"""
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = base_rays(s, w, h, kind)
    counted = name == "random3"
    if counted:
        sc = shade_ref.ShadeScene(s)
        counter = CastCounter(monkeypatch)
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        base = lens(ds, o, d, bounces=b)
        for pname, keep in sparse_patterns(w, h).items():
            what = f"{name} var={var} {pname}"
            so, sd = sparse(o, d, keep)
            assert np.array_equal(lenses.is_masked(so, sd), ~keep)
            got = lens(ds, so, sd, bounces=b)
            n_masked = int((~keep).sum())
            for k in FRAME:   # live pixels: the bits of the unmasked launch
                assert same_bits(got[k][keep], base[k][keep]), f"{what}: {k} of the live pixels"
            assert not np.isnan(got["color"]).any(), what
            assert (got["depth"][~keep] == np.inf).all(), what
            assert same_bits(got["normal"][~keep], np.zeros((n_masked, 3), f32)) and same_bits(got["color"][~keep], np.zeros((n_masked, 3), f32)), what
            assert got["max_depth"] == largest_depth(base["depth"][keep]), what
            if counted and var == 0:
                before = counter.n
                shade_ref.ray_color(sc, o[~keep], normalised(d[~keep]), min_t=1e-3, bounces=b)
                casts = counter.n - before
                print(f"{what}: ray_count {base['ray_count']} -> {got['ray_count']}, reference casts of the {n_masked} masked rays {casts} + {n_masked}")
                assert base["ray_count"] - got["ray_count"] == casts + n_masked, what
    ds.close()


@pytest.mark.parametrize("name,w,h,b,kind", [("random3", 24, 16, 5, "scrambled"), ("bunny", 40, 24, 5, "pinhole")])
def test_repeated_tiles(gpu, name, w, h, b, kind):
    s = host_scene(gpu, name, w, h)
    ds = gpu.DeviceScene(s)
    o, d = base_rays(s, w, h, kind)
    ro, rd = repeated(o, d)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    y0, x0 = (y // 8) * 8, (x // 8) * 8
    for var in (0, gpu.VAR_EXACT_POW):
        ds.set_variant(var)
        base = lens(ds, o, d, bounces=b)
        got = lens(ds, ro, rd, bounces=b)
        # all 64 pixels of a tile hold the bits of the pixel that carried the tile's ray in the base frame
        want = {k: np.ascontiguousarray(base[k][y0, x0]) for k in FRAME}
        assert_same_bits(got, want, f"{name} var={var} repeated")
        assert got["max_depth"] == largest_depth(want["depth"])
    ds.close()
