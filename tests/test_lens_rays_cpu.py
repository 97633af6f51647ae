"""The ray frames of tests/lens_rays.py on the CPU (no GPU): the reference alone stands on them, they show what they are
for, and the permutations and masks are what they claim.  Conditions on the inputs of tests/test_gpu_lens_rays.py, not on
the kernel.

Measured here (24 x 16 = 384 rays, scrambled from RandomState(1), aimed with seed 4, far from the same RandomState
continued), random3 / random5: scrambled rays that hit something 309 / 305, that hit the 800-triangle mesh 17 / 20; aimed rays
that hit the mesh 123 / 178; far rays that hit the mesh, R = 8: 86 / 126, R = 64: 48 / 71, R = 4096: 36 / 70.  The floors
below sit about 20 % under the lowest count of a kind, so that a change of seeds keeps them meaningful."""
import numpy as np
import pytest

from cutrace_amd import lenses
from tests import lens_rays, ray_ref
from tests.lens_rays import FAR_RADII, ONE_LANE, far, inverse, permuted, repeated, shuffle, sparse, sparse_patterns, tile_lane, tile_transpose
from tests.util import same_bits

f32 = np.float32
W, H, BOUNCES = 24, 16, 5


def mesh_hits(sc, cast):
    mesh = [i for i, ob in enumerate(sc.objects) if ob["type"] == ray_ref.OBJ_MESH]
    assert len(mesh) == 1 and sc.objects[mesh[0]]["tri_count"] == 800
    return int(np.isin(cast["object"], mesh).sum())


@pytest.mark.parametrize("name", ["random3", "random5"])
def test_the_reference_stands_on_the_frames(ca, name):
    _, sc, frames = lens_rays.reference(ca, name, W, H, BOUNCES)
    assert list(frames) == ["scrambled", "aimed"] + [f"far {R}" for R in FAR_RADII]
    for fam, fr in frames.items():
        assert fr["o"].shape == fr["d"].shape == (H, W, 3) and fr["o"].dtype == fr["d"].dtype == f32
        assert fr["keep"].all() and not lenses.is_masked(fr["o"], fr["d"]).any(), fam   # no ray is masked
        assert not np.isnan(fr["ref"]["color"]).any(), fam
        assert same_bits(fr["cast"]["t"], fr["ref"]["t"]) and same_bits(fr["cast"]["normal"], fr["ref"]["normal"]), fam
        print(f"{name} {fam}: {int((fr['cast']['object'] >= 0).sum())} of {H * W} rays hit something, {mesh_hits(sc, fr['cast'])} the mesh")
    # the frames show what they are for
    s = frames["scrambled"]
    assert int((s["cast"]["object"] >= 0).sum()) >= 250
    assert mesh_hits(sc, s["cast"]) >= 12
    assert mesh_hits(sc, frames["aimed"]["cast"]) >= 100
    for R in FAR_RADII:
        assert mesh_hits(sc, frames[f"far {R}"]["cast"]) >= 30, R
    # every tile of `scrambled` holds directions from all eight sign octants, and zero components of either sign occur
    tile, _ = tile_lane(W, H)
    octant = (np.signbit(s["d"]) * np.array([1, 2, 4])).sum(-1)
    for t in range(tile.max() + 1):
        assert len(np.unique(octant[tile == t])) == 8, t
    zero = s["d"] == 0
    assert (zero & np.signbit(s["d"])).any() and (zero & ~np.signbit(s["d"])).any()
    # origins inside a sphere and inside the mesh box
    o = s["o"].reshape(-1, 3)
    sph = [ob for ob in sc.objects if ob["type"] == ray_ref.OBJ_SPHERE]
    assert any((np.linalg.norm(o - ob["v0"], axis=1) < ob["f0"]).any() for ob in sph)
    lo, hi = lens_rays.far_box(sc)
    assert ((o >= lo) & (o <= hi)).all(-1).sum() >= H * W // 10
    # aimed: every ray without a zero component passes a mesh vertex within rounding of its length
    a = frames["aimed"]
    verts = sc.tris.reshape(-1, 3).astype(np.float64)
    of, df = a["of"].astype(np.float64), a["df"].astype(np.float64)
    nz = (a["d"].reshape(-1, 3) != 0).all(-1)
    assert nz.sum() > H * W * 3 // 4
    rel = verts[None] - of[nz, None]
    off = np.linalg.norm(np.cross(rel, df[nz, None]), axis=-1).min(1)    # distance of the nearest vertex from the ray's line
    assert (off <= 1e-5).all(), float(off.max())
    # far: the origins lie R box sizes from the box's centre
    ext, c = float((hi - lo).max()), (lo + hi) / 2
    for R in FAR_RADII:
        r = np.linalg.norm(frames[f"far {R}"]["o"].reshape(-1, 3) - c, axis=1)
        assert np.allclose(r, R * ext, rtol=1e-5), R


def test_far_without_a_mesh_aims_at_the_first_sphere(ca):
    s = lens_rays.host_scene(ca, "hall", W, H)
    lo, hi = lens_rays.far_box(s)
    assert np.allclose(hi - lo, 1.2) and np.allclose((lo + hi) / 2, [0.2, -0.3, 0.0])
    o, d = far(s, W, H, 2, 64)
    sphere = ray_ref.RefScene(s).objects[3]
    assert sphere["type"] == ray_ref.OBJ_SPHERE
    with np.errstate(all="ignore"):
        ok, _ = ray_ref.sphere_intersect(sphere, o.reshape(-1, 3), lens_rays.normalised(d.reshape(-1, 3)), f32(1e-3))
    assert int(ok.sum()) >= H * W // 3   # the sphere fills about half of its cube's silhouette (the walls are met first: the origins lie outside the hall)


def test_permutations():
    rng = np.random.RandomState(0)
    for w, h in ((24, 16), (21, 13), (40, 24)):
        o, d = rng.normal(size=(h, w, 3)).astype(f32), rng.normal(size=(h, w, 3)).astype(f32)
        perms = [shuffle(w, h, 7)] + ([tile_transpose(w, h)] if w % 8 == 0 and h % 8 == 0 else [])
        for perm in perms:
            assert np.array_equal(np.sort(perm), np.arange(h * w)) and not np.array_equal(perm, np.arange(h * w))
            po, pd = permuted(o, d, perm)
            assert same_bits(po.reshape(-1, 3)[perm], o.reshape(-1, 3)) and not same_bits(po, o)
            bo, bd = permuted(po, pd, inverse(perm))
            assert same_bits(bo, o) and same_bits(bd, d)
            got = lens_rays.unpermuted(dict(depth=po[..., 0], normal=po, color=pd), perm)
            assert same_bits(got["depth"], o[..., 0]) and same_bits(got["normal"], o) and same_bits(got["color"], d)


def source_tiles_per_wave(w, h):
    tile, _ = tile_lane(w, h)
    src = np.empty(h * w, np.int64)
    src[tile_transpose(w, h)] = tile.reshape(-1)       # the source tile of every destination pixel
    return [np.unique(src[tile.reshape(-1) == t]) for t in range(tile.max() + 1)]


def test_tile_transpose():
    # 64 tiles: lane k of tile t goes to lane t of tile k, and a destination tile holds one lane of each of 64 source tiles
    w = h = 64
    tile, ln = tile_lane(w, h)
    perm = tile_transpose(w, h)
    assert np.array_equal(tile.reshape(-1)[perm], ln.reshape(-1)) and np.array_equal(ln.reshape(-1)[perm], tile.reshape(-1))
    assert all(len(u) == 64 for u in source_tiles_per_wave(w, h))
    assert np.array_equal(inverse(perm), perm)
    # fewer tiles: every destination tile holds lanes of every tile of the frame
    for w, h, n in ((24, 16, 6), (32, 24, 12), (40, 24, 15)):
        assert all(len(u) == n for u in source_tiles_per_wave(w, h)), (w, h)


def test_block_perm():
    w, h, s = 5, 3, 2
    perm = shuffle(w, h, 1)
    big = lens_rays.block_perm(perm, w, h, s)
    assert np.array_equal(np.sort(big), np.arange(s * s * w * h))
    Y, X = np.meshgrid(np.arange(s * h), np.arange(s * w), indexing="ij")
    Y, X = Y.reshape(-1), X.reshape(-1)
    assert np.array_equal(big // (s * w) // s * w + big % (s * w) // s, perm[(Y // s) * w + X // s])   # the block moves as its pixel
    assert np.array_equal(big // (s * w) % s, Y % s) and np.array_equal(big % (s * w) % s, X % s)      # and keeps its inside


def test_sparse_patterns_and_repeated():
    rng = np.random.RandomState(0)
    for w, h in ((24, 16), (40, 24), (21, 13)):
        full = w % 8 == 0 and h % 8 == 0
        tile, ln = tile_lane(w, h)
        n_tiles = tile.max() + 1
        size = np.bincount(tile.reshape(-1), minlength=n_tiles)
        pats = sparse_patterns(w, h)
        assert list(pats) == ["checkerboard"] + [f"lane {k}" for k in ONE_LANE] + ["one row", "one column"]
        live = {k: np.bincount(tile.reshape(-1), weights=keep.reshape(-1), minlength=n_tiles).astype(int) for k, keep in pats.items()}
        cb = live["checkerboard"]
        assert ((cb == 0) | (cb == size)).all() and (cb == 0).any() and (cb == size).any()
        tiles_x = (w + 7) // 8
        for t in range(n_tiles - 1):
            if (t + 1) % tiles_x:
                assert (cb[t] == 0) != (cb[t + 1] == 0)     # an all-masked tile next to a full one
        for k in ONE_LANE:
            assert (live[f"lane {k}"] == 1).all() if full else ((live[f"lane {k}"] <= 1).all() and live[f"lane {k}"].any())
            assert (ln[pats[f"lane {k}"]] == k).all()
        for name in ("one row", "one column"):
            assert (live[name] == 8).all() if full else ((live[name] <= 8).all() and live[name].any())
        assert all(len(np.unique(ln[pats["one row"] & (tile == t)] // 8)) <= 1 for t in range(n_tiles))
        assert all(len(np.unique(ln[pats["one column"] & (tile == t)] % 8)) <= 1 for t in range(n_tiles))
        o, d = rng.normal(size=(h, w, 3)).astype(f32), rng.normal(size=(h, w, 3)).astype(f32)
        for name, keep in pats.items():
            so, sd = sparse(o, d, keep)
            assert np.array_equal(lenses.is_masked(so, sd), ~keep), name
            assert same_bits(sd[keep], d[keep]) and same_bits(so, o)
            assert same_bits(sd[~keep], np.broadcast_to(np.array([0.0, -0.0, 0.0], f32), sd[~keep].shape))
        ro, rd = repeated(o, d)
        for t in range(n_tiles):
            m = tile == t
            first = np.argmax(m.reshape(-1))            # the tile's top left pixel
            assert (ln.reshape(-1)[first] == 0)
            assert same_bits(ro[m], np.broadcast_to(o.reshape(-1, 3)[first], ro[m].shape))
            assert same_bits(rd[m], np.broadcast_to(d.reshape(-1, 3)[first], rd[m].shape))
