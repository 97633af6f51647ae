"""Ray frames for the lens render that no camera produces, and what the lens tests share (a support module: no test here).

The render kernel walks a mesh one wave per 8x8 tile, together: the visiting order comes from one lane, several shortcuts
are decided once per wave, and everything per ray is a 64-bit lane mask.  The frames here put rays into one wave that
share nothing: every direction octant, origins inside and outside spheres and mesh boxes, rays aimed at mesh vertices,
origins thousands of box sizes away, lanes without a ray.  tests/test_lens_rays_cpu.py proves on the CPU that the frames
are what they claim; tests/test_gpu_lens_rays.py renders them.

A frame is (origins, dirs), both (h, w, 3) float32, read as 8x8 tiles in row-major pixel order, as the kernel reads it:
pixel (x, y) is lane (y % 8) * 8 + x % 8 of tile (y // 8) * ceil(w / 8) + x // 8.  Directions are not normalised.

Also here, moved from tests/test_gpu_lens.py and tests/test_gpu_render_ranges.py: `normalised`, `frame_from_rays`, the frame
comparison `assert_frames`, `CastCounter`, and the small launch helpers of the lens tests."""
import numpy as np

from tests import ray_ref
from tests.util import TOL, _random_scene, hall_of_mirrors_json, random_rays, same_bits, sweep_rays

f32 = np.float32
TW = TH = 8          # the kernel's tile
FRAME = ("depth", "normal", "color")
FAR_RADII = (8, 64, 4096)


# ---- what the lens tests share ----
def normalised(d):
    with np.errstate(all="ignore"):
        return ray_ref.vnormalized(np.ascontiguousarray(d, f32)).astype(f32)


def frame_from_rays(h, w, keep, t, normal, color):
    """the frame of a per-ray result for the unmasked rays `keep` (flat bool): the miss values elsewhere"""
    depth = np.full(h * w, np.inf, f32)
    nrm = np.zeros((h * w, 3), f32)
    col = np.zeros((h * w, 3), f32)
    depth[keep], nrm[keep], col[keep] = t, normal, color
    return dict(depth=depth.reshape(h, w), normal=nrm.reshape(h, w, 3), color=col.reshape(h, w, 3))


def assert_frames(got, want, what, color="bits"):
    """depth and normal bit for bit; no NaN in the colour; the colour bit for bit ("bits") or within util.TOL ("tol").
    Every pixel is compared.  Returns the largest colour difference, which it also prints."""
    for k in ("depth", "normal"):
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words"
    diff = float(np.abs(got["color"].astype(np.float64) - want["color"].astype(np.float64)).max()) if got["color"].size else 0.0
    print(f"{what}: colour max|diff| {diff:.3e}")
    assert not np.isnan(got["color"]).any(), what
    if color == "bits":
        assert same_bits(got["color"], want["color"]), f"{what}: colour differs in {int((got['color'].view(np.uint32) != want['color'].view(np.uint32)).sum())} words, max {diff:.3e}"
    else:
        assert diff <= TOL, f"{what}: colour max|diff| {diff:.3e}"
    return diff


class CastCounter:
    """counts the rays of every ray_ref.ray_cast call: the casts of tests/shade_ref.py's ray_color"""

    def __init__(self, monkeypatch):
        self.n = 0
        real = ray_ref.ray_cast

        def counted(scene, start, dirs, *a, **kw):
            self.n += len(start)
            return real(scene, start, dirs, *a, **kw)

        monkeypatch.setattr(ray_ref, "ray_cast", counted)


def host_scene(ca, name, w, h):
    """"random<seed>", "hall", or a scene file's name"""
    from tests.conftest import load_scene
    if name.startswith("random"):
        s = ca.HostScene.parse(_random_scene(int(name[6:]), w, h))
    elif name == "hall":
        s = ca.HostScene.parse(hall_of_mirrors_json(w, h))
    else:
        s = load_scene(ca, name, w, h)
    assert s.ok, name
    return s


def cam_of(s):
    return s.desc.contents.cam


def max_depth_of(counters):
    return float(np.array([int(counters[1]) & 0xFFFFFFFF], np.uint32).view(f32)[0])


def largest_depth(depth):
    """max_depth as every render defines it: the largest finite positive depth, or 0"""
    fin = depth[np.isfinite(depth) & (depth > 0)]
    return float(fin.max()) if fin.size else 0.0


def plain_device(ds, b, rows=None):
    """ctr_render_device of the handle, as numpy: what render_lens is compared with"""
    import torch

    import cutrace_amd
    dev = torch.device("cuda", ds.device)
    n = cutrace_amd.rows_count(ds.h, rows)
    depth = torch.full((n, ds.w), -1.0, device=dev)
    color = torch.full((n, ds.w, 3), -1.0, device=dev)
    normal = torch.full((n, ds.w, 3), -1.0, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    ds.render_device(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), d_counters=counters.data_ptr(),
                     stream=torch.cuda.current_stream(dev).cuda_stream, bounces=b, rows=rows)
    torch.cuda.synchronize()
    c = counters.cpu()
    return dict(depth=depth.cpu().numpy(), color=color.cpu().numpy(), normal=normal.cpu().numpy(), ray_count=int(c[0]), max_depth=max_depth_of(c))


def lens(ds, o, d, **kw):
    r = ds.render_lens(o, d, **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


# ---- the ray frames ----
def _ref_scene(scene):
    return scene if isinstance(scene, ray_ref.RefScene) else ray_ref.RefScene(scene)


def _rng(seed):
    return seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)


def _frame(o, d, w, h):
    return np.ascontiguousarray(o, f32).reshape(h, w, 3), np.ascontiguousarray(d, f32).reshape(h, w, 3)


def scrambled(scene, w, h, seed):
    """util.random_rays with directions of length about 1, one per pixel in draw order: origins across the scene, inside
    spheres and inside mesh boxes, Gaussian directions, 10 % of them with an exact +-0 component.  seed: a number, or a
    RandomState that is drawn from and left where the draw ends."""
    o, d, _ = random_rays(_rng(seed), w * h, _ref_scene(scene), -3.0, 3.0, lengths=(1.0,))
    return _frame(o, d, w, h)


def aimed(scene, w, h, seed):
    """util.sweep_rays with aim = 1: every ray without a zero component points at a mesh vertex from a scattered origin"""
    o, d, _ = sweep_rays(seed, w * h, _ref_scene(scene), aim=1.0)
    return _frame(o, d, w, h)


def far_box(scene):
    """the box `far` aims at: the first mesh's, or — a scene without a mesh — the cube around its first sphere"""
    rs = _ref_scene(scene)
    for ob in rs.objects:
        if ob["type"] == ray_ref.OBJ_MESH and ob["tri_count"]:
            return ob["v0"].astype(np.float64), ob["v1"].astype(np.float64)
    for ob in rs.objects:
        if ob["type"] == ray_ref.OBJ_SPHERE:
            return ob["v0"].astype(np.float64) - float(ob["f0"]), ob["v0"].astype(np.float64) + float(ob["f0"])
    raise ValueError("far: the scene has neither a mesh nor a sphere")


def far(scene, w, h, seed, R):
    """origins uniform on the sphere of radius R x the box's largest extent around the box's centre, each ray aimed at a
    uniform point inside the box (far_box); the direction is target - origin in float32, R box sizes long"""
    rng = _rng(seed)
    lo, hi = far_box(scene)
    n = w * h
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = ((lo + hi) / 2 + u * (R * float((hi - lo).max()))).astype(f32)
    target = rng.uniform(lo, hi, (n, 3))
    d = (target - o.astype(np.float64)).astype(f32)
    return _frame(o, d, w, h)


# ---- tiles, lanes and permutations of the pixels ----
def tile_lane(w, h):
    """(tile, lane) of every pixel, each (h, w)"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (y // TH) * ((w + TW - 1) // TW) + x // TW, (y % TH) * TW + x % TW


def permuted(o, d, perm):
    """pixel perm[i] of the result holds ray i of the frame (pixels numbered row-major); perm: a permutation of range(h*w)"""
    perm = np.asarray(perm)
    n = o.shape[0] * o.shape[1]
    assert perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n)), "perm: a permutation of range(h*w)"
    po, pd = np.empty_like(o), np.empty_like(d)
    po.reshape(-1, 3)[perm] = o.reshape(-1, 3)
    pd.reshape(-1, 3)[perm] = d.reshape(-1, 3)
    return po, pd


def unpermuted(frame, perm):
    """the outputs of a frame rendered from `permuted` rays, back in the order of the rays before"""
    out = dict(frame)
    for k in FRAME:
        v = frame[k]
        out[k] = np.ascontiguousarray(v.reshape((v.shape[0] * v.shape[1],) + v.shape[2:])[perm].reshape(v.shape))
    return out


def inverse(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def shuffle(w, h, seed):
    return np.random.RandomState(seed).permutation(w * h)


def tile_transpose(w, h):
    """The "transpose of tiles" (w, h multiples of 8).  With T tiles, the pixels are a T x 64 array of (tile, lane); the
    permutation sends lane k of tile t to position k * T + t of that array read as one list, and so to lane
    (k * T + t) % 64 of tile (k * T + t) // 64.  With T = 64 this is lane t of tile k: every wave is then made of one lane
    from each of 64 different tiles.  With fewer tiles (a 40 x 24 frame has 15) consecutive lanes of a destination tile
    still come from consecutive source tiles: every wave holds lanes of every tile of the frame."""
    assert w % TW == 0 and h % TH == 0, "tile_transpose: whole tiles"
    tile, ln = tile_lane(w, h)
    T = (w // TW) * (h // TH)
    dest = (ln * T + tile).reshape(-1)                 # position in tile-major order
    dt, dl = dest // 64, dest % 64
    tiles_x = w // TW
    return ((dt // tiles_x) * TH + dl // TW) * w + (dt % tiles_x) * TW + dl % TW   # ... as a row-major pixel number


def block_perm(perm, w, h, s):
    """the permutation of the s*w x s*h sample frame (row-major) that moves each pixel's s x s block of samples together, as
    `perm` moves the pixels of the w x h frame"""
    Y, X = np.meshgrid(np.arange(s * h), np.arange(s * w), indexing="ij")
    dst = np.asarray(perm)[(Y // s) * w + X // s]
    return (((dst // w) * s + Y % s) * (s * w) + (dst % w) * s + X % s).reshape(-1)


# ---- frames with lanes that have no ray ----
def sparse(o, d, keep):
    """the frame masked down to `keep` ((h, w) bool): elsewhere the direction is (0, -0, 0), the header's "no ray here" """
    d = d.copy()
    d[~np.asarray(keep, bool)] = np.array([0.0, -0.0, 0.0], f32)
    return o.copy(), d


ONE_LANE = (0, 1, 31, 32, 63)


def sparse_patterns(w, h):
    """name -> keep (h, w): a checkerboard of whole tiles; tiles with exactly one live lane, at lane 0, 1, 31, 32 or 63;
    tiles whose only live lanes are one row (row t % 8 of tile t) or one column (column (t + 3) % 8).  In a partial tile
    at the frame's edge the chosen lane, row or column may lie outside the frame: that tile is then all masked."""
    tile, ln = tile_lane(w, h)
    tiles_x = (w + TW - 1) // TW
    out = {"checkerboard": ((tile // tiles_x + tile % tiles_x) % 2) == 0}
    for k in ONE_LANE:
        out[f"lane {k}"] = ln == k
    out["one row"] = ln // TW == tile % TH
    out["one column"] = ln % TW == (tile + 3) % TW
    return out


def repeated(o, d):
    """every lane of a tile carries the tile's first ray (its top left pixel): the fully coherent extreme, the control"""
    h, w = o.shape[:2]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    y0, x0 = (y // TH) * TH, (x // TW) * TW
    return np.ascontiguousarray(o[y0, x0]), np.ascontiguousarray(d[y0, x0])


# ---- the CPU reference of a frame on a random scene, computed once and left unchanged ----
_reference = {}


def family_frames(scene, w, h):
    """frames 1 to 3 of a scene, by name: scrambled from RandomState(1), aimed with seed 4, far for every R of FAR_RADII
    from the same RandomState continued"""
    rs = _ref_scene(scene)
    rng = np.random.RandomState(1)
    out = {"scrambled": scrambled(rs, w, h, rng), "aimed": aimed(rs, w, h, 4)}
    for R in FAR_RADII:
        out[f"far {R}"] = far(rs, w, h, rng, R)
    return out


def reference(ca, name, w, h, bounces=5):
    """{family: dict(o, d, keep, cast, ref)} of a random scene: tests/ray_ref.py's ray_cast and tests/shade_ref.py's
    ray_color on the normalised directions of the unmasked rays (all of them, in these families)"""
    from cutrace_amd import lenses
    from tests import shade_ref
    key = (name, w, h, bounces)
    if key not in _reference:
        s = host_scene(ca, name, w, h)
        sc = shade_ref.ShadeScene(s)
        out = {}
        for fam, (o, d) in family_frames(sc, w, h).items():
            keep = ~lenses.is_masked(o, d).reshape(-1)
            of, df = o.reshape(-1, 3)[keep], normalised(d.reshape(-1, 3)[keep])
            ref = shade_ref.ray_color(sc, of, df, min_t=1e-3, bounces=bounces)
            cast = ray_ref.ray_cast(sc, of, df, f32(1e-3))
            for a in (keep, *ref.values(), *cast.values()):   # (the rays stay writable: torch takes no read-only array)
                a.setflags(write=False)
            out[fam] = dict(o=o, d=d, keep=keep, of=of, df=df, cast=cast, ref=ref)
        _reference[key] = (s, sc, out)
    return _reference[key]
