"""The display quantisation of include/cutrace_images.h restated in numpy, float32 step by step, and the inputs the CPU and GPU
tests share.

quantise_depth / _normal / _color follow host/images.cpp:181-209 (the reference's inc/images.hpp:27-29,48-54,73-76): every
operation rounded once to float32, the threshold 1e-6 compared in double, the conversion to a byte truncating.  Outside the
host's contract (a float outside [0, 256)) they saturate as the header documents: clamped to [0, 255], NaN gives 0.

`fused=True` evaluates the same rule as a compiler that contracts a product into the sum it feeds would: each fused
multiply-add is simulated in float64: the product of two float32 values is exact there, the sum is rounded to float64 and
then to float32.  That is two roundings where the hardware makes one; they differ only when the float64 sum lands on a
float32 tie, which is rare, and the simulation only SELECTS inputs — the test asserts plain != fused on what was selected.
  normal  len^2 = fma(z, z, fma(x, x, y*y)); the later 0.5f + 0.5f * a is the same with or without fusion (0.5f * a is exact)
  depth   255 * (max - v) / max has no product that feeds a sum or a difference: there is nothing to contract, and the fused
          evaluation IS the plain one
  colour  255 * c: nothing to contract either
make_contraction_fixture() selects inputs whose bytes differ between the two evaluations (tests/golden/images_contraction.npz).
"""
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images_contraction.npz")
MAX_EXPONENTS = (-20, -12, 0, 12, 24)   # the scaled-scene range of tests/test_gpu_render_ranges.py (util.SCALE_EXPONENTS)


def to_byte(v):
    """clamp to [0, 255] (NaN fails the first comparison: 0), truncate"""
    with np.errstate(invalid="ignore"):
        lo = np.where(v > f32(0), v, f32(0)).astype(f32)
        c = np.where(lo < f32(255), lo, f32(255)).astype(f32)
    return c.astype(np.int32).astype(np.uint8)


def quantise_depth(depth, max_d):
    v = np.ascontiguousarray(depth, f32).reshape(-1)
    m = f32(max_d)
    with np.errstate(all="ignore"):
        t = (m - v).astype(f32)
        p = (f32(255) * t).astype(f32)
        q = (p / m).astype(f32)
        b = np.where(np.isfinite(v), to_byte(q), np.uint8(0)).astype(np.uint8)
    return np.repeat(b[:, None], 3, 1)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def quantise_normal(normal3, fused=False):
    n = np.ascontiguousarray(normal3, f32).reshape(-1, 3)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        if fused:
            s = _fma(z, z, _fma(x, x, (y * y).astype(f32)))
        else:
            s = (((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)
        ln = np.sqrt(s).astype(f32)
        zero = ln.astype(np.float64) <= 1e-6
        f = (f32(1) / ln).astype(f32)
        out = np.zeros((n.shape[0], 3), np.uint8)
        for k in range(3):
            a = (f * n[:, k]).astype(f32)
            h = (f32(0.5) * a).astype(f32)
            m = (f32(0.5) + h).astype(f32)
            out[:, k] = to_byte((f32(255) * m).astype(f32))
    out[zero] = 0
    return out


def quantise_color(color3):
    v = np.ascontiguousarray(color3, f32).reshape(-1)
    with np.errstate(invalid="ignore"):
        lo = np.where(f32(0) < v, v, f32(0)).astype(f32)
        c = np.where(lo < f32(1), lo, f32(1)).astype(f32)
    return to_byte((f32(255) * c).astype(f32)).reshape(-1, 3)


# ---- the inputs of tests/test_images_cpu.py and tests/test_gpu_images.py: all inside the host quantisers' contract ----
def _ulps(v, steps):
    """v and its neighbours `steps` floats away"""
    v = np.asarray(v, f32)
    out = [v]
    for direction in (-np.inf, np.inf):
        w = v
        for _ in range(steps):
            w = np.nextafter(w, f32(direction))
            out.append(w)
    return np.concatenate([np.atleast_1d(a) for a in out]).astype(f32)


def color_cases():
    """0, 1, -0.0, every k/255 and its two neighbours, NaN, +-inf, values above 1 and below 0; a multiple of 3 values"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(f32)
    v = np.concatenate([_ulps(k, 1), np.array([0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, 1.5, 2.0, 255.0, 256.0, 1e30, 3.4e38,
                                               -1e-30, -0.5, -1.0, -300.0, -3.4e38, 1e-45, -1e-45], f32)])
    return np.resize(v, (v.size + 2) // 3 * 3).reshape(-1, 3).copy()


def depth_cases():
    """[(max, depths)]: depths 0 and max, the depths at which 255*(max-v)/max sits within an ulp (here: two floats of v
    either side) of each integer 0..255, and +inf — for max = 2^e over MAX_EXPONENTS and a max that is no power of two"""
    out = []
    for m in [f32(2.0) ** f32(e) for e in MAX_EXPONENTS] + [f32(3.7), f32(1234.567), f32(2.0 ** 24 - 1)]:
        k = np.arange(256, dtype=np.float64)
        v = _ulps((np.float64(m) * (1.0 - k / 255.0)).astype(f32), 2)
        v = v[(v >= 0) & (v <= m)]
        out.append((float(m), np.concatenate([v, np.array([0.0, m, np.inf], f32)]).astype(f32)))
    return out


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def normal_cases(seed=11):
    """lengths around 1e-6 (the float below it, the float above it, exactly zero, 1e-7 .. 1e-5), unit normals, lengths up to
    2^20, the axis normals"""
    rng = np.random.RandomState(seed)
    e6 = f32(1e-6)
    edge = [np.nextafter(e6, f32(0)), e6, np.nextafter(e6, f32(1)), f32(0)]
    rows = []
    for L in edge:   # along each axis (the length is |L| up to the rounding of L*L) and along a diagonal
        for a in range(3):
            for sgn in (1, -1):
                r = np.zeros(3, f32)
                r[a] = sgn * L
                rows.append(r)
        rows.append(np.full(3, L / f32(np.sqrt(3.0)), f32))
    rows = [np.array(rows, f32)]
    rows.append((_directions(rng, 600) * np.logspace(-7, -5, 600)[:, None]).astype(f32))
    rows.append((_directions(rng, 400) * (1e-6 * (1 + rng.uniform(-1e-6, 1e-6, 400)))[:, None]).astype(f32))
    rows.append(_directions(rng, 1500).astype(f32))
    rows.append((_directions(rng, 600) * (2.0 ** rng.uniform(-10, 20, 600))[:, None]).astype(f32))
    rows.append(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32))
    return np.concatenate(rows).astype(f32)


def random_pixels(n, seed=5, max_d=37.5):
    """n in-contract pixels: depths in [0, max] with misses (+inf), colours around [0, 1], normals of mixed lengths and zeros"""
    rng = np.random.RandomState(seed)
    depth = (rng.uniform(0, 1, n) * max_d).astype(f32)
    depth = np.minimum(depth, f32(max_d))
    depth[rng.uniform(size=n) < 0.1] = np.inf
    color = rng.uniform(-0.2, 1.3, (n, 3)).astype(f32)
    normal = (_directions(rng, n) * (2.0 ** rng.uniform(-2, 2, n))[:, None]).astype(f32)
    normal[rng.uniform(size=n) < 0.1] = 0
    return depth, color, normal, f32(max_d)


# ---- inputs on which a contracted evaluation gives other bytes ----
def make_contraction_fixture(seed=3, want=96):
    """Normals whose byte differs between the plain and the fused evaluation.  Search: for random y, z and each byte boundary
    k (the component value g = 2k/255 - 1 at which 255*(0.5+0.5*g) is the integer k), x is solved from x / len = g and
    the 17 floats around it are tried; a candidate is kept where any of its three bytes differs.  Depth and colour: the
    rules have no product feeding a sum, a contracted evaluation cannot differ (module docstring) — nothing to search."""
    rng = np.random.RandomState(seed)
    found = []
    while sum(len(a) for a in found) < want:
        m = 20000
        y = rng.uniform(-1, 1, m)
        z = rng.uniform(-1, 1, m)
        g = 2.0 * rng.randint(1, 255, m) / 255.0 - 1.0
        x0 = (g * np.sqrt((y * y + z * z) / (1.0 - g * g))).astype(f32)
        for step in range(-8, 9):
            x = x0
            for _ in range(abs(step)):
                x = np.nextafter(x, f32(np.inf if step > 0 else -np.inf))
            n = np.stack([x, y.astype(f32), z.astype(f32)], 1).astype(f32)
            keep = (quantise_normal(n) != quantise_normal(n, fused=True)).any(1)
            found.append(n[keep])
    return np.concatenate(found)[:want].astype(f32)


def write_contraction_fixture(path=GOLDEN):
    np.savez(path, normal=make_contraction_fixture())


def contraction_fixture():
    return np.load(GOLDEN)["normal"].astype(f32)


if __name__ == "__main__":
    write_contraction_fixture()
    print(contraction_fixture().shape)
