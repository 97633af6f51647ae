"""NumPy restatement of cutrace_amd/csrc/nearest_point.h (TEST INFRASTRUCTURE): the candidate of a triangle, a sphere and a plane for
a query point, operation for operation in float32 — every constant an np.float32, one operation per ufunc, no fused multiply-add;
np_dop's float64 difference of products as the header defines it — vectorised over points and triangles, and the answer of
ctr_nearest_points as the linear minimum of (d2, object index) over ray_ref.RefScene's objects, inside a mesh of (d2, file
index).  The checker of tests/test_gpu_nearest.py; tests/test_nearest_cpu.py pins it against a float64 brute force."""
import numpy as np

from tests import ray_ref
from tests.ray_ref import OBJ_PLANE, OBJ_SPHERE, OBJ_TRIANGLE, f32

INF = f32(np.inf)
ZERO, ONE = f32(0.0), f32(1.0)
OUTPUTS = ("distance", "object", "prim", "point", "normal")


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _dop(a, b, c, d):
    """np_dop: (float)((double)a * b - (double)c * d)"""
    a, b, c, d = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c, d))
    return (a * b - c * d).astype(f32)


def triangle(a, b, A, p):
    """np_triangle for records (a, b, A), each (m, 3), and points p (n, 3): (d2 (n, m), q (n, m, 3))."""
    ab, ac = -a[None], -b[None]
    abx, aby, abz = ab[..., 0], ab[..., 1], ab[..., 2]
    acx, acy, acz = ac[..., 0], ac[..., 1], ac[..., 2]
    Ax, Ay, Az = A[None, :, 0], A[None, :, 1], A[None, :, 2]
    px, py, pz = p[:, None, 0], p[:, None, 1], p[:, None, 2]
    apx, apy, apz = px - Ax, py - Ay, pz - Az
    aa = _dot(abx, aby, abz, abx, aby, abz)
    cc = _dot(acx, acy, acz, acx, acy, acz)
    d1 = _dot(abx, aby, abz, apx, apy, apz)
    d2 = _dot(acx, acy, acz, apx, apy, apz)
    d3, d6 = d1 - aa, d2 - cc
    cx, cy, cz = acx - abx, acy - aby, acz - abz
    bpx, bpy, bpz = apx - abx, apy - aby, apz - abz
    e1 = (cx * bpx + cy * bpy) + cz * bpz
    e2 = (cx * (acx - apx) + cy * (acy - apy)) + cz * (acz - apz)
    nx, ny, nz = _dop(aby, acz, abz, acy), _dop(abz, acx, abx, acz), _dop(abx, acy, aby, acx)
    vc = ((ny * abz - nz * aby) * apx + (nz * abx - nx * abz) * apy) + (nx * aby - ny * abx) * apz
    vb = ((acy * nz - acz * ny) * apx + (acz * nx - acx * nz) * apy) + (acx * ny - acy * nx) * apz
    va = ((ny * cz - nz * cy) * bpx + (nz * cx - nx * cz) * bpy) + (nx * cy - ny * cx) * bpz
    # the regions in the header's order: the first that holds decides
    r_a = (d1 <= 0) & (d2 <= 0)
    r_b = (d3 >= 0) & (e1 <= 0)
    r_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    r_c = (d6 >= 0) & (e2 <= 0)
    r_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    r_bc = (va <= 0) & (e1 >= 0) & (e2 >= 0)
    w_bc = e1 / (e1 + e2)
    conds = [r_a, r_b, r_ab, r_c, r_ac, r_bc]
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    v = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, ONE - w_bc], zero)
    w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w_bc], zero)
    face = ~(r_a | r_b | r_ab | r_c | r_ac | r_bc)
    tx, ty, tz = v * abx + w * acx, v * aby + w * acy, v * abz + w * acz
    rx, ry, rz = apx - tx, apy - ty, apz - tz
    d2_edge = (rx * rx + ry * ry) + rz * rz
    f = ONE / np.sqrt((nx * nx + ny * ny) + nz * nz)
    hx, hy, hz = nx * f, ny * f, nz * f
    s = (apx * hx + apy * hy) + apz * hz
    out_d2 = np.where(face, s * s, d2_edge)
    q = np.stack([np.where(face, px - s * hx, Ax + tx), np.where(face, py - s * hy, Ay + ty), np.where(face, pz - s * hz, Az + tz)], -1)
    return out_d2.astype(f32), q.astype(f32)


def records(tris):
    """(a, b, A) of file triangles (m, 3, 3), as tri_record.h make_tri stores them: a = p2 - p1, b = p2 - p3, A = p2"""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    return tris[:, 1] - tris[:, 0], tris[:, 1] - tris[:, 2], tris[:, 1].copy()


def sphere(c, R, p):
    """np_sphere: (d2 (n,), q (n, 3))"""
    v = p - c[None]
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    r = -R if R < 0 else R
    s = ln - r
    k = r / ln
    q = np.where((ln == 0)[:, None], (c + np.array([r, ZERO, ZERO], f32))[None], c[None] + v * k[:, None])
    return (s * s).astype(f32), q.astype(f32)


def plane(p0, n, p):
    """np_plane: (d2 (n,), q (n, 3))"""
    f = ONE / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    h = n * f
    s = ((p[:, 0] - p0[0]) * h[0] + (p[:, 1] - p0[1]) * h[1]) + (p[:, 2] - p0[2]) * h[2]
    return (s * s).astype(f32), (p - s[:, None] * h[None]).astype(f32)


def mesh(tris, p, chunk=256):
    """the minimum of (d2, file index) over the finite candidates of one mesh: (d2 (n,) — +inf: none —, k (n,), q (n, 3))"""
    a, b, A = records(tris)
    n = len(p)
    best, win, q = np.full(n, INF, f32), np.full(n, -1, np.int64), np.zeros((n, 3), f32)
    for r0 in range(0, n, chunk):
        d2, qq = triangle(a, b, A, p[r0:r0 + chunk])
        d2 = np.where(d2 < INF, d2, INF)   # a NaN is no candidate
        k = np.argmin(d2, axis=1)          # the first index reaching the minimum: the lower file index on ties
        rows = np.arange(len(k))
        best[r0:r0 + chunk], q[r0:r0 + chunk] = d2[rows, k], qq[rows, k]
        win[r0:r0 + chunk] = np.where(d2[rows, k] < INF, k, -1)
    return best, win, q


def nearest_points(scene, points, max_dist=INF, object=None, skip_planes=False):
    """ctr_nearest_points on a ray_ref.RefScene: dict of distance (+inf on a miss), object (-1), prim (-1), point, normal (zeros)."""
    p = np.ascontiguousarray(points, f32)
    n = len(p)
    md = np.broadcast_to(np.asarray(max_dist, f32), (n,)).astype(f32)
    with np.errstate(all="ignore"):
        live = (md >= 0) & np.isfinite(p).all(axis=1)
        best = np.where(live, md * md, f32(np.nan)).astype(f32)
        obj = np.full(n, -1, np.int64)
        prim = np.full(n, -1, np.int64)
        point = np.zeros((n, 3), f32)
        normal = np.zeros((n, 3), f32)
        for i, o in enumerate(scene.objects):
            if (object is not None and i != object) or (skip_planes and o["type"] == OBJ_PLANE):
                continue
            k = None
            if o["type"] == OBJ_TRIANGLE:
                a, b, A = records(np.stack([o["v0"], o["v1"], o["v2"]]))
                d2, q = triangle(a, b, A, p)
                d2, q = d2[:, 0], q[:, 0]
                nrm = np.broadcast_to(ray_ref.tri_normal(o["v0"], o["v1"], o["v2"]), (n, 3))
            elif o["type"] == OBJ_PLANE:
                d2, q = plane(o["v0"], o["v1"], p)
                nrm = np.broadcast_to(o["v1"], (n, 3))
            elif o["type"] == OBJ_SPHERE:
                d2, q = sphere(o["v0"], o["f0"], p)
                nrm = ray_ref.vnormalized(ray_ref.vsub(q, np.broadcast_to(o["v0"], (n, 3))))
            else:
                if not o["tri_count"]:
                    continue
                tr = scene.tris[o["tri_begin"]:o["tri_begin"] + o["tri_count"]]
                d2, k, q = mesh(tr, p)
                w = tr[np.maximum(k, 0)]
                nrm = ray_ref.tri_normal(w[:, 0], w[:, 1], w[:, 2])
            # the candidate counts: finite, within the limit; the first object in scene order keeps a tie
            upd = (d2 < INF) & ((d2 < best) | ((d2 == best) & (obj == -1)))
            best[upd] = d2[upd]
            obj[upd] = i
            prim[upd] = k[upd] if k is not None else -1
            point[upd] = q[upd]
            normal[upd] = nrm[upd]
        distance = np.where(obj >= 0, np.sqrt(best), INF).astype(f32)
    return dict(distance=distance, object=obj, prim=prim, point=point, normal=normal)
