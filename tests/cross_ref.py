"""NumPy restatement of include/cutrace_inside.h (TEST INFRASTRUCTURE): the crossing count and the signed count of a ray over an
open interval, and the vote of R rays that decides whether a point is inside — built on tests/ray_ref.py's float32 primitives
(det3, tri_intersect, the plane's t0, sphere_intersect's two roots), one numpy operation per reference operation.  Each term is
decided by its primitive alone, so this is a plain sum over the objects; no box, no tree.  Also the float64 winding number the
CPU test holds it against.  `scene` is a ray_ref.RefScene, or anything with its `objects` and `tris`."""
import numpy as np

from tests.ray_ref import (INF, OBJ_MESH, OBJ_PLANE, OBJ_SPHERE, OBJ_TRIANGLE, det3, plane_intersect, tri_intersect, vdot, vnormalized,
                           vsub)

f32, f64 = np.float32, np.float64


def _between(t, lo, hi):
    """finite and inside the OPEN interval"""
    return np.isfinite(t) & (t > lo) & (t < hi)


def tri_terms(tris, start, dirs, min_t, max_t, ray_chunk=1024, tri_chunk=1024):
    """(count, signed) per ray over the triangles `tris` (m, 3, 3): triangle::intersect accepts it and min_t < t0 < max_t;
    +1 where alpha = det[a b d] < 0, else -1"""
    n = len(start)
    cnt, sgn = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r0 in range(0, n, ray_chunk):
        s, d = start[r0:r0 + ray_chunk, None, :], dirs[r0:r0 + ray_chunk, None, :]
        lo, hi = min_t[r0:r0 + ray_chunk, None], max_t[r0:r0 + ray_chunk, None]
        for k0 in range(0, len(tris), tri_chunk):
            tc = tris[k0:k0 + tri_chunk]
            p1, p2, p3 = tc[None, :, 0], tc[None, :, 1], tc[None, :, 2]
            ok, t0 = tri_intersect(p1, p2, p3, s, d, lo)
            hit = ok & _between(t0, lo, hi)
            shape = np.broadcast_shapes(vsub(p2, p1).shape, d.shape)
            alpha = det3(np.broadcast_to(vsub(p2, p1), shape), np.broadcast_to(vsub(p2, p3), shape), np.broadcast_to(d, shape))
            cnt[r0:r0 + ray_chunk] += hit.sum(1)
            sgn[r0:r0 + ray_chunk] += np.where(hit, np.where(alpha < 0, 1, -1), 0).sum(1)
    return cnt, sgn


def sphere_roots(o, start, dirs):
    """sphere::intersect's t0 = (dec - sqrt) / dd and t1 = (dec + sqrt) / dd (ray_ref.sphere_intersect's arithmetic)"""
    d = vnormalized(dirs)
    c = np.broadcast_to(o["v0"], start.shape)
    R = o["f0"]
    dec = -vdot(d, vsub(start, c))
    sub = dec * dec - vdot(d, d) * (vdot(vsub(start, c), vsub(start, c)) - R * R)
    return (dec - np.sqrt(sub)) / vdot(d, d), (dec + np.sqrt(sub)) / vdot(d, d)


def count_crossings(scene, start, dirs, min_t=0.0, max_t=np.inf, object=None, skip_planes=False, skip_triangles=False, solids=False):
    """dict(count, signed), int64 per ray.  solids: meshes and spheres only (what ctr_inside_points counts)."""
    start = np.ascontiguousarray(start, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    n = len(start)
    min_t = np.broadcast_to(np.asarray(min_t, f32), (n,)).astype(f32)
    max_t = np.broadcast_to(np.asarray(max_t, f32), (n,)).astype(f32)
    cnt, sgn = np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for i, o in enumerate(scene.objects):
            if object is not None and i != object:
                continue
            if o["type"] == OBJ_PLANE:
                if skip_planes or solids:
                    continue
                _, t0 = plane_intersect(o, start, dirs, min_t)
                hit = _between(t0, min_t, max_t)
                c, s = hit.astype(np.int64), np.where(hit, np.where(vdot(dirs, np.broadcast_to(o["v1"], dirs.shape)) > 0, 1, -1), 0)
            elif o["type"] == OBJ_SPHERE:
                t0, t1 = sphere_roots(o, start, dirs)
                h0, h1 = _between(t0, min_t, max_t), _between(t1, min_t, max_t)
                c, s = h0.astype(np.int64) + h1, h1.astype(np.int64) - h0
            elif o["type"] == OBJ_TRIANGLE:
                if skip_triangles or solids:
                    continue
                c, s = tri_terms(np.stack([o["v0"], o["v1"], o["v2"]])[None], start, dirs, min_t, max_t)
            else:
                assert o["type"] == OBJ_MESH
                c, s = tri_terms(scene.tris[o["tri_begin"]:o["tri_begin"] + o["tri_count"]], start, dirs, min_t, max_t)
            cnt += c
            sgn += s
    # a ray that is not one counts nothing
    dead = ~np.isfinite(start).all(1) | ~np.isfinite(dirs).all(1) | (dirs == 0).all(1)
    cnt[dead] = 0
    sgn[dead] = 0
    return dict(count=cnt, signed=sgn)


def inside(scene, points, dirs, object=None):
    """dict(inside, votes, count, signed): the vote of the R rays (p, dirs[r]) over (0, +inf) on meshes and spheres; count and
    signed are (R, n), every ray's own answer.  A point that is not finite gets no votes."""
    points = np.ascontiguousarray(points, f32)
    dirs = np.asarray(dirs, f32).reshape(-1, 3)
    R = len(dirs)
    assert R % 2 == 1
    rays = [count_crossings(scene, points, np.broadcast_to(d, points.shape), f32(0), INF, object=object, solids=True) for d in dirs]
    count, signed = np.stack([r["count"] for r in rays]), np.stack([r["signed"] for r in rays])
    votes = (count & 1).sum(0)
    return dict(inside=2 * votes > R, votes=votes.astype(np.uint8), count=count, signed=signed)


def winding_number(tris, points, chunk=512):
    """The float64 winding number of the triangle soup `tris` (m, 3, 3) about every point: the sum of the triangles' signed solid
    angles (van Oosterom and Strackee) over 4 pi, rounded to an integer.  +1 inside a closed surface whose normals
    (p2 - p1) x (p3 - p1) point outwards — the normal ctr_cast_rays reports."""
    t = np.asarray(tris, f64)
    out = np.empty(len(points), np.int64)
    for r0 in range(0, len(points), chunk):
        p = np.asarray(points[r0:r0 + chunk], f64)[:, None, :]
        a, b, c = t[None, :, 0] - p, t[None, :, 1] - p, t[None, :, 2] - p
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = np.einsum("nmi,nmi->nm", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("nmi,nmi->nm", a, b) * lc + np.einsum("nmi,nmi->nm", b, c) * la + np.einsum("nmi,nmi->nm", c, a) * lb
        out[r0:r0 + chunk] = np.rint((2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)).astype(np.int64)
    return out


def box_points(tris, n, seed):
    """n uniform points in the triangles' box widened by 10 % per side"""
    v = np.asarray(tris, f64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    pad = 0.1 * (hi - lo)
    return np.random.default_rng(seed).uniform(lo - pad, hi + pad, (n, 3)).astype(f32)


OFFSETS = (1e-2, -1e-2, 1e-3, -1e-3, 1e-4, -1e-4, 1e-5, -1e-5)


def centroid_points(tris):
    """every triangle's centroid pushed by each of OFFSETS along its normal (p2 - p1) x (p3 - p1), offset-major"""
    t = np.asarray(tris, f64)
    c = t.mean(1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([c + e * nrm for e in OFFSETS]).astype(f32)
