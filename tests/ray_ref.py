"""NumPy restatement of the reference's ray_cast and shadow_intensity, vectorised over rays (TEST INFRASTRUCTURE).

It mirrors oracle/ctr_oracle.c function by function (tri_intersect, bound_intersects, mesh_intersect, plane_intersect,
sphere_intersect, ray_cast, shadow_intensity, uv_of_hit, cam_get_ray) in float32 with the C file's operation order: every
constant is an np.float32 and no Python float takes part in an operation, so nothing is promoted to double except
where the reference itself computes in double (the shadow loop's step, the transparency test).  numpy evaluates one
operation per ufunc, so there is no fused multiply-add.  The checker of tests/test_gpu_rays.py; pinned against the C
oracle by tests/test_rays_cpu.py.
"""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
ZERO, HALF, ONE, TWO, M1 = f32(0.0), f32(0.5), f32(1.0), f32(2.0), f32(-1.0)
PI = f32(np.pi)
NONE = -1
OBJ_TRIANGLE, OBJ_MESH, OBJ_PLANE, OBJ_SPHERE = 0, 1, 2, 3


# ---- inc/vector.hpp (oracle lines 35-67); vectors are (..., 3) arrays ----
def vadd(a, b):
    return np.stack([a[..., 0] + b[..., 0], a[..., 1] + b[..., 1], a[..., 2] + b[..., 2]], -1)


def vsub(a, b):
    return np.stack([a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]], -1)


def vscale(a, f):
    f = np.asarray(f, f32)[..., None]
    return f * a


def vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vcross(a, o):
    return np.stack([a[..., 1] * o[..., 2] - a[..., 2] * o[..., 1], a[..., 2] * o[..., 0] - a[..., 0] * o[..., 2],
                     a[..., 0] * o[..., 1] - a[..., 1] * o[..., 0]], -1)


def vnorm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def vnormalized(a):
    return vscale(a, ONE / vnorm(a))


def det3(c0, c1, c2):
    """vector.hpp:218-224, columns c0, c1, c2: a*e*i + b*f*g + c*d*h - c*e*g - a*f*h - b*d*i, left to right"""
    a, b, c = c0[..., 0], c1[..., 0], c2[..., 0]
    d, e, f = c0[..., 1], c1[..., 1], c2[..., 1]
    g, h, i = c0[..., 2], c1[..., 2], c2[..., 2]
    return a * e * i + b * f * g + c * d * h - c * e * g - a * f * h - b * d * i


def smin(a, b):
    return np.where(b < a, b, a)


def smax(a, b):
    return np.where(a < b, b, a)


class RefScene:
    """The description's arrays (ctr_scene_desc) as numpy: objects in scene order, triangles, materials."""

    def __init__(self, host_scene):
        d = host_scene.desc.contents
        self.objects = []
        for i in range(d.n_objects):
            o = d.objects[i]
            self.objects.append(dict(type=int(o.type), mat=int(o.mat_idx), v0=np.array(o.v0.tup(), f32),
                                     v1=np.array(o.v1.tup(), f32), v2=np.array(o.v2.tup(), f32), f0=f32(o.f0),
                                     tri_begin=int(o.tri_begin), tri_count=int(o.tri_count)))
        n = d.n_triangles
        tr = np.zeros((n, 3, 3), f32)
        for k in range(n):
            t = d.triangles[k]
            tr[k] = [t.p1.tup(), t.p2.tup(), t.p3.tup()]
        self.tris = tr
        self.transparency = np.array([d.materials[m].transparency for m in range(d.n_materials)], f32)
        c = d.cam
        self.cam = dict(pos=np.array(c.pos.tup(), f32), up=np.array(c.up.tup(), f32), forward=np.array(c.forward.tup(), f32),
                        right=np.array(c.right.tup(), f32), w=int(c.w), h=int(c.h))

    def transparent(self, i):
        """material::is_transparent (default_schema.hpp:334): transparency >= 1e-6, a double comparison"""
        return float(np.float64(self.transparency[self.objects[i]["mat"]])) >= 1e-6


def camera_rays(cam):
    """cam::get_ray (oracle cam_get_ray, default_schema.hpp:376-386) for every pixel, row-major: (origins, dirs)."""
    w, h = cam["w"], cam["h"]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = x.reshape(-1).astype(f32), y.reshape(-1).astype(f32)
    aspect = f32(w) / f32(h)
    x_v = vscale(np.broadcast_to(cam["right"], (x.size, 3)), ((x / f32(w)) - HALF) * aspect)
    y_v = vscale(np.broadcast_to(cam["up"], (x.size, 3)), HALF - (y / f32(h)))
    d = vnormalized(vadd(vadd(x_v, y_v), np.broadcast_to(cam["forward"], (x.size, 3))))
    return np.broadcast_to(cam["pos"], (x.size, 3)).astype(f32), d.astype(f32)


# ---- inc/default_schema.hpp primitives (oracle lines 83-163), for rays (n, 3) and one object ----
def tri_intersect(p1, p2, p3, start, dirs, min_t):
    """(ok, t0) of triangle::intersect; p1..p3 broadcast against the rays ((3,) or (n, m, 3) ...)."""
    a, b, c, d = vsub(p2, p1), vsub(p2, p3), dirs, vsub(p2, start)
    a, b = np.broadcast_to(a, d.shape), np.broadcast_to(b, d.shape)
    alpha = det3(a, b, c)
    beta = det3(d, b, c) / alpha
    gamma = det3(a, d, c) / alpha
    t0 = det3(a, b, d) / alpha
    ok = (beta >= 0) & (gamma >= 0) & (beta + gamma <= 1) & np.isfinite(t0) & (min_t <= t0)
    return ok, t0


def tri_normal(p1, p2, p3):
    """default_schema.hpp:72: -1 * normalize((p2 - p3) x (p1 - p3))"""
    return vscale(vnormalized(vcross(vsub(p2, p3), vsub(p1, p3))), M1)


def bound_intersects(bmin, bmax, start, dirs):
    """mesh::bound_intersects, default_schema.hpp:99-114 (tmin starts at 0, IEEE reciprocals, std::min/max)"""
    tmin = np.zeros(len(start), f32)
    tmax = np.full(len(start), INF, f32)
    r_inv = ONE / dirs
    for q in range(3):
        t1 = (bmin[q] - start[:, q]) * r_inv[:, q]
        t2 = (bmax[q] - start[:, q]) * r_inv[:, q]
        tmin = smin(smax(t1, tmin), smax(t2, tmin))
        tmax = smax(smin(t1, tmax), smin(t2, tmax))
    return tmin <= tmax


def mesh_intersect(tris, start, dirs, min_t, ray_chunk=2048, tri_chunk=2048):
    """mesh::intersect without its box test (default_schema.hpp:127-143): the smallest valid t over the triangles, the
    first in file order on ties (strict <).  Returns (ok, dist, k) per ray; k is the winner's file index (last_tri)."""
    n = len(start)
    dist = np.full(n, INF, f32)
    win = np.full(n, NONE, np.int64)
    for r0 in range(0, n, ray_chunk):
        s, dd, mt = start[r0:r0 + ray_chunk, None, :], dirs[r0:r0 + ray_chunk, None, :], min_t[r0:r0 + ray_chunk, None]
        best = dist[r0:r0 + ray_chunk]
        bk = win[r0:r0 + ray_chunk]
        for t0_ in range(0, len(tris), tri_chunk):
            tc = tris[t0_:t0_ + tri_chunk]
            ok, t = tri_intersect(tc[None, :, 0], tc[None, :, 1], tc[None, :, 2], s, dd, mt)
            t = np.where(ok, t, INF)
            m = t.min(axis=1)
            k = np.argmin(t, axis=1)  # the first index reaching the minimum: file order on ties
            upd = m < best            # strict: an earlier chunk keeps a tie
            best[upd] = m[upd]
            bk[upd] = t0_ + k[upd]
    return dist != INF, dist, win


def plane_intersect(o, start, dirs, min_t):
    """plane::intersect, default_schema.hpp:189-201"""
    t0 = vdot(vsub(o["v0"], start), np.broadcast_to(o["v1"], start.shape)) / vdot(dirs, np.broadcast_to(o["v1"], dirs.shape))
    return np.isfinite(t0) & (min_t <= t0), t0


def sphere_intersect(o, start, dirs, min_t):
    """sphere::intersect, default_schema.hpp:226-251: t along the NORMALISED direction"""
    d = vnormalized(dirs)
    c = np.broadcast_to(o["v0"], start.shape)
    R = o["f0"]
    dec = -vdot(d, vsub(start, c))
    sub = dec * dec - vdot(d, d) * (vdot(vsub(start, c), vsub(start, c)) - R * R)
    t0 = (dec - np.sqrt(sub)) / vdot(d, d)
    t1 = (dec + np.sqrt(sub)) / vdot(d, d)
    t0v = np.isfinite(t0) & (min_t <= t0)
    t1v = np.isfinite(t1) & (min_t <= t1)
    dist = np.where(t0v & t1v, smin(t0, t1), np.where(t0v, t0, t1))
    return t0v | t1v, dist


def ray_cast(scene, start, dirs, min_t, ignore_transparent=False):
    """ray_cast, ray_cast.hpp:29-55 (oracle lines 176-205), for every ray: dict of t (+inf on a miss), object (-1),
    prim (winning triangle of a mesh hit, -1 otherwise), point, normal, uv (zeros on a miss)."""
    start = np.ascontiguousarray(start, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    n = len(start)
    min_t = np.broadcast_to(np.asarray(min_t, f32), (n,)).astype(f32)
    with np.errstate(all="ignore"):
        dist_best = np.full(n, INF, f32)
        obj = np.full(n, NONE, np.int64)
        prim = np.full(n, NONE, np.int64)
        for i, o in enumerate(scene.objects):
            if ignore_transparent and scene.transparent(i):
                continue
            k = None
            if o["type"] == OBJ_TRIANGLE:
                ok, d = tri_intersect(o["v0"], o["v1"], o["v2"], start, dirs, min_t)
            elif o["type"] == OBJ_PLANE:
                ok, d = plane_intersect(o, start, dirs, min_t)
            elif o["type"] == OBJ_SPHERE:
                ok, d = sphere_intersect(o, start, dirs, min_t)
            else:
                ok = np.zeros(n, bool)
                d = np.full(n, INF, f32)
                k = np.full(n, NONE, np.int64)
                box = bound_intersects(o["v0"], o["v1"], start, dirs) if o["tri_count"] else np.zeros(n, bool)
                if box.any():
                    tris = scene.tris[o["tri_begin"]:o["tri_begin"] + o["tri_count"]]
                    ok[box], d[box], k[box] = mesh_intersect(tris, start[box], dirs[box], min_t[box])
            # ray_cast.hpp:43: strict >, strict < (the first object in scene order keeps a tie)
            upd = ok & (d > min_t) & (d < dist_best)
            dist_best[upd] = d[upd]
            obj[upd] = i
            prim[upd] = k[upd] if k is not None else NONE
        point, normal, uv = hit_record(scene, start, dirs, dist_best, obj, prim)
    return dict(t=dist_best, object=obj, prim=prim, point=point, normal=normal, uv=uv)


def hit_record(scene, start, dirs, dist, obj, prim):
    """The hit point and normal ray_cast returns and the texture coordinates of the hit (oracle uv_of_hit)."""
    n = len(start)
    point = np.zeros((n, 3), f32)
    normal = np.zeros((n, 3), f32)
    uv = np.zeros((n, 2), f32)
    for i in np.unique(obj[obj >= 0]):
        o = scene.objects[int(i)]
        m = obj == i
        s, d, t = start[m], dirs[m], dist[m]
        if o["type"] == OBJ_SPHERE:
            hit = vadd(s, vscale(vnormalized(d), t))
            nrm = vnormalized(vsub(hit, o["v0"]))
            delta = vnormalized(vsub(hit, o["v0"]))
            u = HALF + (np.arctan2(delta[:, 2], delta[:, 0]) / (TWO * PI))
            v = HALF + (np.arcsin(delta[:, 1]) / PI)
        else:
            hit = vadd(s, vscale(d, t))
            if o["type"] == OBJ_PLANE:
                nrm = np.broadcast_to(o["v1"], hit.shape)
                nv = o["v1"]
                ax1 = vnormalized(np.array([nv[1], -nv[0], ZERO], f32))
                ax2 = vcross(nv, ax1)
                mod_pt = vsub(o["v0"], hit)
                u = vdot(np.broadcast_to(ax1, hit.shape), mod_pt)
                v = vdot(np.broadcast_to(ax2, hit.shape), mod_pt)
            elif o["type"] == OBJ_MESH:
                tr = scene.tris[o["tri_begin"] + prim[m]]
                nrm = tri_normal(tr[:, 0], tr[:, 1], tr[:, 2])
                u, v = hit[:, 0], hit[:, 1]
            else:
                nrm = np.broadcast_to(tri_normal(o["v0"], o["v1"], o["v2"]), hit.shape)
                p2p1, p3p1, xp1 = vsub(o["v1"], o["v0"]), vsub(o["v2"], o["v0"]), vsub(hit, o["v0"])
                p2p1b, p3p1b = np.broadcast_to(p2p1, hit.shape), np.broadcast_to(p3p1, hit.shape)
                proj_u = vscale(p2p1b, vdot(xp1, p2p1b) / vdot(p2p1, p2p1))
                proj_v = vscale(p3p1b, vdot(xp1, p3p1b) / vdot(p3p1, p3p1))
                u = vnorm(proj_u) / vnorm(p2p1)
                v = vnorm(proj_v) / vnorm(p3p1)
        point[m] = hit
        normal[m] = nrm
        uv[m, 0] = u
        uv[m, 1] = v
    return point, normal, uv


def shadow_intensity(scene, start, dirs, max_t):
    """shadow_intensity, shading.hpp:22-45 (oracle lines 208-224): nearest casts from min_dist = (float)(last_hit + 1e-3)
    (a double add narrowed), 1 - transparency per hit below max_t in hit order, 1 once the sum reaches 1."""
    start = np.ascontiguousarray(start, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    n = len(start)
    max_t = np.broadcast_to(np.asarray(max_t, f32), (n,)).astype(f32)
    intensity = np.zeros(n, f32)
    last_hit = np.zeros(n, f32)
    live = np.ones(n, bool)
    with np.errstate(all="ignore"):
        while live.any():
            idx = np.nonzero(live)[0]
            mn = (last_hit[idx].astype(np.float64) + 1e-3).astype(f32)
            r = ray_cast(scene, start[idx], dirs[idx], mn)
            go = (r["object"] >= 0) & (r["t"] < max_t[idx])
            live[idx[~go]] = False
            idx, t, ob = idx[go], r["t"][go], r["object"][go]
            trans = np.array([scene.transparency[scene.objects[int(i)]["mat"]] for i in ob], f32)
            intensity[idx] = intensity[idx] + (ONE - trans)
            full = intensity[idx] >= ONE
            intensity[idx[full]] = ONE
            live[idx[full]] = False
            last_hit[idx] = t
    return intensity
