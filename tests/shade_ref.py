"""NumPy restatement of the reference's phong and ray_color, vectorised over rays (TEST INFRASTRUCTURE).

On top of tests/ray_ref.py's ray_cast and shadow_intensity; mirrors oracle/ctr_oracle.c's phong and ray_color
(inc/shading.hpp:64-99, 116-154) in float32 with the C file's operation order: every constant is an np.float32, nothing is
promoted to double except where the reference computes in double (the comparisons with 1e-6, the shadow loop's step).
The specular pow is computed in float64 and rounded once.  The checker of tests/test_gpu_shade.py; pinned against the C
oracle by tests/test_shade_cpu.py.
"""
import numpy as np

from tests import ray_ref
from tests.ray_ref import INF, M1, ONE, TWO, f32, smax, vadd, vdot, vnorm, vnormalized, vscale, vsub

LIGHT_SUN, LIGHT_POINT = 0, 1


class ShadeScene(ray_ref.RefScene):
    """RefScene plus what shading reads: the lights, the materials' Phong parameters, the camera's ambient factor."""

    def __init__(self, host_scene):
        super().__init__(host_scene)
        d = host_scene.desc.contents
        self.lights = [dict(type=int(d.lights[i].type), v=np.array(d.lights[i].v.tup(), f32),
                            color=np.array(d.lights[i].color.tup(), f32)) for i in range(d.n_lights)]
        m = [d.materials[k] for k in range(d.n_materials)]
        self.mat_color = np.array([x.color.tup() for x in m], f32).reshape(-1, 3)
        self.mat_specular = np.array([x.specular for x in m], f32)
        self.mat_reflexivity = np.array([x.reflexivity for x in m], f32)
        self.mat_phong_exp = np.array([x.phong_exp for x in m], f32)
        self.ambient = f32(d.cam.ambient)
        self.obj_mat = np.array([o["mat"] for o in self.objects], np.int64)


def vmul(a, b):
    return np.stack([a[..., 0] * b[..., 0], a[..., 1] * b[..., 1], a[..., 2] * b[..., 2]], -1)


def phong(sc, in_dirs, hit, obj, normal, ambient):
    """phong, shading.hpp:64-99, for rays that all hit: (n, 3) colours"""
    n = len(hit)
    mat = sc.obj_mat[obj]
    diffuse = sc.mat_color[mat]
    specular = vscale(diffuse, sc.mat_specular[mat])  # default_schema.hpp:328
    phong_exp = sc.mat_phong_exp[mat]
    final = vscale(diffuse, np.full(n, ambient, f32))
    nn = vnormalized(normal)
    in_dn = vnormalized(in_dirs)
    for l in sc.lights:
        if l["type"] == LIGHT_SUN:  # default_schema.hpp:280-283
            direction = np.broadcast_to(vscale(l["v"], M1), (n, 3)).astype(f32)
            distance = np.full(n, INF, f32)
        else:                       # default_schema.hpp:305-308
            diff = vsub(np.broadcast_to(l["v"], (n, 3)), hit)
            direction = vnormalized(diff)
            distance = vnorm(diff)
        nd = vnormalized(direction)
        light_dist = distance * vnorm(direction)
        color = np.broadcast_to(l["color"], (n, 3))
        shadow_fac = ray_ref.shadow_intensity(sc, hit, nd, light_dist)
        fd = smax(np.zeros(n, f32), vdot(nn, nd))
        ld = vmul(diffuse, color)
        h = vnormalized(vadd(vscale(in_dn, M1), nd))
        sx = smax(np.zeros(n, f32), vdot(nn, h))
        fs = np.power(sx.astype(np.float64), phong_exp.astype(np.float64)).astype(f32)  # f64, rounded once
        ls = vmul(specular, color)
        term = vscale(vadd(vscale(ld, fd), vscale(ls, fs)), ONE - shadow_fac)
        lit = shadow_fac < ONE
        final = np.where(lit[:, None], vadd(final, term), final).astype(f32)
    return final


def _ray_color(sc, start, dirs, min_t, ambient, bounces):
    n = len(start)
    rgb = np.zeros((n, 3), f32)  # shading.hpp:119
    r = ray_ref.ray_cast(sc, start, dirs, min_t)
    idx = np.nonzero(r["object"] >= 0)[0]
    if len(idx):
        s, d, t, ob = start[idx], dirs[idx], r["t"][idx], r["object"][idx]
        hit, normal = r["point"][idx], r["normal"][idx]
        c = phong(sc, d, hit, ob, normal, ambient)
        if bounces != 0:
            mat = sc.obj_mat[ob]
            reflective, translucent = sc.mat_reflexivity[mat], sc.transparency[mat]
            child_start = vadd(s, vscale(d, t))  # incoming->start + distance * incoming->dir (a sphere's t too)
            m = reflective.astype(np.float64) >= 1e-6
            if m.any():
                nd, nn = vnormalized(d[m]), vnormalized(normal[m])
                refl = vsub(nd, vscale(nn, TWO * vdot(nn, nd)))  # vector.hpp:204-206
                r_rgb = _ray_color(sc, child_start[m], refl.astype(f32), min_t, ambient, bounces - 1)[0]
                c[m] = vadd(c[m], vscale(r_rgb, reflective[m]))
            m = translucent.astype(np.float64) >= 1e-6
            if m.any():
                t_rgb = _ray_color(sc, child_start[m], d[m], min_t, ambient, bounces - 1)[0]
                c[m] = vadd(vscale(c[m], ONE - translucent[m]), vscale(t_rgb, translucent[m]))
        rgb[idx] = c
    return rgb, r


def ray_color(sc, start, dirs, min_t=1e-3, ambient=None, bounces=5):
    """ray_color<S, bounces>, shading.hpp:116-154, for every ray: dict of color (n, 3) and the first cast's t (+inf on a
    miss), object (-1), normal (zeros)."""
    start = np.ascontiguousarray(start, f32)
    dirs = np.ascontiguousarray(dirs, f32)
    ambient = sc.ambient if ambient is None else f32(ambient)
    with np.errstate(all="ignore"):
        rgb, r = _ray_color(sc, start, dirs, f32(min_t), ambient, int(bounces))
    return dict(color=rgb, t=r["t"], object=r["object"], normal=r["normal"])
