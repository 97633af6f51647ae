"""The checker of the surface shading queries (ctr_shade_points): tests/shade_ref.py's phong driven by material indices
instead of objects, plus the per-light matrix of tests/ray_ref.py's shadow_intensity (TEST INFRASTRUCTURE).

No arithmetic of its own: the colour IS shade_ref.phong, called on a view of the scene whose object -> material table is
the identity; the shadow matrix calls ray_ref.shadow_intensity with the shadow ray and max_dist that phong forms (its
lines, restated with ray_ref's vector functions).  Pinned against the C oracle by tests/test_points_cpu.py.
"""
import copy

import numpy as np

from tests import ray_ref, shade_ref
from tests.ray_ref import INF, M1, f32, vnorm, vnormalized, vscale, vsub


def by_material(sc):
    """`sc` (a shade_ref.ShadeScene) with "object" k standing for material k in phong's material lookup"""
    view = copy.copy(sc)
    view.obj_mat = np.arange(len(sc.mat_specular), dtype=np.int64)
    return view


def light_shadow(sc, points):
    """(n, n_lights): shadow_intensity towards every light as phong calls it (shade_ref.phong's lines 49-59)"""
    points = np.ascontiguousarray(points, f32)
    n = len(points)
    out = np.zeros((n, len(sc.lights)), f32)
    with np.errstate(all="ignore"):
        for j, l in enumerate(sc.lights):
            if l["type"] == shade_ref.LIGHT_SUN:
                direction = np.broadcast_to(vscale(l["v"], M1), (n, 3)).astype(f32)
                distance = np.full(n, INF, f32)
            else:
                diff = vsub(np.broadcast_to(l["v"], (n, 3)), points)
                direction = vnormalized(diff)
                distance = vnorm(diff)
            nd = vnormalized(direction)
            out[:, j] = ray_ref.shadow_intensity(sc, points, nd, distance * vnorm(direction))
    return out


def shade_points(sc, points, normals, view_dirs, materials, ambient=None):
    """phong at every point with the material index given per point (or one int for all): (n, 3) colours"""
    points = np.ascontiguousarray(points, f32)
    n = len(points)
    mat = np.broadcast_to(np.asarray(materials, np.int64), (n,))
    ambient = sc.ambient if ambient is None else f32(ambient)
    if n == 0:
        return np.zeros((0, 3), f32)
    with np.errstate(all="ignore"):
        return shade_ref.phong(by_material(sc), np.ascontiguousarray(view_dirs, f32), points, mat,
                               np.ascontiguousarray(normals, f32), ambient)


def primary_hits(sc):
    """The camera's rays and their first hits: (origins, dirs, ray_cast's dict, mask of the rays that hit)"""
    o, d = ray_ref.camera_rays(sc.cam)
    r = ray_ref.ray_cast(sc, o, d, f32(1e-3))
    return o, d, r, r["object"] >= 0


def oracle_hits(sc, frame):
    """The same from a frame of oracle_render(hit_ids=True) instead of a cast of ray_ref's (a mesh of a thousand triangles
    takes NumPy seconds): object, t and normal are the oracle's, the point is ray_ref.hit_record's (along dir / |dir| on a
    sphere, along dir elsewhere)."""
    o, d = ray_ref.camera_rays(sc.cam)
    obj = frame["hit_id"].reshape(-1).astype(np.int64)
    t = np.ascontiguousarray(frame["depth"].reshape(-1), f32)
    with np.errstate(all="ignore"):
        point, _, _ = ray_ref.hit_record(sc, o, d, t, obj, np.zeros(len(o), np.int64))
    r = dict(t=t, object=obj, point=point, normal=np.ascontiguousarray(frame["normal"].reshape(-1, 3), f32))
    return o, d, r, obj >= 0
