"""Ray builders for DeviceScene.render_lens (include/cutrace_lens.h): numpy float32 data plumbing, no GPU.

Every builder returns (origins, dirs), both (H, W, 3) float32, row-major over the frame; directions are NOT normalised (the
kernel normalises).  A pixel without a ray holds NaN in its direction: the lens render masks it (depth +inf, colour 0).
`cam`: a `_lib.Camera`, or a dict of pos / up / forward / right (as tests/ray_ref.py's RefScene.cam).
"""
import numpy as np

f32 = np.float32


def _cam(cam):
    if isinstance(cam, dict):
        return tuple(np.asarray(cam[k], f32) for k in ("pos", "right", "up", "forward"))
    return tuple(np.array(getattr(cam, k).tup(), f32) for k in ("pos", "right", "up", "forward"))


def is_masked(origins, dirs):
    """The mask rule of include/cutrace_lens.h: a non-finite origin, or a normalised direction v * (1 / sqrt(v.v)) — in
    float32, one rounding per operation — that is not finite or is (0, 0, 0)."""
    o, d = np.asarray(origins, f32), np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        u = (f32(1.0) / n)[..., None] * d
    return ~np.isfinite(o).all(-1) | ~np.isfinite(u).all(-1) | (u == 0).all(-1)


def _pixel_dirs(cam, x, y, w, h):
    """cam::get_ray's direction before it is normalised, (x_v + y_v) + forward, for pixel coordinates x, y (float32 arrays)
    of a w x h frame — the reference's operations in its order (inc/default_schema.hpp:376-386)"""
    _, right, up, fwd = _cam(cam)
    aspect = f32(w) / f32(h)
    x_v = (((x / f32(w)) - f32(0.5)) * aspect)[..., None] * right
    y_v = (f32(0.5) - (y / f32(h)))[..., None] * up
    return ((x_v + y_v) + fwd).astype(f32)


def pinhole(cam, w, h):
    """The camera's own rays: normalised, they are cam::get_ray(x, y) bit for bit, so render_lens gives the plain render."""
    y, x = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    d = _pixel_dirs(cam, x, y, w, h)
    o = np.broadcast_to(_cam(cam)[0], d.shape).astype(f32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def fisheye(cam, w, h, fov_deg):
    """Equidistant fisheye about the camera's forward axis: the angle from the axis grows linearly with the distance from
    the image centre and reaches fov_deg / 2 on the circle inscribed in the frame (pixel centres).  Outside the circle:
    NaN directions, which the lens render masks."""
    pos, right, up, fwd = _cam(cam)
    r_, u_, f_ = _unit(right), _unit(up), _unit(fwd)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rad = min(w, h) / 2.0
    u, v = (x + 0.5 - w / 2.0) / rad, (h / 2.0 - y - 0.5) / rad
    r = np.hypot(u, v)
    theta = r * np.radians(fov_deg) / 2.0
    phi = np.arctan2(v, u)
    d = (np.sin(theta) * np.cos(phi))[..., None] * r_ + (np.sin(theta) * np.sin(phi))[..., None] * u_ + np.cos(theta)[..., None] * f_
    d = np.where((r <= 1.0)[..., None], d, np.nan).astype(f32)
    o = np.broadcast_to(pos, d.shape).astype(f32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def stereo(cam, w, h, baseline):
    """A side-by-side stereo pair in ONE frame: columns [0, w // 2) are the left eye's pinhole image (w // 2 x h), the rest
    the right eye's; the eyes sit at pos -+ baseline / 2 along the camera's right axis."""
    pos, right, _, _ = _cam(cam)
    wl = w // 2
    if wl < 1 or w - wl < 1:
        raise ValueError("stereo: the frame must be at least 2 pixels wide")
    off = (_unit(right) * (baseline / 2.0)).astype(f32)
    o = np.empty((h, w, 3), f32)
    d = np.empty((h, w, 3), f32)
    o[:, :wl], o[:, wl:] = (pos - off).astype(f32), (pos + off).astype(f32)
    d[:, :wl] = pinhole(cam, wl, h)[1]
    d[:, wl:] = pinhole(cam, w - wl, h)[1]
    return o, d


def thin_lens(cam, w, h, samples, aperture, focus, seed):
    """The jittered sample frame of a thin lens: (samples*h, samples*w, 3).  Sample (X, Y) looks through the point
    (X + jx, Y + jy) / samples of the pinhole image, jx, jy uniform in [0, 1); its ray starts at a uniformly drawn point of
    the lens disk (diameter `aperture`, in the plane of the camera's right and up axes) and passes through the point
    where the pinhole ray meets the plane at distance `focus` along the forward axis.  seed: numpy RandomState."""
    pos, right, up, fwd = _cam(cam)
    r_, u_, f_ = _unit(right), _unit(up), _unit(fwd)
    rng = np.random.RandomState(seed)
    H, W = samples * h, samples * w
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    jx, jy = rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W))
    dp = _pixel_dirs(cam, ((x + jx) / samples).astype(f32), ((y + jy) / samples).astype(f32), w, h).astype(np.float64)
    target = pos.astype(np.float64) + dp * (focus / (dp @ f_))[..., None]
    rad, ang = 0.5 * aperture * np.sqrt(rng.uniform(0, 1, (H, W))), rng.uniform(0, 2 * np.pi, (H, W))
    o = pos.astype(np.float64) + (rad * np.cos(ang))[..., None] * r_ + (rad * np.sin(ang))[..., None] * u_
    o = o.astype(f32)
    d = (target - o.astype(np.float64)).astype(f32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)
