"""cutrace_amd — MI355X-native ray-cast + shading path of jay-tux/cutrace.

The product is native: `libcutrace_amd.so` (HIP kernels behind the C-ABI in
include/cutrace_amd.h), `libcutrace_host.so` (scene loader / image writers) and the
`cutrace` CLI.  This package is the thin ctypes plumbing tests and bench.py use.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Camera, Light, Material, Object, RenderStats, Rows, SceneDesc, Triangle, Vec3  # noqa: F401

ROOT = _lib.ROOT

VAR_AUTO = 0
VAR_NO_PREFILTER = 2
VAR_NO_ANYHIT = 4
VAR_NO_CLUSTER = 8
VAR_STATS = 16
VAR_EXACT_POW = 32
VAR_NO_REORDER = 256
VAR_NO_OCC6 = 512
VAR_NO_DIRECT = 1024
VAR_IMAGE_ORDER_FIRST = 2048
VAR_MERGE = 4096
VAR_IGNORE_TRANSPARENT = 8192

# ctr_cast_rays flags (include/cutrace_rays.h)
RAY_IGNORE_TRANSPARENT = 1
RAY_LINEAR = 2
RAY_SHADOW = 4
RAY_OUTPUTS = ("t", "object", "prim", "point", "normal", "uv")
# ctr_shade_rays flags and outputs (include/cutrace_rays.h)
SHADE_LINEAR = 1
SHADE_EXACT_POW = 2
SHADE_OUTPUTS = ("color", "t", "object", "normal")
# ctr_shade_points flags and outputs (include/cutrace_rays.h)
POINTS_LINEAR = 1
POINTS_EXACT_POW = 2
POINTS_OUTPUTS = ("color", "light_shadow")
# ctr_list_hits flags, per-slot outputs and largest max_hits (include/cutrace_hits.h)
HITS_IGNORE_TRANSPARENT = 1
HITS_LINEAR = 2
HITS_OUTPUTS = ("t", "object", "prim", "point", "normal", "uv")
HITS_MAX = 65535
# ctr_nearest_points flags (include/cutrace_nearest.h) and what DeviceScene.nearest_points returns per point
NEAREST_LINEAR = 1
NEAREST_SKIP_PLANES = 2
NEAREST_OUTPUTS = ("distance", "object", "prim", "point", "normal")
# ctr_count_crossings and ctr_inside_points flags, outputs and largest n_dirs (include/cutrace_inside.h)
CROSS_LINEAR = 1
CROSS_SKIP_PLANES = 2
CROSS_SKIP_TRIANGLES = 4
CROSS_OUTPUTS = ("count", "signed")
INSIDE_LINEAR = 1
INSIDE_OUTPUTS = ("inside", "votes")
INSIDE_MAX_DIRS = 15


def inside_default_dirs():
    """the library's default directions of inside(): (3, 3) float32 (ctr_inside_default_dirs)"""
    out = (C.c_float * 9)()
    _lib.hip_lib().ctr_inside_default_dirs(out)
    return np.array(out, np.float32).reshape(3, 3)


# the display planes of render_images / quantise (include/cutrace_images.h)
IMAGE_PLANES = ("color", "depth", "normal")


@contextlib.contextmanager
def _cwd(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def _check(name, st):
    """The one place where a status of the HIP library becomes an exception."""
    if st:
        raise RuntimeError(f"{name} failed ({st}): {_lib.hip_lib().ctr_last_error().decode()}")


def _stats_dict(stats):
    """A RenderStats as the statistics every host-form render returns."""
    return dict(ray_count=int(stats.ray_count), kernel_ms=stats.kernel_ms, total_ms=stats.total_ms,
                max_depth=float(stats.max_depth), rows=int(stats.rows))


def _frame_views(blk, px, n, w):
    """depth (n, w), color (n, w, 3), normal (n, w, 3): views of a block of 7 floats per pixel (depth at 0, color at px,
    normal at 4 * px)."""
    if not n:
        return dict(depth=np.empty((0, w), np.float32), color=np.empty((0, w, 3), np.float32), normal=np.empty((0, w, 3), np.float32))
    return dict(depth=blk[:px].reshape(n, w), color=blk[px:4 * px].reshape(n, w, 3), normal=blk[4 * px:7 * px].reshape(n, w, 3))


def _empty_frame(n, w, uv=False):
    """The pageable frame: fresh numpy buffers."""
    fr = dict(depth=np.empty((n, w), np.float32), color=np.empty((n, w, 3), np.float32), normal=np.empty((n, w, 3), np.float32))
    if uv:
        fr["uv"] = np.empty((n, w, 2), np.float32)
    return fr


def _frame_alloc(px):
    """A page-locked block of 7 * px floats (ctr_frame_alloc): (pointer for ctr_frame_free, the block as a numpy array)."""
    d, c, n = (C.POINTER(C.c_float)() for _ in range(3))
    _check("ctr_frame_alloc", _lib.hip_lib().ctr_frame_alloc(px, C.byref(d), C.byref(c), C.byref(n)))
    return d, np.ctypeslib.as_array(d, shape=(7 * px,))


def _pinned_block(owner, px, grow_only):
    """The page-locked block a DeviceScene / MultiScene keeps for its pinned renders: allocated again when the request
    grows (grow_only) or differs, freed by _free_pinned_block."""
    have = getattr(owner, "_pin_px", 0)
    if have < px or (have != px and not grow_only):
        _free_pinned_block(owner)
        owner._pin_ptr, owner._pin = _frame_alloc(px)
        owner._pin_px = px
    return owner._pin


def _free_pinned_block(owner):
    if getattr(owner, "_pin_px", 0):
        owner._pin = None
        _lib.hip_lib().ctr_frame_free(owner._pin_ptr)
        owner._pin_px = 0


@contextlib.contextmanager
def _on_stream(dev, stream):
    """Enter the device and the stream (None: torch's current stream of that device); yields the raw stream handle."""
    import torch
    with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        yield C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _subset(what, names, allowed, allow_empty=False, unique=False):
    """`names` as a tuple, if it is a subset of `allowed` (non-empty unless allow_empty; unique: no name twice)."""
    names = tuple(names)
    if (not names and not allow_empty) or (unique and len(set(names)) != len(names)) or any(k not in allowed for k in names):
        raise ValueError(f"{what}: a {'' if allow_empty else 'non-empty '}subset of {allowed}, got {names}")
    return names


# what cast_rays and shade_rays return per ray: (trailing shape, dtype)
_RAY_OUT = {"t": ((), "float32"), "object": ((), "int32"), "prim": ((), "int32"), "point": ((3,), "float32"),
            "normal": ((3,), "float32"), "uv": ((2,), "float32"), "color": ((3,), "float32")}


# what nearest_points returns per point
_NEAREST_OUT = {"distance": ((), "float32"), "object": ((), "int32"), "prim": ((), "int32"), "point": ((3,), "float32"),
                "normal": ((3,), "float32")}


def _ray_outputs(names, n, dev):
    import torch
    return {k: torch.empty((n,) + _RAY_OUT[k][0], dtype=getattr(torch, _RAY_OUT[k][1]), device=dev) for k in names}


def _array_check(x, what, dev, dtype, cols):
    """x as a tensor of `dtype` and shape (n, cols) (cols 0: (n,)), still where it was: a tensor on another GPU than `dev`,
    another type, dtype or shape raise.  (Where indices are asked for, an int is welcome too: the caller has dealt with it.)"""
    import torch
    if isinstance(x, torch.Tensor):
        if x.device.type != "cpu" and x.device != dev:
            raise ValueError(f"{what}: tensor on {x.device}, the scene lives on {dev}")
    elif isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    else:
        raise TypeError(f"{what}: expected {'an int, ' if dtype == 'int32' else ''}a torch tensor or a numpy array, got {type(x).__name__}")
    shape_ok = x.dim() == 1 if cols == 0 else (x.dim() == 2 and x.shape[1] == cols)
    if x.dtype != getattr(torch, dtype) or not shape_ok:
        raise ValueError(f"{what}: expected {dtype} of shape {'(n,)' if cols == 0 else f'(n, {cols})'}, "
                         f"got {x.dtype} {tuple(x.shape)}")
    return x


def _ray_pair(origins, dirs, dev, frame=None):
    """(o, d, n): origins and dirs, (n, 3) float32 each, contiguous on `dev` (a tensor already there is used in place, a CPU
    tensor or a numpy array is copied over) once both are valid.  frame = (H, W): the lens render's rays, which may also be
    (H, W, 3) and must be H * W."""
    import torch
    H, W = frame or (0, 0)
    pair = []
    for x, what in ((origins, "origins"), (dirs, "dirs")):
        if frame and isinstance(x, (np.ndarray, torch.Tensor)) and len(x.shape) == 3:
            if tuple(x.shape) != (H, W, 3):
                raise ValueError(f"{what}: expected shape ({H}, {W}, 3) or ({H * W}, 3), got {tuple(x.shape)}")
            x = x.reshape(H * W, 3)
        x = _array_check(x, what, dev, "float32", 3)
        if frame and x.shape[0] != H * W:
            raise ValueError(f"{what}: {x.shape[0]} rays for the {W} x {H} frame ({H * W})")
        pair.append(x)
    o, d = pair
    if d.shape[0] != o.shape[0]:
        raise ValueError(f"dirs: {d.shape[0]} rays for {o.shape[0]} origins")
    return o.to(dev, non_blocking=False).contiguous(), d.to(dev, non_blocking=False).contiguous(), o.shape[0]


def _records(kind, items, what=None):
    """A ctypes array of copies of `items`, a sequence of `kind` (_lib.Light, _lib.Material); anything else raises TypeError."""
    if isinstance(items, (str, bytes)) or not hasattr(items, "__len__") or not hasattr(items, "__getitem__"):
        raise TypeError(f"{what or kind.__name__}: expected a sequence of {kind.__name__}, got {type(items).__name__}")
    arr = (kind * len(items))()
    for k in range(len(items)):
        if not isinstance(items[k], kind):
            raise TypeError(f"{what or kind.__name__}[{k}]: expected {kind.__name__}, got {type(items[k]).__name__}")
        C.memmove(C.byref(arr, k * C.sizeof(kind)), C.byref(items[k]), C.sizeof(kind))
    return arr


class HostScene:
    """A scene loaded by the C++ loader (libcutrace_host.so): owns the flat arrays."""

    def __init__(self, handle, status):
        self._h = handle
        self.status = status

    @classmethod
    def load(cls, json_path, cwd=None):
        """Load a scene JSON. Mesh paths inside it are relative to `cwd` (default: repo root,
        like the reference which expects to be run from its repository root)."""
        L = _lib.host_lib()
        h = C.c_void_p()
        with _cwd(cwd or ROOT):
            st = L.ctr_host_scene_load(os.fsencode(json_path), C.byref(h))
        if not h:
            raise IOError(f"cannot read scene file {json_path}")
        return cls(h, st)

    @classmethod
    def parse(cls, text, cwd=None):
        L = _lib.host_lib()
        h = C.c_void_p()
        with _cwd(cwd or ROOT):
            st = L.ctr_host_scene_parse(text.encode(), C.byref(h))
        return cls(h, st)

    @property
    def ok(self):
        return self.status == 0

    @property
    def desc(self):
        return _lib.host_lib().ctr_host_scene_desc(self._h)

    def set_size(self, w, h):
        _lib.host_lib().ctr_host_scene_set_size(self._h, w, h)

    def set_material(self, idx, **kw):
        d = self.desc.contents
        m = Material()
        C.memmove(C.byref(m), C.byref(d.materials[idx]), C.sizeof(Material))
        for k, v in kw.items():
            if k == "color":
                m.color = Vec3(*v)
            else:
                setattr(m, k, v)
        st = _lib.host_lib().ctr_host_scene_set_material(self._h, idx, C.byref(m))
        if st:
            raise ValueError("bad material index")

    @property
    def size(self):
        cam = self.desc.contents.cam
        return int(cam.w), int(cam.h)

    def close(self):
        if self._h:
            _lib.host_lib().ctr_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_rows(h, rows=None):
    """rows: None (whole frame) | (row_begin,row_end) | (row_begin,row_end,block_rows,part,n_parts)"""
    if rows is None:
        return Rows(0, h, max(h, 1), 0, 1)
    if len(rows) == 2:
        return Rows(rows[0], rows[1], max(h, 1), 0, 1)
    return Rows(*rows)


def rows_count(h, rows):
    r = make_rows(h, rows)
    return int(_lib.host_lib().ctr_rows_count(C.byref(r), h))


class DeviceScene:
    """A scene uploaded to one GPU through the C-ABI (ctr_scene_create)."""

    def __init__(self, host_scene, device=0):
        L = _lib.hip_lib()
        h = C.c_void_p()
        _check("ctr_scene_create", L.ctr_scene_create(host_scene.desc, device, C.byref(h)))
        self._h = h
        self.device = device
        self.w, self.h = host_scene.size
        self._ambient = float(host_scene.desc.contents.cam.ambient)  # shade_rays' and shade_points' default
        self.n_lights = int(host_scene.desc.contents.n_lights)       # the width of shade_points' light_shadow
        d = host_scene.desc.contents
        self._materials = _records(Material, [d.materials[i] for i in range(int(d.n_materials))])  # set_material edits these

    def set_variant(self, bits):
        _check("ctr_set_variant", _lib.hip_lib().ctr_set_variant(self._h, bits))

    def set_size(self, w, h):
        _check("ctr_scene_set_size", _lib.hip_lib().ctr_scene_set_size(self._h, w, h))
        self.w, self.h = w, h

    def _pinned_frame(self, px):
        """One page-locked block for a frame's three buffers (ctr_frame_alloc), kept with the scene handle."""
        return _pinned_block(self, px, grow_only=True)

    def _free_pinned(self):
        _free_pinned_block(self)

    @staticmethod
    def _samples(samples):
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or int(samples) not in (1, 2, 4, 8):
            raise ValueError(f"samples: 1, 2, 4 or 8 per axis, got {samples!r}")
        return int(samples)

    def render(self, fudge=1e-3, bounces=5, rows=None, pinned=False, into=None, samples=1):
        """Host-buffer form (ctr_render): returns numpy buffers + stats.  pinned=True: the buffers are views of
        the scene handle's page-locked frame block (valid until the next pinned render / close).  into: a dict
        returned by an earlier call of the same shape, whose buffers are written again.  samples = 2, 4 or 8: the
        supersampled frame (ctr_render_aa, include/cutrace_aa.h): samples x samples rays per pixel, averaged in the
        kernel; the buffers, `rows` and stats['rows'] stay those of the w x h frame."""
        samples = self._samples(samples)
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        n = rows_count(self.h, rows)
        if into is not None:
            fr = dict(depth=into["depth"], color=into["color"], normal=into["normal"])
            assert fr["depth"].shape == (n, self.w) and fr["color"].shape == (n, self.w, 3) and fr["normal"].shape == (n, self.w, 3)
        elif pinned:
            px = max(n * self.w, 1)
            fr = _frame_views(self._pinned_frame(px), px, n, self.w)
        else:
            fr = _empty_frame(n, self.w)
        ptrs = fr["depth"].ctypes.data, fr["color"].ctypes.data, fr["normal"].ctypes.data
        stats = RenderStats()
        if samples != 1:
            _check("ctr_render_aa", L.ctr_render_aa(self._h, C.c_float(fudge), bounces, samples, C.byref(r), *ptrs, C.byref(stats)))
        else:
            _check("ctr_render", L.ctr_render(self._h, C.c_float(fudge), bounces, C.byref(r), *ptrs, C.byref(stats)))
        return dict(fr, **_stats_dict(stats))

    def render_images(self, fudge=1e-3, bounces=5, rows=None, samples=1, planes=IMAGE_PLANES, pinned=False):
        """ctr_render_images (include/cutrace_images.h): the frame quantised to display bytes on the GPU, as the host's
        ctr_quantise_color / _depth / _normal quantise what render() returns — byte for byte — but only 3 bytes per pixel and
        plane cross to the host.  Returns a dict with a (rows, w, 3) uint8 numpy array per name in `planes` (a non-empty
        subset of "color", "depth", "normal"; depth is replicated to R = G = B) plus render()'s stats.  pinned=True: the
        arrays are page-locked (torch's pinned memory), their copies are queued instead of staged."""
        samples = self._samples(samples)
        planes = _subset("planes", planes, IMAGE_PLANES, unique=True)
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        n = rows_count(self.h, rows)
        if pinned:
            import torch
            keep = {k: torch.empty(n, self.w, 3, dtype=torch.uint8).pin_memory() for k in planes}
            out = {k: v.numpy() for k, v in keep.items()}
        else:
            out = {k: np.empty((n, self.w, 3), np.uint8) for k in planes}
        ptr = {k: (out[k].ctypes.data if k in out else None) for k in IMAGE_PLANES}
        stats = RenderStats()
        _check("ctr_render_images", L.ctr_render_images(self._h, C.c_float(fudge), bounces, samples, C.byref(r), ptr["depth"],
                                                        ptr["color"], ptr["normal"], C.byref(stats)))
        return dict(out, **_stats_dict(stats))

    def quantise(self, depth=None, color=None, normal=None, counters=None, max_depth=None, out=None, stream=None):
        """ctr_quantise_device (include/cutrace_images.h): float planes on the scene's device to display bytes there — what
        follows render_device, render_device_batch and render_lens.  depth (..., ) and color / normal (..., 3): contiguous
        float32 torch tensors on the scene's device, of the same number of pixels; at least one.  With depth, exactly one
        of `counters` (the 16-word int64 block the render accumulated into, read on the device: no synchronisation) and
        `max_depth` (a float).  out: a dict of contiguous uint8 tensors (pixels * 3 bytes each) to write instead of new
        ones.  Returns a dict of uint8 tensors of shape (..., 3) under the names given.  Asynchronous on `stream` (a
        torch.cuda.Stream; default: torch's current stream of the scene's device)."""
        import torch
        dev = self._torch_device()
        given = {k: v for k, v in (("depth", depth), ("color", color), ("normal", normal)) if v is not None}
        if not given:
            raise ValueError("quantise: at least one of depth, color, normal")
        if depth is not None and (counters is None) == (max_depth is None):
            raise ValueError("quantise: depth needs exactly one of counters and max_depth")
        px = None
        for k, v in given.items():
            if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype != torch.float32 or not v.is_contiguous():
                raise ValueError(f"{k}: expected a contiguous float32 tensor on {dev}")
            if k != "depth" and (v.dim() < 1 or v.shape[-1] != 3):
                raise ValueError(f"{k}: expected shape (..., 3), got {tuple(v.shape)}")
            n = v.numel() if k == "depth" else v.numel() // 3
            if px is not None and n != px:
                raise ValueError(f"{k}: {n} pixels, the other planes have {px}")
            px = n
        if counters is not None and (not isinstance(counters, torch.Tensor) or counters.device != dev or counters.dtype != torch.int64
                                     or counters.numel() < 2 or not counters.is_contiguous()):
            raise ValueError(f"counters: expected a contiguous int64 tensor of at least 2 words on {dev}")
        res = {}
        with _on_stream(dev, stream) as raw:
            q = _lib.ImagePlanes()
            q.n_pixels = px
            for k, v in given.items():
                shape = (tuple(v.shape) + (3,)) if k == "depth" else tuple(v.shape)
                if out is not None and k in out:
                    o = out[k]
                    if not isinstance(o, torch.Tensor) or o.device != dev or o.dtype != torch.uint8 or not o.is_contiguous() or o.numel() != 3 * px:
                        raise ValueError(f"out[{k!r}]: expected a contiguous uint8 tensor of {3 * px} bytes on {dev}")
                else:
                    o = torch.empty(shape, dtype=torch.uint8, device=dev)
                res[k] = o
                setattr(q, {"depth": "d_depth", "color": "d_color3", "normal": "d_normal3"}[k], v.data_ptr() or None)
                setattr(q, {"depth": "d_depth8", "color": "d_color8", "normal": "d_normal8"}[k], o.data_ptr() or None)
            if depth is not None:
                if counters is not None:
                    q.d_counters = counters.data_ptr()
                else:
                    q.max_depth = float(max_depth)
            if px:
                _check("ctr_quantise_device", _lib.hip_lib().ctr_quantise_device(self.device, C.byref(q), raw))
        return res

    def render_uv(self, fudge=1e-3, bounces=5, rows=None):
        """ctr_render_uv: the three buffers plus `uv` (n, w, 2): ray_cast's texture coordinates of the primary hit."""
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        n = rows_count(self.h, rows)
        fr = _empty_frame(n, self.w, uv=True)
        stats = RenderStats()
        _check("ctr_render_uv", L.ctr_render_uv(self._h, C.c_float(fudge), bounces, C.byref(r), fr["depth"].ctypes.data,
                                                fr["color"].ctypes.data, fr["normal"].ctypes.data, fr["uv"].ctypes.data, C.byref(stats)))
        return dict(fr, **_stats_dict(stats))

    def render_device(self, d_depth, d_color, d_normal, d_counters=0, stream=0, fudge=1e-3, bounces=5, rows=None, samples=1):
        """Device-buffer form (ctr_render_device): raw device pointers, async on `stream`.  samples = 2, 4 or 8:
        ctr_render_device_aa, the supersampled frame into the same w x h buffers."""
        samples = self._samples(samples)
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        if samples != 1:
            _check("ctr_render_device_aa", L.ctr_render_device_aa(self._h, C.c_float(fudge), bounces, samples, C.byref(r), d_depth,
                                                                  d_color, d_normal, d_counters, stream))
        else:
            _check("ctr_render_device", L.ctr_render_device(self._h, C.c_float(fudge), bounces, C.byref(r), d_depth, d_color,
                                                            d_normal, d_counters, stream))

    def set_cameras(self, cams):
        """Upload a camera path (list of _lib.Camera, same w/h): frames of ctr_render_device_batch."""
        arr = (Camera * len(cams))(*cams)
        _check("ctr_scene_set_cameras", _lib.hip_lib().ctr_scene_set_cameras(self._h, arr, len(cams)))
        self.n_cams = len(cams)

    def render_device_batch(self, d_depth, d_color, d_normal, n_frames, frame_stride_px, first_frame=0, d_counters=0,
                            stream=0, fudge=1e-3, bounces=5, rows=None, part_stride=0):
        """n_frames frames in ONE launch (ctr_render_device_batch)."""
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        _check("ctr_render_device_batch", L.ctr_render_device_batch(self._h, C.c_float(fudge), bounces, C.byref(r), first_frame, n_frames,
                                                                    frame_stride_px, part_stride, d_depth, d_color, d_normal, d_counters,
                                                                    stream))

    def algorithmic_bytes(self, fudge=1e-3, bounces=5, rows=None):
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        b = C.c_uint64()
        n = C.c_uint64()
        _check("ctr_algorithmic_bytes", L.ctr_algorithmic_bytes(self._h, C.c_float(fudge), bounces, C.byref(r), C.byref(b), C.byref(n)))
        return int(b.value), int(n.value)

    def last_counters(self):
        """The 16 counter words of the last host-form render (ctr_last_counters)."""
        out = np.zeros(16, np.uint64)
        _lib.hip_lib().ctr_last_counters(self._h, out.ctypes.data)
        return out

    def last_kernel(self):
        """The build (KV_* bits) of the handle's most recent launch (ctr_debug_last_kernel)."""
        kv = C.c_uint32()
        _check("ctr_debug_last_kernel", _lib.hip_lib().ctr_debug_last_kernel(self._h, C.byref(kv)))
        return int(kv.value)

    def last_shape(self):
        """The launch shape of the handle's most recent launch (ctr_debug_last_shape): 0 general, 1 the one-mesh build."""
        shape = C.c_uint32()
        _check("ctr_debug_last_shape", _lib.hip_lib().ctr_debug_last_shape(self._h, C.byref(shape)))
        return int(shape.value)

    def last_opaque(self):
        """The opaque build of the handle's most recent launch (ctr_debug_last_opaque): 0 the code as it is for every scene,
        1 the one-mesh any-hit build without the pass-through half of the shading."""
        opaque = C.c_uint32()
        _check("ctr_debug_last_opaque", _lib.hip_lib().ctr_debug_last_opaque(self._h, C.byref(opaque)))
        return int(opaque.value)

    def last_phased(self):
        """Whether the handle's most recent launch ran the phased twin of its opaque build (ctr_debug_last_phased): 1 for every
        opaque build unless the handle was created under CUTRACE_NO_PHASE_SPLIT=1, else 0."""
        phased = C.c_uint32()
        _check("ctr_debug_last_phased", _lib.hip_lib().ctr_debug_last_phased(self._h, C.byref(phased)))
        return int(phased.value)

    def room_facts(self):
        """The room facts of the handle's most recent launch (ctr_debug_room_facts): all zero, or what lets any-hit shadow trips
        from inside a plane room skip their plane tests."""
        out = np.zeros(5, np.float32)
        lights = C.c_uint32()
        _check("ctr_debug_room_facts", _lib.hip_lib().ctr_debug_room_facts(self._h, out.ctypes.data, C.byref(lights)))
        return {"c": out[:3].copy(), "r": float(out[3]), "delta": float(out[4]), "lights": int(lights.value)}

    def dark_skip(self):
        """The dark-skip word of the handle's most recent launch (ctr_debug_dark_skip): non-zero when its kernel may leave out the
        shadow casts of lights whose diffuse and specular factors are both zero at the hit."""
        word = C.c_uint32()
        _check("ctr_debug_dark_skip", _lib.hip_lib().ctr_debug_dark_skip(self._h, C.byref(word)))
        return int(word.value)

    @staticmethod
    def lane_stats(reset=True):
        """Live-lane statistics of the VAR_STATS launches since the last reset (ctr_debug_lane_stats), decoded."""
        raw = np.zeros(96, np.uint64)
        _check("ctr_debug_lane_stats", _lib.hip_lib().ctr_debug_lane_stats(raw.ctypes.data, 1 if reset else 0))
        c = [int(x) for x in raw]
        trips, live = c[72], c[73]
        out = {"wave_trips": trips, "live_lanes_per_trip": live / trips if trips else None,
               "live_fraction": live / (64.0 * trips) if trips else None,
               "live_fraction_of_in_image_lanes": (live / trips) / (c[75] / c[74]) if trips and c[74] and c[75] else None,
               "trips_by_live_lanes_1_8_to_57_64": c[64:72], "trips_mixing_kinds": c[76], "waves": c[74],
               "merged_walks": c[78], "merged_walks_redone": c[77],
               "shadow_casts_at_meshes": {"wave_casts": c[80], "receivers_all_off_mesh": c[81], "of_those_unoccluded_by_meshes": c[82],
                                          "unoccluded_by_meshes_any_receiver": c[83]},
               "anyhit_shadow_trips": c[88], "anyhit_shadow_trips_without_planes": c[89],
               "dark_lights": {"lane_light_pairs": c[90], "shadow_trips_all_dark": c[91], "mesh_entries_with_a_dark_lane": c[92]}}
        kinds = {}
        for d in range(16):
            for name, base in (("radiance", 0), ("shadow", 16)):
                if c[32 + base + d]:
                    label = "primary" if (name == "radiance" and d == 0) else f"{name}@depth{d}"
                    kinds[label] = {"lanes": c[base + d], "trips": c[32 + base + d],
                                    "lanes_per_trip": c[base + d] / c[32 + base + d]}
        out["by_kind"] = kinds
        return out

    # ---- ray queries (ctr_cast_rays, include/cutrace_rays.h) ----
    def _torch_device(self):
        import torch
        return torch.device("cuda", self.device)

    def _rays_arg(self, x, what, cols):
        """(n, cols) float32 (cols 0: (n,)) on the scene's device: a tensor already there is used in place (made contiguous),
        a CPU tensor or a numpy array is copied over; another GPU, another shape or dtype raise."""
        dev = self._torch_device()
        return _array_check(x, what, dev, "float32", cols).to(dev, non_blocking=False).contiguous()

    def _cast(self, q, keep, stream):
        """Fill the query's ray pointers from `keep` and launch on the raw stream handle."""
        q.n_rays = keep[0].shape[0]
        q.d_origin, q.d_dir = keep[0].data_ptr() or None, keep[1].data_ptr() or None
        _check("ctr_cast_rays", _lib.hip_lib().ctr_cast_rays(self._h, C.byref(q), stream))

    def _per_ray(self, x, n, what):
        """A scalar, or (n,) float32 per-ray values: (scalar, tensor or None)."""
        if isinstance(x, (int, float, np.integer, np.floating)):
            return float(x), None
        v = self._rays_arg(x, what, 0)
        if v.shape[0] != n:
            raise ValueError(f"{what}: {v.shape[0]} values for {n} rays")
        return 0.0, v

    def cast_rays(self, origins, dirs, min_t=1e-3, ignore_transparent=False, linear=False, outputs=None, stream=None):
        """ray_cast (inc/ray_cast.hpp:29-55) of every ray (origins[k], dirs[k]): a dict of tensors on the scene's device,
        `t` (n,) (+inf: miss), `object` (n,) int32 (-1: miss), `prim` (n,) int32 (file-order triangle of a mesh hit, else -1),
        `point` (n, 3), `normal` (n, 3), `uv` (n, 2) — or the subset named in `outputs`.  origins, dirs: (n, 3) float32;
        min_t: a scalar or (n,) float32.  Directions need not be normalised (a sphere measures t along dir/|dir|).
        linear=True: meshes walked linearly — bit-identical to the reference also for rays in a triangle's plane.
        Asynchronous on `stream` (a torch.cuda.Stream; default: torch's current stream of the scene's device)."""
        outputs = RAY_OUTPUTS if outputs is None else _subset("outputs", outputs, RAY_OUTPUTS)
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            o, d, n = _ray_pair(origins, dirs, dev)
            q = _lib.RayQuery()
            q.flags = (RAY_IGNORE_TRANSPARENT if ignore_transparent else 0) | (RAY_LINEAR if linear else 0)
            q.min_t, mt = self._per_ray(min_t, n, "min_t")
            q.d_min_t = mt.data_ptr() if mt is not None and n else None
            out = _ray_outputs(outputs, n, dev)
            for k, v in out.items():
                setattr(q, "d_" + k, v.data_ptr() if n else None)
            if n:
                self._cast(q, (o, d, mt), raw)
        return out

    def shadow(self, origins, dirs, max_t, linear=False, stream=None):
        """shadow_intensity (inc/shading.hpp:22-45) of every ray: (n,) float32 on the scene's device, 1 = fully blocked.
        max_t: a scalar or (n,) float32.  The loop's first cast starts at (float)(0.0 + 1e-3), as the reference's does."""
        import torch
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            o, d, n = _ray_pair(origins, dirs, dev)
            q = _lib.RayQuery()
            q.flags = RAY_SHADOW | (RAY_LINEAR if linear else 0)
            q.max_t, mx = self._per_ray(max_t, n, "max_t")
            q.d_max_t = mx.data_ptr() if mx is not None and n else None
            out = torch.empty(n, dtype=torch.float32, device=dev)
            q.d_shadow = out.data_ptr() if n else None
            if n:
                self._cast(q, (o, d, mx), raw)
        return out

    # ---- hit lists (ctr_list_hits, include/cutrace_hits.h) ----
    def list_hits(self, origins, dirs, max_hits, min_t=1e-3, max_t=float("inf"), step=1e-3, ignore_transparent=False, linear=False,
                  outputs=None, stream=None):
        """The first `max_hits` hits along every ray (origins[k], dirs[k]): the chain of nearest casts of the reference's
        shadow_intensity (inc/shading.hpp:22-45), each cast restarting at (float)((double)t + step) behind the last hit and the
        chain ending at the first cast that hits nothing below max_t.  A dict of tensors on the scene's device: `count` (n,)
        int32, always, and SLOT-MAJOR per-slot outputs `t` (max_hits, n), `object`, `prim` (max_hits, n) int32, `point`,
        `normal` (max_hits, n, 3), `uv` (max_hits, n, 2) — or the subset named in `outputs`; outputs=() gives the count alone.
        hits["point"][j] is the contiguous batch of every ray's j-th hit, as shade_points and cast_rays take it; slots
        count .. max_hits-1 of a ray hold cast_rays' miss values (t +inf, object and prim -1, zeros).  min_t, max_t: a scalar
        or (n,) float32.  With the defaults the list is what shadow(origins, dirs, max_t) visits until its sum saturates.
        t is in the reference's mixed units (a sphere measures along dir/|dir|), and so is step; a surface less than step
        behind a listed hit is skipped.  Asynchronous on `stream` (default: torch's current stream of the scene's device)."""
        import torch
        outputs = HITS_OUTPUTS if outputs is None else _subset("outputs", outputs, HITS_OUTPUTS, allow_empty=True, unique=True)
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
            raise TypeError(f"max_hits: expected an int, got {type(max_hits).__name__}")
        if not 1 <= max_hits <= HITS_MAX:
            raise ValueError(f"max_hits: 1 .. {HITS_MAX}, got {max_hits}")
        step = float(step)
        if not (0.0 <= step < float("inf")):
            raise ValueError(f"step: finite and not negative, got {step}")
        K = int(max_hits)
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            o, d, n = _ray_pair(origins, dirs, dev)
            q = _lib.HitQuery()
            q.n_rays, q.max_hits, q.step = n, K, step
            q.flags = (HITS_IGNORE_TRANSPARENT if ignore_transparent else 0) | (HITS_LINEAR if linear else 0)
            q.min_t, mn = self._per_ray(min_t, n, "min_t")
            q.max_t, mx = self._per_ray(max_t, n, "max_t")
            if outputs and n * K >= 1 << 31:
                raise ValueError(f"{n} rays x {K} slots: per-slot outputs need n * max_hits below 2^31")
            out = {"count": torch.empty(n, dtype=torch.int32, device=dev)}
            for k in outputs:
                out[k] = torch.empty((K, n) + _RAY_OUT[k][0], dtype=getattr(torch, _RAY_OUT[k][1]), device=dev)
            if n:
                q.d_origin, q.d_dir = o.data_ptr(), d.data_ptr()
                q.d_min_t = mn.data_ptr() if mn is not None else None
                q.d_max_t = mx.data_ptr() if mx is not None else None
                for k, v in out.items():
                    setattr(q, "d_" + k, v.data_ptr())
                _check("ctr_list_hits", _lib.hip_lib().ctr_list_hits(self._h, C.byref(q), raw))
        return out

    # ---- nearest points (ctr_nearest_points, include/cutrace_nearest.h) ----
    def nearest_points(self, points, max_dist=float("inf"), object=None, skip_planes=False, linear=False, outputs=None, stream=None):
        """The closest surface point to every point of `points` ((n, 3) float32): a dict of tensors on the scene's device,
        `distance` (n,) (+inf: nothing within max_dist), `object` (n,) int32 (-1), `prim` (n,) int32 (file-order triangle of a
        mesh, else -1), `point` (n, 3) the closest point, `normal` (n, 3) what cast_rays reports for a hit there — or the subset
        named in `outputs`.  Among equally near candidates the lower object index wins, inside a mesh the lower file index.
        max_dist: a scalar >= 0 or (n,) float32 (a NaN or negative entry: that point misses).  object: only this object index
        (None: every object).  skip_planes: planes are no candidates.  linear=True: no tree, every triangle of every admitted
        mesh — the same bits, the cross-check.  A point with a NaN or an infinity gets the miss values.  Asynchronous on
        `stream` (default: torch's current stream of the scene's device)."""
        import torch
        outputs = NEAREST_OUTPUTS if outputs is None else _subset("outputs", outputs, NEAREST_OUTPUTS, unique=True)
        if object is not None and (isinstance(object, bool) or not isinstance(object, (int, np.integer))):
            raise TypeError(f"object: expected None or an int, got {type(object).__name__}")
        if object is not None and object < 0:
            raise ValueError(f"object: None or an index >= 0, got {object}")
        if isinstance(max_dist, (int, float, np.integer, np.floating)) and not float(max_dist) >= 0.0:
            raise ValueError(f"max_dist: not negative and not NaN, got {max_dist}")
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            p = _array_check(points, "points", dev, "float32", 3)
            n = p.shape[0]
            q = _lib.NearestQuery()
            q.max_dist, md = self._per_ray(max_dist, n, "max_dist")
            p = p.to(dev, non_blocking=False).contiguous()
            q.n_points = n
            q.flags = (NEAREST_LINEAR if linear else 0) | (NEAREST_SKIP_PLANES if skip_planes else 0)
            q.object = -1 if object is None else int(object)
            out = {k: torch.empty((n,) + _NEAREST_OUT[k][0], dtype=getattr(torch, _NEAREST_OUT[k][1]), device=dev) for k in outputs}
            if n:
                q.d_point = p.data_ptr()
                q.d_max_dist = md.data_ptr() if md is not None else None
                for k, v in out.items():
                    setattr(q, {"point": "d_nearest"}.get(k, "d_" + k), v.data_ptr())
                _check("ctr_nearest_points", _lib.hip_lib().ctr_nearest_points(self._h, C.byref(q), raw))
        return out

    # ---- inside queries (ctr_count_crossings, ctr_inside_points, include/cutrace_inside.h) ----
    @staticmethod
    def _object_arg(object):
        """None or an object index >= 0, as the C-ABI's -1 or index"""
        if object is not None and (isinstance(object, bool) or not isinstance(object, (int, np.integer))):
            raise TypeError(f"object: expected None or an int, got {type(object).__name__}")
        if object is not None and object < 0:
            raise ValueError(f"object: None or an index >= 0, got {object}")
        return -1 if object is None else int(object)

    def count_crossings(self, origins, dirs, min_t=0.0, max_t=float("inf"), object=None, skip_planes=False, skip_triangles=False,
                        linear=False, outputs=("count",), stream=None):
        """How many surfaces every ray (origins[k], dirs[k]) crosses over the OPEN interval (min_t, max_t): a dict of (n,) int32
        tensors on the scene's device, `count` and / or `signed` as `outputs` names them.  Every triangle the reference's test
        accepts there counts 1, every root of a sphere 1, a plane 1; `signed` weights a crossing +1 where the ray leaves through
        a face whose normal points along it (a sphere's far root, a plane with dir . normal > 0), -1 otherwise: for a closed,
        outward-oriented mesh and an origin off the surface it is the winding number, and the parity of `count` is containment.
        The reference's triangle test is inclusive on edges, so ONE ray through an edge or a vertex is not a parity oracle:
        inside() votes.  min_t, max_t: a scalar or (n,) float32, in the reference's mixed units (a sphere measures along
        dir/|dir|).  object: only this object index.  skip_planes, skip_triangles: planes / stand-alone triangles are not
        counted.  linear=True: no tree — the same integers.  A ray with a non-finite origin or a NaN, infinite or zero direction
        counts 0.  Asynchronous on `stream` (default: torch's current stream of the scene's device)."""
        import torch
        outputs = _subset("outputs", outputs, CROSS_OUTPUTS, unique=True)
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            o, d, n = _ray_pair(origins, dirs, dev)
            q = _lib.CrossingQuery()
            q.n_rays, q.object = n, self._object_arg(object)
            q.flags = (CROSS_LINEAR if linear else 0) | (CROSS_SKIP_PLANES if skip_planes else 0) | (CROSS_SKIP_TRIANGLES if skip_triangles else 0)
            q.min_t, mn = self._per_ray(min_t, n, "min_t")
            q.max_t, mx = self._per_ray(max_t, n, "max_t")
            out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in outputs}
            if n:
                q.d_origin, q.d_dir = o.data_ptr(), d.data_ptr()
                q.d_min_t = mn.data_ptr() if mn is not None else None
                q.d_max_t = mx.data_ptr() if mx is not None else None
                for k, v in out.items():
                    setattr(q, "d_" + k, v.data_ptr())
                _check("ctr_count_crossings", _lib.hip_lib().ctr_count_crossings(self._h, C.byref(q), raw))
        return out

    @staticmethod
    def _dirs_arg(q, dirs):
        """Fill the query's direction table from `dirs` ((R, 3) floats, R odd, 1 .. 15; None: the default table); returns what
        must stay alive until the call has returned."""
        if dirs is None:
            return None
        a = np.ascontiguousarray(np.asarray(dirs.cpu() if hasattr(dirs, "cpu") else dirs), np.float32)
        if a.ndim != 2 or a.shape[1] != 3 or not 1 <= a.shape[0] <= INSIDE_MAX_DIRS or a.shape[0] % 2 == 0:
            raise ValueError(f"dirs: expected (R, 3) with R odd, 1 .. {INSIDE_MAX_DIRS}, got shape {a.shape}")
        q.n_dirs, q.dirs = a.shape[0], a.ctypes.data_as(C.POINTER(C.c_float))
        return a

    def _inside(self, p, object, dirs, linear, out, distance, raw):
        """ctr_inside_points of the points `p` (on the device, contiguous) into the tensors of `out` and, in place, `distance`"""
        q = _lib.InsideQuery()
        q.n_points, q.object, q.flags = p.shape[0], self._object_arg(object), (INSIDE_LINEAR if linear else 0)
        keep = self._dirs_arg(q, dirs)   # (alive until the call has returned: the library copies the table)
        if p.shape[0]:
            q.d_point = p.data_ptr()
            for k, v in out.items():
                setattr(q, "d_" + k, v.data_ptr())
            if distance is not None:
                q.d_distance = distance.data_ptr()
            _check("ctr_inside_points", _lib.hip_lib().ctr_inside_points(self._h, C.byref(q), raw))
        del keep

    def inside(self, points, object=None, dirs=None, linear=False, outputs=("inside",), stream=None):
        """Whether every point of `points` ((n, 3) float32) lies inside a body of the scene: a dict of (n,) tensors on the scene's
        device, `inside` (bool) and / or `votes` (uint8) as `outputs` names them.  R rays leave every point, over (0, +inf),
        counting meshes and spheres only (count_crossings' terms); `votes` is the number of rays with an odd count and a point is
        inside when that is more than half of R.  dirs: (R, 3), R odd, 1 .. 15 (None: the library's three default directions,
        inside_default_dirs()).  object: only this mesh or sphere (a plane or a stand-alone triangle raises).  Asking for `votes`
        casts all R rays of every point; without it a wave stops once all its points are decided.  A point with a NaN or an
        infinity in it is outside with 0 votes.  Asynchronous on `stream`."""
        import torch
        outputs = _subset("outputs", outputs, INSIDE_OUTPUTS, unique=True)
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            p = _array_check(points, "points", dev, "float32", 3).to(dev, non_blocking=False).contiguous()
            out = {k: torch.empty(p.shape[0], dtype=torch.uint8, device=dev) for k in outputs}
            self._inside(p, object, dirs, linear, out, None, raw)
            if "inside" in out:
                out["inside"] = out["inside"].view(torch.bool)   # the kernel writes 0 or 1
        return out

    def signed_distance(self, points, object=None, max_dist=float("inf"), dirs=None, linear=False, stream=None):
        """The distance of every point of `points` ((n, 3) float32) to the nearest mesh, sphere or stand-alone triangle, negative
        inside a body: (n,) float32 on the scene's device.  nearest_points' distance (skip_planes=True, the same `object`)
        with inside()'s sign, two launches on one stream.  A point farther than max_dist from everything keeps +inf, whatever
        its side.  object: only this mesh or sphere.  dirs, linear: as inside()."""
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            p = _array_check(points, "points", dev, "float32", 3).to(dev, non_blocking=False).contiguous()
            dist = self.nearest_points(p, max_dist=max_dist, object=object, skip_planes=True, linear=linear, outputs=("distance",),
                                       stream=stream)["distance"]
            self._inside(p, object, dirs, linear, {}, dist, raw)
        return dist

    def shade_rays(self, origins, dirs, bounces=5, min_t=1e-3, ambient=None, exact_pow=False, linear=False, outputs=None,
                   stream=None):
        """ray_color<S, bounces> (inc/shading.hpp:116-154) of every ray (origins[k], dirs[k]): Phong shading over every
        light, reflection and transparency recursed to `bounces` (0 .. 15), with the render's numerics.  A dict of tensors
        on the scene's device: `color` (n, 3) always ((0, 0, 0) on a miss), and of the FIRST cast's hit what `outputs`
        names among `t` (n,) (+inf: miss), `object` (n,) int32 (-1: miss), `normal` (n, 3).  origins, dirs: (n, 3) float32;
        directions need not be normalised.  min_t: ray_color's min_t (the render's fudge).  ambient: phong's ambient
        factor; None: that of the camera the scene was created with.  exact_pow=True: the specular term as under
        VAR_EXACT_POW (bitwise the reference's); linear=True: meshes walked linearly, exact also for rays in a triangle's
        plane.  Asynchronous on `stream` (a torch.cuda.Stream; default: torch's current stream of the scene's device)."""
        outputs = ("color",) if outputs is None else _subset("outputs", outputs, SHADE_OUTPUTS, allow_empty=True)
        outputs = ("color",) + tuple(k for k in outputs if k != "color")
        if not 0 <= int(bounces) <= 15:
            raise ValueError(f"bounces: 0 .. 15, got {bounces}")
        dev = self._torch_device()
        with _on_stream(dev, stream) as raw:
            o, d, n = _ray_pair(origins, dirs, dev)
            q = _lib.ShadeQuery()
            q.n_rays = n
            q.flags = (SHADE_LINEAR if linear else 0) | (SHADE_EXACT_POW if exact_pow else 0)
            q.bounces = int(bounces)
            q.min_t = float(min_t)
            q.ambient = float(self._ambient if ambient is None else ambient)
            out = _ray_outputs(outputs, n, dev)
            if n:
                q.d_origin, q.d_dir = o.data_ptr(), d.data_ptr()
                for k, v in out.items():
                    setattr(q, "d_" + k, v.data_ptr())
                _check("ctr_shade_rays", _lib.hip_lib().ctr_shade_rays(self._h, C.byref(q), raw))
        return out

    # ---- surface shading queries (ctr_shade_points, include/cutrace_rays.h) ----
    def shade_points(self, points, normals=None, view_dirs=None, materials=None, objects=None, ambient=None, exact_pow=False,
                     linear=False, outputs=("color",), stream=None):
        """phong (inc/shading.hpp:64-99) at caller-supplied surface points: the direct lighting of points[k] with normal
        normals[k], seen along view_dirs[k] (incoming->dir), over every light of the scene, each with its own shadow loop
        through the scene — with the numerics of shade_rays.  points, normals, view_dirs: (n, 3) float32, normals and view
        directions of any length.  materials: an int (every point's material) or (n,) int32 indices into the scene's
        materials; objects: (n,) int32 indices into the scene's objects — the point gets that object's material, and -1
        (cast_rays' `object` on a miss) gives (0, 0, 0): shade_points on the output of cast_rays is
        shade_rays(bounces=0).  An index outside its range gives NaN.  outputs: a non-empty subset of "color" (n, 3) and
        "light_shadow" (n, n_lights): shadow_intensity towards every light, in light order; for "light_shadow" alone only
        `points` is needed.  ambient: phong's ambient factor; None: that of the camera the scene was created with.
        exact_pow=True: the specular term as under VAR_EXACT_POW (bitwise the reference's); linear=True: meshes walked
        linearly (the default walk is exact for every point already: every ray cast here ends at a light, and the lights
        are guarded).  Returns a dict of tensors on the scene's device.  Asynchronous on `stream` (a torch.cuda.Stream;
        default: torch's current stream of the scene's device)."""
        import torch
        outputs = _subset("outputs", outputs, POINTS_OUTPUTS, unique=True)
        dev = self._torch_device()
        want_color = "color" in outputs
        if materials is not None and objects is not None:
            raise ValueError("materials and objects exclude each other")
        if want_color and materials is None and objects is None:
            raise ValueError("color needs materials or objects")
        if want_color and (normals is None or view_dirs is None):
            raise ValueError("color needs normals and view_dirs")
        pts = _array_check(points, "points", dev, "float32", 3)
        n = pts.shape[0]
        vec = {}
        for x, what in ((normals, "normals"), (view_dirs, "view_dirs")):
            if x is not None:
                vec[what] = _array_check(x, what, dev, "float32", 3)
                if vec[what].shape[0] != n:
                    raise ValueError(f"{what}: {vec[what].shape[0]} rows for {n} points")
        scalar_mat, idx, idx_name = 0, None, None
        if isinstance(materials, (int, np.integer)) and not isinstance(materials, bool):
            scalar_mat = int(materials)
        elif materials is not None:
            idx, idx_name = _array_check(materials, "materials", dev, "int32", 0), "d_material"
        elif objects is not None:
            idx, idx_name = _array_check(objects, "objects", dev, "int32", 0), "d_object"
        if idx is not None and idx.shape[0] != n:
            raise ValueError(f"{'materials' if idx_name == 'd_material' else 'objects'}: {idx.shape[0]} indices for {n} points")
        with _on_stream(dev, stream) as raw:
            # the query's arrays by the name of their field.  (The inputs must outlive the launch: `keep` holds what was
            # copied over until the call returns, and the stream orders the caching allocator's reuse after it)
            keep = {"d_point": pts.to(dev).contiguous()}
            q = _lib.PointQuery()
            q.n_points = n
            q.flags = (POINTS_LINEAR if linear else 0) | (POINTS_EXACT_POW if exact_pow else 0)
            q.material = scalar_mat
            q.ambient = float(self._ambient if ambient is None else ambient)
            shape = {"color": (n, 3), "light_shadow": (n, self.n_lights)}
            out = {k: torch.empty(shape[k], dtype=torch.float32, device=dev) for k in outputs}
            if want_color:
                keep["d_normal"], keep["d_view"] = _ray_pair(vec["normals"], vec["view_dirs"], dev)[:2]
                keep["d_color"] = out["color"]
                if idx is not None:
                    keep[idx_name] = idx.to(dev).contiguous()
            if "light_shadow" in out and self.n_lights:
                keep["d_light_shadow"] = out["light_shadow"]
            if n and (want_color or self.n_lights):
                for field, t in keep.items():
                    setattr(q, field, t.data_ptr())
                _check("ctr_shade_points", _lib.hip_lib().ctr_shade_points(self._h, C.byref(q), raw))
        return out

    # ---- the lens render (ctr_render_device_lens, include/cutrace_lens.h) ----
    def render_lens(self, origins, dirs, fudge=1e-3, bounces=5, rows=None, samples=1, ambient=None, stream=None):
        """The render kernel on caller-supplied primary rays: pixel (x, y) of the scene's current w x h frame holds what the
        plain render holds for the ray (origins[y, x], dirs[y, x].normalized()) in place of the camera's.  origins, dirs:
        float32 of shape (H, W, 3) or (H*W, 3), torch tensors on the scene's device or numpy arrays (uploaded), with
        H, W = samples*h, samples*w — the whole frame also when `rows` selects a part.  samples = 2, 4 or 8: one ray per
        sample, box-filtered in the kernel as render(samples=...) filters.  A ray with a non-finite origin, or a NaN,
        infinite or zero direction, is masked: no cast, depth +inf, normal and colour 0 (`lenses.fisheye` masks what lies
        outside its image circle).  ambient: phong's ambient factor; None: that of the camera the scene was created with.
        Returns tensors on the scene's device — `depth` (n, w), `color` (n, w, 3), `normal` (n, w, 3) for the n selected
        rows — plus `ray_count` and `max_depth`; reading those two waits for the launch, which is otherwise asynchronous on
        `stream` (a torch.cuda.Stream; default: torch's current stream of the scene's device)."""
        import torch
        samples = self._samples(samples)
        L = _lib.hip_lib()
        r = make_rows(self.h, rows)
        n = rows_count(self.h, rows)
        dev = self._torch_device()
        H, W = samples * self.h, samples * self.w
        with _on_stream(dev, stream) as raw:
            o, d, _ = _ray_pair(origins, dirs, dev, frame=(H, W))
            depth = torch.empty(n, self.w, dtype=torch.float32, device=dev)
            color = torch.empty(n, self.w, 3, dtype=torch.float32, device=dev)
            normal = torch.empty(n, self.w, 3, dtype=torch.float32, device=dev)
            counters = torch.zeros(16, dtype=torch.int64, device=dev)
            q = _lib.Lens()
            q.n_rays = H * W
            q.samples = samples
            q.ambient = float(self._ambient if ambient is None else ambient)
            q.d_origin, q.d_dir = o.data_ptr() or None, d.data_ptr() or None
            _check("ctr_render_device_lens", L.ctr_render_device_lens(self._h, C.c_float(fudge), int(bounces), C.byref(q), C.byref(r),
                                                                      depth.data_ptr() or None, color.data_ptr() or None,
                                                                      normal.data_ptr() or None, counters.data_ptr(), raw))
            # (the rays must outlive the launch: tensors made here are kept until the counters have been read)
            c = counters.cpu()
        md = np.array([int(c[1]) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]
        return dict(depth=depth, color=color, normal=normal, ray_count=int(c[0]), max_depth=float(md), rows=n)

    # ---- mesh updates (ctr_scene_update_mesh, include/cutrace_update.h) ----
    def update_mesh(self, obj, triangles, stream=None):
        """New vertices for mesh `obj` (its index in the scene's objects): `triangles` is (n, 3, 3) float32 — n the mesh's
        triangle count, file order, [triangle][p1, p2, p3][x, y, z] — either a contiguous torch tensor on the scene's device
        (read in place) or a numpy array.  The mesh's tree keeps its shape and is refitted on the GPU; afterwards every
        render and query gives, bit for bit, what a scene created with these triangles gives.  The device work is queued on
        `stream` (a torch.cuda.Stream; default: torch's current stream of the scene's device), after whatever produced the
        tensor there; the call returns when the handle is consistent again.  A wrong count, an object that is not a mesh
        or a vertex that is not finite raise RuntimeError and leave the scene as it was."""
        dev = self._torch_device()
        triangles, ptr = self._mesh_triangles(triangles, dev)
        with _on_stream(dev, stream) as raw:
            _check("ctr_scene_update_mesh", _lib.hip_lib().ctr_scene_update_mesh(self._h, int(obj), C.c_void_p(ptr or None),
                                                                                 int(triangles.shape[0]), raw))

    def rebuild_mesh(self, obj, triangles, builder="device", stream=None):
        """update_mesh plus a NEW tree for the mesh (ctr_scene_rebuild_mesh, include/cutrace_rebuild.h): for vertices the old
        tree's shape no longer fits — a fold, a long twist, a cloth.  builder="device": a linear BVH built on the GPU;
        "host": the binned-SAH builder a new scene gets.  The same inputs, stream and errors as update_mesh, the same
        results bit for bit as a scene created with these triangles; only the frame time depends on the builder.  Returns
        what was built: builder (0 device, 1 host), fell_back (1: the device's tree was refused by the host's checks and the
        host built instead), node_count, levels, moved (1: the tree lives in a new range of the node array)."""
        if builder not in ("device", "host"):
            raise ValueError(f"builder: expected 'device' or 'host', got {builder!r}")
        dev = self._torch_device()
        triangles, ptr = self._mesh_triangles(triangles, dev)
        info = _lib.RebuildInfo()
        with _on_stream(dev, stream) as raw:
            _check("ctr_scene_rebuild_mesh", _lib.hip_lib().ctr_scene_rebuild_mesh(
                self._h, int(obj), C.c_void_p(ptr or None), int(triangles.shape[0]), _lib.REBUILD_HOST if builder == "host" else 0, C.byref(info), raw))
        return {k: int(getattr(info, k)) for k in ("builder", "fell_back", "node_count", "levels", "moved")}

    def replace_mesh(self, obj, triangles, builder="device", stream=None):
        """rebuild_mesh with ANOTHER triangle count (ctr_scene_replace_mesh, include/cutrace_replace.h): `triangles` is (n, 3, 3)
        float32 with any n from 1 to 0xFFFFFF — an isosurface extracted anew, a level-of-detail switch, a body that fractures.
        The same inputs, builders and stream as rebuild_mesh, the same results bit for bit as a scene created with these
        triangles; the handle keeps its buffers, its tile history and its other meshes.  Returns what was built and what moved:
        builder, fell_back, node_count, levels as rebuild_mesh; nodes_moved, tris_moved (1: that range of the mesh lives at the
        end of its array now, with room for twice what it had); tri_cap (the triangles the mesh's range has room for now).
        n = 0, an object that is not a mesh or is an empty mesh, or a vertex that is not finite raise RuntimeError and leave the
        scene as it was."""
        if builder not in ("device", "host"):
            raise ValueError(f"builder: expected 'device' or 'host', got {builder!r}")
        dev = self._torch_device()
        triangles, ptr = self._mesh_triangles(triangles, dev)
        info = _lib.ReplaceInfo()
        with _on_stream(dev, stream) as raw:
            _check("ctr_scene_replace_mesh", _lib.hip_lib().ctr_scene_replace_mesh(
                self._h, int(obj), C.c_void_p(ptr or None), int(triangles.shape[0]), _lib.REPLACE_HOST if builder == "host" else 0, C.byref(info), raw))
        return {k: int(getattr(info, k)) for k in ("builder", "fell_back", "node_count", "levels", "nodes_moved", "tris_moved", "tri_cap")}

    @staticmethod
    def _mesh_triangles(triangles, dev):
        """update_mesh's, rebuild_mesh's and replace_mesh's input, checked: (the array or tensor to keep alive, its address)"""
        import torch
        if isinstance(triangles, torch.Tensor):
            if triangles.device != dev:
                raise ValueError(f"triangles: tensor on {triangles.device}, the scene lives on {dev}")
            if not triangles.is_contiguous():
                raise ValueError("triangles: expected a contiguous tensor")
            dtype_ok, ptr = triangles.dtype == torch.float32, triangles.data_ptr()
        elif isinstance(triangles, np.ndarray):
            triangles = np.ascontiguousarray(triangles)
            dtype_ok, ptr = triangles.dtype == np.float32, triangles.ctypes.data
        else:
            raise TypeError(f"triangles: expected a torch tensor or a numpy array, got {type(triangles).__name__}")
        if not dtype_ok or len(triangles.shape) != 3 or tuple(triangles.shape[1:]) != (3, 3):
            raise ValueError(f"triangles: expected float32 of shape (n, 3, 3), got {triangles.dtype} {tuple(triangles.shape)}")
        return triangles, ptr

    def mesh_box(self, obj):
        """The current box of mesh `obj` as the kernels use it (ctr_scene_mesh_box): (min, max), two float32 arrays of 3."""
        lo, hi = Vec3(), Vec3()
        _check("ctr_scene_mesh_box", _lib.hip_lib().ctr_scene_mesh_box(self._h, int(obj), C.byref(lo), C.byref(hi)))
        return np.array(lo.tup(), np.float32), np.array(hi.tup(), np.float32)

    # ---- live lights and materials (include/cutrace_edit.h) ----
    def set_lights(self, lights):
        """Replace the scene's lights (ctr_scene_set_lights): a sequence of _lib.Light, of any length including 0.  Afterwards
        every render and query gives, bit for bit, what a scene created with these lights gives; shade_points' light_shadow
        has the new width.  Synchronous.  A bad light type raises RuntimeError and leaves the scene as it was."""
        arr = _records(Light, lights, "lights")
        _check("ctr_scene_set_lights", _lib.hip_lib().ctr_scene_set_lights(self._h, arr, len(arr)))
        self.n_lights = len(arr)

    def set_materials(self, materials):
        """Replace the scene's materials (ctr_scene_set_materials): a sequence of _lib.Material; the count may change as long
        as every object's material index stays below it.  Afterwards every render and query gives, bit for bit, what a scene
        created with these materials gives.  Synchronous.  A bad material type or a count that leaves an object out of
        range raise RuntimeError and leave the scene as it was."""
        arr = _records(Material, materials, "materials")
        _check("ctr_scene_set_materials", _lib.hip_lib().ctr_scene_set_materials(self._h, arr, len(arr)))
        self._materials = arr

    def set_material(self, idx, **kw):
        """HostScene.set_material on the live scene: material `idx` with the given fields replaced (color: three floats)."""
        if isinstance(idx, bool) or not isinstance(idx, (int, np.integer)) or not 0 <= idx < len(self._materials):
            raise ValueError(f"bad material index {idx!r}")
        arr = _records(Material, self._materials)
        for k, v in kw.items():
            if k not in ("color", "specular", "reflexivity", "phong_exp", "transparency"):
                raise TypeError(f"set_material: no material field {k!r}")
            setattr(arr[idx], k, Vec3(*v) if k == "color" else v)
        self.set_materials(arr)

    # ---- live objects (include/cutrace_objects.h) ----
    # what set_object may change per object type, named as the scene JSON names it -> the field of _lib.Object
    _OBJECT_FIELDS = {0: {"p1": "v0", "p2": "v1", "p3": "v2"}, 1: {}, 2: {"point": "v0", "normal": "v1"}, 3: {"center": "v0", "radius": "f0"}}

    def set_objects(self, objects):
        """Replace the parameters of the scene's objects (ctr_scene_set_objects): a sequence of _lib.Object, one per object of
        the scene, each of the type it was created with.  A sphere's centre and radius, a plane's point and normal, a
        stand-alone triangle's points and any object's material index may differ; a mesh keeps its triangles, tree and box.
        Afterwards every render and query gives, bit for bit, what a scene created with these objects gives.  Synchronous.
        Another count or type, a mesh with another triangle count or a material index out of range raise RuntimeError and
        leave the scene as it was."""
        arr = _records(Object, objects, "objects")
        _check("ctr_scene_set_objects", _lib.hip_lib().ctr_scene_set_objects(self._h, arr, len(arr)))

    def object_count(self):
        """How many objects the scene has (ctr_scene_object_count)."""
        n = C.c_uint64()
        _check("ctr_scene_object_count", _lib.hip_lib().ctr_scene_object_count(self._h, C.byref(n)))
        return int(n.value)

    def get_object(self, i):
        """Object `i` as a _lib.Object that set_objects takes back unchanged (ctr_scene_get_object): its type, current material
        index and current parameters; a mesh with its current box in v0 / v1."""
        o = Object()
        _check("ctr_scene_get_object", _lib.hip_lib().ctr_scene_get_object(self._h, int(i), C.byref(o)))
        return o

    def set_object(self, i, **fields):
        """Object `i` with the given fields replaced, every other object as it is: center, radius (a sphere), point, normal (a
        plane), p1, p2, p3 (a stand-alone triangle), material (any object: an index into the scene's materials)."""
        n = self.object_count()
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < n:
            raise ValueError(f"bad object index {i!r}")
        objs = [self.get_object(k) for k in range(n)]
        own = self._OBJECT_FIELDS.get(int(objs[i].type), {})
        for k, v in fields.items():
            if k == "material":
                objs[i].mat_idx = v
            elif k in own:
                setattr(objs[i], own[k], v if k == "radius" else Vec3(*v))
            else:
                raise TypeError(f"set_object: an object of type {int(objs[i].type)} has no field {k!r}")
        self.set_objects(objs)

    # ---- a live object count (include/cutrace_topology.h) ----
    _OBJECT_KINDS = {"triangle": 0, "plane": 2, "sphere": 3}

    def add_object(self, kind, material=0, **fields):
        """Append a sphere, a plane or a stand-alone triangle (ctr_scene_add_object): `kind` is "sphere", "plane" or "triangle",
        the fields are set_object's — center, radius; point, normal; p1, p2, p3 — and `material` an index into the scene's
        materials.  Returns the new object's index, the object count before the call.  Afterwards every render and query gives,
        bit for bit, what a scene created with the object appended gives.  A mesh is added by add_mesh."""
        if kind not in self._OBJECT_KINDS:
            raise ValueError(f"kind: expected 'sphere', 'plane' or 'triangle', got {kind!r}")
        if isinstance(material, bool) or not isinstance(material, (int, np.integer)) or material < 0:
            raise ValueError(f"bad material index {material!r}")
        o = Object()
        o.type, o.mat_idx = self._OBJECT_KINDS[kind], int(material)
        own = self._OBJECT_FIELDS[int(o.type)]
        for k, v in fields.items():
            if k not in own:
                raise TypeError(f"add_object: a {kind} has no field {k!r}")
            setattr(o, own[k], v if k == "radius" else Vec3(*v))
        index = C.c_uint64()
        _check("ctr_scene_add_object", _lib.hip_lib().ctr_scene_add_object(self._h, C.byref(o), C.byref(index)))
        return int(index.value)

    def add_mesh(self, triangles, material=0, builder="device", stream=None):
        """Append a mesh (ctr_scene_add_mesh): `triangles`, `builder` and `stream` are replace_mesh's, `material` an index into
        the scene's materials.  Afterwards every render and query gives, bit for bit, what a scene created with the mesh
        appended gives.  Returns what was built and where: index (the new object's), builder, fell_back, node_count, levels
        as replace_mesh; tris_reused, nodes_reused (1: the mesh lives in a range of that array that a removed object left
        behind); tri_cap (the triangles its range has room for).  n = 0, a material index out of range or a vertex that is not
        finite raise RuntimeError and leave the scene as it was."""
        if builder not in ("device", "host"):
            raise ValueError(f"builder: expected 'device' or 'host', got {builder!r}")
        if isinstance(material, bool) or not isinstance(material, (int, np.integer)) or material < 0:
            raise ValueError(f"bad material index {material!r}")
        dev = self._torch_device()
        triangles, ptr = self._mesh_triangles(triangles, dev)
        info = _lib.AddInfo()
        with _on_stream(dev, stream) as raw:
            _check("ctr_scene_add_mesh", _lib.hip_lib().ctr_scene_add_mesh(
                self._h, int(material), C.c_void_p(ptr or None), int(triangles.shape[0]), _lib.ADD_HOST if builder == "host" else 0, C.byref(info), raw))
        return {k: int(getattr(info, k)) for k in ("index", "builder", "fell_back", "node_count", "levels", "tris_reused", "nodes_reused", "tri_cap")}

    def remove_object(self, i):
        """Remove object `i`, of any type (ctr_scene_remove_object); the objects behind it move down by one index.  Afterwards
        every render and query gives, bit for bit, what a scene created without the object gives."""
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < self.object_count():
            raise ValueError(f"bad object index {i!r}")
        _check("ctr_scene_remove_object", _lib.hip_lib().ctr_scene_remove_object(self._h, int(i)))

    def room(self):
        """How much of the scene's triangle and node arrays is in use (ctr_scene_room): tris_live, tris_total, nodes4_live,
        nodes4_total — the records inside a range some object owns, and the records of the array."""
        r = _lib.SceneRoom()
        _check("ctr_scene_room", _lib.hip_lib().ctr_scene_room(self._h, C.byref(r)))
        return {k: int(getattr(r, k)) for k in ("tris_live", "tris_total", "nodes4_live", "nodes4_total")}

    def guard_state(self, obj):
        """Test hook (ctr_debug_guard_state): (file indices of mesh `obj`'s triangles in its guard records, ascending, as a
        list; whether the mesh is walked linearly)."""
        L = _lib.hip_lib()
        n, linear = C.c_uint64(), C.c_int()
        _check("ctr_debug_guard_state", L.ctr_debug_guard_state(self._h, int(obj), None, 0, C.byref(n), C.byref(linear)))
        out = (C.c_uint32 * max(int(n.value), 1))()
        _check("ctr_debug_guard_state", L.ctr_debug_guard_state(self._h, int(obj), out, int(n.value), C.byref(n), C.byref(linear)))
        return [int(out[k]) for k in range(int(n.value))], bool(linear.value)

    def tile_costs(self):
        """Per-tile cost of the last launch (ctr_tile_costs), as a uint32 array."""
        L = _lib.hip_lib()
        n = C.c_uint64()
        L.ctr_tile_costs(self._h, None, 0, C.byref(n))
        out = np.zeros(int(n.value), np.uint32)
        if n.value:
            L.ctr_tile_costs(self._h, out.ctypes.data, n.value, C.byref(n))
        return out

    def close(self):
        if self._h:
            self._free_pinned()
            _lib.hip_lib().ctr_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiScene:
    """A scene replicated on several GPUs of this process (ctr_multi_create): one frame per call, row-tiled over the
    devices, gathered to devices[0] (RCCL) and re-interleaved there (ctr_render_multi)."""

    def __init__(self, host_scene, devices):
        L = _lib.hip_lib()
        h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        _check("ctr_multi_create", L.ctr_multi_create(host_scene.desc, devs, len(devices), C.byref(h)))
        self._h = h
        self.devices = list(devices)
        self.w, self.h = host_scene.size

    @property
    def transport(self):
        return _lib.hip_lib().ctr_multi_transport(self._h).decode()

    def set_variant(self, bits):
        _check("ctr_multi_set_variant", _lib.hip_lib().ctr_multi_set_variant(self._h, bits))

    def set_size(self, w, h):
        _check("ctr_multi_set_size", _lib.hip_lib().ctr_multi_set_size(self._h, w, h))
        self.w, self.h = w, h

    def render(self, fudge=1e-3, bounces=5, block_rows=8, pinned=False):
        """pinned=True: the buffers are views of a page-locked frame block of this group (valid until the next pinned
        render / close); device 0 then writes the frame into it directly."""
        L = _lib.hip_lib()
        px = self.w * self.h
        fr = _frame_views(_pinned_block(self, px, grow_only=False), px, self.h, self.w) if pinned else _empty_frame(self.h, self.w)
        stats = RenderStats()
        _check("ctr_render_multi", L.ctr_render_multi(self._h, C.c_float(fudge), bounces, block_rows, fr["depth"].ctypes.data,
                                                      fr["color"].ctypes.data, fr["normal"].ctypes.data, C.byref(stats)))
        return dict(fr, **self._stats(stats))

    def _stats(self, stats):
        ms = (C.c_double * len(self.devices))()
        _lib.hip_lib().ctr_multi_kernel_ms(self._h, ms, len(self.devices))
        return dict(_stats_dict(stats), kernel_ms_per_device=list(ms))

    def alloc_frame(self):
        """A page-locked frame block of the group's size (ctr_frame_alloc): dict of depth / color / normal views + a
        handle to pass to free_frame.  Page-locked destinations keep ctr_multi_submit asynchronous."""
        px = self.w * self.h
        ptr, blk = _frame_alloc(px)
        return dict(_frame_views(blk, px, self.h, self.w), _ptr=ptr)

    @staticmethod
    def free_frame(fr):
        _lib.hip_lib().ctr_frame_free(fr["_ptr"])

    def submit(self, into, fudge=1e-3, bounces=5, block_rows=8):
        """Queue one frame into the buffers of `into` (dict with depth / color / normal arrays of the group's size) and
        return at once (ctr_multi_submit); at most two frames in flight."""
        L = _lib.hip_lib()
        _check("ctr_multi_submit", L.ctr_multi_submit(self._h, C.c_float(fudge), bounces, block_rows, into["depth"].ctypes.data,
                                                      into["color"].ctypes.data, into["normal"].ctypes.data))

    def wait(self):
        """Block until the oldest queued frame is complete (ctr_multi_wait); returns its statistics."""
        stats = RenderStats()
        _check("ctr_multi_wait", _lib.hip_lib().ctr_multi_wait(self._h, C.byref(stats)))
        return self._stats(stats)

    def _free_pinned(self):
        _free_pinned_block(self)

    def close(self):
        if self._h:
            self._free_pinned()
            _lib.hip_lib().ctr_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
