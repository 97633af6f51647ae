"""The supersampled frame's definition (include/cutrace_aa.h) in numpy float32: the s*w x s*h render reduced block by
block — depth and normal of sample (0, 0), colour summed by repeated halving along x, then along y, then scaled."""
import numpy as np

f32 = np.float32


def _halve(a, axis):
    """a[i] = a[2i] + a[2i+1] along `axis` until one value is left there (float32 adds, rounded once each)"""
    a = np.moveaxis(a, axis, 0)
    while a.shape[0] > 1:
        a = (a[0::2] + a[1::2]).astype(f32)
    return np.moveaxis(a, 0, axis)


def reduce_color(color, s):
    """(s*h, s*w, 3) float32 -> (h, w, 3): the tree of the definition"""
    assert s in (1, 2, 4, 8) and color.dtype == f32
    hh, ww, _ = color.shape
    assert hh % s == 0 and ww % s == 0
    a = color.reshape(hh // s, s, ww // s, s, 3)
    a = _halve(a, 3)
    a = _halve(a, 1)
    return (a.reshape(hh // s, ww // s, 3) * f32(1.0 / (s * s))).astype(f32)


def reduce_frame(big, s):
    """the oracle's dict of the s*w x s*h render -> depth / normal / color of the supersampled w x h frame"""
    return dict(depth=np.ascontiguousarray(big["depth"][::s, ::s]), normal=np.ascontiguousarray(big["normal"][::s, ::s]),
                color=reduce_color(np.ascontiguousarray(big["color"], f32), s))


def raster_color(color, s):
    """the same mean summed in raster order (what the definition is NOT): to show that a bitwise test pins the order"""
    hh, ww, _ = color.shape
    a = color.reshape(hh // s, s, ww // s, s, 3)
    acc = np.zeros((hh // s, ww // s, 3), f32)
    for sy in range(s):
        for sx in range(s):
            acc = (acc + a[:, sy, :, sx]).astype(f32)
    return (acc * f32(1.0 / (s * s))).astype(f32)
