"""The Python bindings' shared pieces (cutrace_amd/_lib.py's prototype tables, cutrace_amd/__init__.py's helpers): no GPU."""
import ctypes as C

import numpy as np
import pytest

from cutrace_amd import _lib


def test_symbol_lists_are_the_tables_keys_and_every_prototype_is_applied():
    lists = (_lib.HOST_SYMBOLS, _lib.HIP_SYMBOLS, _lib.RAY_SYMBOLS, _lib.AA_SYMBOLS, _lib.LENS_SYMBOLS, _lib.IMAGES_SYMBOLS)
    tables = [(_lib.host_lib(), _lib.HOST_PROTOS), (_lib.hip_lib(), _lib.HIP_PROTOS)]
    keys = [name for _, protos in tables for symbols in protos.values() for name in symbols]
    assert len(keys) == len(set(keys)) == sum(len(x) for x in lists)  # no symbol twice, in a table or in a list
    assert set(keys) == set().union(*lists)
    assert _lib.LENS_SYMBOLS == sorted(_lib.LENS_SYMBOLS)
    for L, protos in tables:
        for symbols in protos.values():
            for name, proto in symbols.items():
                fn = getattr(L, name)  # both libraries are this tree's: they export everything
                assert (fn.argtypes, fn.restype) == (proto or (None, C.c_int)), name  # (no prototype: ctypes' defaults)


def test_check_returns_on_zero_and_raises_with_status_and_text(ca):
    assert ca._check("ctr_render", 0) is None
    st = _lib.hip_lib().ctr_render(None, C.c_float(1e-3), 5, None, None, None, None, None)
    assert st == 1
    with pytest.raises(RuntimeError) as e:
        ca._check("ctr_render", st)
    assert str(e.value).startswith("ctr_render failed (1): ") and "null scene" in str(e.value)


def test_stats_dict_has_the_five_keys(ca):
    s = ca.RenderStats(kernel_ms=1.5, total_ms=2.5, ray_count=7, rows=3, max_depth=4.25)
    d = ca._stats_dict(s)
    assert d == dict(ray_count=7, kernel_ms=1.5, total_ms=2.5, max_depth=4.25, rows=3) and len(d) == 5
    assert {k: type(v) for k, v in d.items()} == dict(ray_count=int, kernel_ms=float, total_ms=float, max_depth=float, rows=int)


def test_frame_views_share_the_block(ca):
    n, w = 3, 5
    px = n * w
    blk = np.arange(7 * px, dtype=np.float32)
    v = ca._frame_views(blk, px, n, w)
    assert list(v) == ["depth", "color", "normal"]
    assert v["depth"].shape == (n, w) and v["color"].shape == (n, w, 3) and v["normal"].shape == (n, w, 3)
    assert all(np.shares_memory(x, blk) for x in v.values())
    assert v["depth"].ctypes.data == blk.ctypes.data and v["depth"][0, 0] == 0
    assert v["color"].ctypes.data == blk[px:].ctypes.data and v["color"][0, 0, 0] == px
    assert v["normal"].ctypes.data == blk[4 * px:].ctypes.data and v["normal"][0, 0, 0] == 4 * px
    assert v["normal"][-1, -1, -1] == 7 * px - 1
    e = ca._frame_views(np.zeros(7, np.float32), 1, 0, w)  # no rows: px = max(0 * w, 1)
    assert e["depth"].shape == (0, w) and e["color"].shape == (0, w, 3) and e["normal"].shape == (0, w, 3)
    assert all(x.dtype == np.float32 for x in e.values())


def test_empty_frame(ca):
    f = ca._empty_frame(2, 3)
    assert {k: (x.shape, x.dtype) for k, x in f.items()} == dict(depth=((2, 3), np.float32), color=((2, 3, 3), np.float32),
                                                                 normal=((2, 3, 3), np.float32))
    u = ca._empty_frame(2, 3, uv=True)
    assert list(u) == ["depth", "color", "normal", "uv"] and u["uv"].shape == (2, 3, 2) and u["uv"].dtype == np.float32


def test_subset(ca):
    names = ("a", "b", "c")
    assert ca._subset("x", ["c", "a"], names) == ("c", "a")
    with pytest.raises(ValueError, match=r"x: a non-empty subset of \('a', 'b', 'c'\), got \('a', 'z'\)"):
        ca._subset("x", ("a", "z"), names)
    with pytest.raises(ValueError, match="x: a subset of"):
        ca._subset("x", ("z",), names, allow_empty=True)
    assert ca._subset("x", ("a", "a"), names) == ("a", "a")
    with pytest.raises(ValueError):
        ca._subset("x", ("a", "a"), names, unique=True)
    with pytest.raises(ValueError, match="non-empty"):
        ca._subset("x", (), names)
    assert ca._subset("x", (), names, allow_empty=True) == ()


def test_every_ray_output_has_a_shape(ca):
    assert set(ca._RAY_OUT) == set(ca.RAY_OUTPUTS) | set(ca.SHADE_OUTPUTS)


def test_rays_are_validated_before_anything_moves_to_the_device(ca):
    """Every error below is raised on a machine without a GPU too: nothing has been copied to cuda:0 by then."""
    import torch
    dev = torch.device("cuda", 0)
    ok = np.zeros((4, 3), np.float32)
    with pytest.raises(TypeError, match="origins: expected a torch tensor or a numpy array, got list"):
        ca._ray_pair([[0.0, 0.0, 0.0]], ok, dev)
    with pytest.raises(TypeError, match="dirs: expected"):
        ca._ray_pair(ok, [[0.0, 0.0, 0.0]], dev)
    with pytest.raises(ValueError, match=r"origins: expected float32 of shape \(n, 3\), got torch.float64 \(4, 3\)"):
        ca._ray_pair(ok.astype(np.float64), ok, dev)
    with pytest.raises(ValueError, match=r"dirs: expected float32 of shape \(n, 3\), got torch.float32 \(4, 2\)"):
        ca._ray_pair(ok, torch.zeros(4, 2), dev)
    with pytest.raises(ValueError, match="dirs: 5 rays for 4 origins"):
        ca._ray_pair(ok, np.zeros((5, 3), np.float32), dev)
    with pytest.raises(ValueError, match=r"min_t: expected float32 of shape \(n,\)"):
        ca._array_check(ok, "min_t", dev, "float32", 0)
    # the first error wins, as in the calls: origins before dirs, dirs before the count
    with pytest.raises(ValueError, match="origins: expected float32"):
        ca._ray_pair(ok.astype(np.float64), [1], dev)
    # the lens render's rays: (H, W, 3) or (H * W, 3)
    with pytest.raises(ValueError, match=r"origins: expected shape \(2, 2, 3\) or \(4, 3\), got \(2, 3, 3\)"):
        ca._ray_pair(np.zeros((2, 3, 3), np.float32), ok, dev, frame=(2, 2))
    with pytest.raises(ValueError, match=r"dirs: 5 rays for the 2 x 2 frame \(4\)"):
        ca._ray_pair(ok.reshape(2, 2, 3), np.zeros((5, 3), np.float32), dev, frame=(2, 2))


# _array_check(x, what, dev, dtype, cols): float rows of 3, per-ray scalars and int32 indices, each with a wrong type, dtype,
# rank and column count; (dtype, cols, x, the exception, its whole message)
_F3 = "expected float32 of shape (n, 3)"
_F0 = "expected float32 of shape (n,)"
_I0 = "expected int32 of shape (n,)"
ARRAY_CHECK_CASES = [
    ("float32", 3, [[0.0, 0.0, 0.0]], TypeError, "x: expected a torch tensor or a numpy array, got list"),
    ("float32", 3, np.zeros((4, 3), np.float64), ValueError, f"x: {_F3}, got torch.float64 (4, 3)"),
    ("float32", 3, np.zeros(4, np.float32), ValueError, f"x: {_F3}, got torch.float32 (4,)"),
    ("float32", 3, np.zeros((4, 3, 1), np.float32), ValueError, f"x: {_F3}, got torch.float32 (4, 3, 1)"),
    ("float32", 3, np.zeros((4, 2), np.float32), ValueError, f"x: {_F3}, got torch.float32 (4, 2)"),
    ("float32", 0, 1.5, TypeError, "x: expected a torch tensor or a numpy array, got float"),
    ("float32", 0, np.zeros(4, np.int32), ValueError, f"x: {_F0}, got torch.int32 (4,)"),
    ("float32", 0, np.zeros((4, 1), np.float32), ValueError, f"x: {_F0}, got torch.float32 (4, 1)"),
    ("float32", 0, np.zeros((4, 3), np.float32), ValueError, f"x: {_F0}, got torch.float32 (4, 3)"),
    ("int32", 0, "0", TypeError, "x: expected an int, a torch tensor or a numpy array, got str"),
    ("int32", 0, np.zeros(4, np.int64), ValueError, f"x: {_I0}, got torch.int64 (4,)"),
    ("int32", 0, np.zeros(4, np.float32), ValueError, f"x: {_I0}, got torch.float32 (4,)"),
    ("int32", 0, np.zeros((4, 1), np.int32), ValueError, f"x: {_I0}, got torch.int32 (4, 1)"),
    ("int32", 0, np.zeros((4, 3), np.int32), ValueError, f"x: {_I0}, got torch.int32 (4, 3)"),
]


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "torch"])
def test_array_check_names_what_is_wrong(ca, as_tensor):
    import torch
    dev = torch.device("cuda", 0)  # (constructing the device needs no GPU, and nothing below goes there)
    for dtype, cols, x, exc, text in ARRAY_CHECK_CASES:
        if as_tensor and isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        with pytest.raises(exc) as e:
            ca._array_check(x, "x", dev, dtype, cols)
        assert str(e.value) == text, (dtype, cols, text)


def test_array_check_returns_a_cpu_tensor_where_it_was(ca):
    import torch
    dev = torch.device("cuda", 0)
    for dtype, cols, shape in (("float32", 3, (4, 3)), ("float32", 0, (4,)), ("int32", 0, (4,)), ("float32", 3, (0, 3))):
        a = np.zeros(shape, dtype)
        got = ca._array_check(a, "x", dev, dtype, cols)
        assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and tuple(got.shape) == shape
        assert got.data_ptr() == a.ctypes.data or not a.size  # (no copy; an empty tensor has no address)
        t = torch.from_numpy(a)
        assert ca._array_check(t, "x", dev, dtype, cols) is t
