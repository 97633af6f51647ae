"""Display frames (include/cutrace_images.h), what can be checked without a GPU: the two entry points exist, the header is C,
the invalid calls are turned away before the GPU is touched, and the numpy restatement the GPU test expects its bytes from
(tests/images_ref.py) equals the host quantisers and the oracle's on the very inputs the GPU test uses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle

from cutrace_amd import _lib
from tests import images_ref as ir
from tests.checkers import declared

ROOT = _lib.ROOT
f32 = np.float32


def test_library_exports_the_images_entry_points():
    names = declared("cutrace_images.h")
    assert set(names) == set(_lib.IMAGES_SYMBOLS) == {"ctr_quantise_device", "ctr_render_images"}
    assert not set(names) & (set(_lib.HIP_SYMBOLS) | set(_lib.HOST_SYMBOLS))  # cutrace_amd.h and cutrace_host.h are unchanged
    L = _lib.hip_lib()
    for n in names:
        assert hasattr(L, n), f"libcutrace_amd.so does not export {n}"
    assert L.ctr_abi_version() == 3
    assert C.sizeof(_lib.ImagePlanes) == 72


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    src = tmp_path / "images.c"
    src.write_text('#include "cutrace_images.h"\n'
                   "int (*device_form)(int, const ctr_image_planes *, void *) = ctr_quantise_device;\n"
                   "int (*host_form)(ctr_scene *, float, int, uint32_t, const ctr_rows *, uint8_t *, uint8_t *, uint8_t *, ctr_render_stats *) = ctr_render_images;\n"
                   "typedef char planes_size[sizeof(ctr_image_planes) == 72 ? 1 : -1];\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o",
                           str(tmp_path / "images.o"), str(src)])


def _planes(**kw):
    p = _lib.ImagePlanes()
    p.n_pixels = 4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_quantise_device_rejects_before_the_gpu():
    """every CTR_E_INVALID case of ctr_quantise_device: 1 and a message — on a machine with no GPU, and with pointers
    that no kernel may ever see (host memory)"""
    L = _lib.hip_lib()
    host = np.zeros(64, f32)
    a, b = host.ctypes.data, host.ctypes.data + 128

    def bad(p, word):
        st = L.ctr_quantise_device(0, C.byref(p) if p is not None else None, None)
        msg = L.ctr_last_error().decode()
        assert st == 1 and msg.startswith("ctr_quantise_device: ") and word in msg, (st, msg)

    bad(None, "null planes")
    bad(_planes(), "no plane")
    bad(_planes(d_counters=a, max_depth=1.0), "no plane")
    bad(_planes(d_depth=a), "d_depth without d_depth8")
    bad(_planes(d_color8=b), "d_color8 without d_color3")
    bad(_planes(d_color3=a, d_color8=b, d_normal3=a), "d_normal3 without d_normal8")
    bad(_planes(d_color3=a, d_color8=b, reserved=1), "reserved")
    bad(_planes(d_color3=a, d_color8=b), "d_color3 is not device memory of device 0")
    bad(_planes(d_depth=a, d_depth8=b, max_depth=1.0), "d_depth is not device memory")
    # n_pixels == 0: nothing is launched, nothing is looked at
    assert L.ctr_quantise_device(0, C.byref(_planes(n_pixels=0, d_color3=a, d_color8=b)), None) == 0


def test_render_images_rejects_before_the_gpu():
    L = _lib.hip_lib()
    out = np.zeros(64, np.uint8)
    assert L.ctr_render_images(None, C.c_float(1e-3), 5, 1, None, out.ctypes.data, None, None, None) == 1
    assert b"null scene" in L.ctr_last_error()
    assert L.ctr_render_images(None, C.c_float(1e-3), 5, 1, None, None, None, None, None) == 1
    assert b"ctr_render_images: no destination plane" in L.ctr_last_error()


def _host_and_oracle(kind, data, n, *extra):
    outs = []
    for lib, pre in ((_lib.host_lib(), "ctr"), (oracle.oracle_lib(), "orc")):
        out = np.zeros((n, 3), np.uint8)
        getattr(lib, f"{pre}_quantise_{kind}")(data.ctypes.data, n, *extra, out.ctypes.data)
        outs.append(out)
    return outs


def test_numpy_restatement_equals_host_and_oracle_quantisers():
    """pins the GPU test's expectation to the reference's arithmetic as this machine's C compilers evaluate it"""
    c = ir.color_cases()
    for got in _host_and_oracle("color", c, len(c)):
        assert np.array_equal(got, ir.quantise_color(c))
    for m, d in ir.depth_cases():
        want = ir.quantise_depth(d, m)
        assert want[d == m].max() == 0 and want[d == 0].min() == 255 and want[np.isinf(d)].max() == 0
        for got in _host_and_oracle("depth", d, len(d), C.c_float(m)):
            assert np.array_equal(got, want), m
    n = np.concatenate([ir.normal_cases(), ir.contraction_fixture()])
    want = ir.quantise_normal(n)
    for got in _host_and_oracle("normal", n, len(n)):
        assert np.array_equal(got, want)
    depth, color, normal, m = ir.random_pixels(1 << 20)
    for kind, data, want, extra in (("depth", depth, ir.quantise_depth(depth, m), (C.c_float(m),)),
                                    ("color", color, ir.quantise_color(color), ()),
                                    ("normal", normal, ir.quantise_normal(normal), ())):
        for got in _host_and_oracle(kind, data, 1 << 20, *extra):
            assert np.array_equal(got, want), kind


def test_threshold_of_the_normal_rule_is_compared_in_double():
    e6 = f32(1e-6)
    n = np.array([[np.nextafter(e6, f32(0)), 0, 0], [e6, 0, 0], [np.nextafter(e6, f32(1)), 0, 0], [0, 0, 0]], f32)
    got = ir.quantise_normal(n)
    # float32(1e-6) is below the double 1e-6: it and everything under it are "zero", the next float is a normal
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0] and got[3].tolist() == [0, 0, 0]
    assert got[2].tolist() == [255, 127, 127]   # (sqrt(x*x) == x in binary floating point: the length is exact)


def test_saturation_outside_the_hosts_contract():
    """what the header documents for the inputs the host leaves undefined (the GPU test expects these bytes)"""
    d = np.array([-1.0, 5.0, 0.0, 2.0], f32)
    assert ir.quantise_depth(d, 2.0)[:, 0].tolist() == [255, 0, 255, 0]
    assert ir.quantise_depth(np.array([0.0, -1.0, 1.0, np.inf], f32), 0.0)[:, 0].tolist() == [0, 255, 0, 0]
    n = np.array([[np.nan, 0, 1], [np.inf, 1, 0], [-np.inf, 0, 0], [3e38, 3e38, 0], [1, 0, np.nan]], f32)
    assert ir.quantise_normal(n).tolist() == [[0, 0, 0], [0, 127, 127], [0, 127, 127], [127, 127, 127], [0, 0, 0]]


def test_contraction_fixture_separates_the_two_evaluations():
    """tests/golden/images_contraction.npz (images_ref.make_contraction_fixture): at least 64 normals whose bytes differ
    when len^2 is formed with fused multiply-adds — a kernel that contracts fails the GPU test on them.

    Depth: NO search was run, and the helper has no fused evaluation of the depth rule, because there is none to write:
    contraction rewrites a product that feeds a sum or a difference, and 255*(max-v)/max has a difference feeding a
    product feeding a quotient.  The compiled kernel bears that out (test_kernel_assembly_does_not_depend_on_the_contract_mode:
    the depth path is the same instructions under -ffp-contract=fast).  Colour, 255*c: likewise."""
    n = ir.contraction_fixture()
    assert n.dtype == f32 and n.ndim == 2 and n.shape[1] == 3 and len(n) >= 64
    plain, fused = ir.quantise_normal(n), ir.quantise_normal(n, fused=True)
    assert (plain != fused).any(1).all()
    assert len(np.unique(n, axis=0)) == len(n)


@pytest.mark.parametrize("seed", [3])
def test_contraction_fixture_is_what_the_generator_makes(seed):
    assert np.array_equal(ir.make_contraction_fixture(seed=seed, want=8).view(np.uint32), ir.contraction_fixture()[:8].view(np.uint32))


def test_kernel_assembly_does_not_depend_on_the_contract_mode(tmp_path):
    """csrc/frame_images.hip cross-compiled for gfx950 with the library's flags, -ffp-contract=off against =fast (the mode
    that disregards pragmas): the same instruction stream, so a later change of that flag cannot change a byte"""
    from cutrace_amd import build
    base = [f for f in build.HIP_FLAGS if not f.startswith("-ffp-contract")]
    streams = {}
    for mode in ("off", "fast"):
        out = tmp_path / f"{mode}.s"
        subprocess.check_call([build.hipcc(), *base, f"-ffp-contract={mode}", "--offload-device-only", "-S", "-o", str(out),
                               os.path.join(build.CSRC, "frame_images.hip")], stderr=subprocess.DEVNULL)
        streams[mode] = [ln.strip() for ln in out.read_text().splitlines()
                         if ln.startswith("\t") and not ln.strip().startswith((";", ".")) ]
    assert any(ln.startswith("v_mul_f32") for ln in streams["off"]) and len(streams["off"]) > 100
    assert streams["off"] == streams["fast"]
