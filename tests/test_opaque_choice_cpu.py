"""Host logic (CPU, no GPU): opaque_build (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space — every build of both
kernel lists x shape in {0, 1} x the switch CUTRACE_NO_OPAQUE_BUILD —, the LDS the opaque builds ask for at bounces 0..15, and
the lemma the opaque builds rest on: a material whose transparency is anything but +0 or -0 makes the scene not all-opaque, and
no choice of choose_kernel on such a scene is an any-hit build (scripts/opaque_choice_check.cpp).

The rule: the opaque build is for the one-mesh shape of an any-hit build — the four builds of CTR_SHAPE_KERNELS — unless the
switch is set.  It depends on nothing else: an opaque build is built for the waves per SIMD of its parent twin and asks for the
same LDS (the launch's LDS size is a function of the build and the stack alone), so a launch that fits as the one fits as the
other at every bounce count, and there is none at which a launch falls back."""
import struct

from tests.checkers import CHOICE_SOURCES, FLATTEN_SOURCES, HOST_FLAGS, check_output, check_program

# scene_device.h KV_*
PREFILTER, ANYHIT, BVH, FASTPOW, OCC6, HOSTOUT = 1, 2, 8, 32, 64, 128
DEFAULT = PREFILTER | BVH | ANYHIT | FASTPOW
ONE_MESH_BUILDS = {DEFAULT, DEFAULT | OCC6, DEFAULT | HOSTOUT, DEFAULT | OCC6 | HOSTOUT}
KO_PARENT, KO_OPAQUE = 0, 1
GRANULE = 1280


def sections(tmp_path_factory):
    exe = check_program(tmp_path_factory, "opaque_choice_check", HOST_FLAGS, CHOICE_SOURCES + FLATTEN_SOURCES)
    lines = [l for l in check_output(exe, timeout=120).split("\n") if l]
    a, b = lines.index("lds"), lines.index("materials")
    return lines[:a], lines[a + 1:b], lines[b + 1:]


def test_the_opaque_build_is_for_the_one_mesh_shape_of_the_four_builds_unless_switched_off(tmp_path_factory):
    rule, _, _ = sections(tmp_path_factory)
    cases = [(int(kv, 16), int(shape), int(off), int(opq)) for kv, shape, off, opq in (l.split() for l in rule)]
    builds = sorted(set(c[0] for c in cases))
    assert len(builds) == 43 + 10 and len(cases) == 4 * len(builds)   # CTR_RENDER_KERNELS + CTR_LENS_KERNELS, each case once
    assert ONE_MESH_BUILDS <= set(builds)
    for kv, shape, off, opq in cases:
        # (launch_shape gives shape 1 to the four builds only; the rule itself asks for any-hit, which all four are)
        want = KO_OPAQUE if (shape == 1 and kv & ANYHIT and not off) else KO_PARENT
        assert opq == want, (hex(kv), shape, off, opq)
    assert all(opq == KO_PARENT for _, shape, off, opq in cases if shape == 0 or off)
    assert all(opq == KO_OPAQUE for kv, shape, off, opq in cases if kv in ONE_MESH_BUILDS and shape == 1 and not off)


def test_the_lds_of_a_launch_depends_on_the_build_and_the_stack_alone(tmp_path_factory):
    _, lds, _ = sections(tmp_path_factory)
    rows = [tuple(int(x, 16) if i == 0 else int(x) for i, x in enumerate(l.split())) for l in lds]
    assert len(rows) == 4 * 16 * 3 and set(r[0] for r in rows) == ONE_MESH_BUILDS
    for kv, bounces, any_bounce, need_cold, lds in rows:
        frames, nf = (bounces if bounces > 0 and any_bounce else 1), (10 if need_cold else 4)
        # the stack, and the parking granule of the 6-wave builds: nothing in it knows of the opaque build (the function
        # takes none), so KO_OPAQUE and KO_PARENT launches of one build and stack ask for the same bytes
        assert lds == frames * nf * 64 * 4 + (GRANULE if kv & OCC6 else 0), (hex(kv), bounces, lds)
    # the headline launch: bounces 5, reflecting materials, build 107 — five granules per wave, 24 waves per CU
    at5 = {r[0]: r[4] for r in rows if r[1:4] == (5, 1, 0)}
    assert at5[DEFAULT | OCC6] == 6400 and 6400 == 5 * GRANULE


def test_any_nonzero_transparency_takes_the_scene_out_of_the_any_hit_builds(tmp_path_factory):
    _, _, mats = sections(tmp_path_factory)
    rows = [(struct.unpack("<f", struct.pack("<I", int(bits, 16)))[0], int(opaque), int(n)) for bits, opaque, n in (l.split() for l in mats)]
    assert len(rows) == 12
    zeros = [r for r in rows if r[0] == 0.0]
    assert len(zeros) == 2 and all(opaque == 1 and n > 0 for _, opaque, n in zeros)   # +0 and -0: all-opaque, any-hit builds exist
    for t, opaque, n in rows:
        if not t == 0.0:   # denormals, values below the 1e-6 at which a material transmits, negatives, inf, NaN
            assert opaque == 0 and n == 0, (t, opaque, n)
