"""Host logic (CPU, no GPU): launch_shape (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space — every build of both
kernel lists x n_oloop in {0, 1} x head_mesh in {0, 1} (scripts/shape_choice_check.cpp).  The one-mesh shape is for exactly
four builds, the default variant with or without KV_OCC6 and with or without KV_HOSTOUT, on a scene without spheres and
stand-alone triangles whose only mesh rides in the scene head; everything else stays in shape 0."""
from tests.checkers import CHOICE_SOURCES, I_CSRC, I_INCLUDE, check_output, check_program

# scene_device.h KV_*
PREFILTER, ANYHIT, BVH, FASTPOW, OCC6, HOSTOUT = 1, 2, 8, 32, 64, 128
DEFAULT = PREFILTER | BVH | ANYHIT | FASTPOW
ONE_MESH_BUILDS = {DEFAULT, DEFAULT | OCC6, DEFAULT | HOSTOUT, DEFAULT | OCC6 | HOSTOUT}
KS_ONE_MESH = 1


def answers(tmp_path_factory):
    exe = check_program(tmp_path_factory, "shape_choice_check", ("-O2", I_CSRC, I_INCLUDE), CHOICE_SOURCES)
    lines = check_output(exe, timeout=60).split("\n")
    at = lines.index("shapes")
    cases = [(int(kv, 16), int(n), int(hm), int(shape)) for kv, n, hm, shape in (l.split() for l in lines[:at])]
    return cases, [int(x, 16) for x in lines[at + 1:] if x]


def test_the_one_mesh_shape_is_for_exactly_the_four_default_builds(tmp_path_factory):
    cases, shaped = answers(tmp_path_factory)
    builds = sorted(set(kv for kv, _, _, _ in cases))
    assert len(builds) == 43 + 10 and len(cases) == 4 * len(builds)   # CTR_RENDER_KERNELS + CTR_LENS_KERNELS, each case once
    assert len(shaped) == 4 and set(shaped) == ONE_MESH_BUILDS        # CTR_SHAPE_KERNELS: the four, each once
    assert ONE_MESH_BUILDS <= set(builds)                             # ... and each has its general twin
    for kv, n_oloop, head_mesh, shape in cases:
        want = KS_ONE_MESH if (kv in ONE_MESH_BUILDS and n_oloop == 0 and head_mesh == 1) else 0
        assert shape == want, (hex(kv), n_oloop, head_mesh, shape)
    assert sum(1 for c in cases if c[3] == KS_ONE_MESH) == 4
