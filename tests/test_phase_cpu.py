"""Host logic (CPU, no GPU) behind the phased builds of the render kernel (cutrace_amd/csrc/render_kernel.hip "Phased builds";
DESIGN.md "Phased opaque builds").

The invariant (scripts/phase_check.cpp): in an opaque any-hit build all active lanes of a wave cast, in every trip, for the same
reason and towards the same light, and the scalar rule  phase = (phase == n_light) ? 0 : phase + 1  predicts both — searched over
0 ... 33 lights, bounces 0 ... 15, random miss / reflect / occluder / dark patterns and lanes inactive from the start; under the
mutation (a material that transmits: the shadow loop takes a second trip) the search must find lanes that drift apart.

The decision (scripts/phase_choice_check.cpp): phased_build over its whole input space — phased exactly when the launch's build
is the opaque one and CUTRACE_NO_PHASE_SPLIT is unset."""
import re

from tests.checkers import CHOICE_SOURCES, HOST_FLAGS, check_output, check_program

KO_PARENT, KO_OPAQUE = 0, 1
ANYHIT = 2


def counts(line):
    m = re.match(r"checked (\d+) waves, (\d+) trips \((\d+) radiance, (\d+) shadow\), (\d+) lane casts, longest wave (\d+) trips, mutation (\w+): violations (\d+)", line)
    assert m, line
    return [int(g) if g.isdigit() else g for g in m.groups()]


def test_all_active_lanes_share_the_kind_and_the_light_and_the_scalar_phase_predicts_both(tmp_path_factory):
    exe = check_program(tmp_path_factory, "phase_check", ("-O2",))
    for seed in (1, 2):
        waves, trips, radiance, shadow, casts, longest, mutation, violations = counts(check_output(exe, ("20000", "--seed", str(seed)), timeout=120).strip())
        assert (waves, mutation, violations) == (20000, "none", 0)
        # the search saw what it is about: shadow and radiance trips, waves with many trips (33 lights x 16 frames), partly empty waves
        assert radiance > 20000 and shadow > 10 * radiance and longest > 300 and trips < casts < 64 * trips


def test_a_transparent_material_is_found_to_break_the_invariant(tmp_path_factory):
    exe = check_program(tmp_path_factory, "phase_check", ("-O2",))
    *_, mutation, violations = counts(check_output(exe, ("20000", "--transparent"), timeout=120).strip())
    assert mutation == "transparent" and violations > 1000


def test_phased_exactly_when_opaque_and_the_switch_is_unset(tmp_path_factory):
    exe = check_program(tmp_path_factory, "phase_choice_check", HOST_FLAGS, CHOICE_SOURCES)
    lines = [l.split() for l in check_output(exe, timeout=120).split("\n") if l]
    cases = [(int(kv, 16), int(shape), int(no_opq), int(no_split), int(opq), int(phased)) for kv, shape, no_opq, no_split, opq, phased in (l for l in lines if l[0] != "raw")]
    builds = sorted(set(c[0] for c in cases))
    assert len(builds) == 43 + 10 and len(cases) == 8 * len(builds)   # CTR_RENDER_KERNELS + CTR_LENS_KERNELS, each case once
    for kv, shape, no_opq, no_split, opq, phased in cases:
        assert opq == (KO_OPAQUE if (shape == 1 and kv & ANYHIT and not no_opq) else KO_PARENT), (hex(kv), shape, no_opq)
        assert phased == int(opq == KO_OPAQUE and not no_split), (hex(kv), shape, no_opq, no_split, opq, phased)
    assert sum(c[5] for c in cases) == sum(1 for c in cases if c[4] == KO_OPAQUE) // 2 > 0
    raw = [(int(opq), int(no_split), int(phased)) for _, opq, no_split, phased in (l for l in lines if l[0] == "raw")]
    assert len(raw) == 8 and all(phased == int(opq == KO_OPAQUE and not no_split) for opq, no_split, phased in raw)
