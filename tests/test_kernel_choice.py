"""Host logic (CPU, no GPU): choose_kernel (cutrace_amd/csrc/kernel_choice.cpp) over its whole input space — entry point x the
nine CTR_VAR_* bits that matter x scene flags x deliverable x stack shape, 196 608 cases (scripts/kernel_choice_check.cpp) —
against what the launch path chose before there was a chooser (tests/golden/kernel_choice.npz, recorded from that code:
tests/golden/kernel_choice.md)."""
import os

import numpy as np

from tests.checkers import CHOICE_SOURCES, I_CSRC, I_INCLUDE, ROOT, check_output, check_program

GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_choice.npz")
SHAPE = (6, 512, 8, 2, 4)  # entry, user mask, scene flags, deliverable, stack shape
REJECTED = 0xF000          # + KernelReject; 0xFFFF: the chooser's outputs contradict each other


def choices(tmp_path_factory):
    """(cases in SHAPE as uint16, the KVs of CTR_RENDER_KERNELS, cases the tile-order bits changed, cases in which a scene
    outside the fast specular path's domain gets another build than CTR_VAR_EXACT_POW would)"""
    exe = check_program(tmp_path_factory, "kernel_choice_check", ("-O2", I_CSRC, I_INCLUDE), CHOICE_SOURCES)
    words = check_output(exe).split()
    at_list, at_neutral = words.index("list"), words.index("neutral")
    got = np.array([int(x, 16) for x in words[:at_list]], np.uint16)
    assert got.size == int(np.prod(SHAPE))
    at_slow = words.index("slowpow")
    return got.reshape(SHAPE), [int(x, 16) for x in words[at_list + 1:at_neutral]], int(words[at_neutral + 1]), int(words[at_slow + 1])


def test_every_launch_gets_the_build_it_got_before_the_chooser(tmp_path_factory):
    got, builds, moved, slowpow = choices(tmp_path_factory)
    want = np.load(GOLDEN)["choice"].reshape(SHAPE)
    diff = np.argwhere(got != want)
    assert diff.size == 0, [(tuple(i), hex(want[tuple(i)]), hex(got[tuple(i)])) for i in diff[:10]]
    assert moved == 0  # CTR_VAR_NO_REORDER, CTR_VAR_IMAGE_ORDER_FIRST
    # KernelFacts::fast_pow_ok: true in every row of the fixture (the scenes it was recorded from are inside the fast
    # specular path's domain: tests/test_scene_flatten.py); false, the launch is the one CTR_VAR_EXACT_POW gets
    assert slowpow == 0
    assert len(builds) == len(set(builds)) == 43
    chosen = set(int(x) for x in np.unique(got[got < REJECTED]))
    assert chosen <= set(builds), sorted(chosen - set(builds))   # every KV the chooser returns is in the list
    assert set(builds) <= chosen, sorted(set(builds) - chosen)   # every KV in the list is returned for some input
