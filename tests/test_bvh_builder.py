"""Host logic (CPU, no GPU): the BVH builders of cutrace_amd/csrc/bvh.cpp on random and degenerate triangle sets — every
primitive in exactly one leaf, leaf sizes, boxes containing what is below them, depth limits the kernel's lane stacks rely
on (scripts/bvh_check.cpp; the same harness runs under ASan/UBSan in scripts/cpu_sanitize.sh)."""
import os

from tests.checkers import CSRC, I_CSRC, I_INCLUDE, check_output, check_program


def test_bvh_builders_keep_their_invariants(tmp_path_factory):
    exe = check_program(tmp_path_factory, "bvh_check", ("-O2", I_CSRC, I_INCLUDE), (os.path.join(CSRC, "bvh.cpp"),))
    out = check_output(exe)
    assert "all invariants hold" in out, out[-2000:]
