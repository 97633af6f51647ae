"""The lemma behind the dark-light skip (cutrace_amd/csrc/render_kernel.hip "dark lights"; DESIGN.md "Dark lights") on the CPU,
through scripts/dark_light_check.cpp, which states what it checks: a search for (hit, light) pairs that satisfy the kernel's
predicate and whose term nevertheless changes phong's `final` in some bit (10^7 pairs here), the rule of the scene fact
`shade_finite`, and the three mutations of the predicate under which the search must find such pairs."""
import re

import pytest

from tests.checkers import FLATTEN_SOURCES, HOST_FLAGS, check_output, check_program

N = 10000000
N_MUTATION = 2000000
EXPONENTS = (0, 0.5, 1, 2, 200, 1000, 1e5)   # scripts/dark_light_check.cpp EXPS


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return check_program(tmp_path_factory, "dark_light_check", HOST_FLAGS, FLATTEN_SOURCES)


def search(checker, n, *args):
    line = check_output(checker, [str(n), *args]).strip().splitlines()[-1]
    assert line.startswith("checked "), line
    words = line.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1, 2) if re.fullmatch(r"\d+", words[i + 1])}
    print(line)
    return got


@pytest.fixture(scope="module")
def found(checker):
    return search(checker, N)


def test_a_dark_term_never_changes_final(found):
    assert found["cases"] >= N and found["dark"] > N // 10 and found["violations"] == 0, found


def test_the_draws_reach_every_case_the_lemma_names(found):
    got = found
    # cosines within 2^-20 of zero, lanes the -0 guard refuses, denormal specular factors, colours beyond the bound or not
    # finite, negative colours among the dark pairs, both forms of the power
    for key in ("near_zero_cosines", "refused_neg_zero", "refused_denormal_fs", "refused_bound", "refused_nonfinite", "negative_colour_dark"):
        assert got[key] > N // 1000, (key, got)
    assert N // 4 < got["fast_pow"] < 3 * N // 4, got
    for e in range(len(EXPONENTS)):
        assert got[f"exp{e}"] > N // 20, (e, got)
    # phong_exp == 0 gives fs = 1: never dark; every other exponent of the list is dark somewhere
    assert got["dark_exp0"] == 0 and all(got[f"dark_exp{e}"] > N // 1000 for e in range(1, len(EXPONENTS))), got


def test_shade_finite_is_false_exactly_for_a_non_finite_colour_or_specular(found):
    assert found["finite_mismatch"] == 0 and found["refused_nonfinite"] > 0 and found["facts_hold"] > 0, found


@pytest.mark.parametrize("mutation", ["--no-neg-zero-guard", "--denormal-is-zero", "--no-bound"])
def test_the_mutations_are_found(checker, mutation):
    """without the guard on -0 a +0 term turns final = -0 into +0; a denormal specular factor times a colour is not zero;
    finite colours alone let a product overflow, and 0 * inf is NaN"""
    assert search(checker, N_MUTATION, mutation)["violations"] > 0
