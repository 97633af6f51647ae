"""Host logic (CPU, no GPU): the tile scheduler's rule (cutrace_amd/csrc/tile_order_policy.h plan_order: when a launch dispatches by
the stored tile order, when a shape starts centre-out, which launches rebuild the order) against its statement in Python below.
No render test can see this rule, because every order gives the same bits.  scripts/tile_order_policy_check.cpp runs scripted
sequences of launches through plan_order and prints one line per launch; a second copy of the program is built and run with
AddressSanitizer + UBSan where the compiler has them."""
import os
import shutil
import subprocess

import pytest

from cutrace_amd import VAR_IMAGE_ORDER_FIRST, VAR_NO_REORDER, VAR_STATS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_ORDER_MIN_TILES = 8192  # CTR_FIRST_ORDER_MIN_TILES
ORDER_PERIOD = 8              # CTR_ORDER_PERIOD


class State:
    def __init__(self):
        self.valid, self.key, self.age, self.view, self.cap = False, None, 0, 0, 0


def plan(S, key, view, heavy, variant, count):
    """(use_order, order_init, record_cost, write_next), the rule of the issue in a few lines"""
    n = key[0]
    if variant & (VAR_NO_REORDER | VAR_STATS) or count or n == 0 or n > 0x7FFFFFFF:
        return (0, 0, 0, 0)
    if n > S.cap:
        S.valid, S.cap = False, n
    same = S.valid and key == S.key
    use = init = 0
    if same:
        use = 1
    else:
        S.age = 0
        if n >= FIRST_ORDER_MIN_TILES and heavy and not variant & VAR_IMAGE_ORDER_FIRST:
            use = init = 1
    S.key, S.valid = key, True
    same_view = same and view == S.view
    S.view = view
    write_next = int(S.age < 2 or not same_view or S.age % ORDER_PERIOD == 0)
    S.age += 1
    return (use, init, 1, write_next)


def build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *extra, "-I" + os.path.join(ROOT, "cutrace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "scripts", "tile_order_policy_check.cpp")])
    return subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()


def parse(lines):
    """seq -> [(inputs, outputs)], inputs = (key, view, heavy, variant, count, cap_lost), outputs = (use, init, cost, next, age)"""
    out = {}
    for line in lines:
        left, right = line.split("|")
        seq, *w = left.split()
        w = [int(x) for x in w]
        out.setdefault(seq, []).append(((tuple(w[:6]), w[6], w[7], w[8], w[9], w[10]), tuple(int(x) for x in right.split())))
    return out


def test_tile_order_policy_equals_its_statement(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    lines = build_and_run(tmp_path, "tile_order_policy_check", ["-O2"])
    seqs = parse(lines)
    assert sorted(seqs) == list("abcdef")

    # every line against the rule; a sequence of (e) starts a fresh handle every two launches
    for seq, launches in seqs.items():
        S = State()
        for i, ((key, view, heavy, variant, count, cap_lost), got) in enumerate(launches):
            if seq == "e" and i % 2 == 0:
                S = State()
            if cap_lost:
                S.cap = 0
            assert plan(S, key, view, heavy, variant, count) + (S.age,) == got, (seq, i, lines)

    outs = {seq: [o for _, o in launches] for seq, launches in seqs.items()}
    use, init, cost, nxt, age = (lambda seq, col=col: [o[col] for o in outs[seq]] for col in range(5))

    # (a) 20 launches of one shape and view: image order first, the stored order from launch 1 on, rebuilt at 0, 1, 8 and 16 only
    assert len(outs["a"]) == 20 and use("a") == [0] + [1] * 19 and init("a") == [0] * 20 and cost("a") == [1] * 20
    assert [i for i, x in enumerate(nxt("a")) if x] == [0, 1, 8, 16] and age("a") == list(range(1, 21))
    # (b) the view changes every launch: rebuilt every launch
    assert len(outs["b"]) == 20 and use("b") == [0] + [1] * 19 and nxt("b") == [1] * 20
    # (c) A, a smaller shape, A again, A with other rows: every change restarts at age 0 with no stored order
    assert use("c") == [0, 1, 1] * 4 and age("c") == [1, 2, 3] * 4 and init("c") == [0] * 12
    # (d) a shape beyond the capacity, then the same shape after its buffers were lost: the stored order is dropped
    assert use("d") == [0, 1, 1, 0, 1, 1, 0, 1, 1] and age("d") == [1, 2, 3] * 3
    # (e) centre-out only from 8192 tiles on, on a heavy scene, unless CTR_VAR_IMAGE_ORDER_FIRST; the second launch uses the order
    assert [k[0][0] for k, _ in seqs["e"]] == [8191] * 4 + [8192] * 6
    assert init("e") == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0] and use("e") == [0, 1, 0, 1, 0, 1, 1, 1, 0, 1]
    # (f) launches that are not scheduled leave no trace: without them the sequence is (a)
    idle = [o for (k, o) in seqs["f"] if k[3] or k[4] or k[0][0] in (0, 0x80000000)]
    assert len(idle) == 5 and all(o == (0, 0, 0, 0, 5) for o in idle)
    assert [o for (k, o) in seqs["f"] if not (k[3] or k[4] or k[0][0] in (0, 0x80000000))] == outs["a"]

    # the same program under AddressSanitizer + UBSan (a plain CPU executable), where this compiler links them
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode == 0:
        assert build_and_run(tmp_path, "tile_order_policy_check_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                       "-fno-sanitize-recover=all"]) == lines
