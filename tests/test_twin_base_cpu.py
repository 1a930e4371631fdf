"""CPU proof of the mirror rule (allwave_amd/csrc/twin_base.hpp): a stand-alone driver with a scalar WFA
that keeps its full history, built with the system C++ compiler under AddressSanitizer and UBSan, produces the op string
of the swapped pair (T, P) in two ways -- by aligning (T, P), and by backtracing the history of (P, T) through the header --
and fails when the two differ.  The test compares both with the oracle's plain WFA (align_unidirectional: a base case is a
plain WFA with a backtrace) on base-case sized problems: lengths 1-400, optimal penalty at most 250, the tie-rich
families of tests/repeats.py, starts and ends in every gap component."""
import os
import random
import shutil
import subprocess

import pytest

import twin_base_cases as BC
import twin_cases as TC
from util import rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1                # chosen for the condition test_mirror_rule_on_base_case_sized_pairs asserts from the oracle alone
GAP_CASE_MAX = 100      # pairs that cost at most this much also run with forced begin / end components (a forced gap adds to it)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("twin_base") / "twin_base_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), os.path.join(ROOT, "tests", "twin_base_driver.cpp"),
                           "-o", exe])
    return exe


def run(driver, cases):
    """cases: (scores, cb, ce, P, T).  Returns (penalty, ops of (P, T), ops of (T, P), ops of (T, P) by the mirror rule)."""
    lines = []
    for scores, cb, ce, p, t in cases:
        s = list(scores) + ([0, 0, 0] if len(scores) == 4 else [1])
        lines.append("%d %d %d %d %d %d %d %d %s %s\n" % (s[1], s[2], s[3], s[4], s[5], s[6], cb, ce, p.decode(), t.decode()))
    r = subprocess.run([driver], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = [ln.split(" ") for ln in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return [(int(f[0]), f[1].encode(), f[2].encode(), f[3].encode()) for f in out]


@pytest.mark.parametrize("scores", BC.CPU_SETS, ids=lambda s: ",".join(map(str, s)))
def test_mirror_rule_on_base_case_sized_pairs(driver, oracle, scores):
    al = oracle.Aligner(scores)
    kept, want = [], []
    for p, t in BC.cpu_pairs(SEED):
        assert 1 <= len(p) <= 400 and 1 <= len(t) <= 400
        fwd, swp = al.align_unidirectional(p, t), al.align_unidirectional(t, p)
        if fwd[0] <= BC.SCORE_CAP:
            kept.append((p, t))
            want += [fwd, swp]
    n = len(kept)
    differ = TC.not_mirrored(want)
    unequal = sum(1 for p, t in kept if len(p) != len(t))
    print("%s: %d pairs within %d, %d of unequal lengths; the swapped pair's ops are not the I/D swap on %d" % (scores, n, BC.SCORE_CAP, unequal, differ))
    assert n >= 150 and unequal >= 50
    assert 10 * differ >= n, (differ, n)        # so that "swap the I and the D" cannot pass for the mirror rule
    # (1) M to M: both ways of producing the swapped pair's ops equal the oracle's; the driver itself fails when they differ
    got = run(driver, [(scores, BC.C_M, BC.C_M, p, t) for p, t in kept])
    for i, (pen, ops_a, ops_b, ops_m) in enumerate(got):
        assert (pen, ops_a) == want[2 * i] and (pen, ops_b) == want[2 * i + 1] and ops_m == ops_b, (i, kept[i])
    # (2) starts and ends in every component: every (begin, end) combination over the cheaper pairs in turn.  A WFA keeps the
    # furthest point of a diagonal only, so a forced begin or end component is feasible where the sequences call for that gap,
    # as they do at a breakpoint: 1-12 unrelated bases go in front of / behind the sequence that the gap consumes.
    comps = BC.gap_components(scores)
    combos = [(cb, ce) for cb in comps for ce in comps if (cb, ce) != (BC.C_M, BC.C_M)]
    cheap = [kept[i] for i in range(n) if want[2 * i][0] <= GAP_CASE_MAX]
    rng = random.Random("twin-base-cpu/gaps")
    ins, dele = (BC.C_I1, BC.C_I2), (BC.C_D1, BC.C_D2)
    cases = []
    for i, (p, t) in enumerate(cheap):
        for j in range(3):
            cb, ce = combos[(3 * i + j) % len(combos)]
            junk = [rand_seq(rng, rng.randint(1, 12)) for _ in range(4)]
            cases.append((scores, cb, ce, (junk[0] if cb in dele else b"") + p[:375] + (junk[1] if ce in dele else b""),
                          (junk[2] if cb in ins else b"") + t[:375] + (junk[3] if ce in ins else b"")))
    assert set(c[1:3] for c in cases) == set(combos)
    got = run(driver, cases)
    differ2 = sum(1 for _, a, b, _ in got if b != a.translate(TC.SWAP))
    print("%s: %d cases with a begin or end in a gap component, %d not the I/D swap" % (scores, len(cases), differ2))
    for (_, cb, ce, p, t), (pen, ops_a, ops_b, ops_m) in zip(cases, got):
        assert ops_m == ops_b
        for ops, q, r in ((ops_a, p, t), (ops_b, t, p)):     # op strings of the right shape (the driver has no second opinion here)
            assert ops.count(b"M") + ops.count(b"X") + ops.count(b"D") == len(q)
            assert ops.count(b"M") + ops.count(b"X") + ops.count(b"I") == len(r)
