"""CPU tests of the WFA-orientation rule (awv_orient_decide, awv_orient_settling_bound; include/allwave_hip.h).

The rule: with P a strand's optimal penalty and E = #X + #I + #D of any optimal CIGAR of it,
ceil(P / cmax) <= E <= floor(P / cmin).  The reference takes forward iff E_f <= E_r; the engine may answer from penalties or
from proved lower bounds of them only where that comparison is certain.  Checked here against the oracle's CIGARs of both
strands; no GPU is involved (the functions are pure host code of the product library)."""
import os

import pytest

import orient_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PAIRS = 200


@pytest.fixture(scope="module")
def ffi(hip_lib):
    from allwave_amd import ffi as F
    return F


@pytest.fixture(scope="module")
def pairs():
    return OC.rule_pairs(N_PAIRS, "orient/rule")


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("scores", OC.RULE_SCORES, ids=lambda s: ",".join(map(str, s)))
def test_rule_against_oracle(ffi, oracle, pairs, scores):
    cmin, cmax = OC.cmin_cmax(scores)
    al = oracle.Aligner(scores)
    F, R, U = ffi.AWV_ORIENT_FORWARD, ffi.AWV_ORIENT_REVERSE, ffi.AWV_ORIENT_UNDECIDED
    NONE = OC.HI_NONE
    assert len(pairs) >= 200
    decided = 0
    for q, t in pairs:
        (pf, ef), (pr, er) = OC.strand_facts(al, q, t)
        want = F if ef <= er else R
        what = (scores, len(q), len(t), pf, ef, pr, er)
        # the inequality, for both strands' CIGARs
        assert ceil_div(pf, cmax) <= ef <= pf // cmin, what
        assert ceil_div(pr, cmax) <= er <= pr // cmin, what
        # exact penalties: an answer is the reference's
        d = ffi.orient_decide(scores, pf, pf, pr, pr)
        assert d in (F, R, U), what
        if d != U:
            assert d == want, what
            decided += 1
        if ef == er and d != U:
            assert d == F, what  # ties go forward
        # the forward penalty known, the reverse strand bounded from below only
        B = ffi.orient_settling_bound(scores, False, pf)
        assert B >= -1
        assert ffi.orient_decide(scores, pf, pf, B + 1, NONE) == F, what                # the settling bound decides ...
        if B >= 0:
            assert ffi.orient_decide(scores, pf, pf, B, NONE) == U, what               # ... and nothing smaller does
        for L in (B + 1, B, pr):
            if 0 <= L <= pr:  # (a lower bound the search could have proved)
                d = ffi.orient_decide(scores, pf, pf, L, NONE)
                assert d in (U, want), (what, L, d)
        # the reverse penalty known, the forward strand bounded from below only
        B = ffi.orient_settling_bound(scores, True, pr)
        assert B >= 0
        assert ffi.orient_decide(scores, B + 1, NONE, pr, pr) == R, what
        assert ffi.orient_decide(scores, B, NONE, pr, pr) == U, what
        for L in (B + 1, B, pf):
            if 0 <= L <= pf:
                d = ffi.orient_decide(scores, L, NONE, pr, pr)
                assert d in (U, want), (what, L, d)
        # nothing known above: never an answer
        assert ffi.orient_decide(scores, min(pf, 7), NONE, min(pr, 7), NONE) == U
    assert decided > 0  # (the identical pairs at the least: P_f = 0 settles them)


@pytest.mark.parametrize("scores", OC.RULE_SCORES, ids=lambda s: ",".join(map(str, s)))
def test_ties_go_forward(ffi, oracle, scores):
    """identical and palindromic inputs: both strands are the same alignment, E_f == E_r, forward"""
    al = oracle.Aligner(scores)
    for n in (1, 5, 50, 500):
        s = b"ACGT" * n
        assert OC.rc(s) == s
        (pf, ef), (pr, er) = OC.strand_facts(al, s, s)
        assert (pf, ef, pr, er) == (0, 0, 0, 0)
        assert ffi.orient_decide(scores, pf, pf, pr, pr) == ffi.AWV_ORIENT_FORWARD
    cmin, cmax = OC.cmin_cmax(scores)
    if cmin == cmax:  # equal penalties whose edit intervals are single points
        for p in (0, 1, 7, 100, 12345):
            assert ffi.orient_decide(scores, p, p, p, p) == ffi.AWV_ORIENT_FORWARD


def test_settling_bound_default_scores(ffi):
    """0,1,1,1: the losing strand's search stops at 2 P - 2 (forward known) / 2 P (reverse known)"""
    for p in (1, 2, 10, 560, 6000):
        assert ffi.orient_settling_bound((0, 1, 1, 1), False, p) == 2 * p - 2
        assert ffi.orient_settling_bound((0, 1, 1, 1), True, p) == 2 * p
    assert ffi.orient_settling_bound((0, 1, 1, 1), False, 0) == -1
    assert ffi.orient_settling_bound((0, 1, 1, 1), True, 0) == 0


def test_bad_input_is_refused(ffi):
    with pytest.raises(ffi.EngineError):
        ffi.orient_decide((1, 1, 1, 1), 0, 0, 0, 0)      # match != 0
    with pytest.raises(ffi.EngineError):
        ffi.orient_decide((0, 1, 1, 1), 5, 4, 0, 0)      # hi < lo
    with pytest.raises(ffi.EngineError):
        ffi.orient_decide((0, 1, 1, 1), -1, 4, 0, 0)
    with pytest.raises(ffi.EngineError):
        ffi.orient_settling_bound((0, 1, 1, 1), False, -3)


def test_exports_and_signatures(hip_lib, ffi):
    """the new entry points are exported and declared as documented; the ABI version is unchanged"""
    for name in ("awv_score_pairs_bounded", "awv_orient_pairs", "awv_orient_decide", "awv_orient_settling_bound"):
        assert hasattr(hip_lib, name), name
        assert name in ffi.EXPORTS
    hdr = " ".join(open(os.path.join(ROOT, "include", "allwave_hip.h")).read().split())
    for decl in ("int awv_score_pairs_bounded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, "
                 "const int32_t* max_penalty",
                 "int awv_orient_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, int32_t flags, "
                 "awv_orient_result* out",
                 "int awv_orient_decide(const awv_penalties* pen, int32_t lo_f, int32_t hi_f, int32_t lo_r, int32_t hi_r);",
                 "#define AWV_ORIENT_FULL 1", "#define AWV_ORIENT_BY_BOUND 0", "#define AWV_ORIENT_BY_EDITS 1",
                 "#define AWV_ABI_VERSION 3"):
        assert decl in hdr, decl
    assert hip_lib.awv_abi_version() == 3
    assert ffi.ORIENT_DTYPE.itemsize == 48
