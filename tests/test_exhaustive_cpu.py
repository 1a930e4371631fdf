"""CPU tests of the exhaustive lists (tests/exhaustive_cases.py): that the lists are what they claim and that they are traps,
from the oracle alone.  For every (family, layout) and penalty set, on every pair of the list: awo_align and
awo_align_unidirectional return the same penalty, that penalty is the Gotoh DP's (the banded DP with the penalty as bound
in the long layouts), the CIGAR passes cigar_check and re-scores to it; every pair whose two sequences differ has exactly
one breakpoint search in a flanked layout and none bare; and in every flanked layout the BiWFA op string differs from the
unidirectional one on at least 5 % of the pairs -- a condition on the inputs (a flank seed that misses it is changed, never
the threshold).  The shares are printed (pytest -s).

Cost: all six sets of util.PENALTY_SETS run on `balanced` and `long_k12_12`; the other layouts run DEFAULT_2P, (0, 7, 0, 3)
and EDIT.  The pairs of a list are spread over the oracle's thread pool; most of the time goes into the DPs (a full 146 x 146
table per short pair, a band of the penalty's width over 1,206 bases per long one), and the file takes three to five minutes
on eight cores."""
import numpy as np
import pytest

import exhaustive_cases as X
from util import DEFAULT_2P, EDIT, PENALTY_SETS

THREE = [DEFAULT_2P, (0, 7, 0, 3), EDIT]
ALL_SETS = ("balanced", "long_k12_12")
TRAP_SHARE = 0.05


def sets_of(name):
    return PENALTY_SETS if name in ALL_SETS else THREE


def test_sizes_and_determinism():
    assert (len(X.family("AC6")), len(X.family("ACG4"))) == (127, 121)
    assert len(set(X.family("AC6"))) == 127 and len(set(X.family("ACG4"))) == 121
    assert X.family("AC6")[:4] == [b"", b"A", b"C", b"AA"] and max(len(c) for c in X.family("AC6")) == 6
    assert set(b"".join(X.family("ACG4"))) == set(b"ACG") and max(len(c) for c in X.family("ACG4")) == 4
    for fam, n in (("AC6", 127), ("ACG4", 121)):
        cs = X.family(fam)
        for name in X.LAYOUTS:
            seqs, pairs = X.build(fam, name)
            seqs2, pairs2 = X.build(fam, name)
            assert seqs == seqs2 and pairs.tobytes() == pairs2.tobytes() and pairs.dtype == np.int32, (fam, name)
            assert b"\0".join(seqs) == b"\0".join(X.lists(fam, name)[0]) and pairs.tobytes() == X.lists(fam, name)[1].tobytes()
            assert len(pairs) == n * n == {"AC6": 16129, "ACG4": 14641}[fam]
            assert len(set(map(tuple, pairs.tolist()))) == n * n
            lay = X.layout(name)
            assert lay.identical == (name in X.IDENTICAL)
            # entry (i, j) is query(core i) against target(core j)
            for k in (0, 1, n, n * n // 2 + 3, n * n - 1):
                q, t = pairs[k]
                assert (seqs[q], seqs[t]) == (lay.query(cs[k // n]), lay.target(cs[k % n])), (fam, name, k)
                assert (X.core_of(fam, q), X.core_of(fam, t)) == (cs[k // n], cs[k % n])
            if name != "bare":  # above FALLBACK_MIN_LENGTH, so never a top-level base case by length
                assert min(len(s) for s in seqs) > 100, (fam, name)
            else:
                assert max(len(s) for s in seqs) <= 6
            # both orders of every pair are in the twin list
            tseqs, tpairs = X.twin_lists(fam, name)
            have = set(map(tuple, tpairs.tolist()))
            assert all((t, q) in have for q, t in have), (fam, name)
            if not lay.identical:
                assert len(tpairs) == 2 * n * n and (tpairs[0::2] == pairs).all() and (tpairs[1::2] == pairs[:, ::-1]).all()
    lay = X.layout("repeat_flanks")
    assert lay.ql.endswith(b"A" * 10) and lay.qr.startswith(b"AC" * 5) and len(lay.ql) == len(lay.qr) == 70
    assert [len(X.layout(n).ql) + len(X.layout(n).qr) for n in X.IDENTICAL[1:]] == [140] * 4
    for name in X.LONG:
        lay = X.layout(name)
        kl, kr = (int(v) for v in name[6:].split("_"))
        assert len(lay.ql) == len(lay.qr) == X.FLANK_LONG == 600
        assert sum(a != b for a, b in zip(lay.ql, lay.tl)) == kl and sum(a != b for a, b in zip(lay.qr, lay.tr)) == kr
        assert 2 * (2 * X.FLANK_LONG) > 1024  # AWV_MIN_PASS_LEN: the kernels run multi-step passes on these pairs


def test_book_ranges_hold_the_list():
    """The range form of the balanced AC6 list: the substrings are the pair list's sequences on both strands, the query
    intervals begin on every residue modulo 16, and the bases beyond both ends of an interval are a neighbour's flank."""
    seqs, pairs = X.lists("AC6", "balanced")
    books, fwd, rev = X.book_ranges()
    lay = X.layout("balanced")
    assert books[0] == books[1] and books[2] == X.revcomp(books[0]) and len(fwd) == len(rev) == len(pairs)
    for k in list(range(0, len(pairs), 97)) + [len(pairs) - 1]:
        q, t = pairs[k]
        _, _, rc0, qb, qe, tb, te = fwd[k].tolist()
        assert rc0 == 0 and books[0][qb:qe] == seqs[q] and books[1][tb:te] == seqs[t]
        s, _, rc1, qb, qe, tb2, te2 = rev[k].tolist()
        assert (s, rc1, tb2, te2) == (2, 1, tb, te) and X.revcomp(books[2][qb:qe]) == seqs[q]
        if te < len(books[1]):
            assert books[1][te:te + 70] == lay.tl
        if tb > 0:
            assert books[1][tb - 70:tb] == lay.tr
    assert set(int(v) % 16 for v in fwd[:, 3]) == set(range(16)) == set(int(v) % 16 for v in rev[:, 3])
    assert set(int(v) % 16 for v in fwd[:, 5]) == set(range(16))


def _measure(oracle, fam, name, scores):
    """Per pair of the list: (BiWFA penalty, ops, n_breakpoints, n_base, unidirectional penalty, ops, the DP's penalty,
    cigar_check's rc and re-scored penalty)."""
    seqs, pairs = X.lists(fam, name)
    plist = pairs.tolist()
    long = name in X.LONG

    def work(a, b):
        al = oracle.Aligner(scores)
        out = []
        for q, t in plist[a:b]:
            st = oracle.Stats()
            pen, ops = al.align(seqs[q], seqs[t], st)
            upen, uops = al.align_unidirectional(seqs[q], seqs[t])
            dp = oracle.gotoh_penalty_banded(seqs[q], seqs[t], scores, pen) if long else oracle.gotoh_penalty(seqs[q], seqs[t], scores)
            rc, rescored = oracle.cigar_check(ops, seqs[q], seqs[t], scores)
            out.append((pen, ops, st.n_breakpoints, st.n_base, upen, uops, dp, rc, rescored))
        return out

    return seqs, plist, X.in_chunks(oracle, len(plist), work)


CASES = [(fam, name, tuple(scores)) for fam in X.FAMILIES for name in X.LAYOUTS for scores in sets_of(name)]


@pytest.mark.parametrize("fam,name,scores", CASES, ids=["%s-%s-%s" % (f, n, ",".join(map(str, s))) for f, n, s in CASES])
def test_every_pair_by_the_oracle(oracle, fam, name, scores):
    seqs, plist, rows = _measure(oracle, fam, name, scores)
    differ = 0
    for (q, t), (pen, ops, nbp, nbase, upen, uops, dp, rc, rescored) in zip(plist, rows):
        where = (fam, name, scores, X.core_of(fam, q), X.core_of(fam, t))
        assert pen == upen == dp, where + (pen, upen, dp)
        assert (rc, rescored) == (0, pen), where + (rc, rescored, pen)
        if name == "bare":
            assert nbp == 0, where + (nbp, nbase)
        elif seqs[q] != seqs[t]:
            assert nbp == 1 and (nbase == 2 or name not in X.LONG), where + (nbp, nbase)
        else:
            assert nbp == 0 and pen == 0, where + (nbp, pen)
        differ += ops != uops
    share = differ / len(plist)
    same = sum(1 for q, t in plist if seqs[q] == seqs[t])
    print("%s %s %s: BiWFA and unidirectional ops differ on %d of %d pairs (%.1f %%); %d identical pairs" %
          (fam, name, scores, differ, len(plist), 100 * share, same))
    assert same == (0 if name in X.LONG else len(X.family(fam)))
    if name != "bare":
        assert share >= TRAP_SHARE, (fam, name, scores, share)
    if scores == DEFAULT_2P:  # the helper the GPU tests share returns the same answers, in the same order
        want = X.oracle_results(oracle, fam, name, scores)
        assert want.ops == [r[1] for r in rows] and want.pen.tolist() == [r[0] for r in rows]
        assert want.counts.sum(axis=1).tolist() == [len(r[1]) for r in rows]
        assert X.records(want)[:3] == [(r[0], r[1]) for r in rows[:3]]


@pytest.mark.parametrize("fam", list(X.FAMILIES))
def test_twin_list_of_a_long_layout(oracle, fam):
    """The interleaved list of long_k12_11: even entries are the plain list's, odd entries the oracle's answer for the swapped
    orientation -- and that answer is not the I/D swap of the plain one on some pairs, so a kernel that mirrors where the
    oracle does not is caught."""
    scores = DEFAULT_2P
    seqs, both = X.twin_lists(fam, "long_k12_11")
    plain = X.oracle_results(oracle, fam, "long_k12_11", scores)
    want = X.oracle_results(oracle, fam, "long_k12_11", scores, twin=True)
    assert want.ops[0::2] == plain.ops and want.pen[0::2].tolist() == plain.pen.tolist() and len(want.ops) == len(both)
    assert (want.pen[1::2] == want.pen[0::2]).all()
    al = oracle.Aligner(scores)
    for k in range(1, len(both), 1999):
        q, t = both[k]
        assert al.align(seqs[q], seqs[t]) == (int(want.pen[k]), want.ops[k])
    swap = bytes.maketrans(b"ID", b"DI")
    not_mirror = sum(1 for k in range(0, len(both), 2) if want.ops[k + 1] != want.ops[k].translate(swap))
    print("%s long_k12_11: the swapped entry's ops are not the I/D swap on %d of %d pairs" % (fam, not_mirror, len(both) // 2))
    assert not_mirror > 0
