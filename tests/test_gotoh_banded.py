"""CPU tests (-m "not gpu") of the banded Gotoh DP (oracle/gotoh.c, awo_gotoh_penalty_banded), and of the oracle against it
at 20-70 kbp.

The full DP (awo_gotoh_penalty) is the only checker with none of BiWFA's logic, but it is quadratic: a few kbp at most.
The banded DP runs the same recurrences on the diagonals an alignment of cost <= bound can visit, so it is exact up to that
bound at lengths the full DP cannot reach.  It is proved here first -- equal to the full DP, its band wide enough but no
wider than a path can need, and able to catch a penalty that is too high -- and then holds the oracle to the optimum on
long pairs, long forced gaps and long repeat arrays, where an error BiWFA's recursion shared with the kernels would
otherwise go unseen.
"""
import random

import pytest

import long_pairs as LP
import penalty_space as PS
import repeats
from util import DEFAULT_2P, EDIT, mutate, rand_seq, random_pair


def _bounds(g):
    return (g, g + 100, g - 1, None, 0)


def _want(g, bound):
    return g if bound is None or g <= bound else bound + 1


@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_equals_the_full_dp(oracle, name):
    """random_pair inputs and the repeats.SMALL families (shortened) at every accepted set: with bound >= optimum the
    banded DP returns the full DP's optimum; bound = optimum - 1 returns bound + 1 (= the optimum), bound = 0 returns 0
    or 1, no bound returns the optimum."""
    scores = PS.BY_NAME[name]
    rng = random.Random("banded/" + name)
    ab = [random_pair(rng, 400) for _ in range(25)]
    ab += [(b"", b""), (b"", rand_seq(rng, 37)), (rand_seq(rng, 41), b""), (b"A", b""), (b"", b"C")]
    ab += [gen(rng) for gen in (lambda r: repeats.microsatellite(r, flank=(20, 100)),
                                lambda r: repeats.end_runs(r, body=(50, 300)),
                                lambda r: repeats.tandem(r, total=(300, 900), flank=(0, 50)),
                                lambda r: repeats.cnv(r, seg=(20, 200), flank=(30, 100)),
                                lambda r: repeats.low_complexity(r, n=(100, 500)),
                                lambda r: repeats.exact_blocks(r, block=(200, 400), nblocks=(2, 2)))]
    for s, t in ab:
        g = oracle.gotoh_penalty(s, t, scores)
        for bound in _bounds(g):
            assert oracle.gotoh_penalty_banded(s, t, scores, bound) == _want(g, bound), (name, len(s), len(t), g, bound)
            assert oracle.gotoh_penalty_banded(t, s, scores, bound) == _want(g, bound), (name, len(t), len(s), g, bound)


def test_empty_and_zero_bound(oracle):
    """Empty sequences on either side cost one gap; bound 0 passes only identical sequences; a negative bound is exceeded
    by every pair."""
    for scores in (DEFAULT_2P, EDIT, (0, 1, 0, 1)):
        for s, t in ((b"", b""), (b"", b"ACGT" * 10), (b"ACGT" * 10, b""), (b"ACGT", b"ACGT"), (b"ACGT", b"ACGA")):
            g = oracle.gotoh_penalty(s, t, scores)
            if not s or not t:
                assert g == (PS.gap(scores, len(s) + len(t)) if s or t else 0)
            assert oracle.gotoh_penalty_banded(s, t, scores) == g
            assert oracle.gotoh_penalty_banded(s, t, scores, 0) == (0 if g == 0 else 1), (scores, s, t)
            assert oracle.gotoh_penalty_banded(s, t, scores, g) == g
            assert oracle.gotoh_penalty_banded(s, t, scores, -1) == 0
    assert oracle.gotoh_band(0, 40, DEFAULT_2P, PS.gap(DEFAULT_2P, 40) - 1) is None  # the forced gap alone is too dear
    assert oracle.gotoh_band(0, 40, DEFAULT_2P, PS.gap(DEFAULT_2P, 40)) == (0, 40)


def _wandering(rng, n=1500, g=60):
    """A path that leaves the diagonals between 0 and dl: a g-base insertion near the start and a g-base deletion near
    the end (dl = 0; the optimal path runs g diagonals above the main one for most of its length)."""
    a = rand_seq(rng, n)
    b = a[:100] + rand_seq(rng, g) + a[100:n - 100 - g] + a[n - 100:]
    return a, b


@pytest.mark.parametrize("scores", [EDIT, (0, 1, 0, 1), (0, 3, 0, 2), DEFAULT_2P, (0, 4, 6, 2)])
def test_band_contains_the_wandering_path(oracle, scores):
    """The band margin must hold a path that wanders g = 60 diagonals off [0, dl].  Where opening a gap costs less than
    two extensions (EDIT, (0, 1, 0, 1), (0, 3, 0, 2)) the band the optimum gives is exactly that path's excursion
    [-60, 60]: one diagonal fewer on its side and the DP returns more.  Elsewhere the band is wider, and narrowing it to
    the excursion still gives the optimum while one diagonal less does not."""
    rng = random.Random("banded/wander/%s" % (scores,))
    a, b = _wandering(rng)
    g = oracle.gotoh_penalty(a, b, scores)
    assert g == 2 * PS.gap(scores, 60), (scores, g)  # the two gaps are the whole cost: the path is the wandering one
    lo, hi = oracle.gotoh_band(len(a), len(b), scores, g)
    if scores[2] < 2 * scores[3]:
        assert (lo, hi) == (-60, 60), (scores, lo, hi)
    assert lo <= -60 and hi >= 60
    assert oracle.gotoh_penalty_banded(a, b, scores, g) == g
    assert oracle.gotoh_penalty_band(a, b, scores, lo, hi) == g
    assert oracle.gotoh_penalty_band(a, b, scores, 0, 60) == g          # the path: insertion first, above the diagonal
    assert oracle.gotoh_penalty_band(a, b, scores, 0, 59) > g           # one diagonal short of it
    assert oracle.gotoh_penalty_band(a, b, scores, -60, 0) > g
    assert oracle.gotoh_penalty_band(b, a, scores, -60, 0) == g         # the same path with the roles swapped


def test_catches_a_penalty_above_the_optimum(oracle):
    """A deliberately poor CIGAR (the pair aligned base by base, then one gap for the length difference) re-scores to a
    valid cost above the optimum; with that cost as the bound the DP returns less than it -- so a checker that bounds the
    DP by a reported penalty sees a penalty that is too high.  And with bound = optimum - 1 it reports more than the
    bound: a penalty that is too low is seen too."""
    rng = random.Random("banded/poor")
    for scores in (DEFAULT_2P, EDIT, (0, 4, 6, 2)):
        for n, d in ((3000, 0.02), (8000, 0.01)):
            a = rand_seq(rng, n)
            b = mutate(a, d, rng)
            k = min(len(a), len(b))
            poor = bytes(ord("M") if a[i] == b[i] else ord("X") for i in range(k))
            poor += (b"D" if len(a) > k else b"I") * abs(len(a) - len(b))
            rc, cost = oracle.cigar_check(poor, a, b, scores)
            assert rc == 0
            opt, ops = oracle.Aligner(scores).align(a, b)
            assert cost > opt
            got = oracle.gotoh_penalty_banded(a, b, scores, cost)
            assert got < cost and got == opt, (scores, n, cost, got, opt)
            assert oracle.gotoh_penalty_banded(a, b, scores, opt - 1) == opt


def test_thread_pool(oracle):
    """The pool helper gives the same answers as the direct calls, in order, and is never sized past 16 threads."""
    rng = random.Random("banded/pool")
    jobs = []
    for _ in range(12):
        s, t = random_pair(rng, 800)
        jobs.append((s, t, DEFAULT_2P, oracle.gotoh_penalty(s, t, DEFAULT_2P)))
    futs = oracle.gotoh_penalty_banded_many(jobs)
    assert [f.result() for f in futs] == [j[3] for j in jobs]
    assert oracle.dp_pool()._max_workers <= 16


def _align_then_dp(oracle, scores, p, t):
    pen, ops = oracle.Aligner(scores).align(p, t)   # (an aligner of its own: one per thread)
    return pen, ops, oracle.gotoh_penalty_banded(p, t, scores, pen)


def _oracle_vs_dp(oracle, scores, name, seqs, pairs):
    pool = oracle.dp_pool()
    futs = [pool.submit(_align_then_dp, oracle, scores, seqs[a], seqs[b]) for a, b in pairs]
    for (a, b), f in zip(pairs, futs):
        pen, ops, dp = f.result()
        what = (scores, name, len(seqs[a]), len(seqs[b]), pen)
        assert oracle.cigar_check(ops, seqs[a], seqs[b], scores) == (0, pen), what
        assert dp == pen, what + (dp,)


@pytest.mark.parametrize("scores,full", LP.ORACLE_SETS, ids=["%s%s" % (",".join(map(str, s)), "" if f else "/gaps")
                                                             for s, f in LP.ORACLE_SETS])
def test_oracle_is_the_optimum_on_long_pairs(oracle, scores, full):
    """The oracle (BiWFA: breakpoints, recursion, base cases) against the banded DP at 20-70 kbp: random pairs at 1-3 %,
    the very unequal shapes, 12-40 kbp tandem arrays, 4.2 and 16.5 kbp copy deletions and forced gaps around the set's
    piece crossover and of 4 and 17 kbp.  The penalty equals the DP bounded by it and the CIGAR re-scores to it."""
    for name, seqs, pairs in LP.oracle_inputs(scores, full):
        _oracle_vs_dp(oracle, scores, name, seqs, pairs)
