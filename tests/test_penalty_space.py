"""CPU tests (-m "not gpu") over the penalty space of tests/penalty_space.py.

(i) A coverage guard: the named sets must reach every class the engine derives from a penalty set -- every ring depth,
every number of steps per multi-step pass, every number of chained sweeps, every 2-piece shape, both sides of the scope
and base-case history limits -- so that a later edit of the list cannot quietly drop a corner the GPU tests rely on.
(ii) The oracle at every accepted set: it is the judge of tests/test_gpu_penalties.py, so it has to be right there first --
penalty == Gotoh DP == the re-scored CIGAR, BiWFA and plain WFA agree, and the kernel's shortcuts (exact overlap
pre-filter, known-optimum stop) give the same bytes.
"""
import random

import pytest

import penalty_space as PS
import repeats
from util import random_pair


def _accepted():
    return [(n, s, PS.derive(s)) for n, s in PS.ACCEPTED]


def test_names_are_unique():
    names = [n for n, _ in PS.PENALTY_SPACE]
    assert len(names) == len(set(names))
    assert len(set(s for _, s in PS.PENALTY_SPACE)) == len(names)


def test_every_ring_depth_is_reached():
    rings = {d.ring for _, _, d in _accepted()}
    want = set()
    r = 4
    while r <= PS.MAX_RING:
        want.add(r)
        r *= 2
    assert rings == want, sorted(rings)


def test_every_pass_length_and_chain_is_reached():
    acc = _accepted()
    assert {d.multi_T for _, _, d in acc} == {0, 2, 3, 4, 5}
    assert {d.multi_T32 for _, _, d in acc} == {0, 2, 3, 4, 5}
    assert {d.chain_max for _, _, d in acc} == {1, 2, 3}
    # passes with and without chaining at the deepest ring
    assert {d.chain_max for _, _, d in acc if d.ring == PS.MAX_RING and d.multi_T} == {1, 3}
    # the gating: sets whose nearest M source would allow a pass but whose I/D depths have no instance
    gated = [n for n, s, d in acc
             if d.multi_T == 0 and min(d.x, d.o1 + d.e1, d.o2 + d.e2, PS.TMAX) >= 2]
    assert any(PS.derive(PS.BY_NAME[n]).two_piece for n in gated), gated
    assert any(not PS.derive(PS.BY_NAME[n]).two_piece and PS.derive(PS.BY_NAME[n]).e1 == 3 for n in gated), gated


def test_every_two_piece_shape_is_reached():
    seen = set()
    for _, s, _ in _accepted():
        seen |= PS.shapes(s)
    assert seen == {"equal", "usual", "inverted", "crossing", "o2_zero", "piece1_never_cheapest"}, seen
    # inverted with multi-step passes on, crossing of the pieces at a length > 1
    assert any("inverted" in PS.shapes(s) and d.multi_T > 0 for _, s, d in _accepted())
    assert any("crossing" in PS.shapes(s) and "inverted" in PS.shapes(s) for _, s, d in _accepted())


def test_both_sides_of_the_limits():
    acc = _accepted()
    rej = [(n, s, PS.derive(s)) for n, s in PS.REJECTED]
    assert max(d.scope for _, _, d in acc) == PS.MAX_SCOPE
    assert any(d.reason == "scope" and d.scope == PS.MAX_SCOPE + 1 for _, _, d in rej)
    # scope 93 .. 126, beyond what the older suites ran
    assert len({d.scope for _, _, d in acc if d.scope > 92}) >= 4
    assert max(d.sb for _, _, d in acc) == PS.MAX_SB
    assert any(d.reason == "sb" and d.sb == PS.MAX_SB + 1 for _, _, d in rej)
    assert any(1000 < d.sb < PS.MAX_SB for _, _, d in acc)
    assert max(d.ring for _, _, d in acc) == PS.MAX_RING
    reasons = {d.reason for _, _, d in rej}
    assert {"scope", "sb", "match != 0", "need x > 0, o >= 0, e > 0", "need o2 >= 0, e2 > 0"} <= reasons
    assert 28 <= len(acc) <= 40


def test_restatement_on_the_documented_boundaries():
    """The boundaries as worked out by hand from engine.hip."""
    d = PS.derive
    assert d((0, 124, 0, 1)).accepted and d((0, 125, 3, 1)).accepted and not d((0, 126, 3, 1)).accepted
    assert d((0, 20, 0, 20)).sb == 4000 and d((0, 20, 0, 20)).accepted
    assert d((0, 20, 1, 20)).sb == 4001 and not d((0, 20, 1, 20)).accepted
    assert d((0, 1, 0, 1)).ring == 4
    dd = d((0, 5, 8, 2, 24, 1))
    assert (dd.scope, dd.multi_T, dd.multi_T32, dd.chain_max, dd.ring, dd.sb) == (26, 5, 5, 3, 64, 274)
    for s in ((0, 5, 121, 1), (0, 5, 120, 2), (0, 5, 123, 2), (0, 125, 3, 1)):
        assert d(s).ring == 256, s
    # the flags that change the derivation
    dd = d((0, 5, 8, 2, 24, 1), PS.AWV_F_NO_CHAIN)
    assert (dd.multi_T, dd.chain_max, dd.ring) == (5, 1, 32)
    dd = d((0, 5, 8, 2, 24, 1), PS.AWV_F_SINGLE_STEP)
    assert (dd.multi_T, dd.multi_T32, dd.chain_max, dd.ring) == (0, 0, 1, 32)
    # every accepted ring holds the scope and a chained pass: multi_T * chain_max <= ring - scope - 1
    for _, s, x in _accepted():
        assert x.multi_T * x.chain_max <= x.ring - x.scope - 1 and x.ring <= PS.MAX_RING, s


def _check_oracle(oracle, scores, s, t, al, fast, what):
    pen, ops = al.align(s, t)
    pen_u, ops_u = al.align_unidirectional(s, t)
    g = oracle.gotoh_penalty(s, t, scores)
    assert oracle.cigar_check(ops, s, t, scores) == (0, g), (scores, what, len(s), len(t))
    assert oracle.cigar_check(ops_u, s, t, scores) == (0, g), (scores, what, len(s), len(t))
    assert pen == pen_u == g, (scores, what, len(s), len(t), pen, pen_u, g)
    assert fast.align(s, t) == (pen, ops), (scores, what, len(s), len(t))


@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_oracle_optimal_and_valid(oracle, name):
    """random_pair inputs up to 600 bp and two repeat families (microsatellites, periodic / two-letter sequence) at every
    accepted set."""
    scores = PS.BY_NAME[name]
    rng = random.Random("penalty-space/" + name)
    al, fast = oracle.Aligner(scores), oracle.Aligner(scores)
    fast.set_fast_overlap(True)
    for it in range(60):
        s, t = random_pair(rng, 600)
        _check_oracle(oracle, scores, s, t, al, fast, it)
    for family, gen in (("microsatellite", lambda: repeats.microsatellite(rng, flank=(30, 200))),
                        ("low_complexity", lambda: repeats.low_complexity(rng, n=(100, 600)))):
        for it in range(5):
            s, t = gen()
            _check_oracle(oracle, scores, s, t, al, fast, family)
