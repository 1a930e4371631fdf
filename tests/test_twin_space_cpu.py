"""CPU test of the inputs of tests/test_gpu_twin_space.py, from the oracle alone: the both-order lists over the penalty
space must be lists on which the two orders of a pair break ties differently, or the GPU comparisons of the twin path's
per-orientation tie decision would pass without exercising it.  These are conditions on the inputs, not
on the kernel: when a generator changes, the inputs are changed until the counts hold again."""
import penalty_space as PS
import twin_cases as TC


def test_swapped_pairs_cost_the_same_and_break_ties_differently(oracle):
    """Per accepted set, 12 unordered pairs in both orders: penalty(j, i) == penalty(i, j) for every one of them; the pairs
    whose (j, i) CIGAR is not the I/D swap of the (i, j) CIGAR are at least 80 of the 372 (measured: 103), and at least 7 of
    12 under each tie-rich set (measured: affine_e3_o0 11, 2p_T2 7, 2p_o2_zero 10, 2p_piece1_never 8, scope101_T5 10,
    scope125 10, ring256_scope126_T4 11).  And every set's list holds a pair dear enough for a search below the top level
    (twin_cases.second_level), without which "a search below the top level ran shared" could not be asked of it: the 12
    pairs hold one under 26 sets, and under the five DEEP_SETS -- exactly the others -- the four extra pairs all are."""
    differ = {}
    for name, scores in PS.ACCEPTED:
        seqs, pairs = TC.penalty_inputs(name)
        assert all(pairs[k + 1] == pairs[k][::-1] for k in range(0, len(pairs), 2))
        want = TC.oracle_records(oracle, seqs, pairs, scores, key=("twin-penalties", name))
        for k in range(0, len(pairs), 2):
            assert want[k][0] == want[k + 1][0], (name, pairs[k], want[k][0], want[k + 1][0])
        differ[name] = TC.not_mirrored(want[:24])
        deep = [TC.second_level(scores, want[k][0]) for k in range(0, len(pairs), 2)]
        assert len(deep) == (12 + TC.DEEP_EXTRA if name in TC.DEEP_SETS else 12), name
        assert (not any(deep[:12])) == (name in TC.DEEP_SETS), (name, deep)
        assert all(deep[12:]), (name, deep)
    print(" ".join("%s:%d" % kv for kv in differ.items()))
    print("%d of %d unordered pairs: the swapped pair's CIGAR is not the I/D swap" % (sum(differ.values()), 12 * len(differ)))
    assert len(differ) == 31
    assert sum(differ.values()) >= TC.TIE_TOTAL_MIN
    for name in TC.TIE_RICH:
        assert differ[name] >= TC.TIE_RICH_MIN, (name, differ[name])
