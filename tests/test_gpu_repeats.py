"""GPU parity tests (-m gpu) on repeat-rich inputs (tests/repeats.py): microsatellites, tandem arrays, copy-number
changes, low-complexity sequence, long exact blocks and poly-A / poly-T ends.  On these many alignments are optimal,
so the CIGAR is decided by tie-breaking -- the breakpoint search's first hit in ascending k, the backtrace's choice among
equal candidates, min(h, v) in wide16 rows, the known-optimum stop and the step-by-step restart of a search that met
inside a pass -- and every path must still give the oracle's bytes (the sequential WFA2 order is the contract)."""
import os
import random

import numpy as np
import pytest

import repeats as R
from util import DEFAULT_2P, PENALTY_SETS, check_against_oracle, mutate, rand_seq

pytestmark = pytest.mark.gpu

COMP = {65: 84, 84: 65, 67: 71, 71: 67}


def rc(s):
    return bytes(COMP.get(b, 78) for b in reversed(s))


def pair_set(pairs_ab, both_orders=True):
    """(seqs, pairs) from a list of (a, b): each pair as (0, 1)-style indices, and swapped if asked."""
    seqs, pairs = [], []
    for a, b in pairs_ab:
        seqs += [a, b]
        k = len(seqs) - 2
        pairs.append((k, k + 1))
        if both_orders:
            pairs.append((k + 1, k))
    return seqs, pairs


def oracle_all_pairs_check(oracle, seqs, pairs, scores, res, cigs):
    """Penalty and FNV-1a of the op bytes against the oracle's thread-pool driver, pair by pair; (q, t, 1) pairs align the
    reverse complement of q, which the oracle gets as a sequence of its own."""
    extra = []
    opairs = []
    for p in pairs:
        a, b = p[0], p[1]
        if len(p) > 2 and p[2]:
            extra.append(rc(seqs[a]))
            a = len(seqs) + len(extra) - 1
        opairs.append((a, b))
    allseqs = list(seqs) + extra
    data = np.frombuffer(b"".join(allseqs), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in allseqs])]).astype(np.uint64)
    _, ores, _, _ = oracle.all_pairs(data, offs, np.asarray(opairs, dtype=np.int32), scores,
                                     nthreads=min(8, os.cpu_count() or 1))
    assert (ores["status"] == 0).all() and (res["status"] == 0).all()
    for i, (a, b) in enumerate(opairs):
        assert res["penalty"][i] == ores["penalty"][i], (scores, pairs[i], len(allseqs[a]), len(allseqs[b]))
        assert res["q_end"][i] == len(allseqs[a]) and res["t_end"][i] == len(allseqs[b]), (scores, pairs[i])
        assert oracle.fnv1a(cigs[i]) == int(ores["cigar_hash"][i]), (scores, pairs[i], len(allseqs[a]), len(allseqs[b]))


def family_pairs(rng):
    """Two pairs per family, every sequence at most ~12 kbp."""
    gens = (lambda: R.microsatellite(rng), lambda: R.end_runs(rng), lambda: R.tandem(rng, total=(3000, 11000)),
            lambda: R.cnv(rng, seg=(50, 2000), flank=(200, 1500)), lambda: R.low_complexity(rng),
            lambda: R.exact_blocks(rng, block=(2000, 5000), nblocks=(2, 2)))
    return [g() for g in gens for _ in range(2)]


@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_repeat_families_bit_exact(engine, oracle, scores):
    """Every family, both orders of every pair, the six penalty sets: bytes, penalty and op counts equal the oracle's."""
    seqs, pairs = pair_set(family_pairs(random.Random("gpu-families/%s" % (scores,))))
    check_against_oracle(engine, oracle, seqs, pairs, scores)


def test_every_flavour_agrees_on_repeats(oracle):
    """The flag matrix of test_row_width_and_sequence_paths_agree plus the round-2 margin zone (AWV_F_NO_DEEP), passes
    without chained sweeps (AWV_F_NO_CHAIN) and four waves step by step, on a medium repeat set: every flavour equals the
    oracle byte for byte."""
    from allwave_amd import ffi
    rng = random.Random(171)
    ab = [R.microsatellite(rng) for _ in range(3)] + [R.end_runs(rng) for _ in range(3)]
    ab += [R.tandem(rng, total=(1500, 5000)) for _ in range(3)] + [R.cnv(rng, seg=(50, 1200), flank=(100, 800)) for _ in range(3)]
    ab += [R.low_complexity(rng) for _ in range(3)] + [R.exact_blocks(rng, block=(1500, 2500), nblocks=(2, 2))]
    seqs, pairs = pair_set(ab, both_orders=False)
    F = ffi
    for flags in (F.AWV_F_ONE_WAVE, F.AWV_F_FOUR_WAVES, F.AWV_F_ONE_WAVE | F.AWV_F_SINGLE_STEP, F.AWV_F_ONE_WAVE | F.AWV_F_NO_CHAIN,
                  F.AWV_F_FOUR_WAVES | F.AWV_F_SINGLE_STEP, F.AWV_F_ONE_WAVE | F.AWV_F_FORCE_INT32,
                  F.AWV_F_FOUR_WAVES | F.AWV_F_FORCE_INT32, F.AWV_F_ONE_WAVE | F.AWV_F_NO_PACKED_SEQ,
                  F.AWV_F_FOUR_WAVES | F.AWV_F_NO_PACKED_SEQ, F.AWV_F_ONE_WAVE | F.AWV_F_FORCE_INT32 | F.AWV_F_NO_PACKED_SEQ,
                  F.AWV_F_ONE_WAVE | F.AWV_F_NO_DEEP, F.AWV_F_NO_DEEP, F.AWV_F_NO_CHAIN,
                  F.AWV_F_FOUR_WAVES | F.AWV_F_SINGLE_STEP | F.AWV_F_NO_CHAIN):
        e = ffi.Engine(flags=flags)
        try:
            for scores in (DEFAULT_2P, (0, 4, 6, 2)):
                check_against_oracle(e, oracle, seqs, pairs, scores)
        finally:
            e.close()


def test_repeat_paths_reached(oracle):
    """3-12 kbp tandem arrays, and 3-12 kbp arrays with one copy deleted (copy-number change) between sequences 3 % apart,
    under one wave per pair: the work ran where it is meant to -- mostly in multi-step passes, some in the deep margin zone,
    overlap searches and base cases ran -- and the result is bit-exact.  Where the only real difference is one long gap the
    cell-steps go to that gap's wide wavefronts, searched step by step: measured on an MI355X, copy deletions between
    sequences 0.5 % apart ran 4-28 % of their cell-steps in passes (2 %: 33-72 %, 3 %: 58-79 %), and segments duplicated
    2-5 times in place 0-14 %.  For the duplications only the deep zone, the overlap search and the base cases are asserted."""
    from allwave_amd import ffi
    rng = random.Random(3012)
    groups = (("tandem", [R.tandem(rng, total=(3000, 12000)) for _ in range(4)], True),
              ("cnv deletion", [R.cnv_deletion(rng, u, rng.randint(3000, 12000) // u, (50, 300), noise=0.03)
                                for u in (171, 171, rng.randint(20, 500), rng.randint(20, 500))], True),
              ("cnv duplication", [R.cnv_duplication(rng, seg=(300, 2000), flank=(1000, 2000)) for _ in range(2)], False))
    e = ffi.Engine(flags=ffi.AWV_F_ONE_WAVE)
    try:
        for name, ab, passes in groups:
            seqs, pairs = pair_set(ab)
            check_against_oracle(e, oracle, seqs, pairs, DEFAULT_2P)
            st = e.stats()
            print("%s: cell_steps %d multi %d deep %d overlap_scans %d n_base %d restarts %d" %
                  (name, st.cell_steps, st.multi_cell_steps, st.deep_cell_steps, st.overlap_scans, st.n_base, st.restarts))
            if passes:
                assert st.multi_cell_steps > 0.3 * st.cell_steps, (name, st.multi_cell_steps, st.cell_steps)
            assert st.deep_cell_steps > 0 and st.overlap_scans > 0 and st.n_base > 0, \
                (name, st.deep_cell_steps, st.overlap_scans, st.n_base)
    finally:
        e.close()


RESTART_CASES = R.RESTART_CASES


@pytest.mark.parametrize("case", RESTART_CASES, ids=[c[0] for c in RESTART_CASES])
def test_restarted_searches_on_repeats(oracle, case):
    """The restart path ran (a search that met inside a pass, run again step by step) and the answer is still the oracle's,
    byte for byte -- with the engine's own choice of flavour and with one wave per pair."""
    from allwave_amd import ffi
    name, gen, seed = case
    a, b = gen(random.Random(seed))
    for flags in (0, ffi.AWV_F_ONE_WAVE):
        e = ffi.Engine(flags=flags)
        try:
            check_against_oracle(e, oracle, [a, b], [(0, 1), (1, 0)], DEFAULT_2P)
            st = e.stats()
            print("%s flags %d: %d x %d, restarts %d, cell_steps %d multi %d" %
                  (seed, flags, len(a), len(b), st.restarts, st.cell_steps, st.multi_cell_steps))
            assert st.restarts > 0, (seed, flags)
        finally:
            e.close()


def end_run_sets(rng, body, lengths):
    """Sequences with poly-A / poly-T runs at their ends, the first and the last of the set carrying runs at both ends (next
    to the pad words in front of and behind the packed array); every pair forward, and with the query stored
    reverse-complemented as (q, t, 1) -- a poly-T head stored becomes a poly-A tail aligned."""
    ab = [R.end_runs(rng, body=body, lengths=lengths, where="both")]
    ab += [R.end_runs(rng, body=body, lengths=lengths) for _ in range(len(lengths))]
    ab.append(R.end_runs(rng, body=body, lengths=lengths, where="both"))
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b, rc(a)]
        k = len(seqs) - 3
        pairs += [(k, k + 1, 0), (k + 1, k, 0), (k + 2, k + 1, 1)]
    seqs.append(seqs[0])  # the last sequence of the set: runs at both ends up to the end pad
    pairs += [(len(seqs) - 1, 1, 0), (1, len(seqs) - 1, 0), (2, len(seqs) - 1, 1)]
    return seqs, pairs


def test_homopolymer_ends_on_every_probe_path(oracle):
    """Runs of 15-257 A or T at the sequence ends, against the zero (= A) pad words of the packed sequences: the staged
    packed probes (short pairs), the in-place probes of sub-problems too long to stage (seq_mode 2: >= 20 kbp under one wave
    per pair), the raw-byte probes (AWV_F_NO_PACKED_SEQ), 16- and 32-bit rows -- all against the oracle."""
    from allwave_amd import ffi
    rng = random.Random(257)
    short = end_run_sets(rng, (100, 1500), R.END_RUN_LENGTHS)
    long_ = end_run_sets(rng, (20000, 22000), (31, 32, 33, 255, 256, 257))
    F = ffi
    for flags, (seqs, pairs) in ((0, short), (F.AWV_F_ONE_WAVE, short), (F.AWV_F_ONE_WAVE, long_),
                                 (F.AWV_F_NO_PACKED_SEQ, short), (F.AWV_F_ONE_WAVE | F.AWV_F_NO_PACKED_SEQ, long_),
                                 (F.AWV_F_FORCE_INT32, short), (F.AWV_F_ONE_WAVE | F.AWV_F_FORCE_INT32, long_)):
        e = ffi.Engine(flags=flags)
        try:
            e.set_sequences(seqs)
            res, cigs = e.align_pairs(DEFAULT_2P, pairs)
        finally:
            e.close()
        oracle_all_pairs_check(oracle, seqs, pairs, DEFAULT_2P, res, cigs)


def exact_length(rng, s, n):
    return s[:n] + rand_seq(rng, max(0, n - len(s)))


@pytest.mark.parametrize("length", [32759, 32760])
def test_tandem_at_the_row_width_boundary(engine, oracle, length):
    """Tandem arrays exactly 32759 (the longest on 16-bit rows) and 32760 bases long (the shortest on 32-bit rows)."""
    rng = random.Random(length)
    a, b = R.tandem(rng, total=(33500, 34000), unit_len=171)
    check_against_oracle(engine, oracle, [exact_length(rng, a, length), exact_length(rng, b, length)], [(0, 1), (1, 0)],
                         DEFAULT_2P)


def test_wide16_rows_on_tandem_arrays(oracle):
    """A 36 kbp sequence with a tandem array against a 3 kbp infix of it that holds part of the array (wide16 rows: the
    longer sequence >= 32760, the shorter fits 16 bits): field by field against 32-bit rows (AWV_F_NO_WIDE16), and
    against the oracle."""
    from allwave_amd import ffi
    rng = random.Random(36000)
    unit = rand_seq(rng, 171)
    array = b"".join(mutate(unit, rng.uniform(0.01, 0.05), rng) for _ in range(120))   # 20.5 kbp
    long_a = rand_seq(rng, 8000) + array + rand_seq(rng, 8000)
    short = mutate(long_a[6500:9500], 0.02, rng)                                       # flank into the array
    short2 = mutate(long_a[14000:17000], 0.02, rng)                                    # inside the array
    seqs = [long_a, short, short2, rc(short2)]
    pairs = [(0, 1, 0), (1, 0, 0), (0, 2, 0), (2, 0, 0), (3, 0, 1)]
    out = {}
    for name, flags in (("wide16", 0), ("rows32", ffi.AWV_F_NO_WIDE16)):
        e = ffi.Engine(flags=flags)
        try:
            e.set_sequences(seqs)
            out[name] = e.align_pairs(DEFAULT_2P, pairs)
        finally:
            e.close()
    (res, cigs), (res32, cigs32) = out["wide16"], out["rows32"]
    for f in res.dtype.names:
        assert (res[f] == res32[f]).all(), f
    assert cigs == cigs32
    oracle_all_pairs_check(oracle, seqs, pairs, DEFAULT_2P, res, cigs)


def test_long_tandem_pairs_chain_through_lds(oracle):
    """40-70 kbp tandem arrays: 32-bit rows, a top level too long to stage, passes chaining their middle sweep through LDS,
    and the same engine with chaining off (AWV_F_NO_CHAIN) -- both against the oracle."""
    from allwave_amd import ffi
    rng = random.Random(70000)
    ab = [R.tandem(rng, total=(40000, 44000), unit_len=171), R.tandem(rng, total=(68000, 72000))]
    seqs, pairs = pair_set(ab)
    out = []
    for flags in (0, ffi.AWV_F_NO_CHAIN):
        e = ffi.Engine(flags=flags)
        try:
            e.set_sequences(seqs)
            res, cigs = e.align_pairs(DEFAULT_2P, pairs)
            st = e.stats()
            print("chain flags %d: cell_steps %d multi %d restarts %d" % (flags, st.cell_steps, st.multi_cell_steps, st.restarts))
            assert st.multi_cell_steps > 0.3 * st.cell_steps, (flags, st.multi_cell_steps, st.cell_steps)
        finally:
            e.close()
        out.append((res["penalty"].tolist(), cigs))
        oracle_all_pairs_check(oracle, seqs, pairs, DEFAULT_2P, res, cigs)
    assert out[0] == out[1]


def test_cnv_deletions_on_the_wide_flavours(oracle):
    """One copy of a tandem array deleted: 4.2 kbp (|dlen| >= 4096: four waves per pair) and 16.5 kbp (>= 16384: sixteen
    waves), both orders, the engine's own routing and one wave per pair -- against the oracle."""
    from allwave_amd import ffi
    rng = random.Random(16384)
    ab = [R.cnv_deletion(rng, 4200, 3), R.cnv_deletion(rng, 16500, 3)]
    seqs, pairs = pair_set(ab)
    assert abs(len(seqs[0]) - len(seqs[1])) >= 4096 and abs(len(seqs[2]) - len(seqs[3])) >= 16384
    for flags in (0, ffi.AWV_F_ONE_WAVE):
        e = ffi.Engine(flags=flags)
        try:
            e.set_sequences(seqs)
            res, cigs = e.align_pairs(DEFAULT_2P, pairs)
        finally:
            e.close()
        oracle_all_pairs_check(oracle, seqs, pairs, DEFAULT_2P, res, cigs)
