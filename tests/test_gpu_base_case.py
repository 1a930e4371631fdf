"""GPU tests (-m gpu) of the base case -- plain WFA over the history arena and the backtrace through it -- against the CPU
oracle: status, penalty, CIGAR length, M/X/I/D counts, q_end, t_end and every CIGAR byte of every pair.

The inputs are the shapes where the base case can go wrong: config-2 pairs (16 base cases per pair), pairs so short that
the top level is itself a base case, every penalty preset the command line offers (one- and two-piece backtrace
candidates), long indels that breakpoints fall into (base cases that begin / end in an I or D component), and forced gaps
between very unequal lengths inside one base case (rows leave the matrix: the pass is discarded and the rest goes step by
step with trimmed rows)."""
import random

import pytest

from util import DEFAULT_2P, mutate, rand_seq

pytestmark = pytest.mark.gpu

# main.rs:83-124 (parse_ani_preset): ANI >= 95, >= 85 (the default), >= 75, >= 65, below
CLI_PRESETS = [(0, 7, 12, 2, 36, 1), (0, 5, 8, 2, 24, 1), (0, 4, 6, 2, 18, 1), (0, 3, 4, 1), (0, 1, 1, 1)]
FIELDS = ("status", "penalty", "cigar_len", "num_matches", "num_mismatches", "num_ins", "num_del", "q_end", "t_end")


def run(seqs, pairs, scores, base_flags):
    from allwave_amd import ffi
    e = ffi.Engine(flags=base_flags)
    try:
        e.set_sequences(seqs)
        res, cigs = e.align_pairs(scores, pairs)
        return res, cigs, e.stats()
    finally:
        e.close()


def assert_oracle(oracle, out, seq_of, pairs, scores, what):
    """Every pair, field by field and byte by byte."""
    res, cigs, _ = out
    al = oracle.Aligner(scores)
    for i, p in enumerate(pairs):
        s, t = seq_of(p[0]), seq_of(p[1])
        pen, ops = al.align(s, t)
        assert res["status"][i] == 0 and res["penalty"][i] == pen, (what, i, int(res["status"][i]), int(res["penalty"][i]), pen)
        assert cigs[i] == ops, (what, i)
        c = {k: ops.count(k.encode()) for k in "MXID"}
        got = tuple(int(res[f][i]) for f in FIELDS[2:])
        assert got == (len(ops), c["M"], c["X"], c["I"], c["D"], len(s), len(t)), (what, i, got)


def flavours():
    from allwave_amd import ffi
    return (("one_wave", ffi.AWV_F_ONE_WAVE), ("auto", 0))


def test_config2_pairs(oracle):
    """The parity tests' config-2 sample (40 of the 65,280 pairs of 10 kbp)."""
    from allwave_amd import synth
    data, offs, _ = synth.generate(256, 10000, 0.05, 2)
    sample = synth.all_pairs(256)[::1571][:40]
    for fname, bf in flavours():
        out = run((data, offs), sample, DEFAULT_2P, bf)
        assert_oracle(oracle, out, lambda i: bytes(data[offs[i]:offs[i + 1]]), sample, DEFAULT_2P, fname)
        assert int(out[2].n_base) > len(sample) and int(out[2].windows[3]) > 0, "the base cases ran, in passes"


def test_top_level_base_cases(oracle):
    """Pairs of at most 100 bases (A.6: the top level is a base case, no known score) and longer pairs that end at score 0
    or a handful of mismatches."""
    rng = random.Random(9101)
    seqs, pairs = [], []
    for n in (1, 2, 7, 33, 64, 99, 100):
        for d in (0.0, 0.05, 0.3):
            s = rand_seq(rng, n)
            t = mutate(s, d, rng) or b"A"
            seqs += [s, t, rand_seq(rng, max(1, n - n // 3))]
            k = len(seqs) - 3
            pairs += [(k, k + 1), (k + 1, k), (k, k + 2), (k + 2, k), (k, k)]
    for fname, bf in flavours():
        out = run(seqs, pairs, DEFAULT_2P, bf)
        assert_oracle(oracle, out, lambda i: seqs[i], pairs, DEFAULT_2P, fname)


@pytest.mark.parametrize("scores", CLI_PRESETS)
def test_every_cli_preset(oracle, scores):
    """3-8 kbp pairs at 3-12 % under each preset of the command line (two-piece: nine backtrace candidates per M step;
    one-piece: five)."""
    rng = random.Random(7000 + scores[1] * 31 + len(scores))
    seqs, pairs = [], []
    for n, d in ((3000, 0.05), (8000, 0.03), (5000, 0.12)):
        a = rand_seq(rng, n)
        b = mutate(a, d, rng)
        seqs += [a, b, b[: n - n // 7]]
        k = len(seqs) - 3
        pairs += [(k, k + 1), (k + 1, k), (k + 2, k), (k, k + 2)]
    for fname, bf in flavours():
        out = run(seqs, pairs, scores, bf)
        assert_oracle(oracle, out, lambda i: seqs[i], pairs, scores, (fname, scores))


def indel_rich(rng, n, gaps):
    """A low-divergence pair with long insertions and deletions every few hundred bases: breakpoints fall inside them, so the
    sub-problems on either side begin / end in a gap component."""
    a = rand_seq(rng, n)
    b = bytearray()
    i = 0
    while i < n:
        step = rng.randrange(150, 500)
        b += a[i:i + step]
        i += step
        g = rng.choice(gaps)
        if rng.random() < 0.5:
            i += g  # deletion from a
        else:
            b += rand_seq(rng, g)
    return a, mutate(bytes(b), 0.01, rng)


def test_base_cases_that_begin_or_end_in_a_gap(oracle):
    """Long indels (12-220 bases: both gap pieces) close together, default scores and the other 2-piece presets."""
    rng = random.Random(4471)
    seqs, pairs = [], []
    for n, gaps in ((4000, (12, 30, 60)), (6000, (40, 90, 220)), (10000, (15, 25, 120)), (3000, (100, 180))):
        a, b = indel_rich(rng, n, gaps)
        seqs += [a, b]
        k = len(seqs) - 2
        pairs += [(k, k + 1), (k + 1, k)]
    for scores in (DEFAULT_2P, (0, 7, 12, 2, 36, 1)):
        for fname, bf in flavours():
            out = run(seqs, pairs, scores, bf)
            assert_oracle(oracle, out, lambda i: seqs[i], pairs, scores, (fname, scores))


def test_forced_gap_trims_rows_inside_a_base_case(oracle):
    """Very unequal lengths whose whole alignment costs less than the base case's score threshold (250): one forced gap of
    120-200 bases next to 40-120 bases that match.  The wavefronts run off the short side of the matrix (opening the
    second gap piece and crossing the 40-120 diagonals of the short sequence costs far less than the forced gap), a pass
    sees it and is discarded, and the rest of that base case goes step by step with trimmed rows: step-by-step base windows
    are counted."""
    rng = random.Random(3313)
    seqs, pairs = [], []
    for short, gap in ((40, 200), (60, 200), (90, 160), (120, 120), (101, 140)):
        s = rand_seq(rng, short)
        cut = rng.randrange(0, short + 1)
        t = s[:cut] + rand_seq(rng, gap) + s[cut:]
        seqs += [s, t, mutate(t, 0.01, rng)]
        k = len(seqs) - 3
        pairs += [(k, k + 1), (k + 1, k), (k, k + 2), (k + 2, k)]
    for fname, bf in flavours():
        out = run(seqs, pairs, DEFAULT_2P, bf)
        assert_oracle(oracle, out, lambda i: seqs[i], pairs, DEFAULT_2P, fname)
        print(fname, "windows", list(out[2].windows))
        assert int(out[2].windows[2]) > 0, (fname, "no base case left its passes: the rows were never trimmed")
