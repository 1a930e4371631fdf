"""CPU tests (-m "not gpu") that pin the oracle.

The reference holds no golden CIGAR/score for this path ("parity unpinned"), so the
oracle is pinned by (i) an independent Gotoh full DP (optimality), (ii) CIGAR validity + re-scoring
(/root/reference/src/wfa.rs:105-176 restated in oracle/cigar_check.c), (iii) every known-answer
property the reference's own tests assert on this path, (iv) the committed fixtures under
tests/golden/ (oracle-generated, labelled as such; they freeze tie-breaking across rounds).
"""
import json
import os
import random

import statistics

import pytest

import repeats
from util import DEFAULT_2P, EDIT, PENALTY_SETS, mutate, rand_seq, random_pair, rle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def counts(ops):
    return {c: ops.count(c.encode()) for c in "MXID"}


def test_kat_alignment_correctness(oracle):
    """tests/integration_tests.rs:599-672: exactly 2 mismatches, 1 insertion, 1 deletion
    (standard CIGAR letters after the I/D swap) with the default scores => penalty 2*5+2*(8+2)."""
    ref = b"ATCG" * 25
    q = bytearray(ref)
    q[10] = ord("G")
    q[20] = ord("C")
    del q[30]
    q.insert(40, ord("A"))
    pen, ops = oracle.Aligner(DEFAULT_2P).align(bytes(q), ref)
    c = counts(ops)
    assert (c["X"], c["I"], c["D"]) == (2, 1, 1)
    assert pen == 30
    s = rle(ops)
    assert s.count("X") == 2 and s.count("I") == 1 and s.count("D") == 1


def test_kat_identical(oracle):
    """tests/integration_tests.rs:216-260: identical sequences => all matches, identity 1."""
    rng = random.Random(5)
    s = rand_seq(rng, 5000)
    for scores in (DEFAULT_2P, EDIT):
        pen, ops = oracle.Aligner(scores).align(s, s)
        assert pen == 0 and ops == b"M" * 5000


def test_kat_debug_probes(oracle):
    """Expected shapes printed by the reference's lib_wfa2 probes: one X at column 8
    (tests/debug/check_wfa_ops.rs:15-20); 8 matches + 2 gap ops whose letter depends on which
    side is longer (tests/debug/test_cigar_interpretation.rs:38-116, test_wfa_order.rs:1-31)."""
    a = oracle.Aligner((0, 4, 6, 2))  # AffineWavefronts::default() penalties [RECALLED]
    pen, ops = a.align(b"ACGTACGTACGT", b"ACGTACGTTCGT")
    assert ops == b"MMMMMMMMXMMM" and pen == 4
    pen, ops = a.align(b"ACGTACGTAA", b"ACGTACGT")  # query longer: 'D' consumes the query
    assert ops == b"MMMMMMMMDD"
    pen, ops = a.align(b"ACGTACGT", b"ACGTACGTAA")  # target longer: 'I' consumes the target
    assert ops == b"MMMMMMMMII"
    pen, ops = oracle.Aligner((0, 5, 8, 2)).align(b"ACGTACGTACGT", b"ACGTACGTAC")
    assert ops == b"MMMMMMMMMMDD" and pen == 12


def test_edit_mode_is_gap_affine(oracle):
    """allwave's "edit distance" builds gap-affine (x,x,x)
    (/root/reference/src/alignment.rs:265-271), so a 1-bp indel costs 2x, not x."""
    pen, ops = oracle.Aligner(EDIT).align(b"ACGTTACGT", b"ACGTACGT")
    assert pen == 2 and counts(ops)["D"] == 1


def test_empty_and_trivial(oracle):
    a = oracle.Aligner(DEFAULT_2P)
    assert a.align(b"", b"") == (0, b"")
    assert a.align(b"", b"ACGT") == (16, b"IIII")       # min(8+2*4, 24+4)
    assert a.align(b"ACGT", b"") == (16, b"DDDD")
    pen, ops = a.align(b"A", b"C")
    assert pen == 5 and ops == b"X"
    pen, ops = a.align(b"A" * 40, b"")
    assert pen == 64 and ops == b"D" * 40               # second piece: 24 + 40


def test_penalties_rejected(oracle):
    for bad in [(1, 5, 8, 2), (0, 0, 8, 2), (0, 5, 8, 0), (0, 5, -1, 2), (0, 5, 8, 2, 24, 0)]:
        with pytest.raises(ValueError):
            oracle.Aligner(bad)


@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_optimal_and_valid_random(oracle, scores):
    """penalty == Gotoh DP == re-scored CIGAR, BiWFA and plain WFA agree on the penalty."""
    rng = random.Random(hash(scores) & 0xFFFF)
    al = oracle.Aligner(scores)
    for it in range(70):
        s, t = random_pair(rng, 1200)
        st = oracle.Stats()
        pen, ops = al.align(s, t, st)
        pen_u, ops_u = al.align_unidirectional(s, t)
        g = oracle.gotoh_penalty(s, t, scores)
        rc, rescored = oracle.cigar_check(ops, s, t, scores)
        rc_u, rescored_u = oracle.cigar_check(ops_u, s, t, scores)
        assert rc == 0 and rc_u == 0, (scores, len(s), len(t))
        assert pen == g == rescored == pen_u == rescored_u, (scores, len(s), len(t))


def test_biwfa_recursion_exercised(oracle):
    """A 3 kbp / 10% pair must go through breakpoints, base cases and several levels."""
    rng = random.Random(3)
    s = rand_seq(rng, 3000)
    t = mutate(s, 0.10, rng)
    st = oracle.Stats()
    pen, ops = oracle.Aligner(DEFAULT_2P).align(s, t, st)
    assert st.n_breakpoints >= 3 and st.n_base >= 4 and st.max_level >= 2
    assert pen == oracle.gotoh_penalty(s, t, DEFAULT_2P)
    assert oracle.cigar_check(ops, s, t, DEFAULT_2P) == (0, pen)


def test_raw_bytes_and_case(oracle):
    """Bytes are compared verbatim: case-sensitive, 'N' == 'N' (SURVEY Appendix B)."""
    a = oracle.Aligner(EDIT)
    assert a.align(b"acgt", b"ACGT")[0] == 4
    assert a.align(b"ACNNGT", b"ACNNGT") == (0, b"MMMMMM")
    rng = random.Random(9)
    alpha = bytes(range(256))
    for _ in range(30):
        s = rand_seq(rng, rng.choice([10, 120, 400]), alpha)
        t = mutate(s, 0.2, rng, alpha)
        pen, ops = a.align(s, t)
        assert pen == oracle.gotoh_penalty(s, t, EDIT)
        assert oracle.cigar_check(ops, s, t, EDIT) == (0, pen)


def test_golden_fixtures(oracle):
    """tests/golden/oracle_kats.json (written by tests/golden/make_golden.py from this oracle)."""
    with open(os.path.join(GOLDEN, "oracle_kats.json")) as f:
        doc = json.load(f)
    assert doc["provenance"].startswith("oracle-generated")
    for case in doc["cases"]:
        pen, ops = oracle.Aligner(tuple(case["scores"])).align(case["pattern"].encode("latin1"),
                                                              case["text"].encode("latin1"))
        assert pen == case["penalty"], case["name"]
        assert rle(ops) == case["cigar"], case["name"]


def test_all_pairs_driver(oracle):
    """The thread-pool driver (bench cpu_baseline leg) agrees with single calls."""
    import numpy as np
    from allwave_amd import synth
    data, offs, _ = synth.generate(6, 600, 0.05, 7)
    pairs = synth.all_pairs(6)
    secs, res, st, paf = oracle.all_pairs(data, offs, pairs, DEFAULT_2P, nthreads=2, want_paf=True)
    assert len(res) == 30 and (res["status"] == 0).all() and paf > 0
    al = oracle.Aligner(DEFAULT_2P)
    for i, (a, b) in enumerate(pairs):
        pen, ops = al.align(bytes(data[offs[a]:offs[a + 1]]), bytes(data[offs[b]:offs[b + 1]]))
        assert res["penalty"][i] == pen and res["cigar_len"][i] == len(ops)
        assert res["num_matches"][i] == ops.count(b"M")


def test_fast_overlap_mode_is_identical(oracle):
    """The CPU-baseline mode (exact antidiagonal pre-filter in the overlap search; a sub-problem with
    match components at both ends stops searching at its known optimal score -- the two exact
    shortcuts the GPU kernel also takes) must return the same penalties and CIGARs as the plain
    WFA2-order search the checker uses, also on pairs with long gaps (breakpoints inside gaps)."""
    rng = random.Random(77)
    for scores in (DEFAULT_2P, EDIT, (0, 3, 5, 1, 20, 1), (0, 2, 12, 1, 40, 1)):
        plain, fast = oracle.Aligner(scores), oracle.Aligner(scores)
        fast.set_fast_overlap(True)
        for it in range(70):
            s, t = random_pair(rng, 4000)
            if it % 3 == 0:  # cut long gaps out of the text
                for _ in range(rng.randint(1, 3)):
                    cut = rng.randint(0, len(t))
                    t = t[:cut] + t[min(len(t), cut + rng.randint(20, 900)):]
            elif it % 3 == 1:  # or insert unrelated sequence
                cut = rng.randint(0, len(t))
                t = t[:cut] + rand_seq(rng, rng.randint(20, 600)) + t[cut:]
            assert plain.align(s, t) == fast.align(s, t)


def test_pin_files_are_what_the_oracle_gives():
    """tests/golden/pin/ (the FASTA read sets and expected PAF lines a maintainer diffs against a built allwave, pin.sh) and
    tests/golden/oracle_kats.tsv (what integration/hip_parity.rs feeds to lib_wfa2) are regenerated in memory and must equal
    the committed files: a change of the oracle's tie-breaking cannot leave stale pin files behind."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_pin", os.path.join(here, "golden", "make_pin.py"))
    mp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mp)
    for name, cfg_name, nseq, scores in mp.SETS:
        fasta, paf = mp.build(name, cfg_name, nseq, scores)
        assert open(os.path.join(here, "golden", "pin", name + ".fa")).read() == fasta, name
        assert open(os.path.join(here, "golden", "pin", name + ".expected.paf")).read() == paf, name
        assert len(paf.splitlines()) == nseq * (nseq - 1)
    import json
    doc = json.load(open(os.path.join(here, "golden", "oracle_kats.json")))
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(here, "golden", "oracle_kats.tsv")) if not l.startswith("#")]
    assert len(rows) == len(doc["cases"])
    for r, c in zip(rows, doc["cases"]):
        assert r == [c["name"], ",".join(map(str, c["scores"])), c["pattern"], c["text"], str(c["penalty"]), c["cigar"]]


@pytest.mark.parametrize("family", sorted(repeats.SMALL))
@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_repeat_families_optimal_and_valid(oracle, scores, family):
    """Repeat-rich pairs (tests/repeats.py), where co-optimal alignments are many and tie-breaking decides the CIGAR: the
    penalty is the Gotoh optimum, the CIGAR is valid and re-scores to it, BiWFA and plain WFA agree on it, and the mode with
    the kernel's shortcuts (exact overlap pre-filter, known-optimum stop) gives the same bytes as the plain search."""
    rng = random.Random("%s/%s" % (family, scores))
    gen = repeats.SMALL[family]
    al, fast = oracle.Aligner(scores), oracle.Aligner(scores)
    fast.set_fast_overlap(True)
    for it in range(8):
        s, t = gen(rng)
        pen, ops = al.align(s, t)
        pen_u, ops_u = al.align_unidirectional(s, t)
        g = oracle.gotoh_penalty(s, t, scores)
        assert oracle.cigar_check(ops, s, t, scores) == (0, g), (family, it, len(s), len(t))
        assert oracle.cigar_check(ops_u, s, t, scores) == (0, g), (family, it, len(s), len(t))
        assert pen == pen_u == g, (family, it, len(s), len(t))
        assert fast.align(s, t) == (pen, ops), (family, it, len(s), len(t))


def test_repeat_families_are_tie_heavy(oracle):
    """The repeat families must keep the tie-breaking busy: two optimal alignments of a pair -- the oracle's, and the one of
    the reversed pair reversed back -- differ on a median number of DP cells at least 4x that of the random inputs the rest
    of the suite uses (random_pair, and plain 5 % pairs of 1.5 kbp, whichever is larger).  Fails if the generators turn
    bland."""
    al = oracle.Aligner(DEFAULT_2P)
    rng = random.Random(4096)
    rep = [repeats.tie_cells(al, *repeats.SMALL[f](rng)) for f in sorted(repeats.SMALL) for _ in range(10)]
    rnd = [repeats.tie_cells(al, *random_pair(rng, 1500)) for _ in range(60)]
    five = []
    for _ in range(60):
        s = rand_seq(rng, 1500)
        five.append(repeats.tie_cells(al, s, mutate(s, 0.05, rng)))
    base = max(statistics.median(rnd), statistics.median(five))
    assert base > 0
    assert statistics.median(rep) >= 4 * base, (statistics.median(rep), statistics.median(rnd), statistics.median(five))
