"""GPU tests (-m gpu) of WFA orientation from bounded strand scores: awv_orient_pairs (Engine.orient_pairs), the per-pair
bounds of awv_score_pairs_bounded (Engine.score_pairs(max_penalty=<array>)), the host mirror (host.iterate /
host.orient_wfa, orientation_full=) and the CLI's --wfa-orientation-full.

The answer is the reference's: reverse iff not E_f <= E_r, E = #X + #I + #D of the oracle's CIGARs of both strands.  The
race (full=False) and the two full alignments per pair (full=True) must both give it; the proved penalty intervals must
hold the oracle's penalties; and the race must cost a fraction of the full method's cells (deterministic counters)."""
import random
import subprocess

import numpy as np
import pytest

import orient_cases as OC
from util import DEFAULT_2P, EDIT, mutate, rand_seq, random_pair

pytestmark = pytest.mark.gpu
NONE = OC.HI_NONE


@pytest.fixture(scope="module")
def ffi(hip_lib):
    from allwave_amd import ffi as F
    return F


@pytest.fixture(scope="module")
def host(hip_lib):
    from allwave_amd import build, host as H
    build.build_host()
    H.load()
    return H


_FACTS = {}


def facts_of(oracle, key, seqs, pairs, scores):
    """the oracle's strands of a case, once per session (the engine fixture comes in two flavours)"""
    if key not in _FACTS:
        _FACTS[key] = OC.oracle_strands(oracle, seqs, pairs, scores)
    return _FACTS[key]


def check_intervals(ffi, res, facts):
    """the proved intervals contain the oracle's penalties; hi == lo wherever a strand completed"""
    for i, ((pf, _), (pr, _)) in enumerate(facts):
        r = res[i]
        for lo, hi, p in ((int(r["lo_f"]), int(r["hi_f"]), pf), (int(r["lo_r"]), int(r["hi_r"]), pr)):
            assert 0 <= lo <= p <= hi, (i, lo, hi, p)
            if hi != NONE:
                assert lo == hi == p, (i, lo, hi, p)


def orient_both(ffi, engine, oracle, key, seqs, pairs, scores):
    """race and full method against each other and the oracle; returns (race, full, facts)"""
    facts, want = facts_of(oracle, key, seqs, pairs, scores)
    engine.set_sequences(seqs)
    race = engine.orient_pairs(scores, pairs)
    full = engine.orient_pairs(scores, pairs, full=True)
    print("orient %s: %d pairs, BY_BOUND %d, rounds %s" % (key, len(pairs), int((race["how"] == ffi.AWV_ORIENT_BY_BOUND).sum()),
                                                          np.bincount(race["rounds"]).tolist()))
    assert race["is_reverse"].tolist() == want, key
    assert full["is_reverse"].tolist() == want, key
    check_intervals(ffi, race, facts)
    check_intervals(ffi, full, facts)
    assert (full["how"] == ffi.AWV_ORIENT_BY_EDITS).all() and (full["rounds"] == 0).all()
    for i, ((pf, ef), (pr, er)) in enumerate(facts):  # the full method's edit counts are the oracle's
        assert (int(full["edits_f"][i]), int(full["edits_r"][i])) == (ef, er), (key, i)
        assert (int(full["lo_f"][i]), int(full["hi_f"][i]), int(full["lo_r"][i]), int(full["hi_r"][i])) == (pf, pf, pr, pr)
        if race["how"][i] == ffi.AWV_ORIENT_BY_EDITS:
            assert (int(race["edits_f"][i]), int(race["edits_r"][i])) == (ef, er), (key, i)
        else:
            assert int(race["edits_f"][i]) == int(race["edits_r"][i]) == ffi.AWV_ORIENT_NO_EDITS
    return race, full, facts


def read_case(seed, divergences, n=6, length=2000, unrelated=0):
    rng = random.Random(seed)
    seqs, pairs = [], []
    for d in divergences:
        k = len(seqs)
        seqs += OC.reads(rng, n, length, d)
        pairs += OC.all_pairs(k, k + n)
    for _ in range(unrelated):
        seqs += [rand_seq(rng, length), rand_seq(rng, length)]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    return seqs, pairs


def test_reads_5_and_20_percent_all_by_bound(ffi, engine, oracle):
    """(a) 2 kbp reads at 5 % and 20 %, half reverse-complemented, 0,1,1,1: the rule settles every pair"""
    seqs, pairs = read_case("orient/a", (0.05, 0.20))
    race, _, _ = orient_both(ffi, engine, oracle, "a", seqs, pairs, EDIT)
    assert (race["how"] == ffi.AWV_ORIENT_BY_BOUND).all(), np.flatnonzero(race["how"] != ffi.AWV_ORIENT_BY_BOUND).tolist()
    assert 0 < race["is_reverse"].sum() < len(pairs)
    assert (race["rounds"] >= 1).all()


def test_reads_30_percent_and_unrelated(ffi, engine, oracle):
    """(b) the same reads at 30 % plus unrelated pairs: some pairs need the two full alignments, all answers equal"""
    seqs, pairs = read_case("orient/b", (0.30,), unrelated=6)
    race, _, _ = orient_both(ffi, engine, oracle, "b", seqs, pairs, EDIT)
    assert (race["how"] == ffi.AWV_ORIENT_BY_EDITS).sum() >= 1


def test_two_piece_orientation_penalties(ffi, engine, oracle):
    """(c) orientation penalties 0,5,8,2,24,1 (cmax = 10 cmin): the race is skipped or leaves every pair to the edit counts"""
    seqs, pairs = read_case("orient/c", (0.05, 0.30), n=4, length=1200, unrelated=2)
    race, _, _ = orient_both(ffi, engine, oracle, "c", seqs, pairs, DEFAULT_2P)
    assert (race["how"] == ffi.AWV_ORIENT_BY_EDITS).all()


def test_other_penalties(ffi, engine, oracle):
    """0,2,2,2 (an exact rule), 0,3,4,1 and 0,4,6,2 (wide intervals): whatever the rule settles, the answers are the reference's"""
    seqs, pairs = read_case("orient/p", (0.03, 0.15), n=4, length=900, unrelated=2)
    for scores in ((0, 2, 2, 2), (0, 3, 4, 1), (0, 4, 6, 2)):
        orient_both(ffi, engine, oracle, "p%s" % (scores,), seqs, pairs, scores)


def test_very_unequal_lengths(ffi, engine, oracle):
    """(d) 1 kbp against 20 kbp, both orders, both strands, on both flavours of the engine fixture"""
    rng = random.Random("orient/d")
    big = rand_seq(rng, 20000)
    small = [mutate(big[5000:6000], 0.05, rng), OC.rc(mutate(big[12000:13000], 0.05, rng)), rand_seq(rng, 1000)]
    seqs = [big] + small
    pairs = [(i, 0) for i in (1, 2, 3)] + [(0, i) for i in (1, 2, 3)]
    orient_both(ffi, engine, oracle, "d", seqs, pairs, EDIT)


def test_degenerate_pairs(ffi, engine, oracle):
    """empty and one-base sides, identical and palindromic inputs (ties go forward)"""
    rng = random.Random("orient/z")
    s = rand_seq(rng, 300)
    seqs = [b"", b"A", s, s, b"ACGT" * 50, b"ACGT" * 50, OC.rc(s), rand_seq(rng, 40)]
    pairs = [(0, 2), (2, 0), (1, 2), (2, 1), (2, 3), (4, 5), (6, 2), (2, 6), (7, 2), (0, 1), (1, 1), (0, 0)]
    race, _, _ = orient_both(ffi, engine, oracle, "z", seqs, pairs, EDIT)
    assert race["is_reverse"][4] == 0 and race["is_reverse"][5] == 0
    assert race["is_reverse"][6] == 1 and race["is_reverse"][7] == 1


def test_several_launches_per_round(ffi, oracle):
    """(e) max_batch_pairs = 16: every round of the race and the full-alignment tail take several launches"""
    seqs, pairs = read_case("orient/e", (0.04, 0.18, 0.32), n=6, length=600, unrelated=6)
    e = ffi.Engine(device=0, max_batch_pairs=16, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        race, _, _ = orient_both(ffi, e, oracle, "e", seqs, pairs, EDIT)
        e.orient_pairs(EDIT, pairs)
        st = e.stats()
        # round 0 alone: both strands of every pair, 16 entries per launch; the 18 % and 32 % reads cannot complete under its
        # bound (2 * (600 / 32) + 16 = 52), so more rounds follow
        assert st.launches > 2 * len(pairs) // 16
        assert (race["rounds"] >= 2).any()
        assert (race["how"] == ffi.AWV_ORIENT_BY_BOUND).any()
    finally:
        e.close()


def test_score_pairs_per_pair_bounds(ffi, engine, oracle):
    """bounds of P - 1, P, P + 1 and none mixed in one call: COMPLETED with the oracle's penalty when that is <= the pair's own
    bound, ABOVE_BOUND with bound + 1 otherwise"""
    rng = random.Random("orient/bounds")
    ab = [random_pair(rng, maxlen=1200) for _ in range(36)]
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs.append((len(seqs) - 2, len(seqs) - 1, len(pairs) % 2))
    for scores in (EDIT, DEFAULT_2P):
        al = oracle.Aligner(scores)
        P = [al.align(OC.rc(seqs[q]) if r else seqs[q], seqs[t])[0] for q, t, r in pairs]
        bounds = [(p - 1, p, p + 1, -1)[i % 4] for i, p in enumerate(P)]
        engine.set_sequences(seqs)
        got = engine.score_pairs(scores, pairs, max_penalty=np.asarray(bounds, dtype=np.int32))
        for i, (p, b) in enumerate(zip(P, bounds)):
            if b < 0 or p <= b:
                assert (int(got["status"][i]), int(got["penalty"][i])) == (ffi.AWV_ST_COMPLETED, p), (scores, i, p, b)
            else:
                assert (int(got["status"][i]), int(got["penalty"][i])) == (ffi.AWV_ST_ABOVE_BOUND, b + 1), (scores, i, p, b)
        # one bound for the call is the same as that bound for every pair
        B = sorted(P)[len(P) // 2]
        one = engine.score_pairs(scores, pairs, max_penalty=B)
        many = engine.score_pairs(scores, pairs, max_penalty=[B] * len(pairs))
        assert one.tolist() == many.tolist()
    with pytest.raises(ValueError):
        engine.score_pairs(EDIT, pairs, max_penalty=[1, 2])


def host_inputs():
    rng = random.Random("orient/host")
    base = rand_seq(rng, 1500)
    seqs = []
    for i in range(9):
        s = mutate(base, 0.05, rng)
        seqs.append(OC.rc(s) if i % 3 == 1 else s)
    seqs.append(rand_seq(rng, 800))
    return ["s%d" % i for i in range(len(seqs))], seqs


def test_host_iterate_same_lines(host, oracle):
    """host.iterate(orientation="wfa") with and without orientation_full: the same lines on one slot, on two slots and on a
    shard; the strands are the reference's; host.orient_wfa gives them too"""
    ids, seqs = host_inputs()
    sc = "0,5,8,2,24,1"
    full = host.iterate(ids, seqs, sc, orientation="wfa", orientation_full=True)
    race = host.iterate(ids, seqs, sc, orientation="wfa")
    assert race == full and len(race) == len(seqs) * (len(seqs) - 1)
    strands = {(l.split("\t")[0], l.split("\t")[5]): l.split("\t")[4] for l in race}
    assert set(strands.values()) == {"+", "-"}
    pairs = [(i, j) for i in range(len(seqs)) for j in range(len(seqs)) if i != j]
    _, want = OC.oracle_strands(oracle, seqs, pairs, EDIT)  # (the orientation params default to edit distance)
    assert [strands[(ids[i], ids[j])] for i, j in pairs] == ["-" if w else "+" for w in want]
    assert host.orient_wfa(ids, seqs, pairs) == [bool(w) for w in want]
    assert host.orient_wfa(ids, seqs, pairs, full=True) == [bool(w) for w in want]
    kw = dict(devices=[0, 0], min_batch_pairs=8)
    assert sorted(host.iterate(ids, seqs, sc, orientation="wfa", **kw)) == sorted(full)
    assert sorted(host.iterate(ids, seqs, sc, orientation="wfa", orientation_full=True, **kw)) == sorted(full)
    a = host.iterate(ids, seqs, sc, orientation="wfa", shard=(1, 3))
    b = host.iterate(ids, seqs, sc, orientation="wfa", orientation_full=True, shard=(1, 3))
    assert a == b and 0 < len(a) < len(full) and set(a) <= set(full)
    s1 = host.all_pairs_scores(ids, seqs, sc, orientation="wfa")
    s2 = host.all_pairs_scores(ids, seqs, sc, orientation="wfa", orientation_full=True)
    assert s1.tolist() == s2.tolist()
    assert host.all_pairs_paf(ids, seqs, sc, orientation="wfa") == host.all_pairs_paf(ids, seqs, sc, orientation="wfa", orientation_full=True)
    with pytest.raises(ValueError):
        host.iterate(ids, seqs, sc, orientation="mash", orientation_full=True)


def test_cli_wfa_orientation_full(host, tmp_path):
    """--wfa-orientation and --wfa-orientation-full write the same PAF"""
    from allwave_amd import build
    ids, seqs = host_inputs()
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    out = []
    for flag in ("--wfa-orientation", "--wfa-orientation-full"):
        o = tmp_path / (flag.strip("-") + ".paf")
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-p", "none", "--no-progress", flag, "-o", str(o)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out.append(o.read_text())
    assert out[0] == out[1] and out[0].count("\n") == len(seqs) * (len(seqs) - 1)
    assert "\t-\t" in out[0] and "\t+\t" in out[0]


def test_race_cells_at_most_a_quarter(ffi, hip_lib):
    """64 config-2-style reads (10 kbp, 5 %, every second one reverse-complemented), the first 1,024 pairs: the race's
    cell-steps are at most a quarter of the full method's (the oracle's counts put them near a twentieth), the strands equal"""
    from allwave_amd import synth
    data, offs, _ = synth.generate(64, 10000, 0.05, 2)
    seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(64)]
    seqs = [OC.rc(s) if i % 2 else s for i, s in enumerate(seqs)]
    pairs = synth.all_pairs(64)[:1024]
    e = ffi.Engine(device=0)
    try:
        e.set_sequences(seqs)
        race = e.orient_pairs(EDIT, pairs)
        sr = e.stats()
        full = e.orient_pairs(EDIT, pairs, full=True)
        sf = e.stats()
    finally:
        e.close()
    print("cells: race %d (%.1f ms, %d launches), full %d (%.1f ms, %d launches), ratio %.4f; rounds %s, BY_BOUND %d of %d" % (
        sr.cell_steps, sr.kernel_ms, sr.launches, sf.cell_steps, sf.kernel_ms, sf.launches, sr.cell_steps / max(1, sf.cell_steps),
        np.bincount(race["rounds"]).tolist(), int((race["how"] == ffi.AWV_ORIENT_BY_BOUND).sum()), len(pairs)))
    assert race["is_reverse"].tolist() == full["is_reverse"].tolist()
    assert race["is_reverse"].tolist() == [int((int(q) % 2) != (int(t) % 2)) for q, t in pairs]
    assert sf.cell_steps > 0 and sr.launches >= 2
    assert 4 * sr.cell_steps <= sf.cell_steps, (sr.cell_steps, sf.cell_steps)
