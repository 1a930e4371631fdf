"""GPU tests of range alignment (awv_align_ranges / awv_score_ranges / awv_verify_ranges, host.align_ranges, --align-paf,
--check-paf --partial): interval pairs of resident sequences aligned globally, without cutting substrings on the host.

The yardstick is the CPU oracle on the extracted substrings -- pattern = reverse_complement(q[qb:qe]) when reversed --
with penalties and op bytes byte-identical.  Engine.align_pairs on a sequence set made of the same substrings is compared
field by field as well: parity between two paths of this build, not the yardstick."""
import os
import random
import subprocess

import numpy as np
import pytest

from util import DEFAULT_2P, EDIT, mutate, rand_seq, rle

pytestmark = pytest.mark.gpu

_RC = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def rc(s):
    return bytes(c if c in b"ACGT" else ord("N") for c in bytes(s).translate(_RC)[::-1])


def substrings(seqs, r):
    q, t, rev, qb, qe, tb, te = r
    p = seqs[q][qb:qe]
    return (rc(p) if rev else p), seqs[t][tb:te]


def check_ranges(engine, oracle, seqs, ranges, scores, parity=True, res_cigs=None):
    """Every range against the oracle on its substrings (and against align_pairs on the substrings as a set)."""
    if res_cigs is None:
        engine.set_sequences(seqs)
        res_cigs = engine.align_ranges(scores, ranges)
    res, cigs = res_cigs
    al = oracle.Aligner(scores)
    for i, r in enumerate(ranges):
        p, t = substrings(seqs, r)
        pen, ops = al.align(p, t)
        assert res["status"][i] == 0, (scores, r)
        assert res["penalty"][i] == pen and res["score"][i] == -pen, (scores, r, int(res["penalty"][i]), pen)
        assert cigs[i] == ops, (scores, r, rle(cigs[i])[:80], rle(ops)[:80])
        assert res["cigar_len"][i] == len(ops)
        c = {k: ops.count(k.encode()) for k in "MXID"}
        assert (res["num_matches"][i], res["num_mismatches"][i], res["num_ins"][i], res["num_del"][i]) == (c["M"], c["X"], c["I"], c["D"])
        assert res["q_end"][i] == len(p) and res["t_end"][i] == len(t)  # consumed lengths: relative to the range
    if parity:
        subs, pairs = [], []
        for r in ranges:
            p, t = substrings(seqs, r)
            pairs.append((len(subs), len(subs) + 1))
            subs += [p, t]
        engine.set_sequences(subs)
        res2, cigs2 = engine.align_pairs(scores, pairs)
        for name in res.dtype.names:
            if name != "cigar_off":
                assert (res[name] == res2[name]).all(), name
        assert cigs == cigs2
    return res, cigs


# ---- 1. word phases and edges ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def set2k():
    rng = random.Random(101)
    root = rand_seq(rng, 2000)
    return [mutate(root, 0.05, rng) for _ in range(4)]


@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT])
def test_word_phases_and_edges(engine, oracle, set2k, scores):
    seqs = set2k
    n = len(seqs)
    ranges = []
    for qi, ti in ((0, n - 1), (n - 1, 0), (1, 2)):  # the set's first and last sequence
        ql, tl = len(seqs[qi]), len(seqs[ti])
        for rev in (0, 1):
            for qph in (0, 1, 15):
                for tph in (0, 1, 15):
                    qb, tb = 320 + qph, 336 + tph
                    ranges.append((qi, ti, rev, qb, qb + 700 + qph, tb, tb + 690))
            ranges.append((qi, ti, rev, 0, 800, 0, 790))              # touches the start
            ranges.append((qi, ti, rev, ql - 801, ql, tl - 790, tl))  # the end
            ranges.append((qi, ti, rev, 0, ql, 0, tl))                # both
            ranges.append((qi, ti, rev, 0, 17, tl - 15, tl))
    check_ranges(engine, oracle, seqs, ranges, scores)


# ---- 2. flanks that would match -------------------------------------------------------------------------------------------
def test_flanks_that_would_match(engine, oracle):
    rng = random.Random(202)
    f1, f2, b = rand_seq(rng, 200), rand_seq(rng, 200), rand_seq(rng, 1000)
    b2 = mutate(b, 0.05, rng)
    # forward: B against B' between identical flanks; reverse: the query holds rc(F1 + B + F2), so that the pattern of the
    # reversed range is B again and what lies past either end of it matches the target's flanks
    q_f, q_r, t = f1 + b + f2, rc(f1 + b + f2), f1 + b2 + f2
    seqs = [q_f, q_r, t]
    ranges = [(0, 2, 0, 200, 1200, 200, 200 + len(b2)), (1, 2, 1, 200, 1200, 200, 200 + len(b2))]
    for scores in (DEFAULT_2P, EDIT):
        res, cigs = check_ranges(engine, oracle, seqs, ranges, scores)
        assert cigs[0] == cigs[1]  # the same pattern and text
    # the flanks do match: one base more on either side is one more 'M' there
    al = oracle.Aligner(DEFAULT_2P)
    assert al.align(q_f[199:1201], t[199:201 + len(b2)])[1].startswith(b"M")


# ---- 3. degenerate ranges -------------------------------------------------------------------------------------------------
def test_degenerate_ranges(engine, oracle):
    rng = random.Random(303)
    root = rand_seq(rng, 5000)
    seqs = [mutate(root, 0.05, rng) for _ in range(3)]
    ranges = []
    for rev in (0, 1):
        ranges += [(0, 1, rev, 70, 70, 100, 180),     # empty query range: a run of I
                   (0, 1, rev, 100, 163, 90, 90),     # empty target range: a run of D
                   (0, 2, rev, 4999, 4999, 17, 17),   # both empty
                   (0, 2, rev, 0, 0, 0, 0),
                   (1, 2, rev, 33, 34, 2000, 2001),   # one base each
                   (1, 2, rev, 1001, 1101, 1003, 1103),   # 100 x 100: the base case by length
                   (1, 2, rev, 1001, 1102, 1003, 1103),   # 101 x 100
                   (1, 2, rev, 1001, 1101, 1003, 1104),   # 100 x 101
                   (2, 0, rev, 2047, 2148, 2040, 2141)]   # 101 x 101
    for scores in (DEFAULT_2P, EDIT):
        res, cigs = check_ranges(engine, oracle, seqs, ranges, scores)
        assert cigs[0] == b"I" * 80 and cigs[1] == b"D" * 63 and cigs[2] == b"" and res["penalty"][2] == 0


# ---- 4. sequence paths ----------------------------------------------------------------------------------------------------
def test_sequence_paths(hip_lib, oracle):
    from allwave_amd import ffi
    rng = random.Random(404)
    root = rand_seq(rng, 30000)
    a, b = mutate(root, 0.02, rng), mutate(root, 0.02, rng)
    L = len(a)
    # (the second: the same interval through the reverse-complement copy of a third sequence, rc(a))
    ranges = [(0, 1, 0, 5003, 25003, 4990, 24980), (2, 1, 1, L - 25003, L - 5003, 4990, 24980)]
    a_out = a[:100] + b"N" + a[101:]       # an N outside the range: the raw-byte path, equal results
    b_in = b[:12000] + b"N" + b[12001:]    # an N inside the range
    e = ffi.Engine(device=0, flags=ffi.AWV_F_ONE_WAVE | ffi.AWV_F_NO_ARENA_PROBE)
    try:
        r0 = check_ranges(e, oracle, [a, b], ranges[:1], DEFAULT_2P, parity=False)  # unstaged: the packed words probed in place
        e.set_sequences([a_out, b])
        r1 = e.align_ranges(DEFAULT_2P, ranges[:1])
        assert r1[1] == r0[1]
        for name in r0[0].dtype.names:
            assert (r0[0][name] == r1[0][name]).all(), name
        check_ranges(e, oracle, [a, b_in], ranges[:1], DEFAULT_2P, parity=False)
        r2 = check_ranges(e, oracle, [a, b, rc(a)], ranges[1:], DEFAULT_2P, parity=False)  # the reverse-complement copy, start inside a word
        assert r2[1] == r0[1]
    finally:
        e.close()


# ---- 5. row widths --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def set40k():
    rng = random.Random(505)
    root = rand_seq(rng, 41000)
    return [mutate(root, 0.01, rng), mutate(root, 0.01, rng)]


@pytest.fixture(scope="module")
def width_cases(set40k, oracle):
    la, lb = len(set40k[0]), len(set40k[1])
    assert min(la, lb) > 40000
    ranges = [(0, 1, 0, 1001, 34001, 1003, 34003),      # 33 kbp x 33 kbp: 32-bit rows, sub16 children
              (0, 1, 0, 1001, 34001, 1003, 4003),       # 33 kbp x 3 kbp: min(h, v) rows
              (0, 1, 0, 1001, 4001, 1003, 34003),       # 3 kbp x 33 kbp
              (0, 1, 0, 1001, 1001 + 32759, 1003, 1003 + 32759),  # the last lengths with 16-bit rows
              (0, 1, 0, 1001, 1001 + 32760, 1003, 1003 + 32759),  # the first with wider ones
              (0, 1, 0, 1001, 1001 + 32759, 1003, 1003 + 32760)]
    al = oracle.Aligner(DEFAULT_2P)
    return ranges, [al.align(*substrings(set40k, r)) for r in ranges]


@pytest.mark.parametrize("case", range(6))
def test_row_widths(hip_lib, set40k, width_cases, case):
    from allwave_amd import ffi
    ranges, want = width_cases
    r, (pen, ops) = ranges[case], want[case]
    got = []
    for flags in (0, ffi.AWV_F_FORCE_INT32, ffi.AWV_F_SINGLE_STEP):  # single pairs: four waves per pair under flags 0
        e = ffi.Engine(device=0, flags=flags | ffi.AWV_F_NO_ARENA_PROBE)
        try:
            e.set_sequences(set40k)
            res, cigs = e.align_ranges(DEFAULT_2P, [r])
        finally:
            e.close()
        assert res["status"][0] == 0 and res["penalty"][0] == pen, (flags, int(res["status"][0]), int(res["penalty"][0]), pen)
        assert cigs[0] == ops, flags
        got.append((res, cigs))
    for res, cigs in got[1:]:
        for name in res.dtype.names:
            assert (res[name] == got[0][0][name]).all(), name


# ---- 6-8. mixed batch, score-only, verify ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(oracle):
    rng = random.Random(606)
    root = rand_seq(rng, 8000)
    seqs = [mutate(root, 0.04, rng) for _ in range(8)]
    ranges = []
    while len(ranges) < 296:
        q, t = rng.randrange(8), rng.randrange(8)
        n = rng.choice([0, 1, 50, 100, 101, 400, 1500, 3000, 6000])
        n = min(n, len(seqs[q]), len(seqs[t]))
        qb = rng.randrange(0, len(seqs[q]) - n + 1)
        tb = min(max(0, qb + rng.randrange(-20, 21)), len(seqs[t]))
        tn = min(max(0, n + rng.randrange(-15, 16)), len(seqs[t]) - tb, 6000)
        rev = rng.random() < 0.5
        if rev:  # rc(q[qb:qb+n]) is unrelated to the target: keep those short
            n = min(n, 400)
            tn = min(tn, 400)
        ranges.append((q, t, int(rev), qb, qb + n, tb, tb + tn))
    ranges += [ranges[7], ranges[7], (0, 1, 0, 1000, 4000, 1000, 4000), (0, 1, 0, 2000, 5000, 2000, 5000)]  # twice; overlapping
    al = oracle.Aligner(DEFAULT_2P)
    want = [al.align(*substrings(seqs, r)) for r in ranges]
    return seqs, ranges, want


@pytest.fixture(scope="module")
def mixed_run(hip_lib, mixed):
    """The mixed batch through an engine whose first attempt's rows are narrow enough to force re-runs, checked on the device."""
    from allwave_amd import ffi
    seqs, ranges, want = mixed
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, first_row_cols=2048)
    try:
        e.set_sequences(seqs)
        res, cigs, vres = e.align_ranges(DEFAULT_2P, ranges, verify=True)
        st, vst = e.stats(), e.verify_stats()
        scores = e.score_ranges(DEFAULT_2P, ranges)
        pens = np.array([w[0] for w in want], dtype=np.int32)
        lo = e.score_ranges(DEFAULT_2P, ranges, max_penalty=np.maximum(pens - 1, -1))
        hi = e.score_ranges(DEFAULT_2P, ranges, max_penalty=pens)
    finally:
        e.close()
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)  # the same call with rows as wide as the engine likes: no re-run
    try:
        e.set_sequences(seqs)
        res_w, cigs_w = e.align_ranges(DEFAULT_2P, ranges)
        launches_wide = int(e.stats().launches)
    finally:
        e.close()
    assert cigs_w == cigs and (res_w["penalty"] == res["penalty"]).all()
    return dict(res=res, cigs=cigs, vres=vres, launches=int(st.launches), launches_wide=launches_wide, pairs_completed=int(st.pairs_completed), aligned_bp=int(st.aligned_bp),
                vpairs=int(vst.pairs), vfailed=int(vst.failed), scores=scores, lo=lo, hi=hi)


def test_mixed_batch(oracle, mixed, mixed_run):
    seqs, ranges, want = mixed
    res, cigs = mixed_run["res"], mixed_run["cigs"]
    for i, (pen, ops) in enumerate(want):
        assert res["status"][i] == 0 and res["penalty"][i] == pen and cigs[i] == ops, (ranges[i], int(res["status"][i]), int(res["penalty"][i]), pen)
        assert res["q_end"][i] == ranges[i][4] - ranges[i][3] and res["t_end"][i] == ranges[i][6] - ranges[i][5]
    # rows of 2048 columns: the divergent ranges came back CAPACITY and were run again -- launches the same call does not make
    # with wide rows (the groups of a batch are launches of their own in both)
    assert mixed_run["launches"] > mixed_run["launches_wide"]
    assert mixed_run["pairs_completed"] == len(ranges)  # (a range completed on a re-run counts once; none failed)
    assert mixed_run["aligned_bp"] == sum(r[4] - r[3] for r in ranges)


def test_score_only_and_bounds(mixed, mixed_run):
    from allwave_amd import ffi
    seqs, ranges, want = mixed
    pens = np.array([w[0] for w in want])
    sc, lo, hi = mixed_run["scores"], mixed_run["lo"], mixed_run["hi"]
    assert (sc["status"] == 0).all() and (sc["penalty"] == pens).all()
    assert (hi["status"] == ffi.AWV_ST_COMPLETED).all() and (hi["penalty"] == pens).all()
    pos = pens > 0  # (a bound of penalty - 1 < 0 is no bound)
    assert (lo["status"][pos] == ffi.AWV_ST_ABOVE_BOUND).all() and (lo["penalty"][pos] == pens[pos]).all()
    assert (lo["status"][~pos] == ffi.AWV_ST_COMPLETED).all()


def test_verify_ranges(hip_lib, mixed, mixed_run):
    from allwave_amd import ffi
    seqs, ranges, want = mixed
    assert (mixed_run["vres"]["code"] == ffi.AWV_VF_OK).all()
    assert mixed_run["vpairs"] == len(ranges) and mixed_run["vfailed"] == 0
    assert (mixed_run["vres"]["penalty"] == [w[0] for w in want]).all()
    # a range shifted by one base: the record no longer fits its rectangle
    rng = random.Random(808)
    res = mixed_run["res"]
    picks = [i for i in range(len(ranges)) if len(want[i][1]) > 40][:12]
    t_ranges, recs, arena, expect = [], [], bytearray(), []
    for i in picks:
        r, ops, rec = list(ranges[i]), want[i][1], res[i].copy()
        d = 1 if r[4] < len(seqs[r[0]]) else -1
        r[3] += d
        r[4] += d
        rec["cigar_off"] = len(arena)
        arena += ops + b"\0" * (-len(ops) % 16)
        expect.append(ffi.verify_one_host(DEFAULT_2P, *substrings(seqs, r), ops, rec))
        t_ranges.append(tuple(r))
        recs.append(rec)
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        got = e.verify_ranges(DEFAULT_2P, t_ranges, np.array(recs, dtype=ffi.RESULT_DTYPE), bytes(arena))
    finally:
        e.close()
    for k, (g, w) in enumerate(zip(got, expect)):
        assert (int(g["code"]), int(g["column"]), int(g["penalty"])) == (int(w["code"]), int(w["column"]), int(w["penalty"])), (k, t_ranges[k])
    assert any(int(g["code"]) != ffi.AWV_VF_OK for g in got)


def test_verify_ranges_edited_cases(hip_lib):
    """The cases of verify_cases.py applied to ranges: every golden vector and every single edit of it (op flipped, dropped,
    duplicated, I/D swapped, a bad byte, wrong penalty, wrong count, a text base changed) sits inside longer sequences, on
    either strand, with the SAME bases following the pattern and the text -- an op string that runs past the rectangle finds
    real, matching bases there, and only the rectangle's lengths make it AWV_VF_OVERRUN.  The device check must equal
    awv_verify_one_host on the substrings field by field."""
    import collections
    import verify_cases as V
    from allwave_amd import ffi
    rng = random.Random(8080)
    by_scores = collections.defaultdict(list)
    kats = V.load_kats()
    cases = [("intact", vi, k[1], k[2], k[3], k[5], V.record_for(k[1], k[5])) for vi, k in enumerate(kats)] + V.edited_cases()
    for case in cases:
        by_scores[case[2]].append(case)
    seen = collections.Counter()
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        for scores, group in by_scores.items():
            seqs, ranges, recs, arena, expect = [], [], [], bytearray(), []
            for n, (kind, vi, _, pattern, text, ops, rec) in enumerate(group):
                left_q, left_t, right = rand_seq(rng, rng.choice([0, 1, 5, 16, 37])), rand_seq(rng, rng.choice([0, 3, 15, 16, 40])), rand_seq(rng, 48)
                q_fwd, t_seq = left_q + pattern + right, left_t + text + right
                rev = (n & 1) if all(c in b"ACGT" for c in pattern) else 0  # (reverse_complement undoes itself on ACGT only)
                qb = len(left_q)
                if rev:  # the query holds the reverse complement: the interval, on its forward strand, is mirrored
                    q_seq = rc(q_fwd)
                    qb = len(q_fwd) - len(left_q) - len(pattern)
                else:
                    q_seq = q_fwd
                ranges.append((len(seqs), len(seqs) + 1, rev, qb, qb + len(pattern), len(left_t), len(left_t) + len(text)))
                seqs += [q_seq, t_seq]
                r = np.zeros(1, dtype=ffi.RESULT_DTYPE)
                r[0] = tuple(rec)
                r["cigar_off"] = len(arena)
                arena += ops + b"\0" * (-len(ops) % 16)
                recs.append(r[0])
                expect.append(ffi.verify_one_host(scores, pattern, text, ops, r[0]))
            e.set_sequences(seqs)
            got = e.verify_ranges(scores, ranges, np.array(recs, dtype=ffi.RESULT_DTYPE), bytes(arena) + b"\0" * 16)
            for k, (g, w) in enumerate(zip(got, expect)):
                assert (int(g["code"]), int(g["column"]), int(g["penalty"])) == (int(w["code"]), int(w["column"]), int(w["penalty"])), (scores, group[k][:2], ranges[k])
                seen[int(g["code"])] += 1
    finally:
        e.close()
    for code in (V.OK, V.BAD_OP, V.OVERRUN, V.M_DIFFERS, V.X_EQUAL, V.SHORT, V.COUNTS, V.PENALTY):
        assert seen[code] > 0, code


def test_argument_errors(engine, set2k):
    from allwave_amd import ffi
    engine.set_sequences(set2k)
    n, L = len(set2k), len(set2k[0])
    for bad in ((0, 1, 0, -1, 10, 0, 10), (0, 1, 0, 11, 10, 0, 10), (0, 1, 0, 0, L + 1, 0, 10), (0, 1, 1, 0, 10, 5, len(set2k[1]) + 1),
                (n, 1, 0, 0, 10, 0, 10), (0, -1, 0, 0, 10, 0, 10)):
        for call in (lambda r: engine.align_ranges(DEFAULT_2P, [(0, 1, 0, 0, 5, 0, 5), r]), lambda r: engine.score_ranges(DEFAULT_2P, [r]),
                     lambda r: engine.verify_ranges(DEFAULT_2P, [r], np.zeros(1, dtype=ffi.RESULT_DTYPE), b"M" * 16)):
            with pytest.raises(ffi.EngineError) as ei:
                call(bad)
            assert ei.value.code == ffi.AWV_ERR_ARG
    res, cigs = engine.align_ranges(DEFAULT_2P, [])
    assert len(res) == 0 and cigs == []


# ---- 9. CLI and host ------------------------------------------------------------------------------------------------------
def test_cli_and_host(hip_lib, oracle, set2k, tmp_path):
    from allwave_amd import build, host
    build.build_host()
    seqs = set2k
    ids = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    rng = random.Random(909)
    lines, ranges = [], []
    for k in range(40):
        q, t = rng.randrange(4), rng.randrange(4)
        qb, tb = rng.randrange(0, 1000), rng.randrange(0, 1000)
        qe, te = qb + rng.randrange(0, 700), tb + rng.randrange(0, 700)
        strand = "-" if k in (5, 17) else "+"
        qname, qlen = ids[q], len(seqs[q])
        if k == 3:
            qname = "nobody"
        if k == 9:
            qe = qlen + 1
        lines.append("\t".join(str(v) for v in (qname, qlen, qb, qe, strand, ids[t], len(seqs[t]), tb, te, 0, 0, 255)))
        if k not in (3, 9):
            ranges.append((q, t, int(strand == "-"), qb, qe, tb, te))
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(lines) + "\n")
    scores = "0,5,8,2,24,1"
    want = host.align_ranges(ids, seqs, ranges, scores, verify=True)
    assert host.last_verify()["pairs"] == len(ranges) and host.last_verify()["failures"] == []
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--align-paf", str(paf_in), "-s", scores, "--verify"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == want
    err = r.stderr.splitlines()
    assert "4 unknown_name" in err and "10 bad_line" in err and "2 bad lines" in err[-1] and "verified 38 pairs, 0 failed" in err[-1]
    # the lines are the oracle's alignments of the substrings, in the interval's coordinates
    al = oracle.Aligner(DEFAULT_2P)
    for ln, g in zip(want, ranges):
        f = ln.split("\t")
        pen, ops = al.align(*substrings(seqs, g))
        assert f[:9] == [ids[g[0]], str(len(seqs[g[0]])), str(g[3]), str(g[4]), "-" if g[2] else "+", ids[g[1]], str(len(seqs[g[1]])), str(g[5]), str(g[6])]
        assert f[-1] == "cg:Z:" + rle(ops)
    out = tmp_path / "out.paf"
    out.write_text(r.stdout)
    c = subprocess.run([build.CLI_BIN, "-i", str(fa), "--check-paf", str(out), "-s", scores, "--partial", "--check-optimal"], capture_output=True, text=True,
                       timeout=120)
    assert c.returncode == 0 and c.stdout == "", (c.stdout, c.stderr)
    c = subprocess.run([build.CLI_BIN, "-i", str(fa), "--check-paf", str(out), "-s", scores], capture_output=True, text=True, timeout=120)
    proper = [k + 1 for k, g in enumerate(ranges) if not (g[3] == 0 and g[5] == 0 and g[4] == len(seqs[g[0]]) and g[6] == len(seqs[g[1]]))]
    # (an interval pair of two empty ranges at 0 prints the empty record, which the checker skips)
    proper = [k for k in proper if not (ranges[k - 1][3:] == (0, 0, 0, 0))]
    assert c.returncode == 4
    assert [(int(l.split("\t")[0]), l.split("\t")[4]) for l in c.stdout.splitlines()] == [(k, "not_end_to_end") for k in proper]
    rep = host.check_paf(ids, seqs, r.stdout, scores, optimal=True, partial=True)
    assert rep["failures"] == [] and rep["checked"] == len(ranges)
    # two engines on the device: the same lines in the same order, from the CLI and from the host call
    d = subprocess.run([build.CLI_BIN, "-i", str(fa), "--align-paf", str(paf_in), "-s", scores, "--devices", "0,0"], capture_output=True, text=True, timeout=120)
    assert d.returncode == 0 and d.stdout.splitlines() == want, d.stderr
    assert host.align_ranges(ids, seqs, ranges, scores, devices=[0, 0]) == want
    # --score-only (AllPairIterator::scores on a range list): the mapping's nine columns and the optimal penalty
    sc = subprocess.run([build.CLI_BIN, "-i", str(fa), "--align-paf", str(paf_in), "-s", scores, "--score-only"], capture_output=True, text=True, timeout=120)
    assert sc.returncode == 0, sc.stderr
    assert sc.stdout.splitlines() == ["\t".join(ln.split("\t")[:9] + [str(al.align(*substrings(seqs, g))[0])]) for ln, g in zip(want, ranges)]


def test_whole_sequence_ranges_equal_align_pairs(engine):
    from allwave_amd import synth
    data, offs, _ = synth.generate(8, 1000, 0.05, 1)  # config 1
    pairs = synth.all_pairs(8)
    engine.set_sequences((data, offs))
    lens = np.diff(offs).astype(np.int64)
    for rev in (0, 1):
        p3 = [(int(a), int(b), rev) for a, b in pairs]
        ranges = [(a, b, rev, 0, int(lens[a]), 0, int(lens[b])) for a, b, _ in p3]
        res, cigs = engine.align_pairs(EDIT, p3)
        res2, cigs2 = engine.align_ranges(EDIT, ranges)
        assert cigs == cigs2
        for name in res.dtype.names:
            assert (res[name] == res2[name]).all(), name
