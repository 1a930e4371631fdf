"""GPU tests (-m gpu) of alignment verification: the verify kernel (awv_verify_cigars) against the host statement of the same
contract (awv_verify_one_host), field by field, on the CPU test's cases and on op strings built to cross lanes and chunks;
and awv_align_pairs_verified on the engine's own alignments."""
import random

import numpy as np
import pytest

import repeats
import verify_cases as V
from util import DEFAULT_2P, PENALTY_SETS, mutate, rand_seq, random_pair

pytestmark = pytest.mark.gpu

WIDE_2P = (0, 5, 8, 2, 1208, 1)  # the two pieces cross at a gap of 1200 columns (the check has no ring to fit: any o2 goes)


@pytest.fixture(scope="module")
def eng(hip_lib):
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    yield e
    e.close()


def device_vs_host(e, scores, cases, align=1, seed=0):
    """cases: [(pattern, text, ops, record[, revcomp])].  Every case becomes two sequences and one record; the op strings are
    packed `align` bytes apart (1: back to back, so they start at every offset of a 16-byte load).  Compares the kernel's
    (code, column, penalty) with the host function's, and returns the device results."""
    from allwave_amd import ffi
    seqs, pairs, recs, arena = [], [], [], bytearray(b"\xff" * (seed % 16))
    want = []
    for c in cases:
        pattern, text, ops, rec = c[:4]
        rc = len(c) > 4 and c[4]
        seqs += [V.revcomp(pattern) if rc else pattern, text]
        if rc:
            assert V.revcomp(V.revcomp(pattern)) == pattern
        pairs.append((len(seqs) - 2, len(seqs) - 1, 1 if rc else 0))
        rec = list(rec)
        while len(arena) % align:
            arena.append(0xff)
        rec[4] = len(arena)
        arena += ops
        recs.append(rec)
        h = ffi.verify_one_host(scores, pattern, text, ops, tuple(rec))
        want.append((int(h["code"]), int(h["column"]), int(h["penalty"])))
    e.set_sequences(seqs)
    got = e.verify_cigars(scores, pairs, V.as_records(recs), bytes(arena))
    for i, w in enumerate(want):
        assert (int(got["code"][i]), int(got["column"][i]), int(got["penalty"][i])) == w, (i, scores, len(cases[i][2]))
        assert got["reserved"][i] == 0
    st = e.verify_stats()
    assert st.pairs == len(cases)
    assert st.failed == sum(1 for w in want if w[0] not in (V.OK, V.SKIPPED))
    return got, want


def test_golden_vectors_and_their_edits(eng):
    """(a) The CPU test's exact case list, correct and edited."""
    by_scores = {}
    for name, scores, pattern, text, penalty, ops in V.load_kats():
        by_scores.setdefault(scores, []).append((pattern, text, ops, V.record_for(scores, ops)))
    for kind, vi, scores, pattern, text, ops, rec in V.edited_cases():
        by_scores[scores].append((pattern, text, ops, rec))
    for k, (scores, cases) in enumerate(sorted(by_scores.items())):
        got, want = device_vs_host(eng, scores, cases, seed=k)
        n_ok = sum(1 for _, s, *_ in V.load_kats() if s == scores)
        assert all(w[0] == V.OK for w in want[:n_ok])


def _gap_case(rng, scores, left, kind, length, right, tail=b""):
    ops = b"M" * left + kind * length + tail + b"M" * right
    p, t = V.build_from_ops(rng, ops)
    return p, t, ops, V.record_for(scores, ops)


def test_long_gap_runs_across_chunks(eng):
    """(a) Gap runs longer than 1,024 columns that cross chunk boundaries, at the lengths where the second piece takes over."""
    rng = random.Random("verify/gaps")
    cases = []
    for length in (1023, 1024, 1025, 1199, 1200, 1201, 2048, 2049, 5000):
        for kind in (b"I", b"D"):
            for left in (0, 1, 15, 16, 1000, 1023, 1024):
                cases.append(_gap_case(rng, WIDE_2P, left, kind, length, rng.choice((0, 1, 17, 700))))
        # an I run followed directly by a D run: two runs
        cases.append(_gap_case(rng, WIDE_2P, 37, b"I", length, 5, tail=b"D" * (length + 1)))
    for c in cases:
        assert V.rescore(WIDE_2P, c[2]) == c[3][1]
    got, want = device_vs_host(eng, WIDE_2P, cases)
    assert all(w[0] == V.OK for w in want)
    # the same strings with a wrong record penalty, and cut one gap column short
    bad = []
    for p, t, ops, rec in cases[::5]:
        r = list(rec)
        r[1] += 1
        r[2] -= 1
        bad.append((p, t, ops, r))
        i = ops.index(b"I") if b"I" in ops else ops.index(b"D")
        o2 = ops[:i] + ops[i + 1:]
        r2 = V.record_for(WIDE_2P, o2)
        bad.append((p, t, o2, r2))
    got, want = device_vs_host(eng, WIDE_2P, bad, seed=5)
    assert {w[0] for w in want} <= {V.PENALTY, V.SHORT, V.M_DIFFERS, V.OVERRUN} and V.PENALTY in {w[0] for w in want}


def test_long_and_unequal_pairs(eng):
    """(a) 40 kbp against 2 kbp, a 150 kbp pair, empty and one-base sequences."""
    rng = random.Random("verify/long")
    cases = []
    ops = b"M" * 900 + b"X" + b"M" * 99 + b"I" * 38000 + b"M" * 1000
    p, t = V.build_from_ops(rng, ops)
    assert len(p) == 2000 and len(t) == 40000
    cases.append((p, t, ops, V.record_for(DEFAULT_2P, ops)))
    cases.append((t, p, ops.replace(b"I", b"D"), V.record_for(DEFAULT_2P, ops.replace(b"I", b"D"))))
    ops = V.random_ops(rng, 150000)
    p, t = V.build_from_ops(rng, ops)
    assert min(len(p), len(t)) > 140000
    cases.append((p, t, ops, V.record_for(DEFAULT_2P, ops)))
    wrong = (0, ops.index(b"M", 149000), len(ops) - 1)
    for col in wrong:  # the same pair, one column wrong
        o = bytearray(ops)
        o[col] = ord("X") if ops[col] == ord("M") else ord("M")
        cases.append((p, t, bytes(o), V.record_for(DEFAULT_2P, ops)))
    for p, t, ops in ((b"", b"", b""), (b"A", b"", b"D"), (b"", b"A", b"I"), (b"A", b"A", b"M"), (b"A", b"C", b"X"), (b"A", b"C", b"M"),
                      (b"A", b"", b""), (b"", b"", b"M"), (b"A", b"A", b"MM"), (b"A", b"A", b"MI")):
        cases.append((p, t, ops, V.record_for(DEFAULT_2P, ops)))
    got, want = device_vs_host(eng, DEFAULT_2P, cases)
    assert [w[0] for w in want[:3]] == [V.OK] * 3
    assert [w[1] for w in want[3:6]] == list(wrong)


def test_revcomp_and_other_bytes(eng):
    """(a) Reverse-complemented queries; non-ACGT and lower-case bytes, which compare verbatim."""
    rng = random.Random("verify/bytes")
    cases = []
    for n in (1, 15, 16, 17, 1000, 3000):
        ops = V.random_ops(rng, n)
        p, t = V.build_from_ops(rng, ops)
        cases.append((p, t, ops, V.record_for(DEFAULT_2P, ops), True))
        o = bytearray(ops)
        o[rng.randrange(len(o))] = ord("D")
        cases.append((p, t, bytes(o), V.record_for(DEFAULT_2P, ops), True))
        p2, t2 = V.build_from_ops(rng, ops, alphabet=b"ACGTNacgtnRY-")
        cases.append((p2, t2, ops, V.record_for(DEFAULT_2P, ops)))
    # 'a' against 'A' is a mismatch; 'N' against 'N' a match
    cases.append((b"ACgTN", b"ACGTN", b"MMMMM", V.record_for(DEFAULT_2P, b"MMMMM")))
    cases.append((b"ACgTN", b"ACGTN", b"MMXMM", V.record_for(DEFAULT_2P, b"MMXMM")))
    cases.append((b"ACGTN", b"ACGTN", b"MMMMX", V.record_for(DEFAULT_2P, b"MMMMX")))
    # a reverse-complemented query with other bytes: the engine's copy holds 'N' there
    q = b"ACGTRYacgtnn"
    cases.append((V.revcomp(V.revcomp(q)), V.revcomp(V.revcomp(q)), b"M" * len(q), V.record_for(DEFAULT_2P, b"M" * len(q)), True))
    got, want = device_vs_host(eng, DEFAULT_2P, cases)
    assert want[-4][:2] == (V.M_DIFFERS, 2) and want[-3][0] == V.OK and want[-2][:2] == (V.X_EQUAL, 4) and want[-1][0] == V.OK


def test_failing_column_placement(eng):
    """(a) The failing column in the first lane, the last lane and the first lane of a later chunk (op strings on 16-byte
    slots, so column c sits in lane (c / 16) % 64 of chunk c / 1024), and at every lane boundary in between."""
    rng = random.Random("verify/placement")
    ops = b"M" * 4000
    p, t = V.build_from_ops(rng, ops)
    rec = V.record_for(DEFAULT_2P, ops)
    cases = []
    cols = [0, 3, 15, 16, 1008, 1023, 1024, 1030, 2047, 2048, 3999] + [16 * k - 1 for k in range(1, 64, 7)]
    for col in cols:
        for code in (V.M_DIFFERS, V.X_EQUAL, V.BAD_OP):
            tt, o = bytearray(t), bytearray(ops)
            if code == V.M_DIFFERS:
                tt[col] = ord("A") if t[col] != ord("A") else ord("C")
            elif code == V.X_EQUAL:
                o[col] = ord("X")
            else:
                o[col] = 0
            cases.append((p, bytes(tt), bytes(o), rec))
    # two failures in one string: the smaller column wins
    tt = bytearray(t)
    tt[2500] = ord("A") if t[2500] != ord("A") else ord("C")
    o = bytearray(ops)
    o[1500] = ord("X")
    cases.append((p, bytes(tt), bytes(o), rec))
    got, want = device_vs_host(eng, DEFAULT_2P, cases, align=16)
    assert [w[1] for w in want[:-1]] == [c for c in cols for _ in range(3)]
    assert want[-1][:2] == (V.X_EQUAL, 1500)


def test_records_outside_the_arena_are_an_argument_error(eng):
    from allwave_amd import ffi
    eng.set_sequences([b"ACGT", b"ACGT"])
    for off, ln in ((1, 4), (5, 0), (0, 5), (2 ** 40, 1)):
        rec = V.record_for(DEFAULT_2P, b"MMMM")
        rec[3], rec[4] = ln, off
        with pytest.raises(ffi.EngineError) as ei:
            eng.verify_cigars(DEFAULT_2P, [(0, 1)], V.as_records([rec]), b"MMMM")
        assert ei.value.code == ffi.AWV_ERR_ARG
    with pytest.raises(ffi.EngineError) as ei:
        eng.verify_cigars(DEFAULT_2P, [(0, 2)], V.as_records([V.record_for(DEFAULT_2P, b"MMMM")]), b"MMMM")
    assert ei.value.code == ffi.AWV_ERR_ARG


def _inputs():
    rng = random.Random("verify/align")
    ab = [random_pair(rng) for _ in range(48)]
    for family in sorted(repeats.SMALL):
        frng = random.Random("verify/%s" % family)
        ab += [repeats.SMALL[family](frng) for _ in range(3)]
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs.append((len(seqs) - 2, len(seqs) - 1, 0))
    pairs += [(a, b, 1) for a, b, _ in pairs[:12]]  # and some on the reverse-complement strand
    return seqs, pairs


def _check_verified(e, scores, seqs, pairs, plain):
    from allwave_amd import ffi
    res, cigs, vres = e.align_pairs(scores, pairs, verify=True)
    assert (res["status"] == 0).all()
    assert (vres["code"] == ffi.AWV_VF_OK).all(), (scores, np.nonzero(vres["code"])[0][:8], vres[vres["code"] != 0][:8])
    assert (vres["column"] == -1).all() and (vres["penalty"] == res["penalty"]).all()
    st = e.verify_stats()
    assert st.pairs == len(pairs) and st.failed == 0 and st.columns == int(res["cigar_len"].sum()) and st.kernel_ms > 0
    if plain is not None:
        pres, pcigs = plain
        for name in res.dtype.names:
            if name != "cigar_off":  # (relative to a batch's arena: the batches may differ)
                assert (res[name] == pres[name]).all(), name
        if pcigs is not None:
            assert cigs == pcigs
    return res, cigs, vres


@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_align_pairs_verified(eng, scores):
    """(b) Every pair of the engine's own alignments verifies; records and op bytes are those of a plain call."""
    seqs, pairs = _inputs()
    eng.set_sequences(seqs)
    plain = eng.align_pairs(scores, pairs)
    res, cigs, vres = _check_verified(eng, scores, seqs, pairs, plain)
    assert res.tobytes() == plain[0].tobytes()  # one batch either way: byte for byte


def test_align_pairs_verified_engine_variants(hip_lib):
    """(b) With the CIGARs kept on the device, with a first attempt narrow enough to force re-runs, and with an arena budget
    that splits the call into batches."""
    from allwave_amd import ffi
    seqs, pairs = _inputs()
    rng = random.Random(4242)
    a = rand_seq(rng, 6000)
    k = len(seqs)
    seqs += [a, mutate(a, 0.08, rng), mutate(a, 0.01, rng)]
    pairs += [(k + i, k + j, 0) for i in range(3) for j in range(3) if i != j]
    base = ffi.Engine(flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        base.set_sequences(seqs)
        plain = base.align_pairs(DEFAULT_2P, pairs)
    finally:
        base.close()
    for kw, launches in (({"flags": ffi.AWV_F_KEEP_ON_DEVICE}, 1), ({"first_row_cols": 2048}, 2), ({"max_arena_bytes": 16384}, 4)):
        kw["flags"] = kw.get("flags", 0) | ffi.AWV_F_NO_ARENA_PROBE
        e = ffi.Engine(**kw)
        try:
            e.set_sequences(seqs)
            res, cigs, vres = _check_verified(e, DEFAULT_2P, seqs, pairs, (plain[0], plain[1] if not (kw["flags"] & ffi.AWV_F_KEEP_ON_DEVICE) else None))
            assert e.stats().launches >= launches
            if kw["flags"] & ffi.AWV_F_KEEP_ON_DEVICE:
                assert all(c is None for c in cigs)
        finally:
            e.close()


def test_failed_pair_is_skipped(hip_lib):
    """(c) A pair that stays AWV_ST_CAPACITY has nothing to check."""
    from allwave_amd import ffi
    rng = random.Random(4242)
    a = rand_seq(rng, 6000)
    seqs = [a, mutate(a, 0.08, rng), mutate(a, 0.01, rng)]
    pairs = [(i, j) for i in range(3) for j in range(3) if i != j]
    e = ffi.Engine(flags=ffi.AWV_F_NO_RERUN | ffi.AWV_F_NO_ARENA_PROBE, first_row_cols=2048)
    try:
        e.set_sequences(seqs)
        res, cigs, vres = e.align_pairs(DEFAULT_2P, pairs, verify=True)
        failed = res["status"] != 0
        assert failed.any() and not failed.all()
        assert (res["status"][failed] == ffi.AWV_ST_CAPACITY).all()
        assert (vres["code"][failed] == ffi.AWV_VF_SKIPPED).all() and (vres["column"][failed] == -1).all() and (vres["penalty"][failed] == -1).all()
        assert (vres["code"][~failed] == ffi.AWV_VF_OK).all() and (vres["penalty"][~failed] == res["penalty"][~failed]).all()
        st = e.verify_stats()
        assert st.pairs == len(pairs) and st.failed == 0
    finally:
        e.close()


# ---- (d), (e): the host layer and the command-line driver ------------------------------------------------------------------
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, "tests", "golden", "pin")
PIN_SETS = (("c1", "0,1,1,1"), ("c2_8x10k", "0,5,8,2,24,1"))  # the scores tests/golden/make_pin.py used


def _reads(n=7, length=1500, seed=5):
    rng = random.Random(seed)
    a = rand_seq(rng, length)
    seqs = [mutate(a, 0.04, rng) for _ in range(n)]
    seqs[2] = V.revcomp(seqs[2])
    seqs[5] = V.revcomp(seqs[5])
    return ["s%d" % i for i in range(n)], seqs


def test_host_layer_with_verify(hip_lib):
    """(d) with_verify on one slot and on devices=[0, 0], through every consumer: no failures, the PAF of the unverified run,
    and every pair counted."""
    from allwave_amd import host
    ids, seqs = _reads()
    npairs = len(ids) * (len(ids) - 1)
    scores = "0,5,8,2,24,1"
    plain = host.all_pairs_paf(ids, seqs, scores)
    assert len(plain) == npairs
    assert host.last_verify()["pairs"] == 0  # (nothing is checked unless asked)
    for kw in (dict(), dict(devices=[0, 0], min_batch_pairs=8)):
        got = host.all_pairs_paf(ids, seqs, scores, verify=True, **kw)
        lv = host.last_verify()
        assert sorted(got) == sorted(plain), kw
        assert lv["pairs"] == npairs and lv["failed"] == 0 and lv["failures"] == [] and lv["columns"] > 0 and lv["kernel_ms"] > 0, (kw, lv)
    fwd = host.iterate(ids, seqs, scores, mode="for_each")
    for mode in ("for_each", "next", "par_for_each", "par_collect", "process_alignments"):
        for kw in (dict(), dict(devices=[0, 0], min_batch_pairs=8)):
            ref = fwd if mode != "process_alignments" else host.iterate(ids, seqs, scores, mode=mode)
            got = host.iterate(ids, seqs, scores, mode=mode, chunk=10, verify=True, **kw)
            lv = host.last_verify()
            assert sorted(got) == sorted(ref), (mode, kw)
            assert lv["pairs"] == npairs and lv["failed"] == 0 and lv["failures"] == [], (mode, kw, lv)
    nb, nl, _, st = host.all_pairs_paf_count(ids, seqs, scores, verify=True)
    assert nl == npairs and host.last_verify()["pairs"] == npairs and host.last_verify()["failed"] == 0
    nb2, nl2, _, st2 = host.all_pairs_paf_count(ids, seqs, scores)
    assert (nb2, nl2) == (nb, nl) and host.last_verify()["pairs"] == 0


def test_cli_verify_reproduces_the_pin_files(hip_lib, tmp_path):
    """(d) --verify on the pin read sets: exit status 0, the expected PAF, and the count on the summary line; it composes with
    --devices, --shard and the orientation flags."""
    from allwave_amd import build
    for name, scores in PIN_SETS:
        want = sorted(open(os.path.join(PIN, name + ".expected.paf")).read().splitlines())
        for extra in ([], ["--devices", "0,0"]):
            out = subprocess.run([build.CLI_BIN, "-i", os.path.join(PIN, name + ".fa"), "-p", "none", "-s", scores, "-t", "4", "--verify"] + extra,
                                 capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            assert sorted(out.stdout.splitlines()) == want, (name, extra)
            assert re.search(r"verified %d pairs, 0 failed, [0-9.]+ ms" % len(want), out.stderr), out.stderr
    fa = os.path.join(PIN, "c1.fa")
    lines = []
    for r in range(2):
        out = subprocess.run([build.CLI_BIN, "-i", fa, "-p", "none", "-s", "0,1,1,1", "--no-progress", "--verify", "--wfa-orientation", "--shard", "%d/2" % r],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        m = re.search(r"verified (\d+) pairs, 0 failed", out.stderr)
        assert m and int(m.group(1)) == len(out.stdout.splitlines()), out.stderr
        lines += out.stdout.splitlines()
    assert len(lines) == 56


def _fasta(path):
    seqs = {}
    for ln in open(path).read().splitlines():
        if ln.startswith(">"):
            cur = ln[1:].split()[0]
            seqs[cur] = b""
        else:
            seqs[cur] += ln.encode()
    return seqs


def test_check_paf_on_the_pin_files(hip_lib, tmp_path):
    """(e) --check-paf --check-optimal: the committed pin PAFs pass; a copy with a flipped =/X boundary, a swapped strand, a
    wrong column 10 and a valid but non-optimal CIGAR (1X -> 1I1D) fails with exactly those four lines and their classes."""
    from allwave_amd import build, ffi, host
    for name, scores in PIN_SETS:
        fa, paf = os.path.join(PIN, name + ".fa"), os.path.join(PIN, name + ".expected.paf")
        out = subprocess.run([build.CLI_BIN, "-i", fa, "--check-paf", paf, "-s", scores, "--check-optimal"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout == "", (name, out.stdout, out.stderr)
        assert "checked 56 of 56 PAF lines" in out.stderr and ", 0 failed" in out.stderr, out.stderr

        lines = open(paf).read().splitlines()
        seqs = _fasta(fa)
        want = {}
        # line 3: the first "<a>=<b>X" becomes "<a-1>=<b+1>X": an 'X' over equal bases
        f = lines[2].split("\t")
        m = re.search(r"(\d+)=(\d+)X", f[-1])
        assert m and int(m.group(1)) >= 2
        f[-1] = f[-1][:m.start()] + "%d=%dX" % (int(m.group(1)) - 1, int(m.group(2)) + 1) + f[-1][m.end():]
        lines[2] = "\t".join(f)
        want[3] = "x_equal"
        # line 10: the other strand; what that does to the first column is the host yardstick's to say
        f = lines[9].split("\t")
        f[4] = "-" if f[4] == "+" else "+"
        lines[9] = "\t".join(f)
        ops = host.cigar_string_to_bytes(f[-1][5:])
        pattern = seqs[f[0]] if f[4] == "+" else V.revcomp(seqs[f[0]])
        sc = tuple(int(x) for x in scores.split(","))
        h = ffi.verify_one_host(sc, pattern, seqs[f[5]], ops, tuple(V.record_for(sc, ops)))
        assert int(h["code"]) in (V.M_DIFFERS, V.X_EQUAL)
        want[10] = host.VERIFY_CODES[int(h["code"])]
        # line 20: column 10 (#M) off by one
        f = lines[19].split("\t")
        f[9] = str(int(f[9]) + 1)
        lines[19] = "\t".join(f)
        want[20] = "counts"
        # line 30: a valid CIGAR that costs more: the first lone mismatch as an insertion and a deletion
        f = lines[29].split("\t")
        m = re.search(r"(?<![0-9])1X", f[-1])
        assert m
        f[-1] = f[-1][:m.start()] + "1I1D" + f[-1][m.end():]
        lines[29] = "\t".join(f)
        want[30] = "not_optimal"
        bad = tmp_path / (name + ".bad.paf")
        bad.write_text("\n".join(lines) + "\n")
        out = subprocess.run([build.CLI_BIN, "-i", fa, "--check-paf", str(bad), "-s", scores, "--check-optimal"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 4, (out.returncode, out.stderr)
        rows = [r.split("\t") for r in out.stdout.splitlines()]
        assert {int(r[0]): r[4] for r in rows} == want, (name, out.stdout)
        assert len(rows) == 4 and ", 4 failed" in out.stderr
        for r in rows:
            orig = lines[int(r[0]) - 1].split("\t")
            assert r[1:4] == [orig[0], orig[5], orig[4]]
            if r[4] == "not_optimal":
                assert int(r[6]) > int(r[7]) >= 0  # penalty of the op string, then the optimum
        # the same through Python, and without --check-optimal the valid CIGAR passes
        rep = host.check_paf(list(seqs), list(seqs.values()), bad.read_text(), scores, optimal=True)
        assert {f["line"]: f["class"] for f in rep["failures"]} == want and rep["checked"] == 56 and rep["lines"] == 56
        rep = host.check_paf(list(seqs), list(seqs.values()), bad.read_text(), scores)
        assert {f["line"]: f["class"] for f in rep["failures"]} == {k: v for k, v in want.items() if v != "not_optimal"}


def test_check_paf_host_side_classes(hip_lib):
    """Lines that fail without a sequence being read, an empty record, and a good line, in one text."""
    from allwave_amd import host
    ids, seqs = ["a", "b"], [b"ACGTACGT", b"ACGAACGT"]
    good = "a\t8\t0\t8\t+\tb\t8\t0\t8\t7\t8\t60\tgi:f:0.875000\tcg:Z:3=1X4="
    text = "\n".join([
        good,
        good.replace("a\t8", "nobody\t8"),
        good.replace("b\t8\t0\t8", "b\t9\t0\t8"),
        good.replace("a\t8\t0\t8", "a\t8\t1\t8"),
        good.replace("3=1X4=", "3=1Z4="),
        "a\t8\t0\t0\t+\tb\t8\t0\t0\t0\t0\t60\tgi:f:0.000000\tcg:Z:",
        good.replace("\t7\t8\t60", "\t7\t9\t60"),
        good.replace("3=1X4=", "3=1X3="),
        "a\tb",
    ]) + "\n"
    rep = host.check_paf(ids, seqs, text, "0,5,8,2,24,1", optimal=True)
    assert [(f["line"], f["class"]) for f in rep["failures"]] == [(2, "unknown_name"), (3, "length_mismatch"), (4, "not_end_to_end"), (5, "bad_cigar"),
                                                                  (7, "counts"), (8, "short"), (9, "bad_line")]
    assert rep["lines"] == 9 and rep["skipped"] == 1 and rep["checked"] == 3
