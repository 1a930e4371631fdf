"""CPU tests of alignment verification (awv_verify_one_host, the contract of csrc/verify_device.hpp on the host): the golden
vectors verify, a seeded set of single edits of each fails with the class the oracle's CIGAR check gives and with the column
and penalty of a plain Python walk, and the new entry points are declared, exported and built for gfx950."""
import collections
import ctypes as C
import os
import random
import re

import pytest

import verify_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ffi, scores, pattern, text, ops, rec):
    r = ffi.verify_one_host(scores, pattern, text, ops, tuple(rec))
    assert r["reserved"] == 0
    return int(r["code"]), int(r["column"]), int(r["penalty"])


def test_golden_vectors_verify(hip_lib):
    from allwave_amd import ffi
    kats = V.load_kats()
    assert len(kats) >= 108  # (every vector of the file is checked)
    for name, scores, pattern, text, penalty, ops in kats:
        rec = V.record_for(scores, ops)
        assert _host(ffi, scores, pattern, text, ops, rec) == (ffi.AWV_VF_OK, -1, penalty), name


def test_single_edits_fail_as_the_oracle_says(hip_lib, oracle):
    from allwave_amd import ffi
    cases = V.edited_cases()
    applied = collections.Counter(kind for kind, *_ in cases)
    for kind in V.EDIT_KINDS:
        assert applied[kind] >= 20, (kind, applied[kind])
    seen = collections.Counter()
    for kind, vi, scores, pattern, text, ops, rec in cases:
        code, column, penalty = _host(ffi, scores, pattern, text, ops, rec)
        rc, rescored = oracle.cigar_check(ops, pattern, text, scores)
        if rc != 0:
            want = V.ORACLE_CLASS[rc]
        else:  # a valid op string: what is left is the record
            good = V.record_for(scores, ops)
            want = V.COUNTS if (rec[3] != good[3] or rec[5:] != good[5:]) else V.PENALTY if (rec[1] != rescored or rec[2] != -rec[1]) else V.OK
            assert penalty == rescored, (kind, vi)
        assert code == want, (kind, vi, code, want)
        assert (code, column, penalty) == V.walk(scores, pattern, text, ops, rec), (kind, vi)
        seen[code] += 1
    # the edits reach every failure class
    for code in (V.BAD_OP, V.OVERRUN, V.M_DIFFERS, V.X_EQUAL, V.SHORT, V.COUNTS, V.PENALTY):
        assert seen[code] > 0, code


def test_skipped_and_score_sign(hip_lib):
    from allwave_amd import ffi
    scores = (0, 5, 8, 2, 24, 1)
    rec = V.record_for(scores, b"MMMM")
    assert _host(ffi, scores, b"ACGT", b"ACGT", b"MMMM", rec) == (V.OK, -1, 0)
    assert _host(ffi, scores, b"ACGT", b"ACGT", b"MMMM", [1] + rec[1:]) == (V.SKIPPED, -1, -1)
    rec = V.record_for(scores, b"MXMM")
    rec[2] = rec[1]  # score must be -penalty
    assert _host(ffi, scores, b"ACGT", b"AGGT", b"MXMM", rec) == (V.PENALTY, -1, 5)
    # an 'I' run followed directly by a 'D' run is two runs
    ops = b"MM" + b"I" * 3 + b"D" * 2 + b"M"
    rec = V.record_for(scores, ops)
    assert rec[1] == (8 + 3 * 2) + (8 + 2 * 2)
    assert _host(ffi, scores, b"ACTTG", b"ACGGGG", ops, rec) == (V.OK, -1, rec[1])
    assert _host(ffi, scores, b"", b"", b"", V.record_for(scores, b"")) == (V.OK, -1, 0)
    with pytest.raises(ffi.EngineError):
        ffi.verify_one_host((1, 5, 8, 2), b"A", b"A", b"M", V.record_for((0, 5, 8, 2), b"M"))


def test_abi_additions(hip_lib):
    from allwave_amd import ffi
    assert ffi.VERIFY_DTYPE.itemsize == 24
    assert C.sizeof(ffi.VerifyStats) == 32
    new = {"awv_align_pairs_verified", "awv_verify_cigars", "awv_verify_one_host", "awv_engine_verify_stats"}
    assert new <= set(ffi.EXPORTS)
    for s in new:
        assert getattr(hip_lib, s) is not None, s
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    assert re.search(r"#define\s+AWV_ABI_VERSION\s+3\b", hdr) and hip_lib.awv_abi_version() == 3
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_VF_[A-Z_]+)\s+(\d+)", hdr)}
    assert len(defs) == 9
    for k, v in defs.items():
        assert getattr(ffi, k) == v, k
    assert [defs["AWV_VF_" + n] for n in ("OK", "SKIPPED", "BAD_OP", "OVERRUN", "M_DIFFERS", "X_EQUAL", "SHORT", "COUNTS", "PENALTY")] == \
        [V.OK, V.SKIPPED, V.BAD_OP, V.OVERRUN, V.M_DIFFERS, V.X_EQUAL, V.SHORT, V.COUNTS, V.PENALTY]


def test_code_object_has_the_verify_kernel(hip_lib):
    from allwave_amd import ffi
    assert b"awv_verify_kernel" in open(ffi.LIB_PATH, "rb").read()


def test_cg_expansion_round_trips(hip_lib):
    """The PAF checker's expansion of a cg string (host.cigar_string_to_bytes) undoes host.cigar_bytes_to_string."""
    from allwave_amd import host
    for _, _, _, _, _, ops in V.load_kats():
        cg = host.cigar_bytes_to_string(ops)
        assert host.cigar_string_to_bytes(cg) == ops
        assert V.expand_cg(cg) == ops  # (and the tests' own expansion agrees)
    assert host.cigar_string_to_bytes("") == b""
    assert host.cigar_string_to_bytes("2=1X1I3D") == b"MMXDIII"
    for bad in ("3", "=", "0=", "3M", "3=X", "-1=", "3=2"):
        with pytest.raises(ValueError):
            host.cigar_string_to_bytes(bad)


def test_cli_argument_errors(hip_lib, tmp_path):
    """Flag combinations that make no sense are rejected before anything is read or any device is opened."""
    import subprocess
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    for argv, word in ((["--check-optimal"], "--check-paf"),
                       (["--verify", "--score-only"], "--score-only"),
                       (["--verify", "--mash-matrix"], "--mash-matrix"),
                       (["--check-paf", str(tmp_path / "x.paf"), "--verify"], "--check-paf")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (argv, r.returncode, r.stderr)
        assert "error:" in r.stderr and word in r.stderr, (argv, r.stderr)
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--verify" in r.stdout and "--check-paf" in r.stdout and "--check-optimal" in r.stdout


def test_failed_checks_reach_the_caller(hip_lib):
    """A correct engine gives the host layer no failure to report, so the path one takes is driven with made-up verify
    results: two slots' engine calls finishing out of order over a range that starts at pair-list index 100.  Every failure
    keeps its pair-list index, pair and strand, the list comes back sorted, OK and SKIPPED entries are left out, the report
    names each failure, stops at 20 lines, and the exit status is 4 -- or 0 without a failure."""
    from allwave_amd import host
    ids = ["s%d" % i for i in range(8)]
    pairs = [(i, j) for i in range(8) for j in range(8) if i != j]  # the range's 56 pairs
    rng = random.Random(11)
    places = list(range(56))
    rng.shuffle(places)
    calls, want = [], []
    for c in range(4):  # four engine calls of 14 entries, places in no order
        call = []
        for k in sorted(places[14 * c:14 * c + 14]):
            code = rng.choice([V.OK, V.OK, V.SKIPPED, V.BAD_OP, V.M_DIFFERS, V.COUNTS, V.PENALTY])
            rev = rng.random() < 0.5
            col = k * 3 if code in (V.BAD_OP, V.M_DIFFERS) else -1
            pen = -1 if col >= 0 else 1000 + k
            call.append((k, rev, code, col, pen))
            if code not in (V.OK, V.SKIPPED):
                want.append(dict(index=100 + k, query_idx=pairs[k][0], target_idx=pairs[k][1], is_reverse=rev, code=code, column=col, penalty=pen))
        calls.append(call)
    calls = [calls[2], calls[0], calls[3], calls[1]]
    want.sort(key=lambda f: f["index"])
    assert len(want) > 20
    status, report = host.verify_failure_path(ids, pairs, 100, calls)
    assert status == 4
    lv = host.last_verify()
    assert lv["pairs"] == 56 and lv["failed"] == len(want)
    got = [{k: f[k] for k in want[0]} for f in lv["failures"]]
    assert got == want
    assert [f["class"] for f in lv["failures"]] == [host.VERIFY_CODES[f["code"]] for f in want]
    lines = report.splitlines()
    assert len(lines) == 21 and lines[-1] == "verify: ... and %d more" % (len(want) - 20)
    for ln, f in zip(lines[:20], want):
        assert ln == "verify: pair %d s%d s%d %s %s column %d penalty %d" % (f["index"], f["query_idx"], f["target_idx"], "-" if f["is_reverse"] else "+",
                                                                         host.VERIFY_CODES[f["code"]], f["column"], f["penalty"])
    status, report = host.verify_failure_path(ids, pairs, 0, [[(0, False, V.OK, -1, 7), (5, True, V.SKIPPED, -1, -1)]])
    assert (status, report) == (0, "") and host.last_verify()["failures"] == [] and host.last_verify()["pairs"] == 2


def test_nothing_verifies_on_the_host_instead(hip_lib):
    """The host function is a yardstick, not a fallback: whatever asks for a check opens an engine.  Without a device each of
    them fails (AWV_ERR_NO_DEVICE underneath) rather than fall back; with one they run on it."""
    from allwave_amd import ffi, host
    ids, seqs, scores = ["a", "b"], [b"ACGTACGT", b"ACGAACGT"], "0,5,8,2,24,1"
    line = "a\t8\t0\t8\t+\tb\t8\t0\t8\t7\t8\t60\tgi:f:0.875000\tcg:Z:3=1X4="
    try:
        e = ffi.Engine(flags=ffi.AWV_F_NO_ARENA_PROBE)
    except ffi.EngineError as err:
        assert err.code == ffi.AWV_ERR_NO_DEVICE
        with pytest.raises(host.HostError):
            host.check_paf(ids, seqs, line, scores)
        with pytest.raises(host.HostError):
            host.all_pairs_paf(ids, seqs, scores, verify=True)
    else:
        e.close()
        assert host.check_paf(ids, seqs, line, scores)["failures"] == []
        assert len(host.all_pairs_paf(ids, seqs, scores, verify=True)) == 2 and host.last_verify()["pairs"] == 2
    # what needs no sequence is told on the host either way: no device is opened for a PAF whose lines all fail there
    r = host.check_paf(ids, seqs, line.replace("a\t8", "zz\t8") + "\nshort line\n", scores)
    assert [(f["line"], f["class"]) for f in r["failures"]] == [(1, "unknown_name"), (2, "bad_line")] and r["checked"] == 0
