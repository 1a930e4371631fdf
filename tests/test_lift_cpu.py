"""CPU tests of the liftover (csrc/lift_device.hpp): the host yardstick awv_lift_one_host against the Python restatement
(lift_cases.lift_of) and a brute-force reading of the contract, the known answers, properties on random strings, what the case
list holds, the header's rule and the table's row order under sanitizers, and the ABI.  None of them needs a GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import cs_cases as X
import lift_cases as L
import normalize_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_EXAMPLE = b"M" * 6 + b"I" * 3 + b"M" * 10 + b"D" * 3 + b"M" * 4 + b"X" + b"M" * 3  # minimap2's cs example: 27 text and 27 pattern bases
KNOWN = (  # (from, beg, end) -> the 13 fields
    ((L.FROM_TARGET, 4, 12), (L.OK, 4, 12, 4, 4, 4, 12, 4, 9, 5, 0, 3, 0)),
    ((L.FROM_TARGET, 6, 9), L.only(L.UNALIGNED)),
    ((L.FROM_TARGET, 7, 10), (L.OK, 9, 10, 6, 9, 9, 10, 6, 7, 1, 0, 0, 0)),
    ((L.FROM_QUERY, 15, 20), (L.OK, 18, 23, 15, 18, 15, 20, 18, 20, 2, 0, 0, 3)),
)


@pytest.fixture(scope="module")
def cases():
    return L.case_list()


@pytest.fixture(scope="module")
def wanted(cases):
    return L.expected(cases)


def fields(rec):
    return tuple(int(rec[f]) for f in L.FIELDS)


def one_host(ffi, case, frm, beg, end):
    name, q, t, rev, ops, sl, status, _, _ = case
    return fields(ffi.lift_one_host(frm, rev, L.SET_LENS[q], L.SET_LENS[t], ops, beg, end, slice=sl))


def test_restatement_on_the_known_answers():
    for (frm, b, e), want in KNOWN:
        for fn in (L.lift_of, L.brute_of):
            assert fn(CS_EXAMPLE, (0, 27, 0, 27), "+", frm, b, e, 27) == want, (frm, b, e)
    # the same columns under q_revcomp: a query-side interval is turned, and so is what comes back
    assert L.lift_of(CS_EXAMPLE, (0, 27, 0, 27), "-", L.FROM_QUERY, 7, 12, 27) == (L.OK, 18, 23, 15, 18, 7, 12, 18, 20, 2, 0, 0, 3)
    assert L.lift_of(CS_EXAMPLE, (0, 27, 0, 27), "-", L.FROM_TARGET, 4, 12, 27) == (L.OK, 4, 12, 4, 4, 4, 12, 18, 23, 5, 0, 3, 0)
    assert L.lift_of(CS_EXAMPLE, (0, 27, 0, 27), "+", L.FROM_TARGET, 4, 12, 27, status=1) == L.only(L.SKIPPED)
    assert L.lift_of(CS_EXAMPLE + b"=", (0, 30, 0, 30), "+", L.FROM_TARGET, 4, 12, 30) == L.only(L.BAD_OP)
    assert L.lift_of(CS_EXAMPLE, (0, 26, 0, 27), "+", L.FROM_TARGET, 4, 12, 27) == L.only(L.LENGTHS)
    assert L.lift_of(CS_EXAMPLE, (0, 27, 0, 40), "+", L.FROM_TARGET, 27, 40, 27) == L.only(L.OUTSIDE)


def test_the_known_answers_on_the_host(hip_lib):
    from allwave_amd import ffi
    for (frm, b, e), want in KNOWN:
        assert fields(ffi.lift_one_host(L.SIDE_NAMES[frm], 0, 27, 27, CS_EXAMPLE, b, e)) == want


def test_case_list_holds_what_it_names(cases, wanted):
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for n in L.LENGTHS_NAMED:
        assert {c[7] for c in cases if c[0].startswith("runs n=%d " % n) and len(c[4]) == n} == set(L.RESIDUES)
    flat = [(c, q, w) for c, ws in zip(cases, wanted) for q, w in zip(c[8], ws)]
    assert {w[0] for _, _, w in flat} == {L.OK, L.SKIPPED, L.BAD_OP, L.LENGTHS, L.UNALIGNED, L.OUTSIDE}  # every code appears
    # a probe's answer on the last byte of a lane's 16, the first of the next lane, the last of a chunk, the first of the next
    first, last = set(), set()
    for c, _, w in flat:
        if c[0].startswith("answers on lane and chunk edges") and w[0] == L.OK:
            first.add((w[1] + c[7]) % 1024)
            last.add((w[2] - 1 + c[7]) % 1024)
    assert {15, 16, 1023, 0} <= first and {15, 16, 1023, 0} <= last
    # a source-only run across a chunk's end: a begin inside it resolves in the next chunk, an end inside it in the chunk before
    for c, ws in zip(cases, wanted):
        if " run across byte 1024" in c[0]:
            res, ops = c[7], c[4]
            assert ops[1000:1060] in (b"I" * 60, b"D" * 60) and 1000 + res < 1024 <= 1059 + res
            assert ws[0][:2] == (L.OK, 1060) and ws[1][0] == L.OK and ws[1][2] == 1000 and ws[2] == L.only(L.UNALIGNED)
    # a destination-only run at each edge of an interval is excluded, one inside it is not
    n_edges = 0
    for c, ws in zip(cases, wanted):
        if " runs at the edges" in c[0]:
            gap = b"D" if "from the target" in c[0] else b"I"
            assert ws[0][0] == L.OK and c[4][ws[0][1] - 1:ws[0][1]] == gap and c[4][ws[0][2]:ws[0][2] + 1] == gap and ws[0][11] + ws[0][12] == 0
            assert ws[2][0] == L.OK and ws[2][11] + ws[2][12] == 9
            n_edges += 1
    assert n_edges == 2
    assert any(len(c[4]) + 15 <= 1024 and len(c[8]) > 64 for c in cases)  # more than 64 queries answered inside one chunk
    assert any(len(c[4]) > 8 * 1024 and len(c[8]) <= 5 for c in cases)  # many chunks with no query
    assert any(len(set(c[8])) < len(c[8]) for c in cases)  # duplicates
    every = [c for c in cases if c[0].startswith("every 1-base interval")]
    assert len(every) == 2 and set(every[0][4]) == set(b"MXID") and all(any(q == (f, p, p + 1) for q in every[0][8]) for f in L.SIDES for p in range(13))
    # intervals that cover, overhang, touch and miss the span
    short = dict(zip(cases[names.index("a string shorter than its rectangle")][8], wanted[names.index("a string shorter than its rectangle")]))
    assert short[(1, 0, 17)][0] == L.OK and short[(1, 9, 12)][0] == L.OK and short[(1, 10, 12)][0] == L.OUTSIDE and short[(1, 12, 17)][0] == L.OUTSIDE
    behind = dict(zip(cases[names.index("a slice whose span begins behind its skips")][8], wanted[names.index("a slice whose span begins behind its skips")]))
    assert behind[(1, 0, 12)][:3] == (L.OK, 10, 12) and behind[(1, 0, 10)][0] == L.OUTSIDE and behind[(1, 20, 25)][0] == L.OUTSIDE and behind[(1, 19, 25)][0] == L.OK
    assert sum(1 for c, q, w in flat if c[3] and q[0] == L.FROM_QUERY and w[0] == L.OK) >= 50  # q_revcomp pairs lifted from the query side
    assert sum(1 for c, q, w in flat if c[5] is not None and c[5][2] > 0 and w[0] == L.OK) >= 20  # slices with skips
    assert [w[0][0] for c, w in zip(cases, wanted) if c[0] == "not completed"] == [L.SKIPPED]
    stray = cases[names.index("a stray byte behind the last query")]
    assert stray[4].index(b"?") > max(e for _, _, e in stray[8]) and all(w == L.only(L.BAD_OP) for w in wanted[names.index(stray[0])])
    assert all(w == L.only(L.LENGTHS) for n, ws in zip(names, wanted) if n.startswith("one base too long") for w in ws)
    ranges = L.range_case_list()
    assert all(r[3] > 0 and r[5] > 0 for _, r, _, _ in ranges) and {r[2] for _, r, _, _ in ranges} == {0, 1}


def test_lift_one_host_on_the_case_list(hip_lib, cases, wanted):
    from allwave_amd import ffi
    n = 0
    for case, ws in zip(cases, wanted):
        name, q, t, rev, ops, sl, status, _, queries = case
        if status != 0:
            continue
        span = (0, L.SET_LENS[q], 0, L.SET_LENS[t])
        for (frm, b, e), want in zip(queries, ws):
            assert one_host(ffi, case, frm, b, e) == want, (name, frm, b, e)
            if len(ops) <= 2200:  # (the brute force is quadratic in nothing, but the long strings have many queries)
                assert L.brute_of(ops, span, "-" if rev else "+", frm, b, e, L.SET_LENS[q], sl=sl) == want, (name, frm, b, e)
            n += 1
    assert n > 1500
    lens = L.SET_LENS
    for name, r, ops, queries in L.range_case_list():
        q, t, strand, span = L.span_of_range(r, lens)
        for frm, b, e in queries:
            want = L.lift_of(ops, span, strand, frm, b, e, lens[q])
            assert fields(ffi.lift_one_host(frm, strand == "-", lens[q], lens[t], ops, b, e, span=span)) == want == L.brute_of(ops, span, strand, frm, b, e, lens[q]), (name, frm, b, e)


def test_properties_on_random_strings(hip_lib):
    """An OK slice begins and ends on 'M' / 'X'; its counts are its bytes counted directly; its intervals are where the coverage
    yardstick puts the slice's first and last columns."""
    from allwave_amd import ffi
    rng = random.Random(534)
    n_ok = 0
    for k in range(120):
        n = rng.randint(1, 400)
        ops = N.random_ops_long(rng, n) if k % 2 else X.random_ops(rng, n)
        used_q, used_t = n - ops.count(b"I"), n - ops.count(b"D")
        pad = [rng.randint(0, 5) for _ in range(4)]
        span = (pad[0], pad[0] + used_q, pad[2], pad[2] + used_t)
        qlen, tlen, rev = span[1] + pad[1], span[3] + pad[3], k % 3 == 0
        for _ in range(8):
            frm = rng.choice(L.SIDES)
            length = tlen if frm == L.FROM_TARGET else qlen
            b = rng.randint(0, length - 1)
            e = rng.randint(b + 1, min(length, b + rng.choice([1, 3, 30, 500])))
            r = ffi.lift_one_host(frm, rev, qlen, tlen, ops, b, e, span=span)
            assert fields(r) == L.lift_of(ops, span, "-" if rev else "+", frm, b, e, qlen)
            if int(r["code"]) != L.OK:
                continue
            n_ok += 1
            cb, ce = int(r["col_beg"]), int(r["col_end"])
            core = ops[cb:ce]
            assert core[0] in b"MX" and core[-1] in b"MX"
            assert tuple(int(r[f]) for f in L.FIELDS[9:]) == tuple(core.count(c) for c in (b"M", b"X", b"I", b"D"))
            assert (int(r["q_skip"]), int(r["t_skip"])) == (cb - ops[:cb].count(b"I"), cb - ops[:cb].count(b"D"))
            # the first and the last column as 1-column slices of the coverage yardstick: one base of each sequence
            at = []
            for col in (cb, ce - 1):
                sl = (col, col + 1, col - ops[:col].count(b"I"), col - ops[:col].count(b"D"))
                item, (qa, _), (ta, _) = ffi.coverage_one_host("both", rev, qlen, tlen, ops, span=span, slice=sl)
                assert int(item["code"]) == 0 and qa.sum() == 1 and ta.sum() == 1
                at.append((int(np.flatnonzero(qa)[0]), int(np.flatnonzero(ta)[0])))
            q_iv = (min(at[0][0], at[1][0]), max(at[0][0], at[1][0]) + 1)
            t_iv = (at[0][1], at[1][1] + 1)
            src, dst = (t_iv, q_iv) if frm == L.FROM_TARGET else (q_iv, t_iv)
            assert (int(r["src_beg"]), int(r["src_end"]), int(r["dst_beg"]), int(r["dst_end"])) == src + dst
            assert b <= src[0] < src[1] <= e
    assert n_ok > 300


def test_lift_one_host_refuses(hip_lib):
    from allwave_amd import ffi
    ops = b"M" * 10
    for kw in (dict(frm=0), dict(frm=3), dict(b=5, e=5), dict(b=6, e=5), dict(b=-1), dict(e=21), dict(frm=2, e=13), dict(sl=(3, 2, 0, 0)), dict(sl=(0, 11, 0, 0)),
               dict(sl=(0, 5, -1, 0)), dict(span=(0, 13, 0, 20))):
        with pytest.raises(ffi.EngineError) as err:
            ffi.lift_one_host(kw.get("frm", 1), 0, 12, 20, ops, kw.get("b", 2), kw.get("e", 5), span=kw.get("span"), slice=kw.get("sl"))
        assert err.value.code == ffi.AWV_ERR_ARG, kw
    assert int(ffi.lift_one_host(2, 0, 12, 20, ops, 2, 12)["code"]) == L.OK and int(ffi.lift_one_host(1, 0, 12, 20, ops, 19, 20)["code"]) == L.OUTSIDE


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/lift_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("lift") / "lift_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, "-I" + build.HOST_DIR,
           os.path.join(ROOT, "tests", "lift_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_host_rule_and_row_order_under_sanitizers(driver, cases, wanted):
    """lift_one of csrc/lift_device.hpp behind the slice rule of the cs text as a program of their own, on exact-size copies of the
    op bytes; and row_less: rows in any order come out in the order Python's tuple comparison gives."""
    lines, want = [], []
    for case, ws in zip(cases, wanted):
        name, q, t, rev, ops, sl, status, _, queries = case
        if status != 0:
            continue
        cb, ce, qs, ts = sl if sl is not None else (0, len(ops), 0, 0)
        for (frm, b, e), w in list(zip(queries, ws))[:25]:
            lines.append("L %d %d %d 0 %d 0 %d %s %d %d %d %d %d %d" % (frm, rev, L.SET_LENS[q], L.SET_LENS[q], L.SET_LENS[t], ops.hex() or "-", cb, ce, qs, ts, b, e))
            want.append(" ".join(str(v) for v in w))
    rng = random.Random(535)
    rows = [tuple(rng.choice([-2, 0, 1, 2, 7, 2 ** 31 - 1]) if rng.random() < 0.7 else rng.randint(0, 3) for _ in range(12)) for _ in range(400)]
    rows += rows[:20]
    lines += ["R " + " ".join(str(v) for v in r) for r in rows]
    want += [" ".join(str(v) for v in r) for r in sorted(rows)]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want) > 1000
    for g, w, ln in zip(got, want, lines + [""] * len(rows)):
        assert g == w, ln[:200]


BED_IDS, BED_LENS = ["a", "b c", "d", "a"], [100, 50, 10, 7]
BED_TEXT = ("a\t1\t5\n#comment\n\nb c\t0\t50\tgene 1\t0\t+\na\t5\t5\nz\t1\t2\na\tx\t3\na\t2\nd\t3\t11\ntrack name=x\nd\t9\t10\t\r\n \t\n"
            "a\t99\t100\tend\na\t-1\t3\nd\t0\t99999999999999999999\nbrowser position\na\t7\t8")


def test_bed_reading_and_the_row_format(driver):
    ids, lens = BED_IDS, BED_LENS
    regions, labels, bad = L.parse_bed(BED_TEXT, ids, lens)
    assert regions == [(0, 1, 5), (1, 0, 50), (2, 9, 10), (0, 99, 100), (0, 7, 8)] and labels == [".", "gene 1", ".", "end", "."]
    assert bad == [(5, "bad_line"), (6, "unknown_name"), (7, "bad_line"), (8, "bad_line"), (9, "bad_line"), (14, "bad_line"), (15, "bad_line")]
    # the command-line tool's reader (csrc/host/bed.hpp), as a program of its own under the sanitizers
    r = subprocess.run([driver, "bed"] + ["%d:%s" % (n, i) for i, n in zip(ids, lens)], input=BED_TEXT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.splitlines() == ["G %d %d %d %s" % (g + (lb,)) for g, lb in zip(regions, labels)] + ["B %d %s" % b for b in bad]
    ids, lens = ids[:3], lens[:3]
    rows = [(1, 0, 1, 0, 3, 9, 4, 11, 5, 1, 0, 1), (2, 2, 0, L.ROW_REVCOMP | L.ROW_FROM_QUERY, 9, 10, 40, 41, 1, 0, 0, 0)]
    assert L.format_rows(rows, regions, labels, ids) == ["b c\t3\t9\tgene 1\ta\t4\t11\t+\t5\t1\t0\t1", "d\t9\t10\t.\ta\t40\t41\t-\t1\t0\t0\t0"]
    # rows_of: a region on the target and the same region on the query of the swapped pair
    items = [(0, 1, 0, CS_EXAMPLE, None, None), (1, 0, 1, CS_EXAMPLE, None, None)]
    table = L.rows_of([(1, 4, 12)], 3, items, [27, 27])
    assert table == sorted(table) and [r[:4] for r in table] == [(0, 0, 1, 0), (0, 1, 0, L.ROW_REVCOMP | L.ROW_FROM_QUERY)]
    assert table[0][4:] == (4, 12, 4, 9, 5, 0, 3, 0)


def test_abi_of_the_new_structs(hip_lib):
    from allwave_amd import ffi
    assert ffi.LIFT_QUERY_DTYPE.itemsize == 24 and ffi.LIFT_DTYPE.itemsize == 56 and ffi.REGION_DTYPE.itemsize == 12 and ffi.LIFT_ROW_DTYPE.itemsize == 48
    assert C.sizeof(ffi.LiftStats) == 80
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for text in ("} awv_lift_query; /* 24 bytes */", "} awv_lift_result; /* 56 bytes */", "} awv_region; /* 12 bytes */", "} awv_lift_row; /* 48 bytes */",
                 "} awv_lift_stats; /* 80 bytes */"):
        assert text in hdr
    assert tuple(n for n in ffi.LIFT_DTYPE.names if n != "reserved") == L.FIELDS and ffi.LIFT_ROW_DTYPE.names == L.ROW_FIELDS
    assert (ffi.AWV_LF_OK, ffi.AWV_LF_SKIPPED, ffi.AWV_LF_BAD_OP, ffi.AWV_LF_LENGTHS, ffi.AWV_LF_UNALIGNED, ffi.AWV_LF_OUTSIDE) == (L.OK, L.SKIPPED, L.BAD_OP, L.LENGTHS, L.UNALIGNED,
                                                                                                                                       L.OUTSIDE)
    # the yardstick needs no device and is no product path: nothing but the C entry point names it
    for dirpath, _, files in os.walk(os.path.join(ROOT, "allwave_amd", "csrc")):
        for f in files:
            txt = open(os.path.join(dirpath, f), errors="replace").read()
            assert f == "lift.hip" or "awv_lift_one_host(" not in txt, f


def test_cli_usage_errors_and_help(hip_lib, tmp_path):
    from allwave_amd import build
    build.build_host()
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n")
    bed = tmp_path / "r.bed"
    bed.write_text("a\t1\t5\n")
    paf = tmp_path / "x.paf"
    paf.write_text("")
    out = tmp_path / "lift.tsv"
    for extra, word in ((["--score-only"], "--score-only"), (["--check-paf", str(paf)], "--check-paf"), (["--mash-matrix"], "--mash-matrix")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--liftover", str(bed), "--liftover-out", str(out)] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--liftover" in r.stderr and word in r.stderr, (extra, r.stderr)
    for value in ("all", "Target", "1", ""):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--liftover", str(bed), "--liftover-out", str(out), "--liftover-from", value], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--liftover-from expects target, query or both" in r.stderr, (value, r.stderr)
    for args in (["--liftover", str(bed)], ["--liftover-out", str(out)]):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "'--liftover' and '--liftover-out' require each other" in r.stderr
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--liftover-from", "query"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "'--liftover-from' requires '--liftover'" in r.stderr
    assert not out.exists()
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--liftover BED" in r.stdout and "--liftover-from target|query|both" in r.stdout
    assert "lifted Q queries, R rows, U unaligned, K ms" in r.stdout and "--shard every process writes" in r.stdout
