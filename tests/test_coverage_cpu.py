"""CPU tests of the per-base depth (csrc/coverage_device.hpp): the host yardstick awv_coverage_one_host against the Python
restatement (coverage_cases.coverage_of), all-or-nothing items, order independence, the header's rule under sanitizers, the
ABI, and the options of the host layer and the command-line tool.  None of them needs a GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import coverage_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return V.case_list()


@pytest.fixture(scope="module")
def alignments():
    return V.random_alignments()


def one_host(ffi, roles, strand, lens, span, ops, sl):
    """awv_coverage_one_host into fresh tracks: (code, counts, (qa, qm), (ta, tm))."""
    item, q, t = ffi.coverage_one_host(roles, strand == "-", lens[0], lens[1], ops, span=span, slice=sl)
    return int(item["code"]), (int(item["aligned_cols"]), int(item["matched_cols"]), int(item["boundaries"])), q, t


def test_restatement_on_a_known_answer():
    # 3M 1X 2I 1M 2D 1M over a query and a target of 10 bases, the rectangle [1, 9) x [2, 10)
    ops, span = b"MMMXIIMDDM", (1, 9, 2, 10)
    code, (qa, qm), (ta, tm) = V.coverage_of(ops, span, "+", (0, 0), V.BOTH, (10, 10))
    assert code == V.OK
    assert qa.tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 1, 0] and qm.tolist() == [0, 1, 1, 1, 0, 1, 0, 0, 1, 0]
    assert ta.tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 1, 1] and tm.tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 1, 1]
    # the same columns on the reverse strand: the pattern's base x is the query's forward base 9 - x
    code, (qa_r, qm_r), (ta_r, _) = V.coverage_of(ops, span, "-", (0, 0), V.BOTH, (10, 10))
    assert qa_r.tolist() == qa.tolist()[::-1] and qm_r.tolist() == qm.tolist()[::-1] and ta_r.tolist() == ta.tolist()
    assert V.coverage_of(ops, span, "+", (0, 0), V.TARGET, (10, 10))[1][0].sum() == 0
    assert V.coverage_of(ops, span, "+", (0, 0), V.QUERY, (10, 10))[2][0].sum() == 0
    assert V.counts_of(ops) == (6, 5, 2 * (3 + 3))
    assert V.coverage_of(ops, (1, 8, 2, 10), "+", (0, 0), V.BOTH, (10, 10))[0] == V.LENGTHS
    assert V.coverage_of(ops, (1, 9, 2, 9), "+", (0, 0), V.BOTH, (10, 10))[0] == V.LENGTHS
    assert V.coverage_of(b"MM?", span, "+", (0, 0), V.BOTH, (10, 10))[0] == V.BAD_OP


def test_paf_reading_agrees_with_the_restatement():
    # the query's forward interval [2, 8) of a '-' line is walked from base 7 down
    line = "q\t10\t2\t8\t-\tt\t9\t1\t8\t5\t8\t60\tgi:f:1\tcg:Z:2=1X1I2=2D"
    tr = V.coverage_from_paf([line], ["q", "t"], [10, 9], V.BOTH)
    want = V.Tracks([10, 9])
    # engine ops: the PAF's I consumes the query ('D' in op bytes), its D the target ('I' in op bytes)
    assert want.add(0, 1, b"MMXDMMII", "-", V.BOTH, span=(2, 8, 1, 8)) == V.OK
    assert tr.equals(want.aligned, want.matched)
    assert V.format_tracks(["q", "t"], want)[:3] == ["q\t0\t2\t0\t0", "q\t2\t4\t1\t1", "q\t4\t5\t0\t0"]


def test_coverage_one_host_on_the_case_list(hip_lib, cases):
    from allwave_amd import ffi
    codes = set()
    for roles in V.ROLES:
        for name, q, t, rev, ops, sl, status, _ in cases:
            if status != 0:
                continue
            lens = (V.SET_LENS[q], V.SET_LENS[t])
            strand = "-" if rev else "+"
            span = (0, lens[0], 0, lens[1])
            item_ops, skips = V.case_item((name, q, t, rev, ops, sl, status, 0))
            want = V.coverage_of(item_ops, span, strand, skips, roles, lens)
            code, counts, qt, tt = one_host(ffi, roles, strand, lens, span, ops, sl)
            assert code == want[0], name
            assert counts == (V.counts_of(item_ops) if code == V.OK else (0, 0, 0)), name
            for got, exp in zip(qt + tt, want[1] + want[2]):
                assert np.array_equal(got, exp), (name, roles)
            codes.add(code)
    assert codes == {V.OK, V.BAD_OP, V.LENGTHS}


def test_coverage_one_host_on_random_alignments(hip_lib, alignments):
    from allwave_amd import ffi
    assert len(alignments) == 300
    n_range = n_slice = 0
    for k, (qlen, tlen, span, strand, ops, sl) in enumerate(alignments):
        roles = V.ROLES[k % 3]
        item_ops, skips = (ops, (0, 0)) if sl is None else (ops[sl[0]:sl[1]], (sl[2], sl[3]))
        want = V.coverage_of(item_ops, span, strand, skips, roles, (qlen, tlen))
        code, counts, qt, tt = one_host(ffi, roles, strand, (qlen, tlen), span, ops, sl)
        assert code == want[0] == V.OK and counts == V.counts_of(item_ops)
        for got, exp in zip(qt + tt, want[1] + want[2]):
            assert np.array_equal(got, exp), k
        n_range += span != (0, qlen, 0, tlen)
        n_slice += sl is not None
    assert n_range >= 50 and n_slice >= 50


def test_unsound_items_leave_the_arrays_untouched(hip_lib):
    from allwave_amd import ffi
    q = (np.full(20, 7, dtype=np.uint32), np.full(20, 9, dtype=np.uint32))
    t = (np.full(20, 3, dtype=np.uint32), np.full(20, 5, dtype=np.uint32))
    for ops, sl, code in ((b"MMMM?", None, V.BAD_OP), (b"?MMMM", None, V.BAD_OP), (b"M" * 21, None, V.LENGTHS), (b"M" * 20 + b"D", None, V.LENGTHS),
                          (b"M" * 20 + b"I", None, V.LENGTHS), (b"MMMM", (0, 4, 17, 0), V.LENGTHS), (b"MMMM", (2, 2, 0, 21), V.LENGTHS),
                          (b"M" * 30 + b"?", None, V.BAD_OP)):  # (a stray byte wins over the lengths)
        for rev in (False, True):
            item, _, _ = ffi.coverage_one_host("both", rev, 20, 20, ops, slice=sl, q_tracks=q, t_tracks=t)
            assert (int(item["code"]), int(item["aligned_cols"]), int(item["matched_cols"]), int(item["boundaries"])) == (code, 0, 0, 0)
            assert [int(a.min()) for a in q + t] == [int(a.max()) for a in q + t] == [7, 9, 3, 5]
    # a slice outside the string, a negative skip, a bad mask and a bad rectangle are refused
    for kw in (dict(slice=(3, 2, 0, 0)), dict(slice=(0, 5, 0, 0)), dict(slice=(0, 4, -1, 0)), dict(slice=(0, 4, 0, -1)), dict(span=(0, 21, 0, 20)),
               dict(span=(5, 4, 0, 20)), dict(span=(0, 20, -1, 20))):
        with pytest.raises(ffi.EngineError) as err:
            ffi.coverage_one_host("both", False, 20, 20, b"MMMM", **kw)
        assert err.value.code == ffi.AWV_ERR_ARG
    for roles in (0, 4, -1):
        with pytest.raises(ffi.EngineError) as err:
            ffi.coverage_one_host(roles, False, 20, 20, b"MMMM")
        assert err.value.code == ffi.AWV_ERR_ARG
    with pytest.raises(ValueError):
        ffi.coverage_one_host("all", False, 20, 20, b"MMMM")
    # a null track is not kept: the others still are
    L = ffi.load()
    out = np.zeros(1, dtype=ffi.COV_ITEM_DTYPE)
    ta = np.zeros(20, dtype=np.uint32)
    assert L.awv_coverage_one_host(3, 0, 20, 20, 0, 20, 0, 20, b"MMXM", 4, None, None, None, ta.ctypes.data, None, out.ctypes.data) == ffi.AWV_OK
    assert ta.tolist() == [1] * 4 + [0] * 16 and int(out[0]["code"]) == V.OK
    assert L.awv_coverage_one_host(3, 0, 20, 20, 0, 20, 0, 20, b"MMXM", 4, None, None, None, None, None, None) == ffi.AWV_ERR_ARG


def test_the_sum_does_not_depend_on_the_order(hip_lib, cases):
    from allwave_amd import ffi
    sound = [c for c in cases if c[6] == 0][::3]
    want = V.expected_tracks(sound, V.BOTH)
    assert int(want.aligned.max()) >= 20  # many items share a base
    for seed in (1, 2, 3):
        order = sound[:]
        random.Random(seed).shuffle(order)
        tracks = [(np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)) for n in V.SET_LENS]
        for _, q, t, rev, ops, sl, _, _ in order:
            ffi.coverage_one_host("both", rev, V.SET_LENS[q], V.SET_LENS[t], ops, slice=sl, q_tracks=tracks[q], t_tracks=tracks[t])
        assert want.equals(np.concatenate([a for a, _ in tracks]), np.concatenate([m for _, m in tracks]))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/coverage_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("coverage") / "coverage_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "coverage_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def fnv(arrays):
    h = 1469598103934665603
    for a in arrays:
        for v in a.tolist():
            h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_host_rule_under_sanitizers(driver, cases, alignments):
    """cov_one of csrc/coverage_device.hpp with the slice rule of the cs text as a program of their own, on exact-size arrays:
    every case is what coverage_of says, a bad slice or mask is refused -- and the sanitizers report nothing."""
    lines = []  # (roles, strand, qlen, tlen, span, ops, slice)
    for k, (name, q, t, rev, ops, sl, status, _) in enumerate(cases):
        if status == 0 and len(ops) <= 1100:
            lens = (V.SET_LENS[q], V.SET_LENS[t])
            lines.append((V.ROLES[k % 3], "-" if rev else "+", lens[0], lens[1], (0, lens[0], 0, lens[1]), ops, sl or (0, len(ops), 0, 0)))
    for k, (qlen, tlen, span, strand, ops, sl) in enumerate(alignments[::3]):
        lines.append((V.ROLES[k % 3], strand, qlen, tlen, span, ops, sl or (0, len(ops), 0, 0)))  # rectangles that end on a sequence's last base
    refused = [(3, "+", 4, 4, (0, 4, 0, 4), b"MMXM", (3, 2, 0, 0)), (3, "+", 4, 4, (0, 4, 0, 4), b"MMXM", (0, 5, 0, 0)),
               (3, "-", 4, 4, (0, 4, 0, 4), b"MMXM", (0, 4, -1, 0)), (0, "+", 4, 4, (0, 4, 0, 4), b"MMXM", (0, 4, 0, 0)),
               (4, "+", 4, 4, (0, 4, 0, 4), b"MMXM", (0, 4, 0, 0))]
    lines += refused
    text_in = "".join("%d %d %d %d %d %d %d %d %s %d %d %d %d\n" % ((r, s == "-", ql, tl) + tuple(sp) + (o.hex() or "-",) + tuple(sl))
                      for r, s, ql, tl, sp, o, sl in lines)
    r = subprocess.run([driver], input=text_in, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    codes = set()
    for case, line in zip(lines, got):
        roles, strand, ql, tl, sp, o, sl = case
        if case in refused:
            assert line.split()[:5] == ["0", str(V.SKIPPED), "0", "0", "0"], line
            continue
        item_ops = o[sl[0]:sl[1]]
        code, qt, tt = V.coverage_of(item_ops, sp, strand, (sl[2], sl[3]), roles, (ql, tl))
        counts = V.counts_of(item_ops) if code == V.OK else (0, 0, 0)
        tracks = qt + tt
        assert line == "1 %d %d %d %d %d %d %d %d %d" % ((code,) + counts + tuple(int(a.sum(dtype=np.uint64)) for a in tracks) + (fnv(tracks),)), (line, sl)
        codes.add(code)
    assert codes == {V.OK, V.BAD_OP, V.LENGTHS}


def test_exports_struct_sizes_and_constants(hip_lib):
    from allwave_amd import ffi
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for name in ("awv_coverage_one_host", "awv_engine_coverage_begin", "awv_engine_coverage_read", "awv_coverage_cigars", "awv_coverage_ranges",
                 "awv_engine_coverage_stats"):
        assert name in ffi.EXPORTS and getattr(hip_lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr), name
    assert ffi.COV_ITEM_DTYPE.itemsize == 16 and "} awv_cov_item; /* 16 bytes */" in hdr
    assert [ffi.COV_ITEM_DTYPE.fields[n][1] for n in ("code", "aligned_cols", "matched_cols", "boundaries")] == [0, 4, 8, 12]
    assert [str(ffi.COV_ITEM_DTYPE.fields[n][0]) for n in ("code", "aligned_cols", "matched_cols", "boundaries")] == ["int32", "uint32", "uint32", "uint32"]
    assert C.sizeof(ffi.CovStats) == 48 and [f[0] for f in ffi.CovStats._fields_] == ["kernel_ms", "items", "failed", "columns", "boundaries", "reads"]
    assert "} awv_cov_stats; /* 48 bytes */" in hdr
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_C[OV][V_][A-Z_]*)\s+(\d+)", hdr)}
    assert defs == dict(AWV_COV_TARGET=1, AWV_COV_QUERY=2, AWV_COV_BOTH=3, AWV_CV_OK=0, AWV_CV_SKIPPED=1, AWV_CV_BAD_OP=2, AWV_CV_LENGTHS=3)
    assert all(getattr(ffi, k) == v for k, v in defs.items())
    assert (V.OK, V.SKIPPED, V.BAD_OP, V.LENGTHS) == (ffi.AWV_CV_OK, ffi.AWV_CV_SKIPPED, ffi.AWV_CV_BAD_OP, ffi.AWV_CV_LENGTHS)
    assert (V.TARGET, V.QUERY, V.BOTH) == (ffi.AWV_COV_TARGET, ffi.AWV_COV_QUERY, ffi.AWV_COV_BOTH)
    assert hip_lib.awv_abi_version() == 3 and "#define AWV_ABI_VERSION 3" in hdr
    assert "split, normalize, encode, cs, coverage) launch min(records, workgroups)" in hdr  # the grid cap covers the new kernel
    blob = open(ffi.LIB_PATH, "rb").read()
    assert b"awv_coverage_kernel" in blob and b"awv_cov_scan_kernel" in blob  # native kernels, in the gfx950 code object
    # a null engine is refused before anything else is read: "no device" where there is none (the yardstick needs none), else a bad argument
    for fn in (hip_lib.awv_coverage_cigars, hip_lib.awv_coverage_ranges):
        assert fn(None, None, 0, None, None, 0, None, None) in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)
    assert hip_lib.awv_engine_coverage_begin(None, 3, 0) in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)
    assert hip_lib.awv_engine_coverage_read(None, None, None, 0) in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)
    assert hip_lib.awv_engine_coverage_stats(None, None) == ffi.AWV_ERR_ARG
    for name, want in ((None, 0), ("target", 1), ("query", 2), ("both", 3), (2, 2)):
        assert ffi.coverage_roles(name) == want
    for bad in ("all", True, 0, 4):
        with pytest.raises(ValueError):
            ffi.coverage_roles(bad)


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


def test_host_options_are_checked_before_anything_runs(hip_lib, host_lib):
    host = host_lib
    ids, seqs = ["a", "b"], [b"ACGTACGTAC", b"ACGTTCGTAC"]
    for bad in ("all", True, 3, 0, "Target"):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", coverage=bad)
        with pytest.raises(ValueError):
            host.all_pairs_paf_count(ids, seqs, "0,5,8,2,24,1", coverage=bad)
        with pytest.raises(ValueError):
            host.iterate(ids, seqs, "0,5,8,2,24,1", coverage=bad)
        with pytest.raises(ValueError):
            host.align_ranges(ids, seqs, [(0, 1, 0, 0, 8, 0, 8)], "0,5,8,2,24,1", coverage=bad)
    with pytest.raises(ValueError):  # the other options are still checked first
        host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", coverage="both", clip_min_score=5)
    got = host.last_coverage()
    assert got["offsets"] is None and len(got["aligned"]) == len(got["matched"]) == 0
    assert {k: got[k] for k in ("items", "failed", "columns", "boundaries", "reads", "kernel_ms")} == dict(items=0, failed=0, columns=0, boundaries=0, reads=0,
                                                                                                      kernel_ms=0.0)


def test_cli_usage_errors_and_help(hip_lib, host_lib, tmp_path):
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n")
    paf = tmp_path / "x.paf"
    paf.write_text("")
    cov = tmp_path / "cov.tsv"
    for extra, word in ((["--score-only"], "--score-only"), (["--check-paf", str(paf)], "--check-paf"), (["--mash-matrix"], "--mash-matrix")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--coverage", str(cov)] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--coverage" in r.stderr and word in r.stderr, (extra, r.stderr)
    for value in ("all", "Target", "1", ""):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--coverage", str(cov), "--coverage-of", value], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--coverage-of expects target, query or both" in r.stderr, (value, r.stderr)
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--coverage-of", "query"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "'--coverage-of' requires '--coverage'" in r.stderr
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--coverage"], capture_output=True, text=True, timeout=60)  # no value at all
    assert r.returncode == 2 and r.stdout == ""
    assert not cov.exists()
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--coverage FILE" in r.stdout and "--coverage-of target|query|both" in r.stdout
    assert "coverage I items, B boundaries, K ms" in r.stdout and "--shard every process writes the depth of its own shard" in r.stdout
