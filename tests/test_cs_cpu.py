"""CPU tests of the cs difference string (csrc/cs_device.hpp): the host yardstick awv_cs_one_host against the Python restatement
(cs_cases.cs_of) and its inverse, the slice rule, the header's rule under sanitizers, and the ABI.  None of them needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cs_cases as X
from util import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return X.case_list()


@pytest.fixture(scope="module")
def alignments():
    return X.random_alignments()


def test_known_answer_and_restatement():
    k = X.KNOWN
    assert X.cs_of(k["ops"], k["pattern"], k["text"], "short") == (k["short"], X.OK)
    assert X.cs_of(k["ops"], k["pattern"], k["text"], "long") == (k["long"], X.OK)
    for mode in X.MODES:
        assert X.apply_cs(k["text"], k[mode]) == (k["pattern"], rle(k["ops"]))
    # a slice that cuts the first 'M' run and the 'D' run: an op string of its own from the skips on
    assert X.cs_of(k["ops"], k["pattern"], k["text"], "short", (4, 21, 4, 4)) == (b":2-ata:10+gt", X.OK)


@pytest.mark.parametrize("mode", X.MODES)
def test_cs_one_host_on_the_case_list(hip_lib, cases, mode):
    from allwave_amd import ffi
    codes = set()
    for name, p, t, ops, status, _ in cases:
        want = X.cs_of(ops, p, t, mode)
        text, rec = ffi.cs_one_host(mode, p, t, ops)
        assert (text, int(rec["code"]), int(rec["len"]), int(rec["off"])) == (want[0], want[1], len(want[0]), 0), name
        codes.add(want[1])
    assert codes == {X.OK, X.BAD_OP, X.LENGTHS}
    k = X.KNOWN
    assert ffi.cs_one_host(mode, k["pattern"], k["text"], k["ops"])[0] == k[mode]


def test_cs_one_host_on_random_alignments_and_back(hip_lib, alignments):
    from allwave_amd import ffi
    assert len(alignments) == 300
    for p, t, ops in alignments:
        for mode in X.MODES:
            want = X.cs_of(ops, p, t, mode)
            text, rec = ffi.cs_one_host(mode, p, t, ops)
            assert (text, int(rec["code"])) == want and want[1] == X.OK
            assert X.apply_cs(t, text) == (p, rle(ops))


def test_cs_one_host_slices(hip_lib, alignments):
    from allwave_amd import ffi
    strings = [a[2] for a in alignments]
    picks = X.random_slices(strings)
    n_cut = 0
    for i, sl in picks:
        p, t, ops = alignments[i]
        for mode in X.MODES:
            want = X.cs_of(ops, p, t, mode, sl)
            text, rec = ffi.cs_one_host(mode, p, t, ops, slice=sl)
            assert (text, int(rec["code"])) == want and want[1] == X.OK
        b, e = sl[0], sl[1]
        n_cut += 0 < b < e < len(ops) and ops[b - 1] == ops[b] and ops[e - 1] == ops[e]
    assert n_cut >= 20  # slices cut inside a run at both ends
    # skips that leave too little of a sequence; a slice outside the string and a negative skip are refused
    assert int(ffi.cs_one_host("short", b"ACGT", b"ACGT", b"MMMM", slice=(2, 4, 3, 2))[1]["code"]) == X.LENGTHS
    assert int(ffi.cs_one_host("short", b"ACGT", b"ACGT", b"MMMM", slice=(2, 2, 5, 0))[1]["code"]) == X.LENGTHS
    assert ffi.cs_one_host("long", b"ACGT", b"ACGT", b"MMMM", slice=(2, 4, 2, 2))[0] == b"=GT"
    for bad in ((3, 2, 0, 0), (0, 5, 0, 0), (0, 4, -1, 0), (0, 4, 0, -1)):
        with pytest.raises(ffi.EngineError) as err:
            ffi.cs_one_host("short", b"ACGT", b"ACGT", b"MMMM", slice=bad)
        assert err.value.code == ffi.AWV_ERR_ARG


def test_cs_one_host_measures_without_writing(hip_lib):
    from allwave_amd import ffi
    L = ffi.load()
    k = X.KNOWN
    out = np.zeros(1, dtype=ffi.CS_TEXT_DTYPE)
    args = (k["pattern"], len(k["pattern"]), k["text"], len(k["text"]), k["ops"], len(k["ops"]), None)
    for mode, want in ((ffi.AWV_CS_SHORT, k["short"]), (ffi.AWV_CS_LONG, k["long"])):
        assert L.awv_cs_one_host(mode, *args, None, 0, out.ctypes.data) == ffi.AWV_OK
        assert (int(out[0]["len"]), int(out[0]["code"])) == (len(want), X.OK)
        for cap in (len(want) - 1, 1):  # len > cap writes nothing
            buf = C.create_string_buffer(b"\xee" * 64, 64)
            assert L.awv_cs_one_host(mode, *args, buf, cap, out.ctypes.data) == ffi.AWV_OK
            assert buf.raw == b"\xee" * 64 and int(out[0]["len"]) == len(want)
        buf = C.create_string_buffer(b"\xee" * 64, 64)
        assert L.awv_cs_one_host(mode, *args, buf, len(want), out.ctypes.data) == ffi.AWV_OK
        assert buf.raw == want + b"\xee" * (64 - len(want))
    buf = C.create_string_buffer(64)
    for mode in (0, 3, -1):
        assert L.awv_cs_one_host(mode, *args, buf, 64, out.ctypes.data) == ffi.AWV_ERR_ARG
    assert L.awv_cs_one_host(1, *args, buf, 64, None) == ffi.AWV_ERR_ARG
    assert L.awv_cs_one_host(1, *args, None, 8, out.ctypes.data) == ffi.AWV_ERR_ARG
    assert L.awv_cs_one_host(1, None, 3, k["text"], 3, k["ops"], 3, None, buf, 64, out.ctypes.data) == ffi.AWV_ERR_ARG
    with pytest.raises(ValueError):
        ffi.cs_one_host("medium", b"A", b"A", b"M")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cs_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("cs") / "cs_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "cs_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_host_rule_and_slices_under_sanitizers(driver, cases, alignments):
    """cs_one, slice_ok and apply_slice of csrc/cs_device.hpp as a program of their own, on exact-size buffers: every case is what
    cs_of says, a bad slice or mode is refused, a buffer that is too small stays untouched -- and the sanitizers report nothing."""
    lines = []  # (mode, pattern, text, ops, slice, cap)
    small = [c for c in cases if len(c[3]) <= 3000][::7] + [c for c in cases if c[0].startswith(("one base", "exactly", "a stray", "N,", "an M over", "empty"))]
    for k, (_, p, t, ops, _, _) in enumerate(small):
        mode = X.MODES[k % 2]
        used_p, used_t = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        # (the shared sequences are cut to what the string needs, exactly: one base less would be AWV_CST_LENGTHS)
        pp, tt = (p[:used_p], t[:used_t]) if len(p) > 50000 else (p, t)
        n = len(X.cs_of(ops, pp, tt, mode)[0])
        lines.append((mode, pp, tt, ops, (0, len(ops), 0, 0), n))
    for k, (i, sl) in enumerate(X.random_slices([a[2] for a in alignments])):
        p, t, ops = alignments[i]
        mode = X.MODES[k % 2]
        n = len(X.cs_of(ops, p, t, mode, sl)[0])
        lines.append((mode, p, t, ops, sl, n if k % 4 else max(n - 1, 0)))  # exact-size buffers; every fourth one byte short
    refused = [("short", b"ACGT", b"ACGT", b"MMXM", (3, 2, 0, 0), 8), ("short", b"ACGT", b"ACGT", b"MMXM", (0, 5, 0, 0), 8),
               ("long", b"ACGT", b"ACGT", b"MMXM", (0, 4, -1, 0), 8), ("medium", b"ACGT", b"ACGT", b"MMXM", (0, 4, 0, 0), 8)]
    lines += refused
    lines += [("short", b"ACGT", b"ACGT", b"MM", (0, 2, 9, 0), 8), ("long", b"ACGT", b"ACGT", b"", (0, 0, 0, 5), 0)]  # a skip beyond its sequence
    hexed = lambda b: b.hex() or "-"
    text_in = "".join("%d %s %s %s %d %d %d %d %d\n" % ((dict(short=1, long=2).get(m, 7), hexed(p), hexed(t), hexed(o)) + tuple(sl) + (cap,))
                      for m, p, t, o, sl, cap in lines)
    r = subprocess.run([driver], input=text_in, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    n_short = 0
    codes = set()
    for (m, p, t, o, sl, cap), line in zip(lines, got):
        if (m, p, t, o, sl, cap) in refused:
            assert line == "0 %d 0 0 -" % X.SKIPPED, line
            continue
        want, code = X.cs_of(o, p, t, m, sl)
        fits = len(want) <= cap and len(want) > 0
        assert line == "1 %d %d %d %s" % (code, len(want), int(fits), want.hex() if fits else "-"), (line, sl, cap)
        n_short += len(want) > cap
        codes.add(code)
    assert n_short >= 30 and codes == {X.OK, X.BAD_OP, X.LENGTHS}


def test_exports_struct_sizes_and_constants(hip_lib):
    from allwave_amd import ffi
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for name in ("awv_cs_one_host", "awv_cs_cigars", "awv_cs_ranges", "awv_align_pairs_cs", "awv_align_ranges_cs", "awv_engine_cs_stats"):
        assert name in ffi.EXPORTS and getattr(hip_lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr), name
    assert ffi.CS_TEXT_DTYPE.itemsize == 16 and "} awv_cs_text; /* 16 bytes */" in hdr
    assert [ffi.CS_TEXT_DTYPE.fields[n][1] for n in ("off", "len", "code")] == [0, 8, 12]
    assert ffi.CS_SLICE_DTYPE.itemsize == 16 and "} awv_cs_slice; /* 16 bytes */" in hdr
    assert [ffi.CS_SLICE_DTYPE.fields[n][1] for n in ("col_beg", "col_end", "q_skip", "t_skip")] == [0, 4, 8, 12]
    assert C.sizeof(ffi.CsStats) == 40 and [f[0] for f in ffi.CsStats._fields_] == ["kernel_ms", "pairs", "failed", "text_bytes", "columns"]
    assert "} awv_cs_stats; /* 40 bytes */" in hdr
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_CS[A-Z_]*)\s+(\d+)", hdr)}
    assert defs == dict(AWV_CS_SHORT=1, AWV_CS_LONG=2, AWV_CST_OK=0, AWV_CST_SKIPPED=1, AWV_CST_BAD_OP=2, AWV_CST_LENGTHS=3)
    assert all(getattr(ffi, k) == v for k, v in defs.items())
    assert (X.OK, X.SKIPPED, X.BAD_OP, X.LENGTHS) == (ffi.AWV_CST_OK, ffi.AWV_CST_SKIPPED, ffi.AWV_CST_BAD_OP, ffi.AWV_CST_LENGTHS)
    assert hip_lib.awv_abi_version() == 3 and "#define AWV_ABI_VERSION 3" in hdr
    assert not any(n.endswith("_cs") and "split" in n for n in ffi.EXPORTS)  # the split has no cs form
    blob = open(ffi.LIB_PATH, "rb").read()
    assert b"awv_cs_kernel" in blob and b"awv_text_scan_kernelI11awv_cs_text" in blob  # native kernels, in the gfx950 code object
    # a null engine is refused before anything else is read: "no device" where there is none (the yardstick needs none), else a bad argument
    total = C.c_uint64(0)
    for fn in (hip_lib.awv_cs_cigars, hip_lib.awv_cs_ranges):
        assert fn(None, 1, None, 0, None, None, 0, None, None, None, 0, C.byref(total)) in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)
    assert hip_lib.awv_align_pairs_cs(None, None, None, 0, None, 0, None, None, None, None, 1, None, ffi.CS_SINK_FN(), None) == ffi.AWV_ERR_ARG
    assert hip_lib.awv_engine_cs_stats(None, None) == ffi.AWV_ERR_ARG


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


def test_host_options_are_checked_before_anything_runs(hip_lib, host_lib):
    host = host_lib
    ids, seqs = ["a", "b"], [b"ACGTACGTAC", b"ACGTTCGTAC"]
    with pytest.raises(ValueError):
        host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", cs="short", split=2, split_min_score=10)
    with pytest.raises(ValueError):
        host.align_ranges(ids, seqs, [(0, 1, 0, 0, 8, 0, 8)], "0,5,8,2,24,1", cs="long", split=2, split_min_score=10)
    for bad in ("medium", True, 3):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", cs=bad)
    assert host.last_cs() == dict(pairs=0, failed=0, text_bytes=0, columns=0, kernel_ms=0.0)


def test_cli_usage_errors_and_help(hip_lib, host_lib, tmp_path):
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n")
    paf = tmp_path / "x.paf"
    paf.write_text("")
    for extra, word in ((["--split", "2", "--split-min-score", "10"], "--split"), (["--score-only"], "--score-only"),
                        (["--check-paf", str(paf)], "--check-paf"), (["--mash-matrix"], "--mash-matrix")):
        for mode in X.MODES:
            r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--cs", mode] + extra, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and r.stdout == "" and "--cs" in r.stderr and word in r.stderr, (extra, r.stderr)
    for value in ("medium", "SHORT", "1", ""):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--cs", value], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--cs expects short or long" in r.stderr, (value, r.stderr)
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--cs"], capture_output=True, text=True, timeout=60)  # no value at all
    assert r.returncode == 2 and r.stdout == ""
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cs short|long" in r.stdout and "cs N pairs, F failed, B text bytes, K ms" in r.stdout


def test_delivered_cs_records_follow_the_kept_records(tmp_path):
    """tests/cs_delivery_driver.cpp, under the address and undefined-behaviour sanitizers: in every filtering mode of
    csrc/host/delivery.hpp each kept record comes with its entry's cs record, and a run without cs delivers none."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "cs_delivery_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cs_delivery_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert [tuple(int(v) for v in row[1:4]) for row in rows] == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)]
    kept = [int(row[5]) for row in rows]
    assert kept[0] == 200 and all(0 < k < 200 for k in kept[1:4]) and all(k > 0 for k in kept[4:])
