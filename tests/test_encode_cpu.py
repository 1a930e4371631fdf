"""CPU tests of the run-length CIGAR text (csrc/encode_device.hpp): the host yardstick awv_encode_one_host against the Python
restatement (util.rle) and the host library's cigar_bytes_to_string, the slice rule, the header's rule under sanitizers, the
ABI, and the command-line tool's usage errors.  None of them needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import encode_cases as E
from util import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


@pytest.fixture(scope="module")
def strings():
    """The case list's strings and the 300 random ones, with the Python restatement of their texts (computed once)."""
    ops = [c[1] for c in E.case_list()] + E.random_strings()
    return ops, [rle(s).encode() for s in ops]


def test_encode_one_host_equals_rle_and_the_host_library(hip_lib, host_lib, strings):
    from allwave_amd import ffi
    ops, want = strings
    assert len(ops) >= 2300
    texts = []
    for s, w in zip(ops, want):
        text, rec = ffi.encode_one_host(s)
        assert text == w, (len(s), s[:40])
        assert (int(rec["off"]), int(rec["len"]), int(rec["runs"])) == (0, len(w), sum(1 for c in w if not 48 <= c <= 57))
        texts.append(text)
    for s, w in list(zip(ops, want))[::9]:
        assert host_lib.cigar_bytes_to_string(s).encode() == w
    # the fixed points of the contract
    assert ffi.encode_one_host(b"")[0] == b"" and ffi.encode_one_host(b"MMMXIIDDDDDDDDDDDD?")[0] == b"3=1X2D12I1?"
    assert ffi.encode_one_host(b"M" * 1000000)[0] == b"1000000=" and ffi.encode_one_host(b"MX" * 2048)[0] == b"1=1X" * 2048
    # the layout rule over the whole list: dense, in record order
    tout = np.zeros(len(ops), dtype=ffi.CIGAR_TEXT_DTYPE)
    tout["len"] = [len(t) for t in texts]
    tout["off"] = np.concatenate(([0], np.cumsum(tout["len"].astype(np.uint64))))[:-1]
    assert E.dense(tout) and E.texts_of(b"".join(texts), tout) == texts


def test_encode_one_host_measures_without_writing(hip_lib):
    from allwave_amd import ffi
    L = ffi.load()
    ops = b"MMMMXXIDDDM"
    want = rle(ops).encode()
    out = np.zeros(1, dtype=ffi.CIGAR_TEXT_DTYPE)
    assert L.awv_encode_one_host(ops, len(ops), None, 0, out.ctypes.data) == ffi.AWV_OK
    assert (int(out[0]["len"]), int(out[0]["runs"])) == (len(want), 5)
    for cap in (len(want) - 1, 1):
        buf = C.create_string_buffer(b"\xee" * 64, 64)
        assert L.awv_encode_one_host(ops, len(ops), buf, cap, out.ctypes.data) == ffi.AWV_OK
        assert buf.raw == b"\xee" * 64 and int(out[0]["len"]) == len(want)
    buf = C.create_string_buffer(b"\xee" * 64, 64)
    assert L.awv_encode_one_host(ops, len(ops), buf, len(want), out.ctypes.data) == ffi.AWV_OK
    assert buf.raw == want + b"\xee" * (64 - len(want))
    for bad in ((ops, -1, buf, 64, out.ctypes.data), (None, 3, buf, 64, out.ctypes.data), (ops, len(ops), None, 8, out.ctypes.data),
                (ops, len(ops), buf, 64, None), (ops, 2 ** 31, buf, 64, out.ctypes.data)):
        assert L.awv_encode_one_host(*bad) == ffi.AWV_ERR_ARG


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/encode_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("encode") / "encode_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "encode_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_host_rule_and_slices_under_sanitizers(driver, strings):
    """encode_one, slice_ok and apply_slice of csrc/encode_device.hpp as a program of their own: every case is what the rule
    restated here says -- the text of a slice is rle(ops[b:e]), a bad slice is refused, a record that is not completed has
    no text, a buffer that is too small stays untouched -- and the sanitizers report nothing."""
    ops, _ = strings
    short = [s for s in ops if len(s) <= 3000]
    cases = []  # (ops, status, cigar_off, col_beg, col_end, cap)
    for k, (i, b, e) in enumerate(E.random_slices(short)):
        n = len(rle(short[i][b:e]))
        cases.append((short[i], 0, (5 * k) % 23, b, e, n if k % 4 else max(n - 1, 0)))  # exact-size buffers; every fourth one byte short
    cases += [(s, 0, 3, 0, len(s), 2 * len(s)) for s in short[::17]]
    cases += [(b"MMXX", 0, 0, 3, 2, 8), (b"MMXX", 0, 0, 0, 5, 8), (b"MMXX", 0, 0, 5, 5, 8),  # refused
              (b"MMXX", 1, 0, 3, 2, 8), (b"MMXX", 4, 0, 0, 4, 8), (b"", 0, 0, 0, 0, 0), (b"MMXX", 0, 9, 4, 4, 0), (b"MMXX", 0, 9, 1, 3, 4)]
    text_in = "".join("%s %d %d %d %d %d\n" % (s.hex() or "-", st, off, b, e, cap) for s, st, off, b, e, cap in cases)
    r = subprocess.run([driver], input=text_in, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    n_short = n_cut = 0
    for (s, st, off, b, e, cap), line in zip(cases, got):
        ok = st != 0 or (b <= e <= len(s))
        if not ok:
            assert line == "0 %d %d 0 0 0 -" % (off, len(s)), (line, b, e)
            continue
        body = s[b:e] if st == 0 else b""
        want = rle(body).encode()
        runs = sum(1 for c in want if not 48 <= c <= 57)
        fits = len(want) <= cap and len(want) > 0
        where = (off + b, e - b) if st == 0 else (off, len(s))
        assert line == "1 %d %d %d %d %d %s" % (where[0], where[1], len(want), runs, int(fits), want.hex() if fits else "-"), (line, b, e, cap)
        n_short += len(want) > cap
        n_cut += st == 0 and 0 < b < e < len(s) and s[b - 1] == s[b] and s[e - 1] == s[e]
    assert n_short >= 30 and n_cut >= 20  # buffers too small, and slices that cut a run at either end


def test_exports_struct_sizes_and_constants(hip_lib):
    from allwave_amd import ffi
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for name in ("awv_encode_one_host", "awv_encode_cigars", "awv_align_pairs_encoded", "awv_align_ranges_encoded", "awv_engine_encode_stats"):
        assert name in ffi.EXPORTS and getattr(hip_lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr), name
    assert ffi.CIGAR_TEXT_DTYPE.itemsize == 16 and "} awv_cigar_text; /* 16 bytes */" in hdr
    assert [ffi.CIGAR_TEXT_DTYPE.fields[n][1] for n in ("off", "len", "runs")] == [0, 8, 12]
    assert C.sizeof(ffi.EncodeStats) == 40 and [f[0] for f in ffi.EncodeStats._fields_] == ["kernel_ms", "pairs", "runs", "text_bytes", "columns"]
    assert hip_lib.awv_abi_version() == 3 and "#define AWV_ABI_VERSION 3" in hdr
    assert not any(n.endswith("_encoded") and "split" in n for n in ffi.EXPORTS)  # the split has no encoded form
    blob = open(ffi.LIB_PATH, "rb").read()
    assert b"awv_encode_kernel" in blob and b"awv_text_scan_kernelI14awv_cigar_text" in blob  # native kernels, in the gfx950 code object
    # a null engine is refused before anything else is read: "no device" where there is none (the yardstick needs none), else a bad argument
    total = C.c_uint64(0)
    assert hip_lib.awv_encode_cigars(None, None, 0, None, 0, None, None, None, 0, C.byref(total)) in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)


def test_host_options_are_checked_before_anything_runs(hip_lib, host_lib):
    host = host_lib
    ids, seqs = ["a", "b"], [b"ACGTACGTAC", b"ACGTTCGTAC"]
    with pytest.raises(ValueError):
        host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", device_cigar=True, split=2, split_min_score=10)
    with pytest.raises(ValueError):
        host.align_ranges(ids, seqs, [(0, 1, 0, 0, 8, 0, 8)], "0,5,8,2,24,1", device_cigar=True, split=2, split_min_score=10)
    with pytest.raises(ValueError):
        host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", device_cigar=True, clip=0)
    assert host.last_encode() == dict(pairs=0, runs=0, text_bytes=0, columns=0, kernel_ms=0.0)


def test_cli_usage_errors_and_help(hip_lib, host_lib, tmp_path):
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n")
    paf = tmp_path / "x.paf"
    paf.write_text("")
    for extra, word in ((["--split", "2", "--split-min-score", "10"], "--split"), (["--score-only"], "--score-only"),
                        (["--check-paf", str(paf)], "--check-paf"), (["--mash-matrix"], "--mash-matrix")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--device-cigar"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--device-cigar" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--device-cigar" in r.stdout and "encoded N pairs, R runs, B text bytes, K ms" in r.stdout
