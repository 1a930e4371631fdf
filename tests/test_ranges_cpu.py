"""CPU tests of range alignment (awv_align_ranges, awv_score_ranges, awv_verify_ranges, host.align_ranges' PAF text,
--align-paf's parser and usage errors): what can be told without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("awv_align_ranges", "awv_align_ranges_verified", "awv_score_ranges", "awv_verify_ranges")


def test_range_abi(hip_lib):
    from allwave_amd import ffi
    assert ffi.RANGE_DTYPE.itemsize == 28
    assert ffi.RANGE_DTYPE.names == ("q_idx", "t_idx", "q_revcomp", "q_beg", "q_end", "t_beg", "t_end")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "allwave_hip.h")).read(), flags=re.S)
    assert re.search(r"\}\s*awv_range_pair\s*;", hdr)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert s in ffi.EXPORTS and getattr(hip_lib, s) is not None, s
    assert hip_lib.awv_abi_version() == 3  # additive: the ABI version stays


def test_range_calls_without_an_engine(hip_lib):
    """A null engine: AWV_ERR_ARG from the align calls (as awv_align_pairs), and from the score / verify calls
    AWV_ERR_NO_DEVICE where there is no GPU at all (as awv_score_pairs / awv_verify_cigars), else AWV_ERR_ARG."""
    import torch
    from allwave_amd import ffi
    pen = ffi.Penalties.from_scores((0, 5, 8, 2, 24, 1))
    rg = (C.c_int32 * 7)(0, 1, 0, 0, 4, 0, 4)
    out = (C.c_int32 * 16)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert hip_lib.awv_align_ranges(None, C.byref(pen), p(rg), 1, p(out), ffi.SINK_FN(), None) == ffi.AWV_ERR_ARG
    assert hip_lib.awv_align_ranges_verified(None, C.byref(pen), p(rg), 1, p(out), p(out), ffi.SINK_FN(), None) == ffi.AWV_ERR_ARG
    want = ffi.AWV_ERR_ARG if torch.cuda.is_available() else ffi.AWV_ERR_NO_DEVICE
    assert hip_lib.awv_score_ranges(None, C.byref(pen), p(rg), 1, None, p(out)) == want
    assert hip_lib.awv_verify_ranges(None, C.byref(pen), p(rg), 1, p(out), p(out), 16, p(out)) == want
    if want == ffi.AWV_ERR_NO_DEVICE:
        assert b"no CPU fallback" in hip_lib.awv_last_error()


def test_range_record_paf_text(hip_lib):
    """A range record prints the interval in columns 3-4 and 8-9 and the full lengths in columns 2 and 7."""
    import verify_cases as V
    from allwave_amd import ffi, host
    ops = b"MMMXMMDMMIM"  # 9 M/X + 1 D (query) + 1 I (target): query interval of 10 bases, target of 10
    rec = tuple(V.record_for((0, 5, 8, 2, 24, 1), ops))  # the engine's record: q_end = t_end = 10, relative to the range
    assert rec[9:] == (10, 10)
    line = host.range_record_paf("ctgA", 1000, "ctgB", 1200, (0, 1, 1, 40, 50, 700, 710), rec, ops)
    assert line == "ctgA\t1000\t40\t50\t-\tctgB\t1200\t700\t710\t8\t10\t60\tgi:f:0.888889\tcg:Z:3=1X2=1I2=1D1="
    # a failed range: its starts twice, an empty cg
    failed = (ffi.AWV_ST_CAPACITY,) + (0,) * 10
    assert host.range_record_paf("ctgA", 1000, "ctgB", 1200, (0, 1, 0, 40, 50, 700, 710), failed) == \
        "ctgA\t1000\t40\t40\t+\tctgB\t1200\t700\t700\t0\t0\t60\tgi:f:0.000000\tcg:Z:"


def test_align_paf_parser_classes(hip_lib):
    from allwave_amd import host
    txt = open(os.path.join(ROOT, "tests", "golden", "align_paf_lines.paf"), "rb").read()
    got = host.parse_paf_ranges(["ctgA", "ctgB", "ctgA"], [1000, 1200, 5], txt)
    assert got == [(1, "", (0, 1, 0, 10, 500, 20, 510)),
                   (2, "", (0, 1, 1, 0, 1000, 0, 1200)),   # columns past the ninth are not read
                   (4, "unknown_name", None),              # (line 3 is empty)
                   (5, "length_mismatch", None),
                   (6, "bad_line", None),                  # qe > qlen: not an interval of the sequence
                   (7, "bad_line", None),                  # qs > qe
                   (8, "bad_line", None),                  # strand
                   (9, "bad_line", None),                  # eight columns
                   (10, "bad_line", None),                 # not a number
                   (11, "", (1, 0, 0, 5, 5, 9, 9))]        # empty intervals are legal; CRLF


@pytest.fixture(scope="module")
def cli(hip_lib):
    from allwave_amd import build
    build.build_host()
    return build.CLI_BIN


def test_align_paf_usage_errors(cli, tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    paf = tmp_path / "m.paf"
    paf.write_text("a\t4\t0\t4\t+\tb\t4\t0\t4\n")
    for extra in (["-p", "none"], ["--wfa-orientation"], ["--wfa-orientation-full"], ["--forward-only"], ["--shard", "0/2"], ["--mash-matrix"],
                  ["--check-paf", str(paf)]):
        r = subprocess.run([cli, "-i", str(fa), "--align-paf", str(paf)] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (extra, r.returncode, r.stderr)
        assert "error:" in r.stderr and "--align-paf" in r.stderr, (extra, r.stderr)
    r = subprocess.run([cli, "-i", str(fa), "--partial"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "'--partial' requires '--check-paf'" in r.stderr
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--align-paf" in r.stdout and "--partial" in r.stdout
