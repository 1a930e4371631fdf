"""CPU tests of clipping to the best-scoring segment (awv_clip_one_host, the contract of csrc/clip_device.hpp on the host):
the yardstick against a brute force of the segment definition, hand-built cases, the ABI additions, and clip_one itself
under the address and undefined-behaviour sanitizers in a stand-alone host program."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import clip_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yardstick_equals_the_segment_definition(hip_lib):
    """clip_one_host against an O(n^2) brute force of the definition, tie-break included: 0 .. 40 columns in runs of 1 .. 9,
    every penalty set, bonuses 1, 2, 3 and 5."""
    from allwave_amd import ffi
    rng = random.Random(20)
    seen = {K.OK: 0, K.EMPTY: 0}
    for scores in K.PENALTY_SETS:
        for a in K.BONUSES:
            for _ in range(250):
                alphabet = rng.choice([b"MXID", b"MMMXID", b"MMMMMMXID", b"MID"])
                ops = K.random_ops(rng, rng.randint(0, 40), alphabet=alphabet)
                got = K.as_tuple(ffi.clip_one_host(scores, a, ops))
                assert got == K.brute_force(scores, a, ops), (scores, a, ops)
                seen[got[0]] += 1
    assert seen[K.OK] > 3000 and seen[K.EMPTY] > 100, seen


def test_fixed_cases(hip_lib):
    from allwave_amd import ffi
    for name, scores, a, ops, want in K.fixed_cases():
        assert K.brute_force(scores, a, ops) == want, name  # (the expectation is the definition's)
        assert K.as_tuple(ffi.clip_one_host(scores, a, ops)) == want, name
    # a clip never cuts a gap run and begins and ends with a match
    rng = random.Random(21)
    for _ in range(300):
        ops = K.random_ops(rng, rng.randint(1, 300), alphabet=b"MMMMXID")
        r = ffi.clip_one_host((0, 5, 8, 2, 24, 1), 2, ops)
        if r["code"] == K.OK:
            b, e = int(r["col_beg"]), int(r["col_end"])
            assert ops[b] == ord("M") and ops[e - 1] == ord("M")
            assert K.as_tuple(r) == K.segment_record((0, 5, 8, 2, 24, 1), 2, ops, b, e)


def test_abi_additions(hip_lib):
    from allwave_amd import ffi
    assert ffi.CLIP_DTYPE.itemsize == 56
    assert C.sizeof(ffi.ClipStats) == 32
    new = {"awv_clip_one_host", "awv_clip_cigars", "awv_align_pairs_clipped", "awv_align_ranges_clipped", "awv_engine_clip_stats"}
    assert new <= set(ffi.EXPORTS)
    for s in new:
        assert getattr(hip_lib, s) is not None, s
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    assert re.search(r"#define\s+AWV_ABI_VERSION\s+3\b", hdr) and hip_lib.awv_abi_version() == 3
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_CL_[A-Z_]+)\s+(\d+)", hdr)}
    assert defs == {"AWV_CL_OK": K.OK, "AWV_CL_SKIPPED": K.SKIPPED, "AWV_CL_EMPTY": K.EMPTY, "AWV_CL_BAD_OP": K.BAD_OP}
    for k, v in defs.items():
        assert getattr(ffi, k) == v, k
    assert ffi.RESULT_DTYPE.itemsize == 48 and ffi.VERIFY_DTYPE.itemsize == 24  # (awv_result and awv_verify_result are unchanged)
    assert b"awv_clip_kernel" in open(ffi.LIB_PATH, "rb").read()


def test_bad_arguments(hip_lib):
    from allwave_amd import ffi
    for a in (0, 32768, -1):
        with pytest.raises(ffi.EngineError) as err:
            ffi.clip_one_host((0, 5, 8, 2), a, b"MMM")
        assert err.value.code == ffi.AWV_ERR_ARG, a
    assert ffi.clip_one_host((0, 5, 8, 2), 32767, b"MMM")["score"] == 3 * 32767
    with pytest.raises(ffi.EngineError):
        ffi.clip_one_host((1, 5, 8, 2), 1, b"MMM")  # (the penalties are checked as everywhere)
    for ops, col in K.bad_op_cases():
        r = ffi.clip_one_host((0, 5, 8, 2), 1, ops)
        assert K.as_tuple(r) == (K.BAD_OP, 0, 0, col, col, 0, 0, 0, 0, 0, 0, 0, 0), ops


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "clip_device.hpp"
struct Case { awv_penalties pen; int a; const char* ops; long long n; int code; long long score; unsigned b, e; };
int main() {
  const awv_penalties p2{0, 5, 8, 2, 24, 1, 1}, p1{0, 4, 6, 2, 0, 0, 0};
  std::vector<char> big(150, 'M');
  std::memset(big.data() + 60, 'D', 30);
  const Case cases[] = {
      {p2, 1, "", 0, AWV_CL_EMPTY, 0, 0, 0},
      {p2, 2, "MMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMMM", 37, AWV_CL_OK, 74, 0, 37},
      {p2, 1, "XXXXXXXXX", 9, AWV_CL_EMPTY, 0, 0, 0},
      {p2, 1, "IIIIIDDDDDDDI", 13, AWV_CL_EMPTY, 0, 0, 0},
      {p1, 3, "M", 1, AWV_CL_OK, 3, 0, 1},
      {p1, 1, "MMMMMMMMMMIIMMMMMMMMMM", 22, AWV_CL_OK, 10, 0, 10},
      {p1, 1, "XMMMMMMMMMMDDMMMMMMMMMMX", 24, AWV_CL_OK, 10, 1, 11},
      {p2, 1, big.data(), 150, AWV_CL_OK, 66, 0, 150},
      {p2, 1, "MMMNMM", 6, AWV_CL_BAD_OP, 0, 3, 3},
  };
  int failed = 0;
  for (const Case& c : cases) {
    // an exact-size heap copy: a read past either end of the op string is the sanitizer's to report
    std::vector<unsigned char> ops(c.ops, c.ops + c.n);
    const awv_clip_result r = awvc::clip_one(c.pen, c.a, ops.data(), c.n);
    if (r.code != c.code || r.score != c.score || r.col_beg != c.b || r.col_end != c.e) {
      std::fprintf(stderr, "case %s: code %d score %lld [%u, %u)\n", c.ops, r.code, (long long)r.score, r.col_beg, r.col_end);
      ++failed;
    }
  }
  return failed ? 1 : 0;
}
"""


def test_clip_one_under_sanitizers(tmp_path):
    """clip_one of csrc/clip_device.hpp, compiled for the host only into a stand-alone program under the address and
    undefined-behaviour sanitizers (host options: nothing is built for or run on a GPU), on the fixed cases: it exits 0 and
    the sanitizers report nothing."""
    from allwave_amd import build
    src = tmp_path / "clip_sanitized.cpp"
    src.write_text(SANITIZER_MAIN)
    exe = tmp_path / "clip_sanitized"
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, str(src), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


def test_cli_argument_errors(hip_lib, tmp_path):
    """--clip goes with alignments only, --clip-min-score with --clip only: usage errors, before anything is read."""
    from allwave_amd import build
    build.build_host()
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    for argv, word in ((["--clip", "1", "--score-only"], "--score-only"),
                       (["--clip", "1", "--mash-matrix"], "--mash-matrix"),
                       (["--clip", "1", "--check-paf", str(tmp_path / "x.paf")], "--check-paf"),
                       (["--clip-min-score", "5"], "--clip"),
                       (["--clip", "0"], "--clip"),
                       (["--clip", "32768"], "--clip"),
                       (["--clip", "2", "--clip-min-score", "0"], "--clip-min-score")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (argv, r.returncode, r.stderr)
        assert "error:" in r.stderr and word in r.stderr, (argv, r.stderr)
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--clip A" in r.stdout and "--clip-min-score" in r.stdout


def test_host_arguments(hip_lib):
    """clip= and clip_min_score= are checked before any device is opened."""
    from allwave_amd import build, host
    build.build_host()
    ids, seqs = ["a", "b"], [b"ACGTACGT", b"ACGAACGT"]
    for kw in (dict(clip=0), dict(clip=32768), dict(clip_min_score=3), dict(clip=2, clip_min_score=0)):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", **kw)
    assert host.last_clip()["pairs"] == 0
