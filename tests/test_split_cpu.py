"""CPU tests of splitting into all good segments (awv_split_one_host, the contract of csrc/split_device.hpp on the host): the
yardstick against the recursion over a Python clip walk, the properties a split has by definition against a brute force, the
slot bound, and the ABI additions."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import clip_cases as K
import split_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yardstick_equals_the_recursion(hip_lib):
    """split_one_host against the recursion in Python on 2,592 seeded strings of up to 80 columns: two op mixes, three penalty
    sets, a in {1, 2, 5}, min_score in {1, 3, 10, 40}; the first six strings of every combination (n <= 40) also against the
    brute-force properties."""
    from allwave_amd import ffi
    rng = random.Random(31)
    strings = several = most = 0
    for mix in S.OP_MIXES:
        for scores in S.PENALTY_SETS:
            for a in S.BONUSES:
                for min_score in S.MIN_SCORES:
                    for k in range(36):
                        n = rng.randint(0, 40 if k < 6 else 80)
                        ops = K.random_ops(rng, n, runs=(1, 7), alphabet=mix)
                        want = S.expected(scores, a, min_score, ops)
                        index, segs = ffi.split_one_host(scores, a, min_score, ops)
                        assert S.got(index, segs) == want, (scores, a, min_score, ops)
                        if k < 6:
                            S.check_properties(scores, a, min_score, ops, [(r[3], r[4]) for r in want[1]])
                        strings += 1
                        several += want[0][1] > 1
                        most = max(most, want[0][1])
    assert strings >= 2000 and several > 300 and most >= 7, (strings, several, most)


def test_clip_is_the_top_segment(hip_lib):
    from allwave_amd import ffi
    rng = random.Random(32)
    for _ in range(300):
        ops = K.random_ops(rng, rng.randint(1, 200), alphabet=b"MMMMXID")
        for min_score in (1, 12):
            cl = ffi.clip_one_host((0, 5, 8, 2, 24, 1), 2, ops)
            index, segs = ffi.split_one_host((0, 5, 8, 2, 24, 1), 2, min_score, ops)
            if cl["code"] == K.OK and cl["score"] >= min_score:
                top = max(segs, key=lambda s: int(s["score"]))
                assert K.as_tuple(cl) in [K.as_tuple(s) for s in segs] and int(top["score"]) == int(cl["score"])
            else:
                assert int(index["code"]) == K.EMPTY and len(segs) == 0


def test_slot_bound(hip_lib):
    from allwave_amd import ffi
    assert ffi.split_slots(1, 1, 0) == 0 and ffi.split_slots(1, 1, 7) == 7 and ffi.split_slots(2, 5, 7) == 2
    assert ffi.split_slots(5, 40, 80) == 10 and ffi.split_slots(32767, 1, 2 ** 32 - 1) == 32767 * (2 ** 32 - 1)
    assert ffi.split_slots(1, 2 ** 62, 10) == 0
    for a, min_score, m in ((0, 1, 5), (32768, 1, 5), (-1, 1, 5), (1, 0, 5), (1, -3, 5), (1, 1, -1)):
        assert hip_lib.awv_split_slots(a, min_score, m) == -1, (a, min_score, m)
        with pytest.raises(ffi.EngineError):
            ffi.split_slots(a, min_score, m)
    # the bound is attained: blocks of exactly ceil(min_score / a) matches, one X apart (x = 50 >= a block's score: none is worth bridging)
    for a, min_score in ((1, 1), (1, 7), (2, 7), (5, 40)):
        block = -(-min_score // a)
        ops = b"X".join([b"M" * block] * 9)
        index, segs = ffi.split_one_host((0, 50, 8, 2), a, min_score, ops)
        assert int(index["count"]) == 9 and ffi.split_slots(a, min_score, 9 * block) >= 9
    # fewer slots offered than segments found: all are counted, the offered ones are written
    index, segs = ffi.split_one_host((0, 5, 8, 2), 1, 1, b"MXMXMXM", cap=2)
    assert int(index["count"]) == 4 and len(segs) == 2


def test_abi_additions(hip_lib):
    from allwave_amd import ffi
    assert ffi.SPLIT_INDEX_DTYPE.itemsize == 16 and ffi.CLIP_DTYPE.itemsize == 56
    assert C.sizeof(ffi.SplitStats) == 48
    new = {"awv_split_slots", "awv_split_layout_pairs", "awv_split_layout_ranges", "awv_split_one_host", "awv_split_cigars",
           "awv_align_pairs_split", "awv_align_ranges_split", "awv_engine_split_stats"}
    assert new <= set(ffi.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for s in new:
        assert getattr(hip_lib, s) is not None, s
        assert re.search(r"\b%s\s*\(" % s, hdr), s
    assert re.search(r"}\s*awv_split_index;", hdr) and re.search(r"}\s*awv_split_stats;", hdr)
    assert re.search(r"#define\s+AWV_ABI_VERSION\s+3\b", hdr) and hip_lib.awv_abi_version() == 3
    assert ffi.RESULT_DTYPE.itemsize == 48  # (awv_result is unchanged)
    lib = open(ffi.LIB_PATH, "rb").read()
    assert b"awv_split_kernel" in lib and b"awv_clip_kernel" in lib


def test_bad_arguments_give_the_clips_answer(hip_lib):
    from allwave_amd import ffi
    for a in (0, 32768, -1):
        with pytest.raises(ffi.EngineError) as err:
            ffi.split_one_host((0, 5, 8, 2), a, 1, b"MMM", cap=3)
        assert err.value.code == ffi.AWV_ERR_ARG, a
    for min_score in (0, -1, -2 ** 40):
        with pytest.raises(ffi.EngineError) as err:
            ffi.split_one_host((0, 5, 8, 2), 1, min_score, b"MMM", cap=3)
        assert err.value.code == ffi.AWV_ERR_ARG, min_score
    with pytest.raises(ffi.EngineError):
        ffi.split_one_host((1, 5, 8, 2), 1, 1, b"MMM")  # (the penalties are checked as everywhere)
    index, segs = ffi.split_one_host((0, 5, 8, 2), 32767, 2 ** 40, b"MMM")
    assert int(index["code"]) == K.EMPTY and int(index["column"]) == -1
    for ops, col in K.bad_op_cases():
        index, segs = ffi.split_one_host((0, 5, 8, 2), 1, 1, ops)
        assert S.got(index, segs) == ((K.BAD_OP, 0, col), []), ops
    # a bad op inside what would be a remainder: the first scan covers the whole string
    for ops, col in ((b"M" * 30 + b"XXXNXX" + b"M" * 10, 33), (b"XNX" + b"M" * 30, 1), (b"M" * 30 + b"XX\x00", 32)):
        assert K.as_tuple(ffi.clip_one_host((0, 5, 8, 2), 1, ops))[0] == K.BAD_OP
        index, segs = ffi.split_one_host((0, 5, 8, 2), 1, 5, ops)
        assert S.got(index, segs) == ((K.BAD_OP, 0, col), []), ops


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "split_device.hpp"
int main() {
  const awv_penalties p2{0, 5, 8, 2, 24, 1, 1};
  std::vector<unsigned char> ops;
  const int blocks[] = {30, 50, 32, 70, 34, 52, 36};
  for (int k = 0; k < 7; ++k) {
    if (k) ops.insert(ops.end(), 40, 'X');
    ops.insert(ops.end(), blocks[k], 'M');
  }
  int failed = 0;
  for (long long min_score : {1ll, 20ll, 33ll, 1000ll}) {
    // exact-size heap buffers: a read or write past either end is the sanitizer's to report
    const long long cap = awvs::slots(1, min_score, (long long)ops.size());
    std::vector<awv_clip_result> out((size_t)cap);
    std::vector<awvs::Interval> stack((size_t)cap + 1);
    const awv_split_index ix = awvs::split_one(p2, 1, min_score, ops.data(), (long long)ops.size(), out.data(), cap, stack.data());
    const int want = min_score <= 30 ? 7 : min_score == 33 ? 5 : 0;
    if (ix.count != want || ix.code != (want ? AWV_CL_OK : AWV_CL_EMPTY)) {
      std::fprintf(stderr, "min_score %lld: code %d count %d\n", min_score, ix.code, ix.count);
      ++failed;
    }
    for (int i = 1; i < ix.count; ++i) failed += out[i - 1].col_end > out[i].col_beg;
  }
  return failed ? 1 : 0;
}
"""


def test_split_one_under_sanitizers(tmp_path):
    """split_one of csrc/split_device.hpp, compiled for the host only into a stand-alone program under the address and
    undefined-behaviour sanitizers, with slot and stack buffers of exactly the documented sizes."""
    from allwave_amd import build
    src = tmp_path / "split_sanitized.cpp"
    src.write_text(SANITIZER_MAIN)
    exe = tmp_path / "split_sanitized"
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, str(src), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)


def test_cli_argument_errors(hip_lib, tmp_path):
    """--split needs --split-min-score (no default can be derived), excludes --clip and goes with alignments only: usage
    errors, before anything is read."""
    from allwave_amd import build
    build.build_host()
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    ok = ["--split", "1", "--split-min-score", "5"]
    for argv, word in ((["--split", "1"], "--split-min-score"),
                       (["--split-min-score", "5"], "--split"),
                       (ok + ["--clip", "1"], "--clip"),
                       (ok + ["--score-only"], "--score-only"),
                       (ok + ["--mash-matrix"], "--mash-matrix"),
                       (ok + ["--check-paf", str(tmp_path / "x.paf")], "--check-paf"),
                       (["--split", "0", "--split-min-score", "5"], "--split"),
                       (["--split", "32768", "--split-min-score", "5"], "--split"),
                       (["--split", "2", "--split-min-score", "0"], "--split-min-score")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (argv, r.returncode, r.stderr)
        assert "error:" in r.stderr and word in r.stderr, (argv, r.stderr)
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--split A" in r.stdout and "--split-min-score" in r.stdout


def test_host_arguments(hip_lib):
    """split= and split_min_score= are checked before any device is opened."""
    from allwave_amd import build, host
    build.build_host()
    ids, seqs = ["a", "b"], [b"ACGTACGT", b"ACGAACGT"]
    for kw in (dict(split=0, split_min_score=5), dict(split=32768, split_min_score=5), dict(split_min_score=3), dict(split=2),
               dict(split=2, split_min_score=0), dict(split=2, split_min_score=5, clip=1)):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", **kw)
    assert host.last_split()["pairs"] == 0
