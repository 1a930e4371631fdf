"""CPU tests of gap-run normalization (awv_normalize_one_host, the contract of csrc/normalize_device.hpp on the host): the
yardstick against an independent step-by-step shifter, the properties of every output, hand-made traps with stated
expectations, refusals, the ABI additions, and the oracle's view of the lists the GPU tests align."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import normalize_cases as N
import verify_cases as V
from util import DEFAULT_2P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yardstick_equals_the_step_by_step_shifter(hip_lib):
    """6,000 random edit scripts of 0 .. 200 columns over 1- to 4-letter alphabets, both directions: the closed form's bytes
    are the single-step definition's, and every output keeps its runs, is a fixed point, still verifies with the unchanged
    record under a 1-piece and a 2-piece penalty set, and right is the mirror image of left."""
    from allwave_amd import ffi
    rng = random.Random(30)
    moved = {"left": 0, "right": 0}
    linked = 0
    for k in range(6000):
        p, t, ops = N.random_script(rng)
        for direction in ("left", "right"):
            got, rec = ffi.normalize_one_host(direction, p, t, ops)
            want, steps = N.step_normal(direction, p, t, ops)
            assert got == want, (direction, p, t, ops)
            assert N.as_tuple(rec)[0] == N.OK and int(rec["columns_moved"]) == steps, (direction, p, t, ops)
            assert N.runs(got) != [] or ops == b""
            assert N.gap_runs(got) == N.gap_runs(ops) and [r[0] for r in N.runs(got) if r[0] != ord("M")] == [r[0] for r in N.runs(ops) if r[0] != ord("M")]
            again, rec2 = ffi.normalize_one_host(direction, p, t, got)
            assert again == got and N.as_tuple(rec2) == (N.OK, 0, 0, 0, 0)
            moved[direction] += int(rec["runs_moved"])
            linked += int(rec["max_shift"]) > 12  # (further than the longest 'M' run: only a linked run gets there)
            if k % 4 == 0:
                for scores in (N.P1, DEFAULT_2P):
                    claimed = V.record_for(scores, ops)  # the record of the INPUT string
                    assert int(ffi.verify_one_host(scores, p, t, got, claimed)["code"]) == ffi.AWV_VF_OK, (direction, scores, p, t, ops)
        left, _ = ffi.normalize_one_host("left", p[::-1], t[::-1], ops[::-1])
        assert ffi.normalize_one_host("right", p, t, ops)[0] == left[::-1]
    assert moved["left"] > 5000 and moved["right"] > 5000 and linked > 50, (moved, linked)


def test_traps(hip_lib):
    from allwave_amd import ffi
    names = set()
    for name, direction, p, t, ops, want in N.traps():
        assert int(ffi.verify_one_host(N.P1, p, t, ops, V.record_for(N.P1, ops))["code"]) == ffi.AWV_VF_OK, name  # (the case is a true alignment)
        got, rec = ffi.normalize_one_host(direction, p, t, ops)
        assert got == want, name
        assert N.step_normal(direction, p, t, ops)[0] == want, name
        assert int(rec["code"]) == N.OK and (int(rec["runs_moved"]) > 0) == (want != ops), name
        names.add(name)
    for k in (15, 16, 17, 63, 64, 65, 1023, 1024, 1025):
        _, _, p, t, ops, _ = next(c for c in N.traps() if c[0] == "shift of %d stopped by a base" % k)
        assert N.as_tuple(ffi.normalize_one_host("left", p, t, ops)[1]) == (N.OK, 1, k, k, 0)
    assert len(names) == len(N.traps()) >= 50


def test_refusals_leave_the_bytes_alone(hip_lib):
    from allwave_amd import ffi
    for name, p, t, ops, code, col in N.refusals():
        for direction in ("left", "right"):
            got, rec = ffi.normalize_one_host(direction, p, t, ops)
            assert got == ops and N.as_tuple(rec) == (code, 0, col, 0, 0), name
    for bad in ("up", 3, True):
        with pytest.raises(ValueError):
            ffi.normalize_one_host(bad, b"A", b"A", b"M")
    with pytest.raises(ffi.EngineError):  # (off is a mode, not a direction)
        ffi.normalize_one_host(None, b"A", b"A", b"M")
    rec = np.zeros(1, dtype=ffi.NORM_DTYPE)
    assert hip_lib.awv_normalize_one_host(0, b"A", 1, b"A", 1, b"M", 1, C.create_string_buffer(1), rec.ctypes.data) == ffi.AWV_ERR_ARG
    assert hip_lib.awv_normalize_one_host(1, b"A", -1, b"A", 1, b"M", 1, C.create_string_buffer(1), rec.ctypes.data) == ffi.AWV_ERR_ARG
    # in place: the output may be the input
    buf = C.create_string_buffer(b"MMMMMMMI", 8)
    assert hip_lib.awv_normalize_one_host(1, b"A" * 7, 7, b"A" * 8, 8, buf, 8, buf, rec.ctypes.data) == 0 and buf.raw == b"IMMMMMMM"


def test_abi_additions(hip_lib):
    from allwave_amd import ffi
    assert ffi.NORM_DTYPE.itemsize == 24 and C.sizeof(ffi.NormStats) == 56
    new = {"awv_normalize_one_host", "awv_normalize_cigars", "awv_normalize_ranges", "awv_engine_set_normalize", "awv_engine_normalize_stats"}
    assert new <= set(ffi.EXPORTS)
    for s in new:
        assert getattr(hip_lib, s) is not None, s
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    assert re.search(r"#define\s+AWV_ABI_VERSION\s+3\b", hdr) and hip_lib.awv_abi_version() == 3
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_(?:NM|NORM)_[A-Z_]+)\s+(\d+)", hdr)}
    assert defs == {"AWV_NORM_OFF": 0, "AWV_NORM_LEFT": 1, "AWV_NORM_RIGHT": 2, "AWV_NM_OK": N.OK, "AWV_NM_SKIPPED": N.SKIPPED,
                    "AWV_NM_BAD_OP": N.BAD_OP, "AWV_NM_LENGTHS": N.LENGTHS}
    for k, v in defs.items():
        assert getattr(ffi, k) == v, k
    m = re.search(r"typedef struct \{([^}]*)\} awv_norm_result;", hdr)
    assert re.findall(r"(int32_t|int64_t)\s+(\w+);", m.group(1)) == [("int32_t", "code"), ("int32_t", "runs_moved"), ("int64_t", "columns_moved"),
                                                                       ("int32_t", "max_shift"), ("int32_t", "reserved")]
    assert ffi.RESULT_DTYPE.itemsize == 48  # (awv_result is unchanged)
    assert b"awv_normalize_kernel" in open(ffi.LIB_PATH, "rb").read()


def test_device_entry_points_refuse_without_a_gpu(hip_lib):
    """A null engine: AWV_ERR_NO_DEVICE where there is no GPU, AWV_ERR_ARG where there is one; never a crash, never a result."""
    from allwave_amd import ffi
    rec = np.zeros(1, dtype=ffi.RESULT_DTYPE)
    nres = np.zeros(1, dtype=ffi.NORM_DTYPE)
    pair = np.zeros(1, dtype=ffi.PAIR_DTYPE)
    rng_ = np.zeros(1, dtype=ffi.RANGE_DTYPE)
    arena = np.zeros(16, dtype=np.uint8)
    for fn, first in ((hip_lib.awv_normalize_cigars, pair), (hip_lib.awv_normalize_ranges, rng_)):
        rc = fn(None, ffi.AWV_NORM_LEFT, first.ctypes.data, 1, rec.ctypes.data, arena.ctypes.data, 16, nres.ctypes.data)
        assert rc in (ffi.AWV_ERR_NO_DEVICE, ffi.AWV_ERR_ARG)
        if rc == ffi.AWV_ERR_NO_DEVICE:
            assert b"no HIP device" in hip_lib.awv_last_error()
    assert hip_lib.awv_engine_set_normalize(None, 1) == ffi.AWV_ERR_ARG
    assert hip_lib.awv_engine_normalize_stats(None, None) == ffi.AWV_ERR_ARG


def test_skipped_is_a_code_of_its_own(hip_lib):
    """AWV_NM_SKIPPED belongs to records, which the host walk does not see: its value is fixed and differs from the others."""
    from allwave_amd import ffi
    assert len({ffi.AWV_NM_OK, ffi.AWV_NM_SKIPPED, ffi.AWV_NM_BAD_OP, ffi.AWV_NM_LENGTHS}) == 4 and ffi.AWV_NM_SKIPPED == 1


def test_device_case_lists_are_what_they_claim(hip_lib):
    """The caller-supplied strings of the GPU tests: true alignments of their pairs (so the yardstick normalizes them), with
    moved runs in both directions, q_revcomp pairs, N and lower-case sequences, strings of several chunks."""
    from allwave_amd import ffi
    seqs, pairs, ranges, seen_p, seen_r = N.device_cases()
    assert len(pairs) == len(ranges) == len(seen_p) and set(pairs[:, 2]) == {0, 1} and set(ranges[:, 2]) == {0, 1}
    moved = {"left": 0, "right": 0}
    for k, (p, t, ops) in enumerate(seen_p):
        q, tt, rev = pairs[k]
        assert seqs[tt] == t and (V.revcomp(seqs[q]) if rev else seqs[q]) == p
        rq, rt, rrev, qb, qe, tb, te = ranges[k]
        assert seqs[rt][tb:te] == t and (V.revcomp(seqs[rq][qb:qe]) if rrev else seqs[rq][qb:qe]) == p
        for direction in moved:
            moved[direction] += int(ffi.normalize_one_host(direction, p, t, ops)[1]["runs_moved"]) > 0
    assert moved["left"] >= 60 and moved["right"] >= 60, moved
    assert any(b"N" in s for s in seqs) and any(s != s.upper() for s in seqs) and max(len(o) for _, _, o in seen_p) > 3 * 1024
    p, t, ops = N.homopolymer_case()
    assert len(p) > 29000 and len(N.gap_runs(ops)) >= 300
    rec = ffi.normalize_one_host("left", p, t, ops)[1]
    assert int(rec["code"]) == N.OK and int(rec["runs_moved"]) >= 300 and int(rec["columns_moved"]) > 20 * len(ops)


def test_oracle_alignments_of_the_repeat_set_have_movable_runs(hip_lib, oracle):
    """The pair list the GPU tests align, through the CPU oracle under both penalty sets: in every generator class at least one
    alignment has a run the yardstick moves -- so the GPU comparison cannot pass on strings that normalization leaves as they
    are."""
    from allwave_amd import ffi
    seqs, pairs, names = N.repeat_set()
    assert sorted(set(names)) == sorted(N.GENERATORS)
    for scores in N.ALIGN_SCORES:
        al = oracle.Aligner(scores)
        moved = dict.fromkeys(N.GENERATORS, 0)
        for (q, t, _), name in zip(pairs, names):
            _, ops = al.align(seqs[q], seqs[t])
            ops = bytes(ops)
            got, rec = ffi.normalize_one_host("left", seqs[q], seqs[t], ops)
            assert int(rec["code"]) == N.OK
            assert int(ffi.verify_one_host(scores, seqs[q], seqs[t], got, V.record_for(scores, ops))["code"]) == ffi.AWV_VF_OK
            moved[name] += int(rec["runs_moved"])
        assert all(v >= 1 for v in moved.values()), (scores, moved)


def test_cli_argument_errors(hip_lib, tmp_path):
    """--normalize goes with alignments only and takes left or right: usage errors, before any device is opened."""
    from allwave_amd import build
    build.build_host()
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    for argv, word in ((["--normalize", "left", "--score-only"], "--score-only"),
                       (["--normalize", "right", "--check-paf", str(tmp_path / "x.paf")], "--check-paf"),
                       (["--normalize", "left", "--mash-matrix"], "--mash-matrix"),
                       (["--normalize", "up"], "--normalize"),
                       (["--normalize", ""], "--normalize"),
                       (["--normalize"], "--normalize")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (argv, r.returncode, r.stderr)
        assert "error:" in r.stderr and word in r.stderr and "no HIP device" not in r.stderr, (argv, r.stderr)
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--normalize left|right" in r.stdout and "normalized N pairs, R runs moved, K ms" in r.stdout


def test_host_arguments(hip_lib):
    """normalize= is checked before any device is opened, and a refused call leaves no mode behind."""
    from allwave_amd import build, host
    build.build_host()
    ids, seqs = ["a", "b"], [b"ACGTACGT", b"ACGAACGT"]
    for bad in ("up", 3, True, "LEFT"):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", normalize=bad)
        with pytest.raises(ValueError):
            host.align_ranges(ids, seqs, [(0, 1, 0, 0, 8, 0, 8)], "0,5,8,2,24,1", normalize=bad)
    with pytest.raises(ValueError):
        host.all_pairs_paf(ids, seqs, "0,5,8,2,24,1", normalize="left", clip=0)
    assert host.last_normalize() == dict(pairs=0, records_moved=0, runs=0, runs_moved=0, columns_moved=0, columns=0, kernel_ms=0.0)


SANITIZER_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "normalize_device.hpp"
struct Case { bool mirror; std::string p, t, ops, want; int code; };
int main() {
  const std::string a1000(1000, 'A');
  const Case cases[] = {
      {false, "AAAAAAA", "AAAAAAAA", "MMMMMMMI", "IMMMMMMM", AWV_NM_OK},
      {true, "AAAAAAA", "AAAAAAAA", "IMMMMMMM", "MMMMMMMI", AWV_NM_OK},
      {false, "AAAAAA", "AAAAAA", "MMIMMDM", "IDMMMMM", AWV_NM_OK},
      {false, "AAAAA", "AAAAAAA", "MMIMMIM", "IMIMMMM", AWV_NM_OK},
      {false, "AACAA", "AAGAAA", "MMXMMI", "MMXIMM", AWV_NM_OK},
      {false, "AA", "AA", "IIDD", "IIDD", AWV_NM_OK},
      {false, "", "", "", "", AWV_NM_OK},
      {false, a1000, a1000 + "AA", std::string(1000, 'M') + "II", "II" + std::string(1000, 'M'), AWV_NM_OK},
      {true, a1000 + "AA", a1000, "DD" + std::string(1000, 'M'), std::string(1000, 'M') + "DD", AWV_NM_OK},
      {false, "AAAA", "AAAA", "MMNM", "MMNM", AWV_NM_BAD_OP},
      {false, "AAAAA", "AAAA", "MMMM", "MMMM", AWV_NM_LENGTHS},
      {false, "A", "", "", "", AWV_NM_LENGTHS},
  };
  int failed = 0;
  for (const Case& c : cases) {
    // exact-size heap copies: a read or a write past either end of a sequence or of the op string is the sanitizer's to report
    std::vector<unsigned char> p(c.p.begin(), c.p.end()), t(c.t.begin(), c.t.end()), in(c.ops.begin(), c.ops.end()), out(c.ops.begin(), c.ops.end());
    const awv_norm_result r = awvn::normalize_one(c.mirror, p.data(), (int)p.size(), t.data(), (int)t.size(), in.data(), (long long)in.size(), out.data());
    const awv_norm_result q = awvn::normalize_one(c.mirror, p.data(), (int)p.size(), t.data(), (int)t.size(), in.data(), (long long)in.size(), in.data());  // in place
    if (r.code != c.code || std::string(out.begin(), out.end()) != c.want || q.code != c.code || std::string(in.begin(), in.end()) != c.want) {
      std::fprintf(stderr, "case %s: code %d\n", c.ops.substr(0, 40).c_str(), r.code);
      ++failed;
    }
  }
  return failed ? 1 : 0;
}
"""


def test_normalize_one_under_sanitizers(tmp_path):
    """normalize_one of csrc/normalize_device.hpp, compiled for the host only into a stand-alone program under the address
    and undefined-behaviour sanitizers (host options: nothing is built for or run on a GPU): it exits 0 and the sanitizers
    report nothing."""
    from allwave_amd import build
    src = tmp_path / "normalize_sanitized.cpp"
    src.write_text(SANITIZER_MAIN)
    exe = tmp_path / "normalize_sanitized"
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, str(src), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
