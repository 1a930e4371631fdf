"""CPU tests of the device pass that tallies the allele table (csrc/variants.hip, csrc/variants_fold.hip): the kernel's walk --
lanes of 16 bytes, chunks of 1,024, runs owned by breaks, the segmented hash scan and its carries -- emulated serially with the
kernel's own __host__ __device__ functions (tests/variants_walk_driver.cpp) under the address and undefined-behaviour sanitizers,
against var_one and against the Python restatement; and the ABI of the pass.  None of them needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import variants_cases as R
from verify_cases import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUES = (0, 1, 15)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/variants_walk_driver.cpp, compiled for the host only (nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("variants_walk") / "variants_walk_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "variants_walk_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def fnv(rows):
    h = 1469598103934665603
    for r in rows:
        for f in ("t_idx", "pos", "type", "len", "hash", "rep", "count"):
            h = ((h ^ int(r[f])) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run(driver, lines):
    """lines: [(residue, q, t, rev, tlen, span, pattern, ops, slice)] -> the driver's output lines."""
    text_in = "".join("W %d %d %d %d %d %d %d %d %d %s %s %d %d %d %d\n" % ((res, q, t, rev, tl) + tuple(sp) + (p.hex() or "-", o.hex() or "-") + tuple(sl))
                      for res, q, t, rev, tl, sp, p, o, sl in lines)
    r = subprocess.run([driver], input=text_in, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def check(lines, got):
    codes = set()
    for (res, q, t, rev, tl, sp, p, o, sl), line in zip(lines, got):
        code, events = R.events_of(q, t, rev, p, o[sl[0]:sl[1]], sp, (sl[2], sl[3]))
        want = "1 %d %d %d %d %d %d" % ((code,) + R.counts_of(events) + (len(events), fnv(R.as_rows(events))))
        assert line == want, (line, want, res, sl, o[:40])
        codes.add(code)
    return codes


def test_the_walk_reproduces_var_one_on_the_case_list(driver):
    """The whole case list at residues 0, 1 and 15: the emulated decomposition equals var_one byte for byte (the driver's first
    field) and the restatement (the rest of the line), and the sanitizers report nothing."""
    seqs, cl = R.resident_set(), R.case_list()
    lines = []
    for name, q, t, rev, ops, sl, status, _ in cl:
        if status != 0:
            continue
        for res in RESIDUES:
            lines.append((res, q, t, rev, len(seqs[t]), (0, len(seqs[q]), 0, len(seqs[t])), revcomp(seqs[q]) if rev else seqs[q], ops, sl or (0, len(ops), 0, 0)))
    assert len(lines) >= 3 * 150
    assert check(lines, run(driver, lines)) == {R.OK, R.BAD_OP, R.LENGTHS}


def test_the_walk_reproduces_var_one_on_random_items(driver):
    lines = [(RESIDUES[k % 3], q, t, rev, tlen, span, pattern, ops, sl or (0, len(ops), 0, 0))
             for k, (q, t, rev, pattern, tlen, span, ops, sl) in enumerate(R.random_items())]
    assert len(lines) == 300
    assert check(lines, run(driver, lines)) == {R.OK}


def test_the_segmented_combine_is_associative(driver):
    r = subprocess.run([driver], input="A 20000 1\nA 20000 77\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.split() == ["1", "1"], (r.returncode, r.stdout, r.stderr[-2000:])


def test_exports_and_struct_sizes(hip_lib):
    from allwave_amd import ffi
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for name in ("awv_engine_variants_begin", "awv_engine_variants_end", "awv_engine_variants_read", "awv_engine_variants_stats", "awv_variants_cigars", "awv_variants_ranges",
                 "awv_variants_fold"):
        assert name in ffi.EXPORTS and getattr(hip_lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr), name
    assert C.sizeof(ffi.VariantsStats) == 88 and "} awv_variants_stats; /* 88 bytes */" in hdr
    assert [f[0] for f in ffi.VariantsStats._fields_] == ["kernel_ms", "fold_ms", "items", "failed", "columns", "snv", "ins", "del_", "rows", "folds", "capacity_rows"]
    assert ffi.AWV_VTAB_EVENTS == 0 and ffi.AWV_VTAB_FOLDED == 1 and ffi.AWV_VTAB_ACCUMULATE == 2
    for k in ("AWV_VTAB_EVENTS", "AWV_VTAB_FOLDED", "AWV_VTAB_ACCUMULATE"):
        assert re.search(r"#define\s+%s\s+%d\b" % (k, getattr(ffi, k)), hdr), k
    assert hip_lib.awv_abi_version() == 3 and "#define AWV_ABI_VERSION 3" in hdr
    # nothing of the pass runs without an engine: a null one is refused
    assert hip_lib.awv_engine_variants_stats(None, None) == ffi.AWV_ERR_ARG
