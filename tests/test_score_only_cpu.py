"""CPU tests of score-only alignment (awv_score_pairs, AllPairIterator::scores, allwave_hip --score-only): the new entry point
is declared and exported, its status constant agrees between the header and the ctypes binding, it refuses without a GPU,
and the CLI rejects --max-penalty without --score-only before any device is opened."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "allwave_hip.h")).read()


def test_score_pairs_declared_and_exported(hip_lib):
    from allwave_amd import ffi
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+awv_score_pairs\s*\(", hdr)
    assert re.search(r"\}\s*awv_score_result\s*;", hdr)
    assert "awv_score_pairs" in ffi.EXPORTS
    assert getattr(hip_lib, "awv_score_pairs") is not None
    assert ffi.SCORE_DTYPE.itemsize == 8  # awv_score_result: two int32


def test_above_bound_status_matches_header():
    from allwave_amd import ffi
    m = re.search(r"#define\s+AWV_ST_ABOVE_BOUND\s+(\d+)", _header())
    assert m and int(m.group(1)) == 4
    assert ffi.AWV_ST_ABOVE_BOUND == 4


def test_header_maps_compute_score_scope():
    """The mapping table at the top of the header names the entry point that replaces lib_wfa2's ComputeScore scope."""
    top = _header().split("#ifndef ALLWAVE_HIP_H")[0]
    line = [l for l in top.splitlines() if "ComputeScore" in l]
    assert line and "awv_score_pairs" in line[0]


def test_score_pairs_without_gpu(hip_lib):
    """No GPU: no engine can exist, and awv_score_pairs says so (no CPU fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from allwave_amd import ffi
    out = (C.c_int32 * 2)()
    pen = ffi.Penalties.from_scores((0, 5, 8, 2, 24, 1))
    pairs = (C.c_int32 * 3)(0, 1, 0)
    rc = hip_lib.awv_score_pairs(None, C.byref(pen), C.cast(pairs, C.c_void_p), 1, -1, C.cast(out, C.c_void_p))
    assert rc == ffi.AWV_ERR_NO_DEVICE
    assert b"no CPU fallback" in hip_lib.awv_last_error()


@pytest.fixture(scope="module")
def cli(hip_lib):
    from allwave_amd import build
    build.build_host()
    return build.CLI_BIN


def test_cli_max_penalty_needs_score_only(cli, tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTACCTAC\n")
    out = tmp_path / "out.txt"
    r = subprocess.run([cli, "-i", str(fa), "-p", "none", "--max-penalty", "10", "-o", str(out)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "'--max-penalty' requires '--score-only'" in r.stderr
    assert not out.exists() and r.stdout == ""


@pytest.mark.parametrize("value", ["-1", "x", "", "99999999999"])
def test_cli_max_penalty_value_checked(cli, tmp_path, value):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTACCTAC\n")
    r = subprocess.run([cli, "-i", str(fa), "-p", "none", "--score-only", "--max-penalty", value], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--max-penalty expects a penalty N >= 0" in r.stderr
    assert r.stdout == ""


def test_cli_help_lists_score_only(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--score-only" in r.stdout and "--max-penalty" in r.stdout
