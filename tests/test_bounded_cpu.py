"""CPU tests of bounded full alignment (awv_align_pairs_bounded, awv_align_ranges_bounded, awv_divergence_bound,
allwave_hip --max-align-penalty / --max-divergence): the new entry points are declared and exported without moving the ABI,
the divergence bound has the properties its header comment states and is sound against the oracle's alignments, and the CLI
refuses bad values and combinations before any device is opened."""
import ctypes as C
import math
import os
import random
import re
import subprocess

import pytest

from bounded_cases import DIVERGENCES, SCORE_SETS, divergence_bound, edits_columns
from util import mutate, rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -2 ** 31
NEW_SYMBOLS = ("awv_align_pairs_bounded", "awv_align_ranges_bounded", "awv_divergence_bound")


def _header():
    return open(os.path.join(ROOT, "include", "allwave_hip.h")).read()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(hip_lib):
    from allwave_amd import ffi
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+awv_align_pairs_bounded\s*\(\s*awv_engine\s*\*\s*e\s*,\s*const\s+awv_penalties\s*\*\s*pen\s*,\s*const\s+awv_pair\s*\*\s*pairs\s*,"
                     r"\s*int64_t\s+npairs\s*,\s*const\s+int32_t\s*\*\s*max_penalty\s*,\s*awv_result\s*\*\s*out\s*,\s*awv_verify_result\s*\*\s*vout\s*,"
                     r"\s*awv_sink\s+sink\s*,\s*void\s*\*\s*user\s*\)", hdr)
    assert re.search(r"\bint\s+awv_align_ranges_bounded\s*\(\s*awv_engine\s*\*\s*e\s*,\s*const\s+awv_penalties\s*\*\s*pen\s*,\s*const\s+awv_range_pair\s*\*\s*ranges\s*,"
                     r"\s*int64_t\s+n\s*,\s*const\s+int32_t\s*\*\s*max_penalty\s*,", hdr)
    assert re.search(r"\bint32_t\s+awv_divergence_bound\s*\(\s*const\s+awv_penalties\s*\*\s*pen\s*,\s*int32_t\s+plen\s*,\s*int32_t\s+tlen\s*,\s*double\s+d\s*\)", hdr)
    for s in NEW_SYMBOLS:
        assert s in ffi.EXPORTS
        assert getattr(hip_lib, s) is not None, s


def test_abi_version_and_struct_sizes_unchanged(hip_lib):
    from allwave_amd import ffi
    assert hip_lib.awv_abi_version() == 3
    assert re.search(r"#define\s+AWV_ABI_VERSION\s+3\b", _header())
    assert C.sizeof(ffi.EngineConfig) == 40
    assert C.sizeof(ffi.Penalties) == 28
    assert C.sizeof(ffi.Stats) == 8 * 36
    assert C.sizeof(ffi.VerifyStats) == 32
    assert ffi.RESULT_DTYPE.itemsize == 48 and ffi.VERIFY_DTYPE.itemsize == 24


def test_header_states_the_contract():
    txt = " ".join(_header().split())
    assert "status and penalty are what awv_score_pairs_bounded reports under the same bounds" in txt
    assert "the whole record and the op bytes are awv_align_pairs's, byte for byte" in txt
    assert "B = cmax * (floor(d (plen + tlen) / (2 - d)) + 1)" in txt


def test_null_engine_is_refused_like_the_sibling_calls(hip_lib):
    """awv_align_pairs / awv_align_ranges answer a null engine with AWV_ERR_ARG, with or without a GPU; so do these."""
    from allwave_amd import ffi
    pen = ffi.Penalties.from_scores((0, 5, 8, 2, 24, 1))
    pairs = (C.c_int32 * 3)(0, 1, 0)
    ranges = (C.c_int32 * 7)(0, 1, 0, 0, 1, 0, 1)
    bound = (C.c_int32 * 1)(5)
    none = ffi.SINK_FN()
    want = hip_lib.awv_align_pairs(None, C.byref(pen), C.cast(pairs, C.c_void_p), 1, None, none, None)
    assert want == ffi.AWV_ERR_ARG
    assert hip_lib.awv_align_ranges(None, C.byref(pen), C.cast(ranges, C.c_void_p), 1, None, none, None) == want
    assert hip_lib.awv_align_pairs_bounded(None, C.byref(pen), C.cast(pairs, C.c_void_p), 1, C.cast(bound, C.c_void_p), None, None, none, None) == want
    assert b"null engine" in hip_lib.awv_last_error()
    assert hip_lib.awv_align_ranges_bounded(None, C.byref(pen), C.cast(ranges, C.c_void_p), 1, C.cast(bound, C.c_void_p), None, None, none, None) == want
    assert hip_lib.awv_align_ranges_bounded(None, C.byref(pen), C.cast(ranges, C.c_void_p), 1, None, None, None, none, None) == want


def test_python_binding_checks_max_penalty_before_the_engine():
    """Engine.align_pairs(max_penalty=...) validates its argument on the host (no engine needed to see that)."""
    from allwave_amd import ffi
    e = ffi.Engine.__new__(ffi.Engine)  # (no device here: only the argument checks are reached)
    e._h = C.c_void_p()
    with pytest.raises(ValueError, match="max_penalty must be >= 0"):
        e.align_pairs((0, 1, 1, 1), [(0, 1)], max_penalty=-1)
    with pytest.raises(ValueError, match="one bound per pair"):
        e.align_pairs((0, 1, 1, 1), [(0, 1)], max_penalty=[1, 2])
    with pytest.raises(ValueError, match="one bound per pair"):
        e.align_ranges((0, 1, 1, 1), [(0, 1, 0, 0, 1, 0, 1)], max_penalty=[1, 2])


# ---- awv_divergence_bound -------------------------------------------------------------------------------------------------
def test_divergence_bound_closed_form_on_a_grid(hip_lib):
    from allwave_amd import ffi
    for scores in SCORE_SETS + ((0, 3, 5, 1, 20, 1), (0, 7, 0, 3), (0, 2, 12, 1, 40, 1)):
        for plen in (0, 1, 80, 1000, 17000, 1 << 20):
            for tlen in (0, 3, 100, 2000, 1 << 22):
                for d in DIVERGENCES + (0.5, 0.999):
                    assert ffi.divergence_bound(scores, plen, tlen, d) == divergence_bound(scores, plen, tlen, d), (scores, plen, tlen, d)


def test_divergence_bound_is_monotone(hip_lib):
    from allwave_amd import ffi
    rng = random.Random("bounded/monotone")
    for scores in SCORE_SETS:
        for _ in range(300):
            plen, tlen = rng.randrange(0, 50000), rng.randrange(0, 50000)
            d0, d1 = sorted((rng.random() * 0.999, rng.random() * 0.999))
            b = ffi.divergence_bound(scores, plen, tlen, d0)
            assert 0 <= b <= ffi.divergence_bound(scores, plen, tlen, d1)
            assert b <= ffi.divergence_bound(scores, plen + rng.randrange(0, 500), tlen, d0)
            assert b <= ffi.divergence_bound(scores, plen, tlen + rng.randrange(0, 500), d0)


def test_divergence_bound_no_bound_and_bad_input(hip_lib):
    from allwave_amd import ffi
    pen = ffi.Penalties.from_scores((0, 5, 8, 2, 24, 1))
    assert ffi.divergence_bound((0, 5, 8, 2, 24, 1), 1000, 1000, 1.0) == -1
    assert ffi.divergence_bound((0, 5, 8, 2, 24, 1), 1000, 1000, 7.5) == -1
    assert ffi.divergence_bound((0, 5, 8, 2, 24, 1), 1000, 1000, math.inf) == -1
    # overflow: lengths of 2^30 with cmax 60 -- 60 * (floor(0.5 * 2^31 / 1.5) + 1) is far past INT32_MAX
    assert ffi.divergence_bound((0, 60, 58, 2), 1 << 30, 1 << 30, 0.5) == -1
    assert ffi.divergence_bound((0, 60, 58, 2), 1 << 30, 1 << 30, 0.0) == 60
    for d in (-0.01, -1.0, math.nan, -math.inf):
        assert hip_lib.awv_divergence_bound(C.byref(pen), 100, 100, C.c_double(d)) == INT32_MIN, d
        with pytest.raises(ffi.EngineError):
            ffi.divergence_bound((0, 5, 8, 2, 24, 1), 100, 100, d)
    for bad in ((1, 5, 8, 2), (0, 0, 8, 2), (0, 5, -1, 2), (0, 5, 8, 0), (0, 5, 8, 2, 24, 0)):
        p = ffi.Penalties.from_scores(bad)
        assert hip_lib.awv_divergence_bound(C.byref(p), 100, 100, C.c_double(0.1)) == INT32_MIN, bad
    assert hip_lib.awv_divergence_bound(None, 100, 100, C.c_double(0.1)) == INT32_MIN
    assert hip_lib.awv_divergence_bound(C.byref(pen), -1, 100, C.c_double(0.1)) == INT32_MIN


@pytest.fixture(scope="module")
def oracle_pairs():
    """About 200 seeded pairs of at most 80 bp: mutations at 2 - 40 %, and unrelated pairs."""
    rng = random.Random("bounded/soundness")
    out = []
    for k in range(170):
        s = rand_seq(rng, rng.randrange(1, 81))
        out.append((s, mutate(s, rng.uniform(0.02, 0.40), rng)[:80]))
    for k in range(30):
        out.append((rand_seq(rng, rng.randrange(1, 81)), rand_seq(rng, rng.randrange(1, 81))))
    return out


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_divergence_bound_sound_against_oracle(hip_lib, oracle, oracle_pairs, scores):
    """Whenever the oracle's optimal CIGAR has E <= d * columns, its penalty is at most awv_divergence_bound: a pair above the
    bound can be abandoned without losing an alignment the filter would have kept."""
    from allwave_amd import ffi
    al = oracle.Aligner(scores)
    within = above_at_1pct = 0
    for a, b in oracle_pairs:
        pen, ops = al.align(a, b)
        e, cols = edits_columns(ops)
        for d in DIVERGENCES:
            bound = ffi.divergence_bound(scores, len(a), len(b), d)
            assert bound >= 0, (scores, len(a), len(b), d)
            if float(e) <= d * float(cols):
                within += 1
                assert pen <= bound, (scores, a, b, d, pen, bound, e, cols)
        above_at_1pct += pen > ffi.divergence_bound(scores, len(a), len(b), 0.01)
    assert within > len(oracle_pairs)  # (the implication was tested, many times over)
    assert above_at_1pct >= 1          # (and the bound does cut: some pair lies above it at d = 0.01)


# ---- CLI, no device -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(hip_lib):
    from allwave_amd import build
    build.build_host()
    return build.CLI_BIN


@pytest.fixture()
def fasta(tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTACCTAC\n")
    return str(fa)


@pytest.mark.parametrize("flag,value", [("--max-align-penalty", "10"), ("--max-divergence", "0.1")])
@pytest.mark.parametrize("other,named", [(["--score-only"], "'--score-only'"), (["--check-paf", "nowhere.paf"], "'--check-paf'"),
                                         (["--mash-matrix"], "'--mash-matrix'")])
def test_cli_rejected_combinations(cli, fasta, tmp_path, flag, value, other, named):
    out = tmp_path / "out.paf"
    extra = [] if other[0] == "--check-paf" else ["-o", str(out)]
    r = subprocess.run([cli, "-i", fasta, "-p", "none", flag, value] + other + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "the argument '%s' cannot be used with %s" % (flag, named) in r.stderr
    assert "no HIP device" not in r.stderr  # (refused before any device is opened)
    assert not out.exists() and r.stdout == ""


@pytest.mark.parametrize("value", ["-1", "1", "abc", "", "1.5", "nan"])
def test_cli_max_divergence_value_checked(cli, fasta, value):
    r = subprocess.run([cli, "-i", fasta, "-p", "none", "--max-divergence", value], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--max-divergence expects a divergence D with 0 <= D < 1" in r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("value", ["-1", "abc", "", "99999999999", "1.5"])
def test_cli_max_align_penalty_value_checked(cli, fasta, value):
    r = subprocess.run([cli, "-i", fasta, "-p", "none", "--max-align-penalty", value], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--max-align-penalty expects a penalty N >= 0" in r.stderr
    assert r.stdout == ""


def test_cli_help_lists_both_flags(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--max-align-penalty N" in r.stdout and "--max-divergence D" in r.stdout
    assert "--max-penalty N" in r.stdout  # (the score-only bound keeps its flag)


def test_host_binding_checks_bounds_before_the_device():
    from allwave_amd import host
    with pytest.raises(ValueError, match="max_penalty must be >= 0"):
        host.all_pairs_paf(["a", "b"], [b"ACGT", b"ACGA"], "0,1,1,1", max_penalty=-1)
    for d in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError, match="max_divergence must be in"):
            host.iterate(["a", "b"], [b"ACGT", b"ACGA"], "0,1,1,1", max_divergence=d)
    assert host.last_bounds() == dict(pairs=0, above_penalty=0, above_divergence=0)
