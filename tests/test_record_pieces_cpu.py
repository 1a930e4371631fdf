"""CPU test of how a call on caller-supplied records is cut into launches (allwave_amd/csrc/record_pieces.hpp):
a stand-alone driver, built with the system C++ compiler under AddressSanitizer and UBSan, cuts small record lists into
pieces, plays the device's part on every piece (each staged byte XOR 0xA5) and scatters the pieces back.  Its output is
checked against the rule restated here -- pieces(), scattered() -- and against the properties the record kernels rely on."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPLETED, OTHER = 0, 1                      # awv_result.status: AWV_ST_COMPLETED, any other
NM_OK, NM_OTHER = 0, 3                       # awv_norm_result.code: AWV_NM_OK, any other
LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025)
MAX_ARENA = (16, 64, 8192, 1 << 40)
MAX_RECORDS = (1, 3, 1 << 20, 0)             # 0: the header's default, 2^20
DEVICE = 0xA5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("record_pieces") / "record_pieces_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "record_pieces_driver.cpp"), "-o", exe])
    return exe


def ceil16(x):
    return (x + 15) // 16 * 16


def pieces(recs, max_arena, max_records, keep):
    """The rule: recs [(status, cigar_off, cigar_len, code)] -> [(first, bytes, [staged cigar_off])], greedy and in order."""
    out, first = [], 0
    while first < len(recs):
        total, offs = 0, []
        while first + len(offs) < len(recs) and len(offs) < max_records:
            status, off, ln, _ = recs[first + len(offs)]
            sh = off % 16 if keep else 0
            need = ceil16(sh + ln) if status == COMPLETED else 0
            if offs and total + need > max_arena:
                break
            offs.append(total + sh)
            total += need
        out.append((first, total, offs))
        first += len(offs)
    return out


def scattered(arena, recs, cut):
    """The caller's arena after every piece of `cut` was staged, changed by the device and scattered back, in order."""
    arena = bytearray(arena)
    for first, _, offs in cut:
        staged = [bytes(arena[off:off + ln]) if status == COMPLETED else b"" for status, off, ln, _ in recs[first:first + len(offs)]]
        for (status, off, ln, code), s in zip(recs[first:first + len(offs)], staged):
            if status == COMPLETED and code == NM_OK:
                arena[off:off + ln] = bytes(b ^ DEVICE for b in s)
    return bytes(arena)


def grid_list():
    """32 records, every length of LENS four times, one behind the other with 16 .. 31 bytes no record names between them,
    at residues that cover 0 .. 15; every fifth one is not completed (one of those points far outside the arena) and every
    second one comes back with a code that leaves it where it is."""
    recs, end = [], 0
    for i in range(32):
        ln, r = LENS[i % 8], (5 * i + 3 + 9 * (i // 8)) % 16
        off = ceil16(end) + 16 + r
        recs.append((OTHER if i % 5 == 4 else COMPLETED, off if i != 9 else 10 ** 12, ln, NM_OK if i % 2 == 0 else NM_OTHER))
        end = off + ln
    return recs, end + 7


def shared_list():
    """Two records on one string, two that overlap, a zero-length one at the arena's end, in an arena with unnamed bytes."""
    return [(COMPLETED, 33, 40, NM_OK), (COMPLETED, 33, 40, NM_OTHER), (COMPLETED, 100, 50, NM_OK), (OTHER, 0, 300, NM_OK),
            (COMPLETED, 120, 50, NM_OK), (COMPLETED, 256, 0, NM_OK), (COMPLETED, 239, 17, NM_OTHER), (COMPLETED, 33, 40, NM_OK)], 256


def all_cases():
    rng = random.Random("record-pieces")
    cases = []
    for recs, arena_bytes in (grid_list(), shared_list(), ([], 5), ([(OTHER, 7, 9, NM_OK)] * 4, 0)):
        arena = bytes(rng.choice(b"MXID") for _ in range(arena_bytes))
        for max_arena in MAX_ARENA:
            for max_records in MAX_RECORDS:
                for keep in (True, False):
                    cases.append((recs, arena, max_arena, max_records, keep))
    return cases


def run(driver, cases):
    """-> per case ([(first, n, bytes, [staged cigar_off], stage)], the arena afterwards)"""
    text = []
    for recs, arena, max_arena, max_records, keep in cases:
        text.append("%d %d %d %d %d\n%s\n" % (len(recs), len(arena), max_arena, max_records, keep, arena.hex() or "-"))
        text += ["%d %d %d %d\n" % r for r in recs]
    r = subprocess.run([driver], input="".join(text), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    out = []
    for _ in cases:
        cut = []
        for ln in lines:
            if ln == "arena":
                break
            _, first, n, total = ln.split()
            offs = [int(x) for x in next(lines).split()]
            stage = next(lines)
            cut.append((int(first), int(n), int(total), offs, b"" if stage == "-" else bytes.fromhex(stage)))
        after = next(lines)
        out.append((cut, b"" if after == "-" else bytes.fromhex(after)))
    assert next(lines, None) is None
    return out


def test_the_inputs_reach_every_path():
    """From the restated rule alone: several pieces, a piece of one record over its budget, every residue."""
    cases = all_cases()
    cuts = [pieces(recs, max_arena, max_records or 1 << 20, keep) for recs, _, max_arena, max_records, keep in cases]
    assert any(len(cut) >= 3 for cut in cuts)
    assert any(len(offs) == 1 and total > c[2] for c, cut in zip(cases, cuts) for _, total, offs in cut)
    assert any(len(offs) > 3 for cut in cuts for _, _, offs in cut) and any(len(cut) == 1 and len(c[0]) > 1 for c, cut in zip(cases, cuts))
    assert {off % 16 for status, off, ln, _ in grid_list()[0] if status == COMPLETED and ln} == set(range(16))
    assert {ln for status, _, ln, _ in grid_list()[0] if status == COMPLETED} == set(LENS)


def test_pieces_and_scatter_back(driver):
    cases = all_cases()
    for (recs, arena, max_arena, max_records, keep), (cut, after) in zip(cases, run(driver, cases)):
        where = (len(recs), max_arena, max_records, keep)
        cap = max_records or 1 << 20
        want = pieces(recs, max_arena, cap, keep)
        assert [(first, total, offs) for first, _, total, offs, _ in cut] == want, where
        # the pieces partition [0, n_all) in order
        at = 0
        for first, n, total, offs, stage in cut:
            assert first == at and n >= 1 and len(offs) == n and len(stage) == total and total % 16 == 0, where
            at += n
            assert n <= cap and (n == 1 or total <= max_arena), where
            # every completed record owns a slot of whole 16 bytes that holds its bytes at its residue; the slots lie one
            # behind the other and fill the piece, so a record that is not completed takes nothing; all else is zero
            covered, end = bytearray(total), 0
            before = scattered(arena, recs, [c for c in want if c[0] < first])  # (the pieces before this one have come back)
            for (status, off, ln, _), at_stage in zip(recs[first:first + n], offs):
                if status != COMPLETED:
                    continue
                sh = off % 16 if keep else 0
                assert at_stage % 16 == sh and at_stage - sh == end, (where, first)
                end += ceil16(sh + ln)
                assert stage[at_stage:at_stage + ln] == before[off:off + ln], (where, first)
                covered[at_stage:at_stage + ln] = b"\1" * ln
            assert end == total, (where, first)
            assert all(c or b == 0 for c, b in zip(covered, stage)), (where, first)
        assert at == len(recs), where
        # scatter-back: the flagged strings hold what the device left, every other byte of the caller's arena is as it was
        assert after == scattered(arena, recs, want), where
        flagged = bytearray(len(arena))
        for status, off, ln, code in recs:
            if status == COMPLETED and code == NM_OK:
                flagged[off:off + ln] = b"\1" * ln
        assert all(f or a == b for f, a, b in zip(flagged, after, arena)), where
        assert not any(flagged) or after != arena, where
