"""CPU test of the row archive's arithmetic (allwave_amd/csrc/row_reuse.hpp): a stand-alone driver around the
header, built with the system C++ compiler under AddressSanitizer and UBSan.  The layout is compared with a restatement
here; an archive of exactly the planned size is filled the way a recording search fills it, with the widest hull a row can
have at its score, and read back the way a taking search with another column origin reads it -- any access outside the
buffer stops the driver; the box test, the boundary choice and the host's pass plan are asked case by case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_WORDS, P_WORDS, NCOMP = 16, 4, 5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("row_reuse") / "row_reuse_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), os.path.join(ROOT, "tests", "row_reuse_driver.cpp"),
                           "-o", exe])
    return exe


def ask(driver, lines):
    r = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def layout(P, T, nid):
    """row_reuse.hpp's Layout, restated: header, pass table, per-score hulls, rows."""
    scores = P * T
    cols = (2 * (scores + 8) + 8 + 3) & ~3
    table = H_WORDS * 4
    meta = table + 2 * P * P_WORDS * 4
    rows = (meta + 2 * scores * NCOMP * 4 + 15) & ~15
    total = (rows + 2 * P * (T + nid) * cols * 2 + 255) & ~255
    return cols, table, meta, rows, total


SHAPES = [(4, 15, 6), (47, 15, 6), (7, 5, 6), (9, 4, 4), (5, 3, 2), (33, 2, 4), (273, 15, 6)]


def test_layout(driver):
    out = ask(driver, ["layout %d %d %d" % s for s in SHAPES])
    for s, line in zip(SHAPES, out):
        got = tuple(int(x) for x in line.split())
        assert got == layout(*s), s
        cols, table, meta, rows, total = got
        assert cols % 4 == 0 and rows % 16 == 0 and total % 256 == 0 and table < meta < rows < total


def test_archive_round_trip_stays_inside_its_buffer(driver):
    """Recording and taking origins of every residue mod 4, far apart and equal, positive and negative."""
    cmds, want = [], []
    for (P, T, nid), (e1, e2) in zip(SHAPES[:6], ((2, 1), (2, 1), (2, 1), (2, 0), (1, 0), (2, 0))):
        assert 2 * e1 + 2 * e2 == nid
        for kp, kc in ((-5230, -5230), (-5231, -1777), (-5232, -1200), (-5233, -3001), (-700, -5230), (3, -2)):
            cmds.append("roundtrip %d %d %d %d %d %d %d" % (P, T, nid, e1, e2, kp, kc))
            want.append("ok %d" % (2 * sum(2 * s + 1 for s in range(1, P * T + 1))))
    assert ask(driver, cmds) == want


def test_box_test(driver):
    cases = [((2000, 1800, 1000, 1000), 1), ((2001, 1800, 1000, 1000), 0), ((2000, 2001, 1000, 1000), 0), ((0, 0, 1, 1), 1),
             ((3, 2, 1, 1), 0), ((2, 3, 1, 1), 0), ((1999, 401, 200, 1000), 0), ((1999, 400, 200, 1000), 1)]
    out = ask(driver, ["box %d %d %d %d" % c for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]


def test_boundary_choice(driver):
    """A child's pass is taken only when it is as long as the archive's passes, starts on one of their boundaries and is there."""
    cases = [((10, 15, 6, 10, 0, 15), 0), ((10, 15, 6, 10, 15, 15), 1), ((10, 15, 6, 10, 135, 15), 9), ((10, 15, 6, 10, 150, 15), -1),
             ((10, 15, 6, 3, 45, 15), -1), ((10, 15, 6, 3, 30, 15), 2), ((10, 15, 6, 10, 30, 10), -1), ((10, 15, 6, 10, 30, 5), -1),
             ((10, 15, 6, 10, 20, 15), -1), ((10, 15, 6, 0, 0, 15), -1), ((10, 4, 4, 10, 8, 4), 2), ((10, 4, 4, 10, 8, 3), -1)]
    out = ask(driver, ["pass %d %d %d %d %d %d" % c for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]


def test_pass_plan(driver):
    """maxsum / 28 scores in whole passes, at most 4096 scores; three quarters as many until the slots fit; none below 4."""
    def plan(maxsum, T, nid, nslots, avail):
        if T < 2 or nslots <= 0:
            return 0
        p = min(maxsum // 28, 4096) // T
        while p >= 4 and layout(p, T, nid)[4] * nslots > avail:
            p = p * 3 // 4
        return p if p >= 4 else 0
    cases = [(20000, 15, 6, 4096, 100 << 30), (20000, 15, 6, 4096, 8 << 30), (20000, 15, 6, 4096, 1 << 20), (7000, 15, 6, 2, 1 << 30),
             (1500, 15, 6, 16, 1 << 30), (400000, 15, 6, 64, 1 << 40), (7000, 4, 4, 2, 1 << 30), (7000, 1, 2, 2, 1 << 30),
             (7000, 15, 6, 0, 1 << 30), (7000, 15, 6, 2, 0)]
    out = ask(driver, ["plan %d %d %d %d %d" % c for c in cases])
    assert [int(x) for x in out] == [plan(*c) for c in cases]
    assert int(out[0]) == 47 and int(out[2]) == 0 and int(out[4]) == 0 and int(out[5]) == 273
