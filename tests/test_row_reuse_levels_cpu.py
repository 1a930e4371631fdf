"""CPU test of who may take rows from a top-level search's archive (awvrr::take_dir in allwave_amd/csrc/row_reuse.hpp, DESIGN.md
4.28): a stand-alone driver around the header, built with the system C++ compiler under AddressSanitizer and UBSan.  The rule
is restated here by a task's path below the top-level search: the chain of left halves shares its origin and begin component
and takes forward rows, the chain of right halves shares its end and takes reverse rows, nothing else takes anything; with the
level-1 pin only the two halves themselves do."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LV_ALL, LV_ONE = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("row_reuse_levels") / "row_reuse_levels_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), os.path.join(ROOT, "tests", "row_reuse_levels_driver.cpp"),
                           "-o", exe])
    return exe


def ask(driver, root, tasks, levels):
    lines = ["take %d %d %d %d %d  %d %d %d %d %d %d  %d" % (tuple(root) + tuple(t) + (levels,)) for t in tasks]
    r = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]


def tree(rng, plen, tlen, depth, comps=(0, 1, 2, 3, 4)):
    """The tasks below a top-level search, as the kernel's DFS hands them down (left half first), with their paths:
    a task (pb, pe, tb, te, cb, ce) whose search breaks at (bv, bh) in component c becomes (pb, pb + bv, tb, tb + bh, cb, c)
    and (pb + bv, pe, tb + bh, te, c, ce).  Every breakpoint lies in the middle half of its task.  Returns (root id, [(path, task)])."""
    out = []

    def split(t, path):
        pb, pe, tb, te, cb, ce = t
        if len(path) == depth or pe - pb < 2 or te - tb < 2:
            return None
        bv, bh, c = rng.randrange((pe - pb) // 4, 3 * (pe - pb) // 4 + 1), rng.randrange((te - tb) // 4, 3 * (te - tb) // 4 + 1), rng.choice(comps)
        for side, child in (("L", (pb, pb + bv, tb, tb + bh, cb, c)), ("R", (pb + bv, pe, tb + bh, te, c, ce))):
            out.append((path + side, child))
            split(child, path + side)
        return bv, bh, c

    bv, bh, c = split((0, plen, 0, tlen, 0, 0), "")
    return (plen, tlen, bv, bh, c), out


def expected(path, levels):
    if path in ("L", "R"):
        return (0 if path == "L" else 1, 1)
    if levels == LV_ALL and set(path) == {"L"}:
        return (0, 0)
    if levels == LV_ALL and set(path) == {"R"}:
        return (1, 0)
    return (-1, 0)


@pytest.mark.parametrize("comps", [(0,), (1, 2, 3, 4), (0, 1, 2, 3, 4)])
def test_four_level_trees(driver, comps):
    """Every task of 40 random four-level trees, breakpoints in M only, in gap components only, and mixed."""
    rng = random.Random("row-reuse-levels/%s" % (comps,))
    for _ in range(40):
        root, tasks = tree(rng, rng.randrange(1024, 20000), rng.randrange(1024, 20000), 4, comps)
        for levels in (LV_ALL, LV_ONE):
            got = ask(driver, root, [t for _, t in tasks], levels)
            assert got == [expected(p, levels) for p, _ in tasks], (root, levels)
        paths = [p for p, _ in tasks]
        assert paths[:4] == ["L", "LL", "LLL", "LLLL"] and "RRRR" in paths  # (the order the kernel runs them in: the archive is the running unit's throughout)


def test_mismatches(driver):
    """The archive's corner with another component, the component at another corner, and a task in the middle."""
    root = (1000, 900, 400, 380, 3)
    cases = [((0, 200, 0, 190, 3, 0), (-1, 0)),      # begins at the origin, but inside a gap
             ((0, 200, 1, 190, 0, 0), (-1, 0)),      # M, one text base off the origin
             ((1, 200, 0, 190, 0, 0), (-1, 0)),
             ((700, 1000, 600, 900, 0, 2), (-1, 0)),  # ends at the end, but inside a gap
             ((700, 1000, 600, 899, 0, 0), (-1, 0)),
             ((700, 999, 600, 900, 0, 0), (-1, 0)),
             ((400, 700, 380, 600, 3, 0), (-1, 0)),   # the right half's left half: neither corner
             ((0, 400, 0, 380, 0, 3), (0, 1)),        # the left half itself
             ((400, 1000, 380, 900, 3, 0), (1, 1)),   # the right half itself
             ((0, 400, 0, 380, 0, 1), (0, 0)),        # the left half's box with another end component: the end is no part of the equality
             ((0, 1000, 0, 900, 0, 0), (0, 0))]       # both corners (a degenerate child over the whole rectangle): forward
    got = ask(driver, root, [t for t, _ in cases], LV_ALL)
    assert got == [w for _, w in cases]
    got = ask(driver, root, [t for t, _ in cases], LV_ONE)
    assert got == [w if w[1] else (-1, 0) for _, w in cases]


FR_A, FR_B, FR_SHARED = 0, 1, 2


def test_frames_of_a_non_mirror_split(driver):
    """A replay of the task loop's frames.  A twin unit's top-level search is shared; while breakpoints mirror, its tasks stay
    shared; a search with two breakpoints that are no mirror images hands down four tasks, A's two in A's frame and B's two in
    B's (pattern and text swapped).  The archive was recorded in the shared frame, which is A's: shared and A tasks may take,
    B tasks never.  A unit that is run again per orientation records in that orientation's frame, and only its own tasks take."""
    def frames(root, task):
        r = subprocess.run([driver], input="frame %d %d\n" % (root, task), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == ""
        return int(r.stdout)

    # the unit's DFS: shared top level -> shared halves -> the left half splits four ways (A, B, A, B), the right half stays shared
    dfs = [("L", FR_SHARED), ("LL/A", FR_A), ("LL/B", FR_B), ("LR/A", FR_A), ("LR/B", FR_B), ("R", FR_SHARED), ("RR", FR_SHARED)]
    assert [frames(FR_SHARED, f) for _, f in dfs] == [1, 1, 0, 1, 0, 1, 1]
    assert [frames(FR_A, f) for f in (FR_A, FR_B, FR_SHARED)] == [1, 0, 0]   # a lone pair, or A run again alone
    assert [frames(FR_B, f) for f in (FR_A, FR_B, FR_SHARED)] == [0, 1, 0]   # B run again alone: B's frame throughout
