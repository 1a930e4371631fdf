"""CPU test of the twin pairing (allwave_amd/csrc/twin_plan.hpp): a stand-alone driver around the header, built with the
system C++ compiler under AddressSanitizer and UBSan, pairs the entries of a list that exercises every rule and of
config 2's all-pairs list."""
import os
import shutil
import subprocess

import pytest

import twin_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("twin_plan") / "twin_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), os.path.join(ROOT, "tests", "twin_plan_driver.cpp"),
                           "-o", exe])
    return exe


def run(driver, entries):
    text = "".join("%d %d %d\n" % tuple(e) for e in entries)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_pairing_list(driver):
    E = TC.PAIRING_LIST
    units = run(driver, E)
    TC.check_plan(E, units)
    by_first = dict(units)
    twins = {(E[f][:2]): E[w][:2] for f, w in units if w >= 0}
    assert twins == {(0, 1): (1, 0), (2, 3): (3, 2), (1, 2): (2, 1), (0, 6): (6, 0), (7, 8): (8, 7), (9, 10): (10, 9),
                     (11, 9): (9, 11), (5, 0): (0, 5)}
    for i, (q, t, rc) in enumerate(E):  # the excluded kinds stay single
        if rc or q == t:
            assert by_first.get(i) == -1, (i, E[i])
    assert by_first[E.index((0, 2, 0))] == -1 and by_first[E.index((3, 4, 0))] == -1 and by_first[E.index((4, 1, 0))] == -1
    assert [by_first[i] for i in (7, 8)] == [-1, -1]  # (4, 5) twice, no twin
    # (2, 3) twice and (3, 2) once: exactly one copy has the twin
    assert sorted(by_first.get(i, "twin") for i in (4, 5)) == [-1, 6]
    assert run(driver, []) == []


def test_all_pairs_of_256(driver):
    from allwave_amd import synth
    E = [(int(p[0]), int(p[1]), 0) for p in synth.all_pairs(256)]
    assert len(E) == 65280
    units = run(driver, E)
    assert len(units) == 32640 and all(w >= 0 for _, w in units)
    TC.check_plan(E, units)
    # the same list in another order (most-expensive-first reorders entries before the pairing sees them)
    E2 = E[::-1][1000:] + E[::-1][:1000]
    units = run(driver, E2)
    assert len(units) == 32640
    TC.check_plan(E2, units)
