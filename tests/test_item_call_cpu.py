"""CPU test of the prologue of a call on caller-supplied records with slices (allwave_amd/csrc/item_call.hpp): a
stand-alone driver, built with the system C++ compiler under AddressSanitizer and UBSan, resolves small calls; its output is
checked against the rule restated here -- resolve().  The checks come in an order a caller can observe: every range or index of
the whole list; then, record by record, the op bytes' place in the arena and then the slice; the length limit last."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPLETED, OTHER = 0, 1           # awv_result.status: AWV_ST_COMPLETED, any other
RANGE, INDEX, ARENA, SLICE = 1, 2, 3, 4  # ItemCall::Refusal
LENS = (0, 1, 17, 40)
ARENA_BYTES = 200
MAX_COLUMNS = 1 << 30
WORDS = {RANGE: "who: range %d names a sequence index or an interval out of range", INDEX: "who: sequence index out of range",
         ARENA: "who: a record's op bytes lie outside the CIGAR arena",
         SLICE: "who: slice %d does not lie inside its op string, or skips a negative number of bases"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("item_call") / "item_call_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "item_call_driver.cpp"), "-o", exe])
    return exe


def resolve(lens, ranges, lst, recs, arena_bytes, slices):
    """The rule.  lst: (q, t, rc) or (q, t, rc, q_beg, q_end, t_beg, t_end); recs: (status, cigar_off, cigar_len); slices: None or
    (col_beg, col_end, q_skip, t_skip).  -> ("refused", why, at) or ("ok", [(q, t, rc, pb, pe, tb, te, status, off, len)])."""
    n, spans = len(lens), []
    for i, e in enumerate(lst):
        q, t, rc = e[:3]
        if not (0 <= q < n and 0 <= t < n):
            return ("refused", RANGE if ranges else INDEX, i)
        qb, qe, tb, te = e[3:] if ranges else (0, lens[q], 0, lens[t])
        if ranges and not (0 <= qb <= qe <= lens[q] and 0 <= tb <= te <= lens[t]):
            return ("refused", RANGE, i)
        spans.append([lens[q] - qe, lens[q] - qb, tb, te] if rc else [qb, qe, tb, te])
    for i, (status, off, ln) in enumerate(recs):
        if status == COMPLETED and off + ln > arena_bytes:
            return ("refused", ARENA, i)
        if slices is not None:
            cb, ce, qs, ts = slices[i]
            if qs < 0 or ts < 0 or (status == COMPLETED and not cb <= ce <= ln):
                return ("refused", SLICE, i)
    out = []
    for i, (e, (status, off, ln)) in enumerate(zip(lst, recs)):
        pb, pe, tb, te = spans[i]
        if slices is not None and status == COMPLETED:
            cb, ce, qs, ts = slices[i]
            off, ln, pb, tb = off + cb, ce - cb, min(pb + qs, pe + 1), min(tb + ts, te + 1)
        out.append((e[0], e[1], 1 if e[2] else 0, pb, pe, tb, te, status, off, ln))
    return ("ok", out)


def too_long(rows, max_columns):
    return next((i for i, r in enumerate(rows) if r[7] == COMPLETED and r[9] > max_columns), -1)


# ---- the cases: (ranges, list, records, arena_bytes, slices, max_columns) ----------------------------------------------------

SOUND_PAIRS = [(3, 2, 0), (2, 3, 1), (1, 0, 0), (0, 0, 1), (3, 3, 0)]
SOUND_RANGES = [(3, 2, 0, 5, 40, 0, 17),   # to the query's end
                (3, 2, 1, 5, 38, 3, 3),    # the other strand; an empty text interval
                (2, 3, 1, 17, 17, 40, 40),  # both empty, at the sequences' ends
                (0, 1, 0, 0, 0, 0, 1),     # on the sequence without a base
                (0, 0, 1, 0, 0, 0, 0)]
# residues 0, 1 and 15; one string that ends exactly with the arena; one record that is not completed and points far outside
SOUND_RECS = [(COMPLETED, 16, 30), (COMPLETED, 49, 12), (COMPLETED, 95, 0), (OTHER, 10 ** 12, 4000000000), (COMPLETED, 160, 40)]
SOUND_SLICES = [(0, 30, 0, 0),     # full
                (5, 5, 0, 0),      # empty
                (0, 0, 100, 3),    # a skip that runs past its sequence: pb = pe + 1
                (4000000000, 5, 0, 0),  # not completed: any columns will do
                (3, 40, 2, 70)]


def faulty(ranges, what, i):
    """The sound call with one fault at record i, as (list, records, slices) edits."""
    lst, recs, slices = list(SOUND_RANGES if ranges else SOUND_PAIRS), list(SOUND_RECS), list(SOUND_SLICES)
    if what == "list":
        lst[i] = (lst[i][0], 4) + lst[i][2:]
    elif what == "arena":
        recs[i] = (COMPLETED, ARENA_BYTES - 10, 11)  # one byte past the arena
    else:
        recs[i] = (COMPLETED, 16, 30)
        slices[i] = (0, 31, 0, 0)  # col_end = len + 1
    return lst, recs, slices


def merge(ranges, faults):
    lst, recs, slices = list(SOUND_RANGES if ranges else SOUND_PAIRS), list(SOUND_RECS), list(SOUND_SLICES)
    for what, i in faults:
        l2, r2, s2 = faulty(ranges, what, i)
        lst[i], recs[i], slices[i] = l2[i], r2[i], s2[i]
    return lst, recs, slices


def all_cases():
    cases = []
    for ranges in (False, True):
        lst = SOUND_RANGES if ranges else SOUND_PAIRS
        cases.append((ranges, lst, SOUND_RECS, ARENA_BYTES, None, MAX_COLUMNS))
        cases.append((ranges, lst, SOUND_RECS, ARENA_BYTES, SOUND_SLICES, MAX_COLUMNS))
        cases.append((ranges, [], [], 0, None, MAX_COLUMNS))
        # the length limit, as a small number: on the records as they are, and on the slices (the first record's slice is its whole
        # string of 30 columns, the last one's has 37)
        for limit in (40, 39, 29, 0):
            cases.append((ranges, lst, SOUND_RECS, ARENA_BYTES, None, limit))
        for limit in (37, 36, 29):
            cases.append((ranges, lst, SOUND_RECS, ARENA_BYTES, SOUND_SLICES, limit))
        # one fault each: the arena's bounds
        for rec in ((COMPLETED, ARENA_BYTES, 0), (COMPLETED, ARENA_BYTES + 1, 0), (COMPLETED, ARENA_BYTES - 10, 11), (COMPLETED, 1 << 63, 1),
                    (COMPLETED, (1 << 64) - 1, 2), (OTHER, ARENA_BYTES, 1)):
            cases.append((ranges, lst[:1], [rec], ARENA_BYTES, None, MAX_COLUMNS))
        # ... the slices
        for sl in ((6, 5, 0, 0), (0, 31, 0, 0), (30, 30, 0, 0), (0, 30, -1, 0), (0, 30, 0, -1), (0, 0, 2147483647, 2147483647)):
            cases.append((ranges, lst[:1], [(COMPLETED, 16, 30)], ARENA_BYTES, [sl], MAX_COLUMNS))
            cases.append((ranges, lst[:1], [(OTHER, 16, 30)], ARENA_BYTES, [sl], MAX_COLUMNS))
        # two and three different faults at different indices, in every order of index
        for kinds in (("list", "arena"), ("list", "slice"), ("arena", "slice"), ("list", "arena", "slice")):
            for where in itertools.permutations((0, 2, 4), len(kinds)):
                l2, r2, s2 = merge(ranges, list(zip(kinds, where)))
                cases.append((ranges, l2, r2, ARENA_BYTES, s2, MAX_COLUMNS))
    # one fault each: the list
    for p in ((-1, 0, 0), (0, -1, 0), (4, 0, 0), (0, 4, 1)):
        cases.append((False, [SOUND_PAIRS[0], p], SOUND_RECS[:2], ARENA_BYTES, None, MAX_COLUMNS))
    for r in ((3, 2, 0, 0, 41, 0, 17), (3, 2, 1, 0, 40, 0, 18), (3, 2, 0, -1, 40, 0, 17), (3, 2, 0, 6, 5, 0, 17), (3, 2, 1, 0, 40, 9, 8), (0, 1, 0, 0, 1, 0, 1),
              (1, 0, 1, 0, 1, 0, 1), (4, 2, 0, 0, 0, 0, 0), (3, -1, 0, 0, 0, 0, 0)):
        cases.append((True, [SOUND_RANGES[0], r], SOUND_RECS[:2], ARENA_BYTES, None, MAX_COLUMNS))
    return cases


def run(driver, cases):
    text = []
    for ranges, lst, recs, arena_bytes, slices, limit in cases:
        text.append("%d %s\n%d %d %d %d %d\n" % (len(LENS), " ".join(map(str, LENS)), ranges, len(lst), arena_bytes, slices is not None, limit))
        text += [" ".join(map(str, row)) + "\n" for rows in (lst, recs, slices or []) for row in rows]
    r = subprocess.run([driver], input="".join(text), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    out = []
    for ranges, lst, recs, arena_bytes, slices, limit in cases:
        head = next(lines).split(" ", 3)
        if head[0] == "refused":
            out.append(("refused", int(head[1]), int(head[2]), head[3]))
            continue
        assert head == ["ok", "1"]  # the records are the caller's own without slices, copies with them
        rows = [tuple(int(x) for x in next(lines).split()) for _ in lst]
        out.append(("ok", rows, int(next(lines).split()[1])))
    assert next(lines, None) is None
    return out


def test_the_inputs_reach_every_branch():
    """From the restated rule alone."""
    cases = all_cases()
    got = [resolve(LENS, c[0], c[1], c[2], c[3], c[4]) for c in cases]
    for ranges in (False, True):
        mine = [g for c, g in zip(cases, got) if c[0] == ranges]
        assert {g[1] for g in mine if g[0] == "refused"} == {RANGE if ranges else INDEX, ARENA, SLICE}
        assert {g[2] for g in mine if g[0] == "refused"} >= {0, 2, 4}
        assert any(g[0] == "ok" and any(r[3] == r[4] + 1 for r in g[1]) for g in mine)  # a skip past its sequence
    assert {off % 16 for _, off, _ in SOUND_RECS[:3]} == {0, 1, 15} and SOUND_RECS[4][1] + SOUND_RECS[4][2] == ARENA_BYTES
    limits = [(c[5], too_long(g[1], c[5])) for c, g in zip(cases, got) if g[0] == "ok" and c[5] != MAX_COLUMNS]
    assert {at for _, at in limits} == {-1, 0, 4}


def test_the_prologue_resolves_and_refuses_by_the_rule(driver):
    cases = all_cases()
    for (ranges, lst, recs, arena_bytes, slices, limit), got in zip(cases, run(driver, cases)):
        want = resolve(LENS, ranges, lst, recs, arena_bytes, slices)
        where = (ranges, lst, recs, slices, limit)
        if want[0] == "refused":
            words = WORDS[want[1]] % want[2] if "%d" in WORDS[want[1]] else WORDS[want[1]]
            assert got == want + (words,), where
        else:
            assert got == want + (too_long(want[1], limit),), where


def test_which_of_several_faults_wins():
    """The order itself, spelled out: a fault of the list wins wherever it stands; of the other two the lower index wins."""
    for ranges in (False, True):
        for a, b in itertools.permutations((0, 2, 4), 2):
            for other in ("arena", "slice"):
                l2, r2, s2 = merge(ranges, [("list", a), (other, b)])
                assert resolve(LENS, ranges, l2, r2, ARENA_BYTES, s2)[1:] == (RANGE if ranges else INDEX, a)
            l2, r2, s2 = merge(ranges, [("arena", a), ("slice", b)])
            assert resolve(LENS, ranges, l2, r2, ARENA_BYTES, s2)[1:] == ((ARENA, a) if a < b else (SLICE, b))
