"""CPU test of which entries of an engine call reach a run's consumer, and as what (allwave_amd/csrc/host/delivery.hpp,
DESIGN.md 4.26): a stand-alone driver, built with the system C++ compiler under AddressSanitizer and UBSan against that
header alone, runs described sink calls through deliver().  Its output -- the kept records, strands, pair-list indices and
clips, and the counters -- is checked against the rule restated here, model(), and segment_record() field by field."""
import collections
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPLETED, CAPACITY, MAX_STEPS, ABOVE_BOUND = 0, 1, 3, 4   # awv_result.status (AWV_ST_*)
CL_OK, CL_SKIPPED, CL_EMPTY, CL_BAD_OP = 0, 1, 2, 3        # awv_clip_result.code, awv_split_index.code (AWV_CL_*)
DIV, MIN_SCORE = 0.25, 10
# (#M, #X, #I, #D) of a full record: well under DIV; E == DIV * columns exactly (5 of 20: kept); just over it (5 of 19: dropped)
LOW, EXACT, ON, OVER = (18, 1, 0, 1), (20, 0, 0, 0), (15, 2, 2, 1), (14, 2, 2, 1)
BELOW, EQUAL, ABOVE = MIN_SCORE - 1, MIN_SCORE, MIN_SCORE + 1
# mode: (bounded, divergence bound, clipping, splitting)
MODES = {"plain": (0, 0, 0, 0), "penalty": (1, 0, 0, 0), "divergence": (1, 1, 0, 0), "clip": (0, 0, 1, 0), "split": (0, 0, 0, 1),
         "bounds+clip": (1, 1, 1, 0), "bounds+split": (1, 1, 0, 1)}

# The hand-built list: status, counts, by_div, rev, the clip's code and score, the split index's code and count.
HAND = [
    (COMPLETED, LOW, 0, 0, CL_OK, ABOVE, CL_OK, 1),
    (COMPLETED, LOW, 0, 0, CL_OK, EQUAL, CL_OK, 3),
    (COMPLETED, LOW, 0, 1, CL_OK, BELOW, CL_EMPTY, 0),
    (ABOVE_BOUND, (0, 0, 0, 0), 0, 0, CL_SKIPPED, 0, CL_SKIPPED, 0),
    (ABOVE_BOUND, (0, 0, 0, 0), 1, 1, CL_SKIPPED, 0, CL_SKIPPED, 0),
    (CAPACITY, (0, 0, 0, 0), 0, 0, CL_SKIPPED, 0, CL_SKIPPED, 0),
    (COMPLETED, ON, 1, 0, CL_OK, ABOVE, CL_OK, 3),
    (COMPLETED, OVER, 1, 0, CL_OK, ABOVE, CL_OK, 1),
    (COMPLETED, LOW, 0, 0, CL_EMPTY, 0, CL_OK, 1),
    (COMPLETED, LOW, 0, 1, CL_BAD_OP, 0, CL_BAD_OP, 0),
    (COMPLETED, LOW, 1, 0, CL_OK, ABOVE, CL_OK, 3),
    (MAX_STEPS, (0, 0, 0, 0), 1, 1, CL_SKIPPED, 0, CL_SKIPPED, 0),
    (COMPLETED, ON, 0, 1, CL_OK, BELOW, CL_EMPTY, 0),
    (COMPLETED, OVER, 0, 0, CL_EMPTY, 0, CL_OK, 3),
    (COMPLETED, EXACT, 0, 0, CL_OK, EQUAL, CL_OK, 1),
    (COMPLETED, LOW, 0, 1, CL_OK, ABOVE, CL_OK, 3),
]
assert len(HAND) == 16

Entry = collections.namedtuple("Entry", "status penalty off length counts rev by_div clip split segs slack")


def a_clip(code, score, length, salt):
    """(code, score, col_beg, col_end, q_skip, t_skip, #M, #X, #I, #D, penalty): every field its own value, #I != #D."""
    if code != CL_OK:
        return (code, 0, salt % 3 if code == CL_BAD_OP else 0, salt % 3 if code == CL_BAD_OP else 0, 0, 0, 0, 0, 0, 0, 0)
    beg = salt % 3
    return (CL_OK, score, beg, max(beg, length - salt % 2), 3 + salt % 5, 9 + salt % 4, 6 + salt % 7, 1 + salt % 2, 2 + salt % 3, 5 + salt % 3, 17 + salt)


def entry(row, k):
    status, counts, by_div, rev, ccode, cscore, scode, scount = row
    length = sum(counts)
    segs = [a_clip(CL_OK, MIN_SCORE + j, length, 11 * k + j + 1) for j in range(scount)]
    return Entry(status, 3 * sum(counts[1:]) + (7 if status == ABOVE_BOUND else 0), 1000 * k + 13, length, counts, rev, by_div,
                 a_clip(ccode, cscore, length, k), (scode, scount), segs, k % 3)


def random_list(rng):
    """0 to 24 entries over the hand list's alphabets."""
    rows = []
    for _ in range(rng.randrange(25)):
        status = rng.choice((COMPLETED, COMPLETED, COMPLETED, ABOVE_BOUND, CAPACITY))
        if status != COMPLETED:
            rows.append((status, (0, 0, 0, 0), rng.randrange(2), rng.randrange(2), CL_SKIPPED, 0, CL_SKIPPED, 0))
            continue
        ccode = rng.choice((CL_OK, CL_OK, CL_OK, CL_EMPTY, CL_BAD_OP))
        scount = rng.choice((0, 1, 3))
        rows.append((COMPLETED, rng.choice((LOW, EXACT, ON, OVER)), rng.randrange(2), rng.randrange(2), ccode,
                     rng.choice((BELOW, EQUAL, ABOVE)) if ccode == CL_OK else 0, CL_OK if scount else rng.choice((CL_EMPTY, CL_BAD_OP)), scount))
    return [entry(r, k) for k, r in enumerate(rows)]


def segment_record(e, cl):
    """awv_result fields (status penalty score cigar_off cigar_len #M #X #I #D q_end t_end) of e's record rewritten into cl."""
    _, _, beg, end, _, _, m, x, i, d, pen = cl
    return (e.status, pen, -pen, e.off + beg, end - beg, m, x, i, d, m + x + d, m + x + i)


def record(e):
    m, x, i, d = e.counts
    return (e.status, e.penalty, -e.penalty, e.off, e.length, m, x, i, d, m + x + d, m + x + i)


def model(entries, mode, idx, cuts, seen=None):
    """The five rules, entry by entry in call order -> ([kept per sink call], the nine counters).  kept: record + (rev, idx)
    [+ clip]; seen (optional) counts the outcomes."""
    bounded, use_div, clipping, splitting = mode
    st = dict.fromkeys(("above_penalty", "above_divergence", "c_pairs", "c_empty", "c_below", "s_pairs", "s_segments", "s_empty"), 0)
    seen = collections.Counter() if seen is None else seen
    calls = []
    for first, cnt in cuts:
        kept = []
        for k in range(first, first + cnt):
            e = entries[k]
            where = (e.rev, idx[k] if idx else k)
            m, x, i, d = e.counts
            if bounded and e.status == ABOVE_BOUND:                                   # rule 1
                by_div = e.by_div if use_div else 0  # (as case_text hands it over)
                st["above_divergence" if by_div else "above_penalty"] += 1
                seen["above bound, by_div %d" % by_div] += 1
                continue
            if bounded and use_div and e.status == COMPLETED:                       # rule 2
                edits = x + i + d
                if not float(edits) <= DIV * (edits + m):
                    st["above_divergence"] += 1
                    seen["just over the divergence bound"] += e.counts == OVER
                    continue
                seen["on the divergence bound"] += e.counts == ON
            if splitting:                                                            # rule 3
                if e.status != COMPLETED:
                    kept.append(record(e) + where + (CL_SKIPPED,) + (0,) * 10)
                    seen["split, not completed"] += 1
                    continue
                st["s_pairs"] += 1
                seen["split, count %d" % e.split[1]] += 1
                if e.split[0] != CL_OK:
                    st["s_empty"] += 1
                    continue
                st["s_segments"] += e.split[1]
                kept += [segment_record(e, s) + where + s for s in e.segs]
            elif clipping:                                                           # rule 4
                if e.status != COMPLETED:
                    kept.append(record(e) + where + e.clip)
                    seen["clip, not completed"] += 1
                    continue
                st["c_pairs"] += 1
                if e.clip[0] != CL_OK:
                    st["c_empty"] += 1
                    seen["clip, code not OK"] += 1
                elif e.clip[1] < MIN_SCORE:
                    st["c_below"] += 1
                    seen["clip, score below"] += 1
                else:
                    kept.append(segment_record(e, e.clip) + where + e.clip)
                    seen["clip, score equal" if e.clip[1] == MIN_SCORE else "clip, score above"] += 1
            else:                                                                    # rule 5
                kept.append(record(e) + where)
                seen["as it is, status %s" % ("completed" if e.status == COMPLETED else "other")] += 1
        calls.append(kept)
    return calls, (0, st["above_penalty"], st["above_divergence"], st["c_pairs"], st["c_empty"], st["c_below"], st["s_pairs"], st["s_segments"], st["s_empty"])


OUTCOMES = ("above bound, by_div 0", "above bound, by_div 1", "just over the divergence bound", "on the divergence bound", "split, not completed",
            "split, count 0", "split, count 1", "split, count 3", "clip, not completed", "clip, code not OK", "clip, score below", "clip, score equal",
            "clip, score above", "as it is, status completed", "as it is, status other")


def hand_cases():
    entries = [entry(r, k) for k, r in enumerate(HAND)]
    perm = [(7 * k + 3) % 16 for k in range(16)]
    assert sorted(perm) == list(range(16))
    for name, mode in MODES.items():
        for idx in (None, perm):
            for cuts in ([(0, 16)], [(k, 1) for k in range(16)], [(0, 5), (5, 0), (5, 11)]):
                yield entries, mode, idx, cuts


def random_cases():
    rng = random.Random("delivery")
    for _ in range(300):
        entries = random_list(rng)
        n = len(entries)
        for mode in MODES.values():
            idx = rng.sample(range(n), n) if rng.randrange(2) else None
            marks = sorted(rng.randrange(n + 1) for _ in range(rng.randrange(4)))
            yield entries, mode, idx, [(a, b - a) for a, b in zip([0] + marks, marks + [n])]


def case_text(entries, mode, idx, cuts):
    bounded, use_div, clipping, splitting = mode
    out = ["%d %d %d %d %d %r %d %d" % (len(entries), bounded, clipping, splitting, idx is not None, DIV if use_div else -1.0, MIN_SCORE, len(cuts))]
    slots = 0
    for k, e in enumerate(entries):
        by_div = e.by_div if use_div else 0  # (without a divergence bound no entry's bound derives from one)
        out.append(" ".join(map(str, (e.status, e.penalty, e.off, e.length) + e.counts + (e.rev, idx[k] if idx else 0, by_div) + e.clip + e.split + (slots,))))
        slots += len(e.segs) + e.slack  # (the engine's layout leaves a pair more slots than it fills)
    out.append(str(slots))
    for e in entries:
        out += [" ".join(map(str, s)) for s in e.segs] + [" ".join(map(str, a_clip(CL_EMPTY, 0, 0, 0)))] * e.slack
    return "\n".join(out + ["%d %d" % c for c in cuts]) + "\n"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("delivery") / "delivery_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "delivery_driver.cpp"), "-o", exe])
    return exe


def run(driver, cases):
    """-> per case (filters(), [kept per sink call], the nine counters)"""
    r = subprocess.run([driver], input="".join(case_text(*c) for c in cases), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = iter(r.stdout.splitlines())
    out = []
    for _, _, _, cuts in cases:
        head = next(lines).split()
        assert head[0] == "case"
        calls = []
        for _ in cuts:
            tag, kept = next(lines).split()
            assert tag == "call"
            calls.append([tuple(int(x) for x in next(lines).split()) for _ in range(int(kept))])
        stats = next(lines).split()
        assert stats[0] == "stats"
        out.append((int(head[1]), calls, tuple(int(x) for x in stats[1:])))
    assert next(lines, None) is None
    return out


def test_the_inputs_reach_every_outcome():
    """From the restated rule alone: the hand list meets every branch, the random lists every outcome at least 20 times."""
    seen = collections.Counter()
    for entries, mode, idx, cuts in hand_cases():
        calls, _ = model(entries, mode, idx, cuts, seen)
        if cuts == [(0, 5), (5, 0), (5, 11)]:
            assert calls[1] == []
    assert all(seen[o] for o in OUTCOMES), seen
    seen = collections.Counter()
    sizes = set()
    for entries, mode, idx, cuts in random_cases():
        model(entries, mode, idx, cuts, seen)
        sizes.add(len(entries))
    assert all(seen[o] >= 20 for o in OUTCOMES), seen
    assert {0, 24} <= sizes and any(c[1] == 0 for *_, cuts in random_cases() for c in cuts)


def check(driver, cases):
    for (entries, mode, idx, cuts), (filters, calls, stats) in zip(cases, run(driver, cases)):
        where = (mode, idx is not None, cuts)
        want_calls, want_stats = model(entries, mode, idx, cuts)
        assert filters == int(any(mode)), where
        assert calls == want_calls, where
        assert stats == want_stats, where  # (BoundStats.pairs is the batch preparation's to count, not the sink's)
        for (first, cnt), kept in zip(cuts, calls):
            assert cnt or not kept, where  # (an empty sink call delivers nothing)
        if not any(mode):  # a run without a setting: every entry, as it is, in order
            assert [k[:11] for c in calls for k in c] == [record(e) for first, cnt in cuts for e in entries[first:first + cnt]], where


def test_hand_list(driver):
    cases = list(hand_cases())
    assert len(cases) == 7 * 2 * 3
    check(driver, cases)
    # an empty sink call counts nothing either: the counters of the 5 / 0 / 11 cut are those of the single call
    got = run(driver, cases)
    for k in range(0, len(cases), 3):
        assert got[k][2] == got[k + 1][2] == got[k + 2][2]
        assert [x for c in got[k][1] for x in c] == [x for c in got[k + 1][1] for x in c] == [x for c in got[k + 2][1] for x in c]


def test_random_lists(driver):
    check(driver, list(random_cases()))


def test_segment_record_field_by_field(driver):
    """One finished pair through a clipping call: every field of the delivered record, by name."""
    e = entry((COMPLETED, LOW, 0, 1, CL_OK, ABOVE, CL_OK, 1), 5)
    code, score, beg, end, q_skip, t_skip, m, x, i, d, pen = e.clip
    assert code == CL_OK and beg > 0 and end < e.length and len({m, x, i, d}) == 4 and pen != e.penalty
    (_, calls, _), = run(driver, [([e], MODES["clip"], None, [(0, 1)])])
    (got,), = calls
    names = "status penalty score cigar_off cigar_len num_matches num_mismatches num_ins num_del q_end t_end".split()
    assert dict(zip(names, got)) == {"status": COMPLETED, "penalty": pen, "score": -pen, "cigar_off": e.off + beg, "cigar_len": end - beg,
                                     "num_matches": m, "num_mismatches": x, "num_ins": i, "num_del": d, "q_end": m + x + d, "t_end": m + x + i}
    assert got[11:13] == (1, 0) and got[13:] == e.clip  # the strand, the pair-list index, the clip handed on unchanged
