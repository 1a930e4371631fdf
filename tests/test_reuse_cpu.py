"""CPU tests of the reuse lists (tests/reuse_cases.py): that the traps are traps, from the references alone.  Every list's
processing order at one workgroup is its list order; every adjacency the GPU half relies on is present, the kinds decided
by the host yardsticks (scan records) and by the oracle (pairs); and for every carry trap a plain model of the leak -- B
scanned from the state A left -- gives an answer for B that differs from the yardstick's, which is what makes
tests/test_gpu_reuse.py fail on a kernel that forgets a reset."""
import random
import re

import numpy as np
import pytest

import clip_cases as K
import repeats
import reuse_cases as RC
import twin_cases as TC
import verify_cases as V
from util import DEFAULT_2P, EDIT

P1 = (0, 4, 6, 2)
UNIT = (0, 1, 1, 1)
SCAN_SETS = (DEFAULT_2P, P1, UNIT)
ALIGN_SETS = (DEFAULT_2P, P1, EDIT)


def adjacent(recs, a, b):
    """[(A, B)] of the list's adjacent records of kinds a, b."""
    return [(x, y) for x, y in zip(recs, recs[1:]) if x.kind == a and y.kind == b]


# ---- scan records -------------------------------------------------------------------------------------------------------------

def test_scan_lists_are_processed_in_list_order():
    for name, recs in RC.scan_lists().items():
        keys = [RC.scan_key(r) for r in recs]
        assert RC.dispatch_order(keys) == list(range(len(recs))), name
        if name != "zero":  # (the key-0 list: the sort's stability alone)
            assert all(x > y for x, y in zip(keys, keys[1:])), name
            assert 150 <= len(recs) <= 270 and keys[0] == 5000 and keys[-1] <= 3, (name, len(recs))
            offs = np.concatenate(([0], np.cumsum(keys)))[:-1]
            assert sorted(set(int(o) % 16 for o in offs)) == list(range(16)), name
    recs, begs = RC.verify_ranges_list()
    keys = [RC.scan_key(r) for r in recs]
    assert all(x > y for x, y in zip(keys, keys[1:]))
    zero = RC.scan_lists()["zero"]
    assert [RC.scan_key(r) for r in zero[2:]] == [0] * 24 and all(r.status in (1, 2, 3, 4) for r in zero if r.kind == "skipped")


def test_scan_adjacencies_by_the_yardsticks(hip_lib):
    """Every row of the record table, in both main lists: A and B are what they are called by verify_one_host, clip_one_host
    and split_one_host."""
    from allwave_amd import ffi
    sc, a, ms = DEFAULT_2P, 1, 20

    def verify(r):
        built = bytes(b if b in b"MXID" else ord("M") for b in r.ops)
        rec = V.record_for(sc, built, r.status)
        rec[3] = len(r.ops)
        h = ffi.verify_one_host(sc, r.pattern, r.text, r.ops, tuple(rec))
        return int(h["code"]), int(h["column"])

    def clip(r):
        return int(ffi.clip_one_host(sc, a, r.ops)["code"])

    def nseg(r):
        ix, _ = ffi.split_one_host(sc, a, ms, r.ops)
        return int(ix["code"]), int(ix["count"])

    def correct(r):
        return verify(r)[0] == V.OK and clip(r) == K.OK

    for name in ("main-I", "main-D"):
        recs = RC.scan_lists()[name]
        g = name[-1].encode()
        offs = np.concatenate(([0], np.cumsum([len(r.ops) for r in recs])))
        # a gap run open at A's last chunk boundary and last column, B begins with a run of the same op
        gaps = [(k, x, y) for k, (x, y) in enumerate(zip(recs, recs[1:])) if x.kind == "gap_tail" and y.kind == "gap_head"]
        assert len(gaps) >= 8
        for k, x, y in gaps:
            assert x.ops[-1:] == g == y.ops[:1] and verify(x)[0] == V.OK and verify(y)[0] == V.OK
            # wherever the string begins: the verify kernel gets it on a 16-byte slot, clip and split at its own offset
            assert RC.open_at_last_chunk_boundary(x.ops, 0) and RC.open_at_last_chunk_boundary(x.ops, int(offs[k]) % 16)
        assert sum(1 for _, x, _ in gaps if len(x.ops) > 2 * RC.CHUNK) >= 2 and sum(1 for _, x, _ in gaps if len(x.ops) < RC.CHUNK) >= 2
        for x, y in adjacent(recs, "pos_tail", "x_then_m"):
            assert RC.end_state(sc, a, x.ops)[0] >= min(250, len(x.ops) // 2) and y.ops.endswith(b"M") and (y.ops.startswith(b"X") or len(y.ops) <= 40) and len(y.ops.strip(b"X")) <= 40
        for x, y in adjacent(recs, "neg_tail", "all_m"):
            assert RC.end_state(sc, a, x.ops)[0] <= -2 * len(x.ops) or len(x.ops) < 12
            assert set(y.ops) == {ord("M")}
        assert len(adjacent(recs, "pos_tail", "x_then_m")) >= 8 and len(adjacent(recs, "neg_tail", "all_m")) >= 8
        for kind, col in (("bad3", lambda r: 3), ("bad1030", lambda r: 1030), ("badlast", lambda r: len(r.ops) - 1)):
            found = adjacent(recs, kind, "plain")
            assert len(found) >= 2, (name, kind)
            for x, y in found:
                assert verify(x) == (V.BAD_OP, col(x)) and clip(x) == K.BAD_OP and nseg(x)[0] == K.BAD_OP and correct(y)
                assert int(ffi.clip_one_host(sc, a, x.ops)["col_beg"]) == col(x)
        for kind in ("all_x", "all_gaps"):
            found = adjacent(recs, kind, "plain")
            assert len(found) >= 4
            for x, y in found:
                assert clip(x) == K.EMPTY and nseg(x) == (K.EMPTY, 0) and verify(x)[0] == V.OK and correct(y)
        for kind, code in (("m_differs0", V.M_DIFFERS), ("x_equal0", V.X_EQUAL)):
            (x, y), = adjacent(recs, kind, "plain")
            assert 2 * RC.CHUNK < len(x.ops) <= 3 * RC.CHUNK and verify(x)[0] == code and 0 <= verify(x)[1] < RC.CHUNK and correct(y)
        for kind, code in (("overrun", V.OVERRUN), ("short", V.SHORT)):
            found = adjacent(recs, kind, "exact")
            assert len(found) >= 4
            for x, y in found:
                assert verify(x)[0] == code and verify(y)[0] == V.OK
        found = adjacent(recs, "revcomp", "forward")
        assert len(found) >= 4 and all(x.rc == 1 and y.rc == 0 and verify(x)[0] == V.OK and verify(y)[0] == V.OK for x, y in found)
        # fifteen segments -> one -> none -> fifteen -> one -> none
        kinds = [r.kind for r in recs]
        i = kinds.index("seg15")
        assert kinds[i:i + 3] == ["seg15", "seg1", "seg0"] and [nseg(r) for r in recs[i:i + 3]] == [(K.OK, 15), (K.OK, 1), (K.EMPTY, 0)]
        i = kinds.index("seg15_short")
        assert kinds[i - 1:i + 3] == ["seg0", "seg15_short", "seg1", "seg0"]
        assert [nseg(r) for r in recs[i - 1:i + 3]] == [(K.EMPTY, 0), (K.OK, 15), (K.OK, 1), (K.EMPTY, 0)]
    zero = RC.scan_lists()["zero"]
    for x, y in adjacent(zero, "skipped", "len0"):
        assert verify(x) == (V.SKIPPED, -1) and verify(y)[0] == V.OK and clip(y) == K.EMPTY
    assert len(adjacent(zero, "skipped", "len0")) == 8 and len(adjacent(zero, "len0", "len0")) == 8 and len(adjacent(zero, "len0", "skipped")) == 7
    assert sorted(set(r.status for r in zero if r.kind == "skipped")) == [1, 2, 3, 4]
    recs, begs = RC.verify_ranges_list()
    odd = [(x, y) for (x, y), (bx, by) in zip(zip(recs, recs[1:]), zip(begs, begs[1:])) if x.kind == "range" and y.kind == "forward"
           and bx[0] % 4 and bx[1] % 4 and by == (0, 0)]
    assert len(odd) >= 15 and sum(x.rc for x, _ in odd) >= 6


@pytest.mark.parametrize("scores", SCAN_SETS, ids=["2-piece", "1-piece", "unit"])
def test_leaked_run_carry_changes_the_penalty(scores):
    """verify.hip's c_prev / c_start carried from A into B: B's first run would be the rest of A's last one, and B's penalty
    rescore(A + B) - rescore(A) instead of rescore(B)."""
    n = 0
    for name in ("main-I", "main-D"):
        recs = RC.scan_lists()[name]
        for x, y in adjacent(recs, "gap_tail", "gap_head"):
            assert V.rescore(scores, x.ops + y.ops) - V.rescore(scores, x.ops) != V.rescore(scores, y.ops), (name, len(x.ops))
            n += 1
    assert n >= 16


@pytest.mark.parametrize("a", [1, 2])
@pytest.mark.parametrize("scores", SCAN_SETS, ids=["2-piece", "1-piece", "unit"])
def test_leaked_scan_state_changes_the_clip(hip_lib, scores, a):
    """clip_scan.hpp's running score and minimum carried from A into B: B's clip from that start state is not
    clip_one_host(B) -- for the score traps, and for the gap traps (a run that goes on costs no second open)."""
    from allwave_amd import ffi
    n = 0
    for name in ("main-I", "main-D"):
        recs = RC.scan_lists()[name]
        for ka, kb in (("pos_tail", "x_then_m"), ("neg_tail", "all_m")):
            for x, y in adjacent(recs, ka, kb):
                s0, min0 = RC.end_state(scores, a, x.ops)
                h = ffi.clip_one_host(scores, a, y.ops)
                clean = (int(h["score"]), int(h["col_beg"]), int(h["col_end"])) if h["code"] == K.OK else None
                assert RC.clip_from(scores, a, y.ops) == clean, "the model without a leak is the yardstick"
                assert RC.clip_from(scores, a, y.ops, s0, min0) != clean, (name, ka, len(x.ops), len(y.ops))
                n += 1
    assert n >= 32


# ---- align pairs --------------------------------------------------------------------------------------------------------------

def test_align_lists_are_processed_in_list_order():
    for name, (seqs, pairs, kinds) in RC.align_lists().items():
        keys = RC.align_keys(seqs, pairs)
        assert RC.dispatch_order(keys) == list(range(len(pairs))), name
        for k, (x, y) in enumerate(zip(keys, keys[1:])):  # strictly, but for the two (c) entries: the same indices
            assert x > y or (kinds[k], kinds[k + 1]) == ("c-revcomp", "c-forward"), (name, k)
        assert all(100 <= len(s) <= 3000 or len(s) == 0 or kinds[i // 2].startswith(("small", "f-")) for i, s in enumerate(seqs)) or name == "bytes"
        assert kinds[-2:] == ["small", "small"] and all(len(seqs[i]) <= 100 for p in pairs[-2:] for i in p[:2]), name
        plain = set((q, t) for q, t, rc in pairs if not rc)
        assert not any((t, q) in plain for q, t in plain), name  # no pair together with its swap
    seqs, pairs, divergent = RC.capacity_list()
    assert RC.dispatch_order(RC.align_keys(seqs, pairs)) == list(range(12)) and sum(divergent) == 4
    # the range form: every residue modulo 16, on both strands, and the same pattern and text
    first, qres, tres, strands = 0, set(), set(), set()
    for name, (seqs, pairs, kinds) in RC.align_lists().items():
        res, ranges = RC.as_ranges(seqs, pairs, first)
        for (q, t, rc, qb, qe, tb, te), (q0, t0, rc0) in zip(ranges.tolist(), pairs):
            qres.add(qb % 16)
            tres.add(tb % 16)
            strands.add(rc)
            p = res[q][qb:qe]
            assert (TC.rc(p) if rc else p) == (TC.rc(seqs[q0]) if rc0 else seqs[q0]) and res[t][tb:te] == seqs[t0]
        assert RC.dispatch_order([RC.pair_key(r[4] - r[3], r[6] - r[5]) for r in ranges.tolist()]) == list(range(len(pairs)))
        first += len(pairs)
    assert qres == tres == set(range(16)) and strands == {0, 1}


def _oracle(oracle, name, scores):
    seqs, pairs, kinds = RC.align_lists()[name]
    return seqs, pairs, kinds, TC.oracle_records(oracle, seqs, pairs, scores, key=("reuse", name))


def test_align_adjacencies_by_the_oracle(oracle):
    """Rows (a) to (i) of the pair table under the default penalties: A and B are what they are called."""
    sc = DEFAULT_2P

    def runs(ops, n):
        return [m.group(0) for m in re.finditer(rb"I+|D+", ops) if len(m.group(0)) >= n]

    seqs, pairs, kinds, want = _oracle(oracle, "deep", sc)
    by = {k: want[i] for i, k in enumerate(kinds)}
    assert kinds[:2] == ["a-divergent", "a-three-mismatches"]
    assert TC.second_level(sc, by["a-divergent"][0] // 4)  # searches three levels deep, whatever the breakpoints
    assert by["a-three-mismatches"] == (15, by["a-three-mismatches"][1]) and by["a-three-mismatches"][1].count(b"X") == 3
    for i, k in enumerate(kinds):
        if k == "h-indel-rich":
            assert kinds[i + 1] == "h-mismatch-only" and TC.second_level(sc, want[i][0]) and len(runs(want[i][1], 12)) >= 4
            assert 1000 <= len(seqs[pairs[i][0]]) <= 1500
            assert not runs(want[i + 1][1], 1) and want[i + 1][1].count(b"X") >= 10
    seqs, pairs, kinds, want = _oracle(oracle, "bytes", sc)
    assert kinds[:3] == ["b-with-N", "b-acgt", "b-with-N"]
    has_n = [b"N" in seqs[q] or b"N" in seqs[t] for q, t, _ in pairs]
    assert has_n[:3] == [True, False, True] and not any(has_n[3:])
    i = kinds.index("d-identical")
    assert want[i] == (0, b"M" * 2400) and kinds[i + 1] == "d-divergent" and TC.second_level(sc, want[i + 1][0])
    i = kinds.index("c-revcomp")
    assert pairs[i][:2] == pairs[i + 1][:2] and (pairs[i][2], pairs[i + 1][2]) == (1, 0) and want[i][0] < want[i + 1][0] // 4
    seqs, pairs, kinds, want = _oracle(oracle, "gaps", sc)
    assert kinds[:2] == ["e-empty", "plain"] and want[0][1] == b"I" * 500
    forced = [i for i, k in enumerate(kinds) if k == "f-forced-gap"]
    assert len(forced) == 5
    for i in forced:
        ql, tl = len(seqs[pairs[i][0]]), len(seqs[pairs[i][1]])
        assert kinds[i + 1] == "f-equal-length" and len(seqs[pairs[i + 1][0]]) == len(seqs[pairs[i + 1][1]])
        assert want[i][0] <= 250 and len(runs(want[i][1], 120)) == 1 and abs(ql - tl) >= 120 and min(ql, tl) <= 120
    for name in ("restart-ab", "restart-ba"):
        seqs, pairs, kinds, want = _oracle(oracle, name, sc)
        assert kinds[:2] == ["g-restart", "plain"]
    a, b = repeats.RESTART_CASES[2][1](random.Random(repeats.RESTART_CASES[2][2]))  # (repeats.py: its searches restart on the device)
    assert RC.align_lists()["restart-ab"][0][:2] == [a, b] and RC.align_lists()["restart-ba"][0][:2] == [b, a]


@pytest.mark.parametrize("scores", ALIGN_SETS, ids=["2-piece", "1-piece", "edit"])
def test_bounds_abandon_a_third_and_complete_a_third(oracle, scores):
    for name in RC.align_lists():
        seqs, pairs, kinds, want = _oracle(oracle, name, scores)
        for every in (2, 3):
            bounds = RC.bounds_for(want, every)
            gone = sum(1 for b, (pen, _) in zip(bounds, want) if b >= 0 and pen > b)
            if every == 2:
                assert 3 * gone >= len(pairs), (name, every, gone)
            assert gone >= len(pairs) // every - 1 and 3 * (len(pairs) - gone) >= len(pairs), (name, every, gone)
