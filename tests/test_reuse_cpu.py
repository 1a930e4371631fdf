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
import coverage_cases as CV
import cs_cases as X
import normalize_cases as N
import repeats
import reuse_cases as RC
import twin_cases as TC
import variants_cases as VR
import verify_cases as V
from util import DEFAULT_2P, EDIT, rle

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


# ---- the five newer record passes ----------------------------------------------------------------------------------------------

PASS_LISTS = ("pass-I", "pass-D")
NORM_LISTS = {"norm-left": "left", "norm-right": "right"}
OKC = 0  # AWV_CST_OK = AWV_CV_OK = AWV_VR_OK = AWV_NM_OK


def instances(recs, a, b):
    """[(k, A, B)]: record k of kind a directly before one of kind b."""
    return [(k, x, y) for k, (x, y) in enumerate(zip(recs, recs[1:])) if x.kind == a and y.kind == b]


def spread(found, need=4):
    """The conditions every trap group meets: four instances or more, two of them behind an A of more than two chunks and two
    behind an A of less than one."""
    return len(found) >= need and sum(1 for _, x, _ in found if len(x.ops) > 2 * RC.CHUNK) >= 2 and sum(1 for _, x, _ in found if len(x.ops) < RC.CHUNK) >= 2


def op_runs(ops):
    """[(op, first column, length)] of the maximal runs."""
    return [(m.group(0)[:1], m.start(), m.end() - m.start()) for m in re.finditer(rb"(.)\1*", ops, re.S)]


def consumed(ops):
    return len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")


def test_pass_lists_are_processed_in_list_order():
    for name, recs in RC.pass_lists().items():
        keys = [RC.scan_key(r) for r in recs]
        assert RC.dispatch_order(keys) == list(range(len(recs))), name
        assert all(x > y for x, y in zip(keys, keys[1:])), name
        assert 150 <= len(recs) <= 270 and keys[0] == 5000 and keys[-1] <= 3, (name, len(recs))
        assert sorted(set(o % 16 for o in RC.offsets_of(recs))) == list(range(16)), name
        assert all(r.status == 0 for r in recs), name
    assert len(RC._PASS_GROUPS) == 10 and len(RC._NORM_GROUPS) == 4


def _codes(ffi, recs):
    """Per record its code under cs, coverage, variants and normalize (left), by the yardsticks."""
    seqs = RC.verify_inputs(recs, DEFAULT_2P)[0]
    return (RC.cs_want(ffi, "short", recs)[0]["code"], RC.coverage_want(ffi, "both", recs, seqs)[0]["code"], RC.variants_want(ffi, recs, seqs)[0]["code"],
            RC.normalize_want(ffi, "left", recs)[1]["code"])


def test_old_lists_serve_the_newer_passes(hip_lib):
    """What the issue counted on the existing main lists: most records sound under every pass, the others BAD_OP and LENGTHS, and
    the gap and 'M' adjacencies that are there without having been chosen."""
    from allwave_amd import ffi
    for name in ("main-I", "main-D"):
        recs = RC.scan_lists()[name]
        for codes in _codes(ffi, recs):
            assert 2 * int((codes == OKC).sum()) > len(recs) and set(int(c) for c in codes) == {0, 2, 3}, name
        assert sum(1 for x, y in zip(recs, recs[1:]) if x.ops[-1:] in (b"I", b"D") and x.ops[-1:] == y.ops[:1]) >= 8, name
        assert sum(1 for x, y in zip(recs, recs[1:]) if x.ops[-1:] == b"M" == y.ops[:1]) >= 100, name


def test_pass_groups_by_the_yardsticks(hip_lib):
    """Every trap group of pass-I and pass-D is there, often enough and behind long and short records, and A and B are what they are
    called by encode_one_host, cs_one_host, coverage_one_host, variants_one_host and normalize_one_host."""
    from allwave_amd import ffi
    for name in PASS_LISTS:
        recs = RC.pass_lists()[name]
        g = name[-1].encode()
        offs = RC.offsets_of(recs)
        seqs = RC.verify_inputs(recs, DEFAULT_2P)[0]
        enc = RC.encode_want(ffi, recs)[0]
        cs = RC.cs_want(ffi, "long", recs)[0]
        cov = RC.coverage_want(ffi, "both", recs, seqs)[0]
        var, events = RC.variants_want(ffi, recs, seqs)
        for codes in _codes(ffi, recs):
            assert 2 * int((codes == OKC).sum()) > len(recs), name

        def sound(k):
            return cs[k]["code"] == cov[k]["code"] == var[k]["code"] == OKC

        for a, b, aligned in RC._PASS_GROUPS:
            found = instances(recs, a, b)
            assert spread(found), (name, a, b, len(found))
            assert all(sound(k + 1) for k, _, _ in found), (name, a, b)
            if aligned:
                assert all(offs[k + 1] % 16 == 0 for k, _, _ in found), (name, a, b)
        for k, x, y in instances(recs, "gap_tail", "gap_head"):
            assert x.ops[-1:] == g == y.ops[:1] and sound(k) and RC.open_at_last_chunk_boundary(x.ops, offs[k] % 16)
            assert int(var[k + 1]["ins" if g == b"D" else "del"]) >= 1
        for k, x, y in instances(recs, "many_runs", "one_run"):
            assert int(enc[k]["runs"]) >= max(len(x.ops) // 4, 1) and int(enc[k]["len"]) >= 2 * int(enc[k]["runs"]) and int(enc[k + 1]["runs"]) == 1
        for k, x, y in instances(recs, "many_runs", "one_event"):
            # (an 'X' pick of 1 .. 3 columns is as many events, a gap pick one: about a third of the columns; an eighth is asserted)
            assert len(events[k]) >= max(len(x.ops) // 8, 2) or len(x.ops) < 16
            assert (len(events[k + 1]), int(var[k + 1]["snv"])) == (1, 1)
        firsts = set()
        for k, x, y in instances(recs, "pos_tail", "digits"):
            assert x.ops[-1:] == b"M" == y.ops[:1] and sound(k)
            firsts.add(op_runs(y.ops)[0][2])
        assert firsts >= set(RC.DIGITS), (name, sorted(firsts))
        for k, x, y in instances(recs, "plain", "x_first"):
            assert y.ops[:1] == b"X" and sound(k) and (min(consumed(x.ops)) >= 1000 or len(x.ops) < 1200)
        assert all(x.rc == 1 and y.rc == 0 and sound(k) for k, x, y in instances(recs, "revcomp", "forward"))
        for kind, col in (("bad3", lambda r: 3), ("badlast", lambda r: len(r.ops) - 1)):
            for k, x, y in instances(recs, kind, "plain"):
                assert cs[k]["code"] == ffi.AWV_CST_BAD_OP and cov[k]["code"] == ffi.AWV_CV_BAD_OP and var[k]["code"] == ffi.AWV_VR_BAD_OP
                h = ffi.normalize_one_host("left", x.pattern, x.text, x.ops)[1]
                assert (int(h["code"]), int(h["columns_moved"])) == (ffi.AWV_NM_BAD_OP, col(x))
        for k, x, y in instances(recs, "overrun", "plain"):
            assert cs[k]["code"] == ffi.AWV_CST_LENGTHS and cov[k]["code"] == ffi.AWV_CV_LENGTHS and var[k]["code"] == ffi.AWV_VR_LENGTHS
            assert ffi.normalize_one_host("left", x.pattern, x.text, x.ops)[1]["code"] == ffi.AWV_NM_LENGTHS
        for k, x, y in instances(recs, "all_gaps", "plain"):
            assert int(cov[k]["aligned_cols"]) == 0 and cov[k]["code"] == OKC and x.ops[-1:] == b"D" and y.ops[:1] == b"M"


def test_the_yardsticks_are_the_restatements(hip_lib):
    """The C yardsticks against plain Python: the run-length text and cs_of on every record of every list, coverage_of, events_of
    and the step-by-step shifter on every record of a trap pair."""
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs = RC.verify_inputs(recs, DEFAULT_2P)[0]
        enc, text = RC.encode_want(ffi, recs)
        assert text.decode() == "".join(rle(r.ops) for r in recs if r.status == 0), name
        assert [int(v) for v in enc["len"]] == [len(rle(r.ops)) if r.status == 0 else 0 for r in recs], name
        for mode in X.MODES:
            out, text = RC.cs_want(ffi, mode, recs)
            want = [X.cs_of(r.ops, r.pattern, r.text, mode) if r.status == 0 else (b"", X.SKIPPED) for r in recs]
            assert text == b"".join(w[0] for w in want) and [int(c) for c in out["code"]] == [w[1] for w in want], (name, mode)
        cov = RC.coverage_want(ffi, "both", recs, seqs)[0]
        for k, r in enumerate(recs):
            if r.status == 0 and cov[k]["code"] == OKC:
                assert tuple(int(cov[k][f]) for f in ("aligned_cols", "matched_cols", "boundaries")) == CV.counts_of(r.ops), (name, k)
        picked = sorted(set(k + d for k, (x, y) in enumerate(zip(recs, recs[1:])) for d in (0, 1)
                            if (x.kind, y.kind) in (("gap_tail", "gap_head"), ("pos_tail", "digits"), ("many_runs", "one_event"), ("revcomp", "forward"),
                                                    ("n_tail_unmoved", "n_head_moves"), ("n_moves_many", "n_blocked"))))
        picked = picked[:2] + [k for k in picked if len(recs[k].ops) <= 1200][:14]  # (the restatements take a column at a time)
        for roles in CV.ROLES:
            for k in picked[:8]:
                r = recs[k]
                ql, tl = len(seqs[2 * k]), len(seqs[2 * k + 1])
                item, qt, tt = ffi.coverage_one_host(roles, r.rc, ql, tl, r.ops)
                code, (qa, qm), (ta, tm) = CV.coverage_of(r.ops, (0, ql, 0, tl), "-" if r.rc else "+", (0, 0), roles, (ql, tl))
                assert int(item["code"]) == code and all(np.array_equal(u, v) for u, v in zip(qt + tt, (qa, qm, ta, tm))), (name, k, roles)
        for k in picked:
            r = recs[k]
            item, ev = ffi.variants_one_host(2 * k, 2 * k + 1, r.rc, r.pattern, len(r.text), r.ops)
            code, want = VR.events_of(2 * k, 2 * k + 1, r.rc, r.pattern, r.ops, (0, len(r.pattern), 0, len(r.text)), (0, 0))
            assert int(item["code"]) == code and VR.same(ev, VR.as_rows(want)), (name, k)
            for direction in ("left", "right"):
                ops, h = ffi.normalize_one_host(direction, r.pattern, r.text, r.ops)
                if h["code"] == OKC:
                    want, steps = N.step_normal(direction, r.pattern, r.text, r.ops)
                    assert ops == want and int(h["columns_moved"]) == steps, (name, k, direction)


def test_leaked_run_carry_changes_the_texts():
    """RunCarry from A into B (encode.hip, cs.hip in short mode, variants.hip): the carried start reaches every lane of B's first
    chunk that has no break below it, so B's first run comes out `start` columns shorter than it is -- a wrong number, a wrong
    count of digits, a wrong event length.  It differs whenever A has a second run; the run-merging leak of a walk without the
    column-0 rule (the tail of encode(A + B) against encode(B)) differs where A ends in the op B begins with."""
    n = {"gap": 0, "digits": 0}
    for name in PASS_LISTS:
        recs = RC.pass_lists()[name]
        for a, b, key in (("gap_tail", "gap_head", "gap"), ("pos_tail", "digits", "digits")):
            for k, x, y in instances(recs, a, b):
                start = op_runs(x.ops)[-1][1]      # what carry.start holds behind A
                first = op_runs(y.ops)[0][2]
                if start == 0:
                    continue  # (A is one run: nothing to carry)
                assert (first - start) % (1 << 32) != first  # (the kernel's own arithmetic; the models below are the merged runs)
                merged = rle(x.ops + y.ops)[len(rle(x.ops[:start])):]
                assert merged != rle(y.ops) and merged.endswith(rle(y.ops[first:])), (name, k)
                if key == "digits":  # cs, short mode: the ':N' of the 'M' run B begins with
                    clean = X.cs_of(y.ops, y.pattern, y.text, "short")[0]
                    leaked = X.cs_of(x.ops + y.ops, x.pattern + y.pattern, x.text + y.text, "short")[0][len(X.cs_of(x.ops[:start], x.pattern, x.text, "short")[0]):]
                    assert clean.startswith(b":%d" % first) and leaked.startswith(b":%d" % (first + len(x.ops) - start)) and leaked != clean, (name, k)
                else:                # variants: the length of the gap run B begins with
                    ev = VR.events_of(0, 1, 0, y.pattern, y.ops, (0, len(y.pattern), 0, len(y.text)), (0, 0))[1]
                    clean = [e for e in ev if e[2] != VR.SNV][0]
                    assert clean[3] == first
                    # events_of over the join: the run that spans it is one event, A's last run and B's first together -- another
                    # length, and for a 'D' run another hash (an 'I' run has none: 0 on both sides)
                    p2, t2 = x.pattern + y.pattern, x.text + y.text
                    joined = VR.events_of(0, 1, 0, p2, x.ops + y.ops, (0, len(p2), 0, len(t2)), (0, 0))[1]
                    before = VR.events_of(0, 1, 0, x.pattern, x.ops[:start], (0, len(x.pattern), 0, len(x.text)), (0, 0))[1]
                    span = joined[len(before)]
                    assert span[2] == clean[2] and span[3] == len(x.ops) - start + first != clean[3], (name, k)
                    assert (span[4] != clean[4]) == (name == "pass-D"), (name, k)
                    # and what the kernel's own arithmetic would give: the break's column less the stale start, as the event's int32
                    assert first - start != first and first - start < first
                n[key] += 1
    assert n["gap"] >= 16 and n["digits"] >= 16, n


def test_leaked_counts_and_positions_change_the_answers(hip_lib):
    """c_text / c_runs (encode.hip), c_text (cs.hip), c_ev (variants.hip): B's text would begin, and its counts go on, where A's
    ended.  cq / ct (cs.hip, variants.hip): B's first column would read its sequences where A's last column read A's -- beyond
    the end of B's own, which are as long as B needs.  bad / l_bad: B would be refused for A's stray byte."""
    from allwave_amd import ffi
    n = 0
    for name in PASS_LISTS:
        recs = RC.pass_lists()[name]
        for k, x, y in instances(recs, "many_runs", "one_run"):
            ex, ey = ffi.encode_one_host(x.ops)[1], ffi.encode_one_host(y.ops)[1]
            last = len(rle(x.ops)) - len(rle(x.ops[:op_runs(x.ops)[-1][1]]))
            assert int(ex["len"]) - last > 0 and int(ex["runs"]) - 1 > 0  # what c_text and c_runs hold behind A: added to B's len and runs
            for mode in X.MODES:
                assert len(X.cs_of(x.ops, x.pattern, x.text, mode)[0]) > len(X.cs_of(y.ops, y.pattern, y.text, mode)[0]) or len(y.ops) < 8
        for k, x, y in instances(recs, "many_runs", "one_event"):
            item = ffi.variants_one_host(0, 1, 0, x.pattern, len(x.text), x.ops)[0]
            assert int(item["snv"]) + int(item["ins"]) + int(item["del"]) >= 2  # c_ev behind A: B's one row would go to a place it has not got
        for k, x, y in instances(recs, "plain", "x_first") + instances(recs, "gap_tail", "gap_head"):
            cq, ct = consumed(x.ops)
            sl = (0, len(y.ops), cq, ct)
            for mode in X.MODES:
                clean = X.cs_of(y.ops, y.pattern, y.text, mode)
                assert clean[1] == X.OK and X.cs_of(y.ops, y.pattern, y.text, mode, slice=sl) != clean, (name, k)
                assert (ffi.cs_one_host(mode, y.pattern, y.text, y.ops, slice=sl)[1]["code"] != ffi.AWV_CST_OK)
            span = (0, len(y.pattern), 0, len(y.text))
            clean = VR.events_of(0, 1, 0, y.pattern, y.ops, span, (0, 0))
            assert clean[0] == VR.OK and len(clean[1]) >= 1 and VR.events_of(0, 1, 0, y.pattern, y.ops, span, (cq, ct)) != clean, (name, k)
            n += 1
        for kind in ("bad3", "badlast"):
            for k, x, y in instances(recs, kind, "plain"):
                assert X.cs_of(x.ops, x.pattern, x.text, "long")[1] == X.BAD_OP and X.cs_of(y.ops, y.pattern, y.text, "long")[1] == X.OK
                assert CV.code_of(x.ops, (0, len(x.pattern), 0, len(x.text)), (0, 0)) == CV.BAD_OP
    assert n >= 32


def cov_boundaries(ops, prev=(False, False)):
    """coverage.hip's count, column by column: a boundary where a column's class (aligned; matched) differs from the one before
    it, and one for each class the last column has; prev: the classes before column 0."""
    pa, pm = prev
    count = 0
    for op in ops:
        a, m = op in b"MX", op == ord("M")
        count += (a != pa) + (m != pm)
        pa, pm = a, m
    return count + pa + pm


def cov_depth(ops, prev=(False, False)):
    """coverage.hip's target tracks of a whole forward item, the way the kernel makes them: +1 / -1 (modulo 2^32) into a difference
    track at every boundary, at the text position of the column (behind the last one for a run that ends with the string), then
    the prefix sum.  (aligned, matched) over the text's bases; prev: the classes before column 0."""
    tlen = len(ops) - ops.count(b"D")
    diff = [[0] * (tlen + 1), [0] * (tlen + 1)]
    last = list(prev)
    y = 0
    for op in ops:
        for t, cls in enumerate((op in b"MX", op == ord("M"))):
            if cls != last[t]:
                diff[t][y] += 1 if cls else -1
            last[t] = cls
        y += op != ord("D")
    for t in (0, 1):
        diff[t][y] -= last[t]
    out = []
    for d in diff:
        acc, depth = 0, []
        for v in d[:tlen]:
            acc = (acc + v) % (1 << 32)
            depth.append(acc)
        out.append(np.array(depth, dtype=np.uint32))
    return out


def test_leaked_column_class_changes_the_depth(hip_lib):
    """coverage.hip's `prev` from A into B: where both A's last column and B's first are aligned (matched), B's first column opens
    no run -- one boundary less, and the +1 that raises the depth over B's first run is never added.  It can only happen where B
    begins in lane 0's byte 0; the groups that are built to do so stand in the lists, and ('M' after 'M') by chance in the old ones."""
    from allwave_amd import ffi
    n = 0
    for name in PASS_LISTS:
        recs = RC.pass_lists()[name]
        offs = RC.offsets_of(recs)
        for k, x, y in instances(recs, "pos_tail", "digits"):
            item = ffi.coverage_one_host("both", 0, len(y.pattern), len(y.text), y.ops)[0]
            assert cov_boundaries(y.ops) == int(item["boundaries"]) == CV.counts_of(y.ops)[2]
            last = (x.ops[-1:] in (b"M", b"X"), x.ops[-1:] == b"M")
            assert last == (True, True) and cov_boundaries(y.ops, last) == int(item["boundaries"]) - 2 and offs[k + 1] % 16 == 0, (name, k)
            # the depth: without a leak the model is the yardstick's and coverage_of's; with A's class before column 0 the +1 of B's
            # first run is missing, so the run's bases stay at 0 and every base behind it is one too low (modulo 2^32)
            _, _, (ta, tm) = ffi.coverage_one_host("target", 0, len(y.pattern), len(y.text), y.ops)
            want = CV.coverage_of(y.ops, (0, len(y.pattern), 0, len(y.text)), "+", (0, 0), CV.TARGET, (len(y.pattern), len(y.text)))[2]
            clean, leaked = cov_depth(y.ops), cov_depth(y.ops, last)
            assert all(np.array_equal(u, v) and np.array_equal(u, w) for u, v, w in zip(clean, (ta, tm), want)), (name, k)
            first = op_runs(y.ops)[0][2]
            for c, l in zip(clean, leaked):
                assert (c[:first] == 1).all() and (l[:first] == 0).all() and np.array_equal(l, c - np.uint32(1)), (name, k)
            n += 1
        for k, x, y in instances(recs, "all_gaps", "plain"):  # behind a gap nothing is carried: the model says so too
            assert cov_boundaries(y.ops, (False, False)) == CV.counts_of(y.ops)[2]
    assert n >= 16
    for name in ("main-I", "main-D"):
        recs = RC.scan_lists()[name]
        offs = RC.offsets_of(recs)
        assert sum(1 for k, (x, y) in enumerate(zip(recs, recs[1:])) if x.ops[-1:] == b"M" == y.ops[:1] and offs[k + 1] % 16 == 0) >= 3, name


def test_leaked_hash_changes_the_allele():
    """variants.hip's hcarry from A into B: B's first 'D' run has no break before it and no reset, so its hash would be that of
    A's last run followed by it."""
    n = 0
    recs = RC.pass_lists()["pass-D"]
    offs = RC.offsets_of(recs)
    for k, x, y in instances(recs, "gap_tail", "gap_head"):
        ra, rb = op_runs(x.ops)[-1], op_runs(y.ops)[0]
        assert ra[0] == rb[0] == b"D" and RC.open_at_last_chunk_boundary(x.ops, offs[k] % 16)
        tail = x.pattern[len(x.pattern) - ra[2]:]  # the bases A's last run inserts: the end of its pattern
        head = y.pattern[:rb[2]]
        ev = VR.events_of(0, 1, 0, y.pattern, y.ops, (0, len(y.pattern), 0, len(y.text)), (0, 0))[1][0]
        assert ev[2:5] == (VR.INS, rb[2], VR.hash_of(head)) and VR.hash_of(tail + head) != VR.hash_of(head), k
        n += 1
    assert n >= 8
    recs = RC.pass_lists()["pass-I"]   # 'I' runs have no hash: the same adjacency traps the carried start alone (above)
    assert all(op_runs(x.ops)[-1][0] == op_runs(y.ops)[0][0] == b"I" for _, x, y in instances(recs, "gap_tail", "gap_head"))


def first_run_shift(rec, linked=False, prev_type=0, prev_s=0):
    """normalize_device.hpp's rule for a string's first gap run alone, as the frame of a left-normalizing wave sees it: M^m g^L
    moves by the bases that agree, no further than shift_bound and than column 0."""
    (op0, _, m), (g, c, L) = op_runs(rec.ops)[:2]
    assert op0 == b"M" and g in (b"I", b"D")
    seq, p = (rec.pattern, c) if g == b"D" else (rec.text, c)
    bound = m + prev_s - (1 if g[0] == prev_type else 0) if linked else m
    s = 0
    while s < min(bound, c) and seq[p - 1 - s] == seq[p + L - 1 - s]:
        s += 1
    return s


def test_leaked_link_state_changes_the_shift(hip_lib):
    """normalize.hip's c_pp, prev_type and prev_s from A into B.  A's last gap run, of type g, stays where it is and 'M' columns end
    the string, so behind A the op before the run in progress is g and the run before it is (g, 0); B is M^m g^L in a homopolymer
    and its run goes to column 0 -- but a run linked to an unmoved one of its own type stops one column short.  The other way
    round -- A's last run moved far, B's first run stopped by a base -- is in the lists and is no trap: a larger bound changes
    nothing, a string's first run cannot go beyond column 0 (asserted here, so that nobody counts on it).  For norm-right the
    records are mirrored and so is the walk: the model reads them mirrored back.
    In normalize.hip as it stands the link state cannot reach B at all: column 0 is a break with no op before it, so the 'M' run
    before B's first gap run is never "linked" (a library with c_pp, prev_type and prev_s kept from record to record gives the same
    bytes).  The model is that of a walk without that rule, which is what a refactor could write; what does
    survive a record in today's kernel are the four counters (below) and c_prev, which only a column-free record reads (the
    key-0 list)."""
    from allwave_amd import ffi
    for name, direction in NORM_LISTS.items():
        recs = RC.pass_lists()[name]
        view = (lambda r: r) if direction == "left" else RC.mirrored
        for a, b, _ in RC._NORM_GROUPS:
            assert spread(instances(recs, a, b)), (name, a, b)
        results = RC.normalize_want(ffi, direction, recs)[1]
        assert (results["code"] == OKC).all()
        n = 0
        for k, x, y in instances(recs, "n_tail_unmoved", "n_head_moves"):
            xv, yv = view(x), view(y)
            ra, rb = op_runs(xv.ops), op_runs(yv.ops)
            if len(ra) < 3 or len(rb) < 2 or rb[0][0] != b"M" or ra[-2][0] != rb[1][0]:
                continue  # (the shortest records: not a whole trap)
            g = ra[-2][0]
            out = view(x._replace(ops=ffi.normalize_one_host(direction, x.pattern, x.text, x.ops)[0])).ops
            assert ra[-1][0] == b"M" and g in (b"I", b"D") and op_runs(out)[-2:] == ra[-2:], (name, k)  # A's last run: of type g, unmoved
            m = rb[0][2]
            got = view(y._replace(ops=ffi.normalize_one_host(direction, y.pattern, y.text, y.ops)[0])).ops
            assert first_run_shift(yv) == m and got.startswith(g * rb[1][2] + b"M" * m), (name, k)  # the model without a leak is the yardstick
            assert first_run_shift(yv, True, g[0], 0) == m - 1, (name, k)
            n += 1
        assert n >= 16, (name, n)
        n = 0
        for k, x, y in instances(recs, "n_tail_moved", "n_head_blocked"):
            xv, yv = view(x), view(y)
            ra, rb = op_runs(xv.ops), op_runs(yv.ops)
            if len(ra) < 3 or len(rb) < 2 or rb[0][0] != b"M" or ra[-2][2] > 5 or ra[-3][2] < 40:
                continue
            assert int(results[k]["max_shift"]) >= 40
            assert first_run_shift(yv) == first_run_shift(yv, True, ra[-2][0][0], 40) == first_run_shift(yv, True, rb[1][0][0] ^ 13, 40) < rb[0][2], (name, k)
            n += 1
        assert n >= 8, (name, n)
        n = 0
        for k, x, y in instances(recs, "n_gap_tail", "n_gap_head_other"):
            xv, yv = view(x), view(y)
            if len(x.ops) > 40:
                assert xv.ops[-1:] in (b"I", b"D") and yv.ops[:1] in (b"I", b"D") and xv.ops[-1:] != yv.ops[:1], (name, k)
                # no trap, and asserted so that nobody counts on it: cur_g, cur_c, cur_m, cur_p and cur_linked are all written when a
                # run starts, before anything reads them, and a run at column 0 cannot move whatever they held: the yardstick leaves
                # B's first run where it is
                got = view(y._replace(ops=ffi.normalize_one_host(direction, y.pattern, y.text, y.ops)[0])).ops
                r0 = op_runs(yv.ops)[0]
                assert op_runs(got)[0][:2] == r0[:2] and op_runs(got)[0][2] >= r0[2], (name, k)
                n += 1
        assert n >= 8
        n = 0
        for k, x, y in instances(recs, "n_moves_many", "n_blocked"):  # runs_moved, cols_moved, max_shift behind A against B's zeros
            if len(x.ops) > 100:
                assert int(results[k]["runs_moved"]) >= 2 and int(results[k]["columns_moved"]) > int(results[k]["max_shift"]) >= 5, (name, k)
                n += 1
            # the leak: B's counters go on from A's, so B's record would hold A's sums and A's maximum
            a_rec, b_rec = N.as_tuple(results[k]), N.as_tuple(results[k + 1])
            leaked = (OKC, a_rec[1] + b_rec[1], a_rec[2] + b_rec[2], max(a_rec[3], b_rec[3]), 0)
            assert b_rec == (OKC, 0, 0, 0, 0) and (leaked != b_rec or len(x.ops) <= 100), (name, k)
        assert n >= 8
