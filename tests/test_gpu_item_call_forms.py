"""GPU test of the ten calls on caller-supplied records with slices -- awv_{cs,coverage,variants,lift,msa}_{cigars,ranges} -- as
callers see their shared prologue (allwave_amd/csrc/item_call.hpp): which of two faults in one list is reported,
under whose name, that a refusal leaves the pass's stats, kernel_ms included, as they were (all zero in cs and msa, whose stats are
the last call's and are cleared when a call opens), and that the engine that refused answers a sound list as the pass's host
yardstick does (awv_*_one_host / awv_msa_host).  Four sequences of at most 40 bases and six records with op
strings of 0 to 40 bytes; tests/test_item_call_cpu.py holds the prologue's own cases."""
import random

import numpy as np
import pytest

import clip_cases as K

pytestmark = pytest.mark.gpu

PASSES = ("cs", "coverage", "variants", "lift", "msa")
FORMS = ("cigars", "ranges")
NOT_COMPLETED = 1
COMP = bytes.maketrans(b"ACGT", b"TGCA")
# (q_idx, t_idx, q_revcomp), the op string (None: a record that is not completed) and the range form's intervals (q_beg, q_end,
# t_beg, t_end; None: the whole of both).  No string consumes more than its rectangle, whole or not.
RECORDS = [((0, 1, 0), b"M" * 10 + b"X" + b"M" * 9 + b"DDD" + b"M" * 17, None),          # 40 columns: 40 pattern and 37 text bases
           ((1, 2, 1), b"M" * 12 + b"II" + b"M" * 8 + b"X" + b"M" * 10, None),           # 33 columns: 31 and 33
           ((2, 3, 0), b"", None),
           ((3, 0, 0), b"M" * 5 + b"DDDD" + b"M" * 8 + b"III" + b"XX" + b"MM", (2, 24, 5, 30)),  # 24 columns: 21 and 20
           ((0, 2, 0), None, None),
           ((1, 3, 1), b"X" + b"M" * 7 + b"D" + b"M" * 8, (4, 30, 3, 24))]              # 17 columns: 17 and 16
SEQ_LENS = (40, 37, 33, 24)
# the sound list's slices: a proper one, whole strings, and on the record that is not completed columns far outside any string
SLICES = [(5, 30, 5, 5), (0, 33, 0, 0), (0, 0, 0, 0), (0, 24, 0, 0), (1000, 2000, 0, 0), (0, 17, 0, 0)]
TARGETS = [1, 2, 3, 0]


def revcomp(s):
    return s.translate(COMP)[::-1]


@pytest.fixture(scope="module")
def world(hip_lib):
    """The engine with its sequences, the records and their arena (strings at odd residues), and the lists of both forms."""
    from allwave_amd import ffi
    rng = random.Random("item-call-forms")
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in SEQ_LENS]
    results, arena = K.pack_arena([ops or b"MMMMMMM" for _, ops, _ in RECORDS], offsets_mod16=[3, 0, 15, 1, 9, 6],
                                  status=[NOT_COMPLETED if ops is None else 0 for _, ops, _ in RECORDS])
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    e.set_sequences(seqs)
    e.coverage_begin("both")
    pairs = e._pair_array([p for p, _, _ in RECORDS])
    ranges = e._range_array([(q, t, rc) + (iv or (0, len(seqs[q]), 0, len(seqs[t]))) for (q, t, rc), _, iv in RECORDS])
    yield ffi, e, seqs, results, arena, {"cigars": pairs, "ranges": ranges}
    e.close()


def spans_of(seqs, form):
    """The records' rectangles (pb, pe, tb, te), the pattern's in the coordinates of the aligned copy."""
    out = []
    for (q, t, rc), _, iv in RECORDS:
        ql, tl = len(seqs[q]), len(seqs[t])
        qb, qe, tb, te = iv if form == "ranges" and iv else (0, ql, 0, tl)
        out.append((ql - qe, ql - qb, tb, te) if rc else (qb, qe, tb, te))
    return out


def lift_queries(seqs):
    """Two queries on every completed record, one from each side, inside the source sequence."""
    return [(k, side, 2, min(len(seqs[t if side == "target" else q]), 20)) for k, ((q, t, _), ops, _) in enumerate(RECORDS) if ops is not None
            for side in ("target", "query")]


def call(ffi, e, name, form, lst, results, arena, slices, seqs, queries=None):
    """One of the ten calls; what it returns, the pass's accumulators read where it has some.  queries: lift's (None: lift_queries)."""
    args = (lst, results, arena)
    if name == "cs":
        return getattr(e, "cs_" + form)("short", *args, slices=slices)
    if name == "coverage":
        return getattr(e, "coverage_" + form)(*args, slices=slices), e.coverage_read()
    if name == "variants":
        return getattr(e, "variants_" + form)(*args, slices=slices)
    if name == "lift":
        return getattr(e, "lift_" + form)(*args, lift_queries(seqs) if queries is None else queries, slices=slices)
    return getattr(e, "msa_" + form)(*args, TARGETS, slices=slices)


def stats_of(e, name):
    st = getattr(e, name + "_stats")()
    return tuple(getattr(st, f) for f, _ in st._fields_)


def check_sound(ffi, name, form, got, seqs, times):
    """The sound list's answer against the host yardstick, record by record; times: how often the list has been added to the
    engine's depth tracks by now."""
    spans = spans_of(seqs, form)
    aligned = [revcomp(seqs[q]) if rc else seqs[q] for (q, _, rc), _, _ in RECORDS]
    rows = list(zip(RECORDS, spans, SLICES, aligned))
    if name == "cs":
        text, csout, nbytes = got
        at = 0
        for i, (((q, t, rc), ops, _), (pb, pe, tb, te), sl, P) in enumerate(rows):
            if ops is None:
                assert (int(csout[i]["code"]), int(csout[i]["len"])) == (ffi.AWV_CST_SKIPPED, 0), i
                continue
            want, rec = ffi.cs_one_host("short", P[pb:pe], seqs[t][tb:te], ops, slice=sl)
            assert (int(csout[i]["code"]), int(csout[i]["len"]), int(csout[i]["off"])) == (int(rec["code"]), len(want), at), (i, csout[i], rec)
            assert bytes(text[at:at + len(want)]) == want, i
            at += len(want)
        assert nbytes == at and at > 40
    elif name == "coverage":
        items, (_, dev_aligned, dev_matched) = got
        tracks = [(np.zeros(len(s), dtype=np.uint32), np.zeros(len(s), dtype=np.uint32)) for s in seqs]
        for i, (((q, t, rc), ops, _), span, sl, _) in enumerate(rows):
            if ops is None:
                assert int(items[i]["code"]) == ffi.AWV_CV_SKIPPED, i
                continue
            item, _, _ = ffi.coverage_one_host("both", rc, len(seqs[q]), len(seqs[t]), ops, span=span, slice=sl, q_tracks=tracks[q], t_tracks=tracks[t])
            assert items[i].tobytes() == item.tobytes(), (i, items[i], item)
        assert (items["code"][[0, 1, 2, 3, 5]] == ffi.AWV_CV_OK).all()
        assert np.array_equal(dev_aligned, times * np.concatenate([a for a, _ in tracks])) and int(dev_aligned.max()) >= times
        assert np.array_equal(dev_matched, times * np.concatenate([m for _, m in tracks]))
    elif name == "variants":
        items, events = got
        at = 0
        for i, (((q, t, rc), ops, _), span, sl, P) in enumerate(rows):
            if ops is None:
                assert int(items[i]["code"]) == ffi.AWV_VR_SKIPPED, i
                continue
            item, ev = ffi.variants_one_host(q, t, rc, P, len(seqs[t]), ops, span=span, slice=sl)
            assert items[i].tobytes() == item.tobytes(), (i, items[i], item)
            assert events[at:at + len(ev)].tobytes() == ev.tobytes(), i
            at += len(ev)
        assert at == len(events) and at >= 8
    elif name == "lift":
        queries = lift_queries(seqs)
        assert len(got) == len(queries) == 10
        for j, (k, side, beg, end) in enumerate(queries):
            (q, t, rc), ops, _ = RECORDS[k]
            want = ffi.lift_one_host(side, rc, len(seqs[q]), len(seqs[t]), ops, beg, end, span=spans[k], slice=SLICES[k])
            assert got[j].tobytes() == want.tobytes(), (j, got[j], want)
        assert int((got["code"] == ffi.AWV_LF_OK).sum()) >= 6
    else:
        items, tgts, buf, size = got
        assert [int(t) for t in tgts["t_idx"]] == TARGETS
        at = 0
        for j, target in enumerate(TARGETS):
            mine = [i for i, ((_, t, _), _, _) in enumerate(RECORDS) if t == target]
            _, width, codes, block = ffi.msa_host(seqs[target], [(aligned[i], RECORDS[i][1], spans[i], SLICES[i]) for i in mine])
            assert [int(items[i]["code"]) for i in mine] == [int(c) for c in codes] and all(int(items[i]["target"]) == j for i in mine), (j, codes)
            assert (int(tgts[j]["rows"]), int(tgts[j]["width"]), int(tgts[j]["off"])) == (block.shape[0], width, at), (j, tgts[j], block.shape)
            assert np.array_equal(buf[at:at + block.size].reshape(block.shape), block), j
            at += block.size
        assert size == at and int((items["code"] == ffi.AWV_MS_OK).sum()) == 5 and int(items["code"][4]) == ffi.AWV_MS_SKIPPED


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", PASSES)
def test_which_fault_a_call_reports_and_that_it_answers_afterwards(world, name, form):
    ffi, e, seqs, results, arena, lists = world
    L = ffi.load()
    who = "%s_%s" % (name, form)
    sound = lists[form]
    slices = e._slice_array(SLICES, len(RECORDS))

    def bad_index(k):
        lst = sound.copy()
        lst["t_idx"][k] = len(seqs)
        return lst

    def bad_arena(k):  # the string ends one byte behind the arena
        res = results.copy()
        res["cigar_off"][k] = len(arena) - int(res["cigar_len"][k]) + 1
        return res

    def bad_slice(k):
        sl = slices.copy()
        sl["col_end"][k] = int(results["cigar_len"][k]) + 1
        return sl

    index_message = "sequence index out of range" if form == "cigars" else "range 4 names a sequence index or an interval out of range"
    faults = [("the index", bad_index(4), bad_arena(1), slices, index_message),
              ("the slice", sound, bad_arena(3), bad_slice(1), "slice 1 does not lie inside its op string"),
              ("the arena", sound, bad_arena(1), bad_slice(3), "a record's op bytes lie outside the CIGAR arena")]

    if name == "coverage":
        e.coverage_begin("both")  # the depth tracks start from zero
    call(ffi, e, name, form, sound[:0], results[:0], b"", None, seqs, queries=[])  # a call without records is accepted
    check_sound(ffi, name, form, call(ffi, e, name, form, sound, results, arena, slices, seqs), seqs, 1)
    # coverage, variants and lift sum since their begin: a refusal leaves every figure, kernel_ms included, as it was.  cs and msa
    # keep the last call's stats and clear them when a call opens, before the list is looked at: a refused call leaves all zero.
    before = stats_of(e, name)
    assert any(before), who
    after_refusal = before if name in ("coverage", "variants", "lift") else (0,) * len(before)
    wrong_names = []
    for what, lst, res, sl, message in faults:
        with pytest.raises(ffi.EngineError) as err:
            call(ffi, e, name, form, lst, res, arena, sl, seqs)
        said = L.awv_last_error().decode()
        assert err.value.code == ffi.AWV_ERR_ARG and message in said, (who, what, err.value.code, said)
        if not said.startswith(who + ": "):
            wrong_names.append((what, said))
        assert stats_of(e, name) == after_refusal, (who, what, stats_of(e, name), before)
    check_sound(ffi, name, form, call(ffi, e, name, form, sound, results, arena, slices, seqs), seqs, 2)
    assert not wrong_names, (who, "a refusal under another function's name", wrong_names)
