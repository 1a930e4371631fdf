"""GPU tests of the per-site allele table tallied on the device (csrc/variants.hip, csrc/variants_fold.hip): the events and rows an
engine returns are compared with the Python restatement (variants_cases.events_of, Table) of the same op bytes -- on the case list
through awv_variants_cigars / awv_variants_ranges, the fold alone against awv_variants_fold_host, the accumulated table, and the
engine's own alignments through the aligning calls.  All comparisons are exact: variants_cases.same on ROW_DTYPE arrays, tuple
equality for items."""
import random

import numpy as np
import pytest

import clip_cases as K
import coverage_cases as V
import split_cases as S
import util
import variants_cases as R
from verify_cases import revcomp

pytestmark = pytest.mark.gpu

SCORES = util.DEFAULT_2P
ITEM_FIELDS = ("code", "snv", "ins", "del")


def rows_of(event_lists):
    return np.concatenate([R.as_rows(ev) for ev in event_lists] + [np.zeros(0, dtype=R.ROW_DTYPE)])


def items_of(got):
    return [tuple(int(g[f]) for f in ITEM_FIELDS) for g in got]


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list packed into one arena, with what the restatement makes of it (computed once)."""
    cl, seqs = R.case_list(), R.resident_set()
    recs, arena = K.pack_arena([c[4] for c in cl], [c[7] for c in cl], [c[6] for c in cl])
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == [0, 1, 15]
    pairs = np.array([(c[1], c[2], c[3]) for c in cl], dtype=np.int32)
    slices = np.array([c[5] if c[5] is not None else (0, len(c[4]), 0, 0) for c in cl], dtype=np.int64)
    items = R.expected_items(seqs, cl)
    assert {i[0] for i in items} == {R.OK, R.SKIPPED, R.BAD_OP, R.LENGTHS}
    events = [R.case_events(seqs, c)[1] for c in cl]
    return cl, seqs, pairs, recs, arena, slices, items, events, R.expected_table(seqs, cl)


def engine(ffi, seqs=None, **kw):
    e = ffi.Engine(device=0, flags=kw.pop("flags", ffi.AWV_F_NO_ARENA_PROBE), **kw)
    if seqs is not None:
        e.set_sequences(seqs)
    return e


def refused(ffi, code, fn, *args, **kw):
    with pytest.raises(ffi.EngineError) as err:
        fn(*args, **kw)
    assert err.value.code == code


# ---- events ------------------------------------------------------------------------------------------------------------------

def test_one_item_one_workgroup(hip_lib):
    """The narrowest run of the pass: one record, one wave."""
    from allwave_amd import ffi
    seqs = R.resident_set()
    ops = b"M" * 9 + b"X" + b"D" * 30 + b"M" * 3 + b"III" + b"X" + b"DD"
    recs, arena = K.pack_arena([ops], [5])
    e = engine(ffi, seqs, workgroups=1)
    try:
        items, rows = e.variants_cigars(np.array([(1, 2, 0)], dtype=np.int32), recs, arena)
        code, events = R.events_of(1, 2, False, seqs[1], ops, (0, len(seqs[1]), 0, len(seqs[2])), (0, 0))
        assert code == R.OK and items_of(items) == [(R.OK,) + R.counts_of(events)] and len(events) == 5
        assert R.same(rows, R.as_rows(events))
    finally:
        e.close()


@pytest.mark.parametrize("workgroups", [1, 2, 0])
def test_events_on_the_case_list(hip_lib, cases, workgroups):
    """workgroups 1 and 2: one wave takes item after item, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, events, table = cases
    e = engine(ffi, seqs, workgroups=workgroups)
    try:
        got, rows = e.variants_cigars(pairs, recs, arena, slices=slices, fold=ffi.AWV_VTAB_EVENTS)
        for k, c in enumerate(cl):
            assert items_of(got[k:k + 1])[0] == items[k], c[0]
        want = rows_of(events)
        assert len(rows) == len(want) == table.events
        at = 0
        for k, c in enumerate(cl):  # case by case, so that a failure names its case
            n = len(events[k])
            assert R.same(rows[at:at + n], want[at:at + n]), c[0]
            at += n
        st = e.variants_stats()
        assert st.items == len(cl) and st.kernel_ms > 0
        assert st.failed == sum(1 for i in items if i[0] in (R.BAD_OP, R.LENGTHS)) >= 8
        assert st.columns == sum(len(R.case_item(c)[0]) for c in cl if c[6] == 0)
        assert (st.snv, st.ins, st.del_) == tuple(sum(i[k] for i in items) for k in (1, 2, 3))
    finally:
        e.close()


def test_unsound_items_add_no_row(hip_lib):
    from allwave_amd import ffi
    seqs = R.resident_set()
    good = b"M" * 5 + b"X" + b"DD" + b"M" * 4 + b"II" + b"X"
    strings = [good, b"XX?XX", good, b"X" * 18, good, b"MMXMM", good]
    status = [0, 0, 0, 0, 0, R.NOT_COMPLETED, 0]
    pairs = np.array([(1, 2, 0), (1, 2, 0), (2, 1, 1), (0, 1, 0), (3, 1, 0), (1, 2, 0), (1, 3, 1)], dtype=np.int32)
    recs, arena = K.pack_arena(strings, [3, 15, 0, 1, 15, 2, 9], status)
    e = engine(ffi, seqs, workgroups=1)
    try:
        got, rows = e.variants_cigars(pairs, recs, arena)
        want = []
        for (q, t, rev), ops, st in zip(pairs, strings, status):
            code, ev = (R.SKIPPED, []) if st else R.events_of(int(q), int(t), int(rev), revcomp(seqs[q]) if rev else seqs[q], ops, (0, len(seqs[q]), 0, len(seqs[t])), (0, 0))
            want.append((code, ev))
        assert [w[0] for w in want] == [R.OK, R.BAD_OP, R.OK, R.LENGTHS, R.OK, R.SKIPPED, R.OK]
        assert items_of(got) == [(c,) + R.counts_of(ev) for c, ev in want]
        assert R.same(rows, rows_of([ev for _, ev in want])) and len(rows) == 4 * 4
    finally:
        e.close()


def test_random_items_through_ranges(hip_lib):
    """The 300 random items, each on a query and a target of its own: rectangles inside longer sequences, both strands, slices."""
    from allwave_amd import ffi
    rng = random.Random(534)
    seqs, ranges, strings, slices, want = [], [], [], [], []
    for k, (_, _, rev, pattern, tlen, span, ops, sl) in enumerate(R.random_items()):
        q, t = 2 * k, 2 * k + 1
        seqs += [revcomp(pattern) if rev else pattern, util.rand_seq(rng, tlen)]
        qlen = len(pattern)
        ranges.append((q, t, int(rev), qlen - span[1], qlen - span[0], span[2], span[3]) if rev else (q, t, 0) + tuple(span))
        strings.append(ops)
        slices.append(sl if sl is not None else (0, len(ops), 0, 0))
        item_ops, skips = (ops, (0, 0)) if sl is None else (ops[sl[0]:sl[1]], (sl[2], sl[3]))
        code, ev = R.events_of(q, t, rev, pattern, item_ops, span, skips)
        assert code == R.OK
        want.append(ev)
    recs, arena = K.pack_arena(strings)
    e = engine(ffi, seqs)
    try:
        got, rows = e.variants_ranges(np.array(ranges, dtype=np.int32), recs, arena, slices=np.array(slices, dtype=np.int64))
        assert items_of(got) == [(R.OK,) + R.counts_of(ev) for ev in want]
        assert R.same(rows, rows_of(want)) and len(rows) > 3000
    finally:
        e.close()


# ---- the fold alone ----------------------------------------------------------------------------------------------------------

def random_rows(n, seed, keys=None):
    """n rows over a pool of `keys` distinct keys (default: about n / 3, so that runs of every short length occur)."""
    rng = np.random.RandomState(seed)
    pool = max(1, n // 3 if keys is None else keys)
    key = np.zeros(pool, dtype=R.ROW_DTYPE)
    key["t_idx"] = rng.randint(0, 4, pool)
    key["pos"] = rng.randint(0, 500, pool)
    key["type"] = rng.randint(0, 3, pool)
    key["len"] = rng.randint(1, 3, pool)
    key["hash"] = rng.randint(0, 3, pool).astype(np.uint64) * np.uint64(0x0123456789abcdef)
    rows = key[rng.randint(0, pool, n)]
    rows["rep"] = rng.randint(0, 1 << 62, n).astype(np.uint64)
    rows["count"] = rng.randint(1, 5, n)
    return rows


@pytest.fixture(scope="module")
def fold_engine(hip_lib):
    from allwave_amd import ffi
    e = engine(ffi)  # the fold needs no sequence set
    yield e
    e.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 70000])
def test_fold_sizes(hip_lib, fold_engine, n):
    from allwave_amd import ffi
    rows = random_rows(n, 540 + n % 97)
    want = ffi.variants_fold_host(rows)
    got = fold_engine.variants_fold(rows)
    assert R.same(got, want) and (n < 63 or len(want) < n) and int(got["count"].sum()) == int(rows["count"].sum())


def test_fold_key_patterns(hip_lib, fold_engine):
    from allwave_amd import ffi
    e = fold_engine
    equal = random_rows(1025, 551, keys=1)  # all keys equal: one row
    got = e.variants_fold(equal)
    assert R.same(got, ffi.variants_fold_host(equal)) and len(got) == 1 and int(got[0]["count"]) == int(equal["count"].sum())
    assert int(got[0]["rep"]) == int(equal["rep"].min())
    distinct = ffi.variants_fold_host(random_rows(5000, 552, keys=1500))[::-1].copy()  # all distinct, reverse sorted
    assert len(distinct) > 1025
    got = e.variants_fold(distinct)
    assert R.same(got, distinct[::-1].copy()) and R.same(got, ffi.variants_fold_host(distinct))
    # rows that are folded already, with counts above 1, fold like events: two tables and more events
    a, b, more = ffi.variants_fold_host(random_rows(3000, 553)), ffi.variants_fold_host(random_rows(3000, 554)), random_rows(500, 555)
    assert int(a["count"].max()) > 4
    mixed = np.concatenate([a, more, b])
    mixed = mixed[np.random.RandomState(556).permutation(len(mixed))]
    got = e.variants_fold(mixed)
    assert R.same(got, ffi.variants_fold_host(mixed)) and R.same(e.variants_fold(got), got)  # (and the fold is idempotent)


def test_fold_key_edges(hip_lib, fold_engine):
    """Keys that differ in exactly one field, at the field's lowest bit, its highest value bit and its sign bit (which no event
    carries: the order is the signed one all the same); hash 0 and 2^61 - 2; pos 0; len 2^30."""
    from allwave_amd import ffi
    base = dict(t_idx=5, pos=1000, type=1, len=6, hash=0x0fedcba987654320)
    keys = [dict(base)]
    for f in ("t_idx", "pos", "type", "len"):
        for bit in (0, 30, 31):
            k = dict(base)
            k[f] = int(np.int32(np.uint32(base[f] ^ (1 << bit))))
            keys.append(k)
    for bit in (0, 60, 61, 63):  # (an event's hash stays below 2^61 - 1; a caller's row may hold any word)
        keys.append(dict(base, hash=base["hash"] ^ (1 << bit)))
    keys += [dict(base, hash=0), dict(base, hash=(1 << 61) - 2), dict(base, pos=0), dict(base, len=1 << 30)]
    rows = np.zeros(3 * len(keys), dtype=R.ROW_DTYPE)
    for j, k in enumerate(keys * 3):
        rows[j] = (k["t_idx"], k["pos"], k["type"], k["len"], k["hash"], 1000 - j, 1 + j % 2, 0)
    rows = rows[np.random.RandomState(557).permutation(len(rows))]
    want = ffi.variants_fold_host(rows)
    got = fold_engine.variants_fold(rows)
    assert len(want) == len(keys) == 21 and R.same(got, want)
    assert sorted(int(r) for r in got["rep"]) == sorted(1000 - j for j in range(2 * len(keys), 3 * len(keys)))  # the smallest of each key's three


# ---- the folded call, pieces and state ---------------------------------------------------------------------------------------

def test_folded_call_on_the_case_list(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, events, table = cases
    e = engine(ffi, seqs)
    try:
        got, rows = e.variants_cigars(pairs, recs, arena, slices=slices, fold=ffi.AWV_VTAB_FOLDED)
        assert items_of(got) == items and R.same(rows, table.array()) and len(rows) < table.events
        # the list three times over: counts times three, rep unchanged
        got3, rows3 = e.variants_cigars(np.tile(pairs, (3, 1)), np.tile(recs, 3), arena, slices=np.tile(slices, (3, 1)), fold=ffi.AWV_VTAB_FOLDED)
        assert items_of(got3) == items * 3 and R.same(rows3, R.expected_table(seqs, cl, times=3).array())
        assert (rows3["count"] == 3 * rows["count"]).all() and (rows3["rep"] == rows["rep"]).all()
        # two different insertions of equal length at one site stay two rows
        site = rows[(rows["t_idx"] == 3) & (rows["pos"] == 10) & (rows["type"] == R.INS) & (rows["len"] == 3)]
        assert len(site) == 2 and site[0]["hash"] != site[1]["hash"]
        # the same alleles through a forward and a q_revcomp query: one row each, count 2, the forward query's rep
        sel = [k for k, c in enumerate(cl) if c[0].startswith(("an alignment of query 4", "the same alignment of query 5"))]
        _, two = e.variants_cigars(pairs[sel], recs[sel], arena, fold=ffi.AWV_VTAB_FOLDED)
        assert len(sel) == 2 and len(two) == len(events[sel[0]]) >= 6 and (two["count"] == 2).all() and (two["rep"] >> np.uint64(32) == 4).all()
        assert R.same(two, R.expected_table(seqs, [cl[k] for k in sel]).array())
    finally:
        e.close()


def test_pieces_caps_and_state(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, events, table = cases
    e = engine(ffi, max_arena_bytes=4096)
    try:
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_begin)  # no sequence set
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_cigars, pairs, recs, arena)
        e.set_sequences(seqs)
        assert e.variants_stats().items == 0
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_read)  # before begin
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_cigars, pairs, recs, arena, fold=ffi.AWV_VTAB_ACCUMULATE)
        refused(ffi, ffi.AWV_ERR_ARG, e.variants_cigars, pairs, recs, arena, fold=3)
        assert len(arena) > 10 * 4096  # more than ten pieces
        for fold, want in ((ffi.AWV_VTAB_EVENTS, rows_of(events)), (ffi.AWV_VTAB_FOLDED, table.array())):
            got, rows = e.variants_cigars(pairs, recs, arena, slices=slices, fold=fold)
            assert items_of(got) == items and R.same(rows, want)
            # a buffer too small is not written: the count says what it takes
            with pytest.raises(ffi.RowsDoNotFit) as small:
                e.variants_cigars(pairs, recs, arena, slices=slices, fold=fold, cap=len(want) - 1)
            assert small.value.n_rows == len(want) and items_of(small.value.items) == items
            buf = np.zeros(len(want), dtype=R.ROW_DTYPE)
            n_rows = ffi.C.c_uint64(0)
            sl = np.ascontiguousarray(e._slice_array(slices, len(recs)))
            pa = e._pair_array(pairs)
            arr = np.frombuffer(arena, dtype=np.uint8)
            rc = ffi.load().awv_variants_cigars(e._h, pa.ctypes.data, len(pa), recs.ctypes.data, arr.ctypes.data, len(arr), sl.ctypes.data, fold, got.ctypes.data,
                                                buf.ctypes.data, len(want) - 1, ffi.C.byref(n_rows))
            assert rc == ffi.AWV_OK and n_rows.value == len(want) and not buf.view(np.uint8).any()
        # refused before anything is launched: an index, an arena, a slice
        bad = pairs.copy()
        bad[5][1] = len(seqs)
        refused(ffi, ffi.AWV_ERR_ARG, e.variants_cigars, bad, recs, arena, slices=slices)
        refused(ffi, ffi.AWV_ERR_ARG, e.variants_cigars, pairs, recs, arena[:len(arena) // 2], slices=slices)
        sl = slices.copy()
        sl[-1] = (0, 0, -1, 0)
        refused(ffi, ffi.AWV_ERR_ARG, e.variants_cigars, pairs, recs, arena, slices=sl)
        # a new set ends the table
        e.variants_begin()
        e.set_sequences(seqs)
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_read)
    finally:
        e.close()


# ---- the accumulator ---------------------------------------------------------------------------------------------------------

def test_accumulator_folds_and_grows(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, events, table = cases
    reserve = 512
    assert len(table.rows) > 4 * reserve  # the table does not fit the first buffer, nor the second: it doubles
    e = engine(ffi, seqs, max_arena_bytes=4096)  # more than ten launches, each appending at the tail
    try:
        e.variants_begin(reserve_rows=reserve)
        got, appended = e.variants_cigars(pairs, recs, arena, slices=slices, fold=ffi.AWV_VTAB_ACCUMULATE)
        assert items_of(got) == items and appended == table.events
        folds = e.variants_stats().folds
        assert folds >= 2
        rows = e.variants_read(cap=len(table.rows))  # (one read: without a cap the binding measures first, which is a read and a fold of its own)
        assert R.same(rows, table.array())
        st = e.variants_stats()
        assert st.folds == folds + 1 and st.capacity_rows > 4 * reserve and st.rows == len(rows) and st.items == len(cl) and st.fold_ms > 0
        assert (st.snv, st.ins, st.del_) == tuple(sum(i[k] for i in items) for k in (1, 2, 3))
        # a buffer too small is not written; the table stays
        with pytest.raises(ffi.RowsDoNotFit) as small:
            e.variants_read(cap=len(rows) - 1)
        assert small.value.n_rows == len(rows)
        # one table read twice, with more items between the reads
        e.variants_cigars(pairs, recs, arena, slices=slices, fold=ffi.AWV_VTAB_ACCUMULATE)
        assert R.same(e.variants_read(), R.expected_table(seqs, cl, times=2).array())
        assert R.same(e.variants_read(), R.expected_table(seqs, cl, times=2).array())
        # a begin starts from nothing; an end ends the table and keeps the stats
        e.variants_begin()
        assert len(e.variants_read()) == 0 and e.variants_stats().items == 0
        e.variants_cigars(pairs[:20], recs[:20], arena, fold=ffi.AWV_VTAB_ACCUMULATE)
        e.variants_end()
        refused(ffi, ffi.AWV_ERR_STATE, e.variants_read)
        assert e.variants_stats().items == 20
        e.variants_end()
    finally:
        e.close()


def test_accumulator_contention(hip_lib, cases):
    """300 copies of one alignment, half through query 4 forward and half through the q_revcomp copy of query 5: every row's count
    is 300 and its rep the smallest, query 4's."""
    from allwave_amd import ffi
    cl, seqs = cases[0], cases[1]
    shared = [c for c in cl if c[0].startswith("an alignment of query 4")][0][4]
    recs, arena = K.pack_arena([shared], [5])
    p = np.array([(5, 3, 1), (4, 3, 0)] * 150, dtype=np.int32)
    e = engine(ffi, seqs)
    try:
        e.variants_begin(reserve_rows=64)
        got, appended = e.variants_cigars(p, np.repeat(recs, 300), arena, fold=ffi.AWV_VTAB_ACCUMULATE)
        want = R.Table()
        want.add(seqs, 4, 3, False, shared, times=150)
        want.add(seqs, 5, 3, True, shared, times=150)
        rows = e.variants_read()
        assert (got["code"] == R.OK).all() and appended == want.events and R.same(rows, want.array())
        assert (rows["count"] == 300).all() and (rows["rep"] >> np.uint64(31) == 8).all() and len(rows) >= 6
    finally:
        e.close()


# ---- the aligning calls ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family():
    """8 sequences of about 600 bp, mutated copies of one; the last four are stored as reverse complements.  All 56 ordered
    pairs, q_revcomp where exactly one of the two is stored reversed (the family of test_gpu_coverage.py)."""
    rng = random.Random(520)
    root = util.rand_seq(rng, 600)
    seqs = [util.mutate(root, 0.04, rng) for _ in range(8)]
    seqs = seqs[:4] + [revcomp(s) for s in seqs[4:]]
    pairs = np.array([(q, t, int((q >= 4) != (t >= 4))) for q in range(8) for t in range(8) if q != t], dtype=np.int32)
    return seqs, pairs


def table_of(seqs, pairs, res, cigars, slices=None, spans=None):
    """The restatement applied to the records and op bytes an aligning call returned.  slices: per pair a list of CLIP_DTYPE-like
    records that contribute (None: the whole string)."""
    tb = R.Table()
    for i, p in enumerate(pairs):
        if int(res[i]["status"]) != 0:
            continue
        q, t, rev = int(p[0]), int(p[1]), int(p[2])
        for sl in ([None] if slices is None else slices[i]):
            ops, skips = (cigars[i], (0, 0)) if sl is None else (cigars[i][int(sl["col_beg"]):int(sl["col_end"])], (int(sl["q_skip"]), int(sl["t_skip"])))
            assert tb.add(seqs, q, t, rev, ops, span=None if spans is None else spans[i], skips=skips) == R.OK
    return tb


def test_align_pairs_accumulates_every_batch(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    got = []
    for max_batch in (0, 16):
        e = engine(ffi, seqs, max_batch_pairs=max_batch)
        try:
            plain, plain_cigars = e.align_pairs(SCORES, pairs)
            e.variants_begin(reserve_rows=1024 if max_batch else 0)
            res, cigars = e.align_pairs(SCORES, pairs)
            assert res.tobytes() == plain.tobytes() and cigars == plain_cigars  # nothing else changes
            want = table_of(seqs, pairs, res, cigars)
            rows = e.variants_read()
            assert want.items == 56 and R.same(rows, want.array()) and int(rows["count"].max()) >= 3
            st = e.variants_stats()
            assert st.items == 56 and st.failed == 0 and st.columns == sum(len(c) for c in cigars) and st.snv + st.ins + st.del_ == want.events
            e.score_pairs(SCORES, pairs)  # a score-only call adds nothing
            e.orient_pairs(util.EDIT, pairs, full=True)  # nor do the strand alignments of an orientation call
            assert R.same(e.variants_read(), want.array()) and e.variants_stats().items == 56
            got.append(rows)
        finally:
            e.close()
    assert len(pairs) > 3 * 16 and R.same(got[0], got[1])  # one batch and four


def test_align_pairs_normalized_bounded_and_failing(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    e = engine(ffi, seqs)
    try:
        e.variants_begin()
        res, cigars = e.align_pairs(SCORES, pairs, normalize="left")
        want = table_of(seqs, pairs, res, cigars)  # of the normalized strings: gap runs count where they end up
        assert R.same(e.variants_read(), want.array())
        e.variants_begin()
        plain = e.align_pairs(SCORES, pairs)[1]
        assert sum(1 for a, b in zip(cigars, plain) if a != b) >= 3
        assert not R.same(e.variants_read(), want.array())
        # pairs above their bound contribute nothing
        e.variants_begin()
        bounds = np.where(np.arange(len(pairs)) % 3 == 0, 5, -1).astype(np.int32)
        res, cigars = e.align_pairs(SCORES, pairs, max_penalty=bounds)
        n_above = int((res["status"] == ffi.AWV_ST_ABOVE_BOUND).sum())
        want = table_of(seqs, pairs, res, cigars)
        assert n_above >= 10 and want.items == len(pairs) - n_above and R.same(e.variants_read(), want.array()) and e.variants_stats().items == want.items
    finally:
        e.close()
    # a pair that fails (rows too narrow, no re-run) contributes nothing
    rng = random.Random(521)
    a = util.rand_seq(rng, 6000)
    wide = [a, util.mutate(a, 0.08, rng), util.mutate(a, 0.01, rng)]
    e = engine(ffi, wide, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_NO_RERUN, first_row_cols=2048)
    try:
        e.variants_begin()
        p = np.array([(i, j, 0) for i in range(3) for j in range(3) if i != j], dtype=np.int32)
        res, cigars = e.align_pairs(SCORES, p)
        failed = res["status"] != 0
        assert failed.any() and not failed.all()
        want = table_of(wide, p, res, cigars)
        assert want.items == int((~failed).sum()) and R.same(e.variants_read(), want.array()) and e.variants_stats().items == want.items
    finally:
        e.close()


def test_align_pairs_clipped_with_a_threshold(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    a = 2
    e = engine(ffi, seqs, max_batch_pairs=20)
    try:
        _, _, clips = e.align_pairs(SCORES, pairs, clip=a)
        threshold = int(np.median(clips["score"])) + 1
        e.variants_begin(clip_min_score=threshold)
        res, cigars, clips = e.align_pairs(SCORES, pairs, clip=a)
        keep = [[c] if int(c["code"]) == ffi.AWV_CL_OK and int(c["score"]) >= threshold else [] for c in clips]
        n_kept = sum(len(k) for k in keep)
        assert 0 < n_kept < len(pairs)  # the threshold drops some pairs, not all
        want = table_of(seqs, pairs, res, cigars, slices=keep)
        assert want.items == n_kept and R.same(e.variants_read(), want.array()) and e.variants_stats().items == n_kept
    finally:
        e.close()


def test_align_pairs_split_adds_every_segment(hip_lib):
    from allwave_amd import ffi
    seqs, pairs = S.island_set()
    e = engine(ffi, seqs, max_batch_pairs=5)
    try:
        e.variants_begin(reserve_rows=256)
        res, cigars, (index, segs) = e.align_pairs(SCORES, pairs, split=(1, 100))
        assert sum(1 for s in segs if len(s) >= 2) >= 6  # islands: several segments per pair
        want = table_of(seqs, pairs, res, cigars, slices=segs)
        assert want.items == sum(len(s) for s in segs) > len(pairs) and R.same(e.variants_read(), want.array()) and e.variants_stats().items == want.items
    finally:
        e.close()


def test_align_ranges_on_both_strands(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    lens = [len(s) for s in seqs]
    ranges = np.array([(q, t, rev, 40 + 7 * k, lens[q] - 30 - k, 25 + 3 * k, lens[t] - 50 + k) for k, (q, t, rev) in enumerate(pairs[::3])], dtype=np.int32)
    for r in ranges:  # a forward interval [b, e) of a reversed query pairs with the target's mirrored interval
        if r[2]:
            r[5], r[6] = max(lens[r[1]] - (r[4] + 10), 0), lens[r[1]] - r[3]
    assert sum(1 for r in ranges if r[2]) >= 5
    e = engine(ffi, seqs, max_batch_pairs=7)
    try:
        e.variants_begin()
        res, cigars = e.align_ranges(SCORES, ranges)
        assert (res["status"] == 0).all()
        spans = [V.span_of_range(r, lens)[3] for r in ranges]
        want = table_of(seqs, ranges, res, cigars, spans=spans)
        assert want.items == len(ranges) and R.same(e.variants_read(), want.array())
    finally:
        e.close()


# ---- the host layer and the command-line tool -------------------------------------------------------------------------------

SCORES_2P = "0,5,8,2,24,1"


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


@pytest.fixture(scope="module")
def small_set():
    seqs, _ = K.flanked_set()
    return ["s%d" % i for i in range(10)], seqs[:10]


def test_host_all_pairs_variants(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs = small_set
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa")
    assert len(host.last_variants()["rows"]) == 0 and len(plain) == 90 and any(ln.split("\t")[4] == "-" for ln in plain)
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", variants=True)  # (WFA orientation's own alignments do not count)
    var = host.last_variants()
    assert got == plain
    want = R.table_from_paf(got, ids, seqs)
    st = var["stats"]
    assert R.same(var["rows"], want.array()) and len(var["rows"]) > 100
    assert (st.items, st.failed, st.rows) == (90, 0, len(want.rows)) and st.snv + st.ins + st.del_ == want.events and st.kernel_ms > 0
    # two slots on one device: the slots' tables merge into the one-slot table exactly
    two = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", variants=True, devices=[0, 0], min_batch_pairs=16)
    var2 = host.last_variants()
    assert sorted(two) == sorted(plain) and R.same(var2["rows"], want.array()) and var2["stats"].items == 90
    # the clip's slices, and only those that reach the least score, after normalization
    clipped = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left", variants=True)
    varc = host.last_variants()
    assert clipped == host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left")
    assert 5 <= len(clipped) < 90 and varc["stats"].items == len(clipped) and R.same(varc["rows"], R.table_from_paf(clipped, ids, seqs).array())
    # every other consumer tallies too: the records' iterator since the list's start, the counting one, the text ones
    for kw in (dict(mode="for_each"), dict(mode="next", chunk=25), dict(mode="par_collect")):
        assert sorted(host.iterate(ids, seqs, SCORES_2P, orientation="wfa", variants=True, **kw)) == sorted(plain)
        assert R.same(host.last_variants()["rows"], want.array()), kw
    host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="wfa", variants=True)
    assert R.same(host.last_variants()["rows"], want.array())
    assert host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", variants=True, coverage="both", cs="short", device_cigar=True, verify=True)[0].startswith(plain[0])
    assert R.same(host.last_variants()["rows"], want.array())
    segs = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", split=2, split_min_score=60, variants=True)
    assert len(segs) >= 5 and R.same(host.last_variants()["rows"], R.table_from_paf(segs, ids, seqs).array())


def test_host_align_ranges_variants(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs = small_set
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30)
    ranges = []
    for ln in plain:  # the clips of a first run, as interval pairs on both strands
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    assert sum(r[2] for r in ranges) >= 2
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, variants=True)
    var = host.last_variants()
    assert len(got) == len(ranges) and R.same(var["rows"], R.table_from_paf(got, ids, seqs).array()) and var["stats"].items == len(ranges)


def test_cli_variants(hip_lib, host_lib, small_set, tmp_path):
    import re
    import subprocess
    from allwave_amd import build
    ids, seqs = small_set
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def cli(out, *args):
        return subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)

    def run(out, *args):
        r = cli(out, *args)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_bytes(), r.stderr.splitlines()[-1]

    plain, summary0 = run("plain.paf", "-p", "none")
    assert " variants " not in summary0
    tsv = tmp_path / "var.tsv"
    got, summary = run("var.paf", "-p", "none", "--variants", str(tsv))
    assert got == plain  # byte for byte
    want = R.table_from_paf(got.decode().splitlines(), ids, seqs)
    lines = tsv.read_text().splitlines()
    assert lines == R.format_table(ids, seqs, want.array()) and len(lines) > 100
    assert {ln.split("\t")[2] for ln in lines} == {"snv", "del", "ins"}
    m = re.search(r"variants (\d+) items, (\d+) events, (\d+) rows, [0-9.]+ ms", summary)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (90, want.events, len(want.rows)), summary
    # --variants-min-count filters
    got2, _ = run("var2.paf", "-p", "none", "--variants", str(tsv), "--variants-min-count", "2")
    lines2 = tsv.read_text().splitlines()
    assert got2 == plain and lines2 == R.format_table(ids, seqs, want.array(), min_count=2) and 0 < len(lines2) < len(lines)
    # with --align-paf, --clip, --normalize and two slots
    paf_in = tmp_path / "map.paf"
    paf_in.write_bytes(b"\n".join(plain.splitlines()[:40]) + b"\n")
    base, _ = run("ranges.paf", "--align-paf", str(paf_in), "--clip", "2", "--normalize", "left")
    got, summary = run("ranges_var.paf", "--align-paf", str(paf_in), "--clip", "2", "--normalize", "left", "--variants", str(tsv), "--devices", "0,0")
    assert sorted(got.splitlines()) == sorted(base.splitlines())
    assert tsv.read_text().splitlines() == R.format_table(ids, seqs, R.table_from_paf(got.decode().splitlines(), ids, seqs).array())
    # usage errors exit as --coverage's do
    for args in (("--score-only",), ("--mash-matrix",), ("--check-paf", str(paf_in))):
        r, c = cli("bad.paf", "-p", "none", "--variants", str(tsv), *args), cli("bad.paf", "-p", "none", "--coverage", str(tsv), *args)
        assert r.returncode == c.returncode != 0 and r.stderr.replace("--variants", "--coverage") == c.stderr, (args, r.stderr, c.stderr)
    for args in (("--variants-min-count", "2"), ("--variants", str(tsv), "--variants-min-count", "0"), ("--variants", "")):
        r, c = cli("bad.paf", "-p", "none", *args), cli("bad.paf", "-p", "none", "--coverage-of", "both")
        assert r.returncode == c.returncode != 0 and "--variants" in r.stderr, (args, r.stderr)
