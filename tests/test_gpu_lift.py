"""GPU tests of the liftover on the device (csrc/lift.hip): every answer of awv_lift_cigars / awv_lift_ranges and every row of an
engine's table is compared, field for field, with the Python restatement (lift_cases.lift_of) of the same op bytes -- on the case
list, in pieces, with one and two waves that take record after record, and on the engine's own alignments through the aligning
calls.  All comparisons are exact equality."""
import numpy as np
import pytest

import clip_cases as K
import lift_cases as L
import util
from verify_cases import revcomp

pytestmark = pytest.mark.gpu

SCORES = util.DEFAULT_2P


def fields(rec):
    return tuple(int(rec[f]) for f in L.FIELDS)


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list packed into one arena, its queries in one shuffled list, and what the restatement makes of them (computed once)."""
    cl = L.case_list()
    recs, arena = K.pack_arena([c[4] for c in cl], [c[7] for c in cl], [c[6] for c in cl])
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == [0, 1, 15]
    pairs = np.array([(c[1], c[2], c[3]) for c in cl], dtype=np.int32)
    slices = np.array([c[5] if c[5] is not None else (0, len(c[4]), 0, 0) for c in cl], dtype=np.int64)
    queries, where = L.flat_queries([c[8] for c in cl])
    want = [None] * len(queries)
    for ws, places in zip(L.expected(cl), where):
        for w, p in zip(ws, places):
            want[p] = w
    assert {w[0] for w in want} == {L.OK, L.SKIPPED, L.BAD_OP, L.LENGTHS, L.UNALIGNED, L.OUTSIDE}
    return cl, L.resident_set(), pairs, recs, arena, slices, queries, want


def check(got, want, queries, cl):
    assert len(got) == len(want)
    for k, w in enumerate(want):
        assert fields(got[k]) == w, (cl[queries[k][0]][0], queries[k])


def code_counts(want):
    return tuple(sum(1 for w in want if w[0] == c) for c in (L.OK, L.SKIPPED, L.BAD_OP, L.LENGTHS, L.UNALIGNED, L.OUTSIDE))


def stats_tuple(st):
    return (st.records, st.columns, st.queries, st.ok, st.skipped, st.bad_op, st.lengths, st.unaligned, st.outside)


def walked(cl, recs_with_query):
    """(records, op bytes) of the completed cases among recs_with_query: what a launch walks, each once"""
    done = [cl[i] for i in sorted(recs_with_query) if cl[i][6] == 0]
    return len(done), sum((c[5][1] - c[5][0]) if c[5] is not None else len(c[4]) for c in done)


@pytest.mark.parametrize("workgroups", [1, 2, 0])
def test_lift_cigars_on_the_case_list(hip_lib, cases, workgroups):
    """workgroups 1 and 2: one wave takes record after record, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, queries, want = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)
    try:
        e.set_sequences(seqs)
        got = e.lift_cigars(pairs, recs, arena, queries, slices=slices)
        check(got, want, queries, cl)
        assert (got["reserved"] == 0).all()
        st = e.lift_stats()
        n_rec, n_cols = walked(cl, {q[0] for q in queries})
        assert stats_tuple(st) == (n_rec, n_cols, len(queries)) + code_counts(want) and st.kernel_ms > 0
        # the single walk: every query three times over walks no byte more
        thrice = e.lift_cigars(pairs, recs, arena, queries * 3, slices=slices)
        check(thrice, want * 3, queries * 3, cl)
        st3 = e.lift_stats()
        assert (st3.records, st3.columns, st3.queries) == (2 * n_rec, 2 * n_cols, 4 * len(queries))
        # only the records that have a query are walked
        some = [q for q in queries if q[0] % 7 == 3]
        got = e.lift_cigars(pairs, recs, arena, some, slices=slices)
        check(got, [w for q, w in zip(queries, want) if q[0] % 7 == 3], some, cl)
        r7, c7 = walked(cl, {q[0] for q in some})
        st7 = e.lift_stats()
        assert 0 < r7 < n_rec and (st7.records, st7.columns) == (2 * n_rec + r7, 2 * n_cols + c7)
        assert len(e.lift_cigars(pairs, recs, arena, [], slices=slices)) == 0 and stats_tuple(e.lift_stats()) == stats_tuple(st7)
    finally:
        e.close()


def test_lift_cigars_in_pieces_refusals_and_state_errors(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, queries, want = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=4096)

    def refused(code, fn, *args, **kw):
        with pytest.raises(ffi.EngineError) as err:
            fn(*args, **kw)
        assert err.value.code == code

    try:
        refused(ffi.AWV_ERR_STATE, e.lift_cigars, pairs, recs, arena, queries)  # no sequence set
        refused(ffi.AWV_ERR_STATE, e.lift_begin, [(0, 0, 5)], "target")
        refused(ffi.AWV_ERR_STATE, e.lift_read)
        e.set_sequences(seqs)
        assert stats_tuple(e.lift_stats()) == (0,) * 9
        refused(ffi.AWV_ERR_STATE, e.lift_read)  # before begin
        assert len(arena) > 10 * 4096  # more than ten pieces
        got = e.lift_cigars(pairs, recs, arena, queries, slices=slices)
        check(got, want, queries, cl)
        before = stats_tuple(e.lift_stats()), e.lift_stats().kernel_ms
        assert before[0][:3] == walked(cl, {q[0] for q in queries}) + (len(queries),)
        # refused before anything is launched: what awv_cs_cigars refuses, then what a query can get wrong
        bad = pairs.copy()
        bad[5][1] = len(seqs)
        refused(ffi.AWV_ERR_ARG, e.lift_cigars, bad, recs, arena, queries, slices=slices)
        refused(ffi.AWV_ERR_ARG, e.lift_cigars, pairs, recs, arena[:len(arena) // 2], queries, slices=slices)
        sl = slices.copy()
        sl[-1] = (0, 0, -1, 0)
        refused(ffi.AWV_ERR_ARG, e.lift_cigars, pairs, recs, arena, queries, slices=sl)
        sl = slices.copy()
        sl[3] = (2, 1, 0, 0)
        refused(ffi.AWV_ERR_ARG, e.lift_cigars, pairs, recs, arena, queries, slices=sl)
        q_len, t_len = L.SET_LENS[cl[40][1]], L.SET_LENS[cl[40][2]]
        for wrong in ((-1, 1, 0, 5), (len(cl), 1, 0, 5), (40, 0, 0, 5), (40, 3, 0, 5), (40, 1, 5, 5), (40, 1, 6, 5), (40, 2, -1, 5), (40, 1, 0, t_len + 1),
                      (40, 2, 0, q_len + 1)):
            refused(ffi.AWV_ERR_ARG, e.lift_cigars, pairs, recs, arena, queries[:50] + [wrong] + queries[50:], slices=slices)
        assert (stats_tuple(e.lift_stats()), e.lift_stats().kernel_ms) == before
        assert fields(e.lift_cigars(pairs, recs, arena, [(40, 1, 0, t_len)], slices=slices)[0])[0] in (L.OK, L.OUTSIDE, L.UNALIGNED)
        # the table's state: a mask, a region, an end
        refused(ffi.AWV_ERR_ARG, e.lift_begin, [(0, 0, 5)], 4)
        for wrong in ((len(seqs), 0, 5), (-1, 0, 5), (0, 5, 5), (0, -1, 5), (0, 0, L.SET_LENS[0] + 1)):
            refused(ffi.AWV_ERR_ARG, e.lift_begin, [(1, 0, 5), wrong], "both")
        refused(ffi.AWV_ERR_STATE, e.lift_read)
        e.lift_begin([(0, 0, 5)], "both")
        assert len(e.lift_read()) == 0 and stats_tuple(e.lift_stats()) == (0,) * 9  # a begin starts from zero
        e.lift_begin(None, None)
        refused(ffi.AWV_ERR_STATE, e.lift_read)
        e.lift_begin([(0, 0, 5)], "query")
        e.set_sequences(seqs)
        refused(ffi.AWV_ERR_STATE, e.lift_read)
    finally:
        e.close()


def test_lift_ranges_on_both_strands(hip_lib):
    from allwave_amd import ffi
    rc = L.range_case_list()
    lens = L.SET_LENS
    recs, arena = K.pack_arena([ops for _, _, ops, _ in rc])
    ranges = np.array([r for _, r, _, _ in rc], dtype=np.int32)
    queries, where = L.flat_queries([qs for _, _, _, qs in rc], seed=536)
    want = [None] * len(queries)
    for (name, r, ops, qs), places in zip(rc, where):
        q, t, strand, span = L.span_of_range(r, lens)
        for (frm, b, e_), p in zip(qs, places):
            want[p] = L.lift_of(ops, span, strand, frm, b, e_, lens[q])
    assert sum(1 for w in want if w[0] == L.OK) > 50 and any(w[0] == L.OUTSIDE for w in want)
    for workgroups in (1, 0):
        e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)
        try:
            e.set_sequences(L.resident_set())
            got = e.lift_ranges(ranges, recs, arena, queries)
            for k, w in enumerate(want):
                assert fields(got[k]) == w, (rc[queries[k][0]][0], queries[k])
            bad = ranges.copy()
            bad[2][4] = lens[bad[2][0]] + 1
            with pytest.raises(ffi.EngineError) as err:
                e.lift_ranges(bad, recs, arena, queries)
            assert err.value.code == ffi.AWV_ERR_ARG
        finally:
            e.close()


def test_a_lifted_slice_goes_into_the_text_passes(hip_lib, cases):
    """Each OK result, passed as an awv_cs_slice to awv_encode_cigars and awv_cs_cigars, gives the host yardsticks' text of that slice."""
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, queries, want = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        got = e.lift_cigars(pairs, recs, arena, queries, slices=slices)
        ok = [k for k in range(len(got)) if int(got[k]["code"]) == L.OK][::5]
        assert len(ok) > 200
        rec_of = [queries[k][0] for k in ok]
        sl = np.array([[int(got[k][f]) for f in ("col_beg", "col_end", "q_skip", "t_skip")] for k in ok], dtype=np.int64)
        texts, tout, _ = e.encode_cigars(recs[rec_of], arena, slices=sl[:, :2])
        cs_texts, csout, _ = e.cs_cigars("short", pairs[rec_of], recs[rec_of], arena, slices=sl)
        for j, i in enumerate(rec_of):
            _, q, t, rev, ops, _, _, _, _ = cl[i]
            cb, ce, qs, ts = (int(v) for v in sl[j])
            text, one = ffi.encode_one_host(ops[cb:ce])
            assert bytes(texts[int(tout[j]["off"]):int(tout[j]["off"]) + int(tout[j]["len"])]) == text and int(tout[j]["runs"]) == int(one["runs"])
            cs_text, cs_one = ffi.cs_one_host("short", revcomp(seqs[q]) if rev else seqs[q], seqs[t], ops, slice=(cb, ce, qs, ts))
            assert int(csout[j]["code"]) == int(cs_one["code"]) == 0
            assert bytes(cs_texts[int(csout[j]["off"]):int(csout[j]["off"]) + int(csout[j]["len"])]) == cs_text
    finally:
        e.close()


# ---- the aligning calls ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family():
    """8 sequences of 300 .. 2,000 bp, mutated prefixes of one root (allwave_amd.synth), two of them with 60 bases cut out and
    the last three stored as reverse complements: the alignments have gap runs long enough to hold a region.  All 56 ordered
    pairs, q_revcomp where exactly one of the two is stored reversed; and regions on several sequences."""
    from allwave_amd import synth
    data, offs, _ = synth.generate(8, 2000, 0.03, 540, mixed_lengths=(300, 2000))
    seqs = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(8)]
    seqs[1] = seqs[1][:150] + seqs[1][210:]
    seqs[6] = seqs[6][:120] + seqs[6][180:]
    seqs = seqs[:5] + [revcomp(s) for s in seqs[5:]]
    lens = [len(s) for s in seqs]
    assert min(lens) >= 240 and max(lens) <= 2000
    pairs = np.array([(q, t, int((q >= 5) != (t >= 5))) for q in range(8) for t in range(8) if q != t], dtype=np.int32)
    regions = []
    for s in (0, 1, 2, 5, 6, 7):
        n = lens[s]
        regions += [(s, 100, 160), (s, 140, 230), (s, 150, 151), (s, 0, n), (s, n - 80, n - 20), (s, 100, 160), (s, 155, 200)]
    return seqs, lens, pairs, regions


def items_of(pairs, res, cigars, lens, slices=None, spans=None):
    """contributing_items' rule, restated: completed records, whole or through the slices given per pair."""
    items = []
    for i, p in enumerate(pairs):
        if int(res[i]["status"]) != 0:
            continue
        q, t, rev = int(p[0]), int(p[1]), int(p[2])
        for sl in ([None] if slices is None else slices[i]):
            items.append((q, t, rev, cigars[i], None if spans is None else spans[i],
                          None if sl is None else tuple(int(sl[f]) for f in ("col_beg", "col_end", "q_skip", "t_skip"))))
    return items


def table(engine):
    rows = engine.lift_read()
    got = [tuple(int(r[f]) for f in L.ROW_FIELDS) for r in rows]
    assert got == sorted(got)  # the stated order
    return got


@pytest.mark.parametrize("side", ["target", "query", "both"])
def test_align_pairs_lifts_every_batch(hip_lib, family, side):
    from allwave_amd import ffi
    seqs, lens, pairs, regions = family
    mask = ffi.lift_from(side)
    tables = []
    for max_batch in (0, 16):
        e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=max_batch)
        try:
            e.set_sequences(seqs)
            plain, plain_cigars = e.align_pairs(SCORES, pairs)
            e.lift_begin(regions, side)
            res, cigars = e.align_pairs(SCORES, pairs)
            assert res.tobytes() == plain.tobytes() and cigars == plain_cigars  # nothing else changes
            want = L.rows_of(regions, mask, items_of(pairs, res, cigars, lens), lens)
            got = table(e)
            assert got == want and len(want) > 100
            st = e.lift_stats()
            on = {g[0] for g in regions}  # a record is walked when a region lies on its source sequence: the rectangle is the whole of it
            hit = [i for i, p in enumerate(pairs) if (mask & 1 and int(p[1]) in on) or (mask & 2 and int(p[0]) in on)]
            assert st.ok == len(want) and st.queries >= st.ok and st.records == len(hit) <= 56 and st.columns == sum(len(cigars[i]) for i in hit)
            e.score_pairs(SCORES, pairs)  # a score-only call lifts nothing
            assert table(e) == want
            tables.append(got)
        finally:
            e.close()
    assert len(pairs) > 3 * 16 and tables[0] == tables[1]  # four batches, one table
    if side == "both":
        assert any(r[3] & L.ROW_REVCOMP and r[3] & L.ROW_FROM_QUERY for r in tables[0]) and any(r[11] >= 30 or r[10] >= 30 for r in tables[0])


def test_align_pairs_normalized_clipped_and_split(hip_lib, family):
    from allwave_amd import ffi
    import split_cases as S
    seqs, lens, pairs, regions = family
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=20)
    try:
        e.set_sequences(seqs)
        e.lift_begin(regions, "both")
        res, cigars = e.align_pairs(SCORES, pairs, normalize="left")
        assert table(e) == L.rows_of(regions, 3, items_of(pairs, res, cigars, lens), lens)  # of the normalized strings
        # the clip's slices, and only those that reach the least score
        _, _, clips = e.align_pairs(SCORES, pairs, clip=2)
        threshold = int(np.median(clips["score"])) + 1
        e.lift_begin(regions, "both", clip_min_score=threshold)
        res, cigars, clips = e.align_pairs(SCORES, pairs, clip=2)
        keep = [[c] if int(c["code"]) == ffi.AWV_CL_OK and int(c["score"]) >= threshold else [] for c in clips]
        assert 0 < sum(len(k) for k in keep) < len(pairs)
        want = L.rows_of(regions, 3, items_of(pairs, res, cigars, lens, slices=keep), lens)
        assert table(e) == want and len(want) > 20
    finally:
        e.close()
    seqs, pairs = S.island_set()
    lens = [len(s) for s in seqs]
    regions = [(s, b, b + 150) for s in range(len(seqs)) for b in (50, 400, 900, 1500) if b + 150 <= lens[s]]
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=5)
    try:
        e.set_sequences(seqs)
        e.lift_begin(regions, "both")
        res, cigars, (index, segs) = e.align_pairs(SCORES, pairs, split=(1, 100))
        assert sum(1 for s in segs if len(s) >= 2) >= 6
        want = L.rows_of(regions, 3, items_of(pairs, res, cigars, lens, slices=segs), lens)
        assert table(e) == want and len(want) > 20
    finally:
        e.close()


def test_align_ranges_on_both_strands(hip_lib, family):
    from allwave_amd import ffi
    seqs, lens, pairs, regions = family
    ranges = np.array([(q, t, rev, 20 + 3 * k, min(lens[q], lens[t]) - 30 - k, 0, 0) for k, (q, t, rev) in enumerate(pairs[::3])], dtype=np.int32)
    for r in ranges:  # the target interval that is homologous to the aligned copy's: the stored reverse complements count from the other end
        q, t, rev, b, e_ = (int(v) for v in r[:5])
        pb, pe = (lens[q] - e_, lens[q] - b) if rev else (b, e_)
        shift = lens[t] - lens[q] if t >= 5 else 0
        tb, te = max(pb + shift - 5, 0), min(pe + shift + 5, lens[t])
        r[5], r[6] = (tb, te) if te - tb >= 20 else (0, min(60, lens[t]))
    assert sum(1 for r in ranges if r[2]) >= 5
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=7)
    try:
        e.set_sequences(seqs)
        plain, plain_cigars = e.align_ranges(SCORES, ranges)
        e.lift_begin(regions, "both")
        res, cigars = e.align_ranges(SCORES, ranges)
        assert res.tobytes() == plain.tobytes() and cigars == plain_cigars and (res["status"] == 0).all()
        spans = [L.span_of_range(r, lens)[3] for r in ranges]
        want = L.rows_of(regions, 3, items_of(ranges, res, cigars, lens, spans=spans), lens)
        assert table(e) == want and len(want) > 30
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
    """10 sequences with partial homology (clip_cases.flanked_set) and regions on most of them: nested, repeated, whole."""
    seqs, _ = K.flanked_set()
    seqs = seqs[:10]
    ids = ["s%d" % i for i in range(10)]
    regions = []
    for s in (0, 1, 2, 3, 5, 8, 9):
        n = len(seqs[s])
        regions += [(s, 10, 90), (s, 40, 60), (s, n // 2, n // 2 + 1), (s, 0, n), (s, n - 120, n - 5), (s, 10, 90)]
    return ids, seqs, regions


def host_rows(host):
    lo = host.last_liftover()
    return [tuple(int(r[f]) for f in L.ROW_FIELDS) for r in lo["rows"]], lo["stats"]


def test_host_all_pairs_liftover(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs, regions = small_set
    lens = [len(s) for s in seqs]
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa")
    assert len(host.last_liftover()["rows"]) == 0 and len(plain) == 90 and any(ln.split("\t")[4] == "-" for ln in plain)
    for side, mask in (("target", 1), ("query", 2), ("both", 3)):
        got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", liftover=regions, liftover_from=side)  # (WFA orientation's own alignments do not count)
        rows, st = host_rows(host)
        assert got == plain
        want = L.rows_of(regions, mask, L.items_from_paf(got, ids, lens), lens)
        assert rows == want and len(want) > 50 and (st.ok, st.skipped, st.bad_op, st.lengths) == (len(want), 0, 0, 0) and st.kernel_ms > 0
    want_both = want
    # regions by name, the default side, two slots on one device: the slots' rows merge into the one-engine table exactly
    named = [(ids[s], b, e) for s, b, e in regions]
    two = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", liftover=named, devices=[0, 0], min_batch_pairs=16)
    rows, st = host_rows(host)
    assert sorted(two) == sorted(plain) and rows == L.rows_of(regions, 1, L.items_from_paf(plain, ids, lens), lens)
    two = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", liftover=regions, liftover_from="both", devices=[0, 0], min_batch_pairs=16)
    assert sorted(two) == sorted(plain) and host_rows(host)[0] == want_both
    # the clip's slices, and only those that reach the least score
    clipped = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left", liftover=regions, liftover_from="both")
    rows, _ = host_rows(host)
    assert clipped == host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left")
    assert 5 <= len(clipped) < 90 and rows == L.rows_of(regions, 3, L.items_from_paf(clipped, ids, lens), lens) and len(rows) > 5
    # every other consumer lifts too
    for kw in (dict(mode="for_each"), dict(mode="next", chunk=25), dict(mode="par_collect")):
        assert sorted(host.iterate(ids, seqs, SCORES_2P, orientation="wfa", liftover=regions, liftover_from="both", **kw)) == sorted(plain)
        assert host_rows(host)[0] == want_both, kw
    host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="wfa", liftover=regions, liftover_from="both")
    assert host_rows(host)[0] == want_both
    segs = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", split=2, split_min_score=60, liftover=regions, liftover_from="both", coverage="both", variants=True)
    assert len(segs) >= 5 and host_rows(host)[0] == L.rows_of(regions, 3, L.items_from_paf(segs, ids, lens), lens)
    for bad in (dict(liftover=regions, liftover_from="all"), dict(liftover_from="query"), dict(liftover=[("nobody", 1, 2)]), dict(liftover=[(0, 1)])):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, SCORES_2P, **bad)


def test_host_align_ranges_liftover(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs, regions = small_set
    lens = [len(s) for s in seqs]
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30)
    ranges = []
    for ln in plain:  # the clips of a first run, as interval pairs on both strands
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    assert sum(r[2] for r in ranges) >= 2
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, liftover=regions, liftover_from="both")
    rows, st = host_rows(host)
    assert len(got) == len(ranges) and rows == L.rows_of(regions, 3, L.items_from_paf(got, ids, lens), lens) and len(rows) > 5
    assert got == host.align_ranges(ids, seqs, ranges, SCORES_2P)


def test_cli_liftover(hip_lib, host_lib, small_set, tmp_path):
    import re
    import subprocess
    from allwave_amd import build
    ids, seqs, regions = small_set
    lens = [len(s) for s in seqs]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    bed = tmp_path / "regions.bed"
    text = "# regions\n" + "".join("%s\t%d\t%d%s\n" % (ids[s], b, e, "\tr%d\t0\t+" % k if k % 2 else "") for k, (s, b, e) in enumerate(regions))
    text += "nobody\t1\t5\ns1\t7\ns2\t5\t5\ns3\t0\t%d\n" % (lens[3] + 1)
    bed.write_text(text)
    parsed, labels, bad = L.parse_bed(text, ids, lens)
    assert parsed == regions and len(bad) == 4 and "r1" in labels and "." in labels

    def run(out, *args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_bytes(), r.stderr.splitlines()

    plain, err0 = run("plain.paf", "-p", "none")
    assert " lifted " not in err0[-1]
    for side, mask in (("target", 1), ("query", 2), ("both", 3)):
        lo = tmp_path / ("lift_%s.tsv" % side)
        got, err = run("lift_%s.paf" % side, "-p", "none", "--liftover", str(bed), "--liftover-out", str(lo), *(() if side == "target" else ("--liftover-from", side)))
        assert got == plain  # byte for byte
        assert err[:4] == ["%d %s" % b for b in bad]  # the bad lines, as --align-paf reports them
        want = L.rows_of(regions, mask, L.items_from_paf(got.decode().splitlines(), ids, lens), lens)
        lines = lo.read_text().splitlines()
        assert lines == L.format_rows(want, regions, labels, ids) and len(lines) > 50
        m = re.search(r"lifted (\d+) queries, (\d+) rows, (\d+) unaligned, [0-9.]+ ms", err[-1])
        assert m and int(m.group(2)) == len(want) and int(m.group(1)) >= len(want) + int(m.group(3)), err[-1]
    # with --align-paf, --clip, two slots, and the other per-batch passes
    paf_in = tmp_path / "map.paf"
    paf_in.write_bytes(b"\n".join(plain.splitlines()[:40]) + b"\n")
    lo = tmp_path / "lift_ranges.tsv"
    base, _ = run("ranges.paf", "--align-paf", str(paf_in), "--clip", "2")
    got, err = run("ranges_lift.paf", "--align-paf", str(paf_in), "--clip", "2", "--liftover", str(bed), "--liftover-out", str(lo), "--liftover-from", "both", "--devices", "0,0",
                   "--coverage", str(tmp_path / "cov.tsv"), "--variants", str(tmp_path / "var.tsv"), "--verify", "--normalize", "left")
    assert sorted(got.splitlines()) == sorted(run("ranges_norm.paf", "--align-paf", str(paf_in), "--clip", "2", "--normalize", "left")[0].splitlines()) and len(base) > 0
    want = L.rows_of(regions, 3, L.items_from_paf(got.decode().splitlines(), ids, lens), lens)
    assert lo.read_text().splitlines() == L.format_rows(want, regions, labels, ids) and len(want) > 5
    # usage errors exit as the others do
    for extra, word in ((["--score-only"], "--score-only"), (["--mash-matrix"], "--mash-matrix"), (["--check-paf", str(paf_in)], "--check-paf")):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--liftover", str(bed), "--liftover-out", str(tmp_path / "no.tsv")] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and "--liftover" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--liftover", str(bed)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "'--liftover' and '--liftover-out' require each other" in r.stderr and not (tmp_path / "no.tsv").exists()
