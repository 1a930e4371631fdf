"""GPU tests of the cs difference string made on the device (csrc/cs.hip): every text and every awv_cs_text is compared, byte for
byte, with the host yardstick (awv_cs_one_host) or with the Python restatement (cs_cases.cs_of) of the same op bytes -- on the
case list through awv_cs_cigars / awv_cs_ranges, and on the engine's own alignments through the cs align calls, where the inverse
(cs_cases.apply_cs) also rebuilds every pattern and CIGAR from the text and the target alone.  All comparisons are exact."""
import re

import numpy as np
import pytest

import clip_cases as K
import cs_cases as X
import encode_cases as E
import normalize_cases as N
from util import DEFAULT_2P, EDIT, rle
from verify_cases import revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list as a resident set, packed into one arena, with the yardstick's text and record for every case in both
    modes (computed once)."""
    from allwave_amd import ffi
    cl = X.case_list()
    seqs, pairs = X.resident(cl)
    recs, arena = X.pack(cl)
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == list(range(16))
    want = {}
    for mode in X.MODES:
        rows = []
        for name, p, t, ops, status, _ in cl:
            if status != 0:
                rows.append((b"", 0, X.SKIPPED))
                continue
            text, rec = ffi.cs_one_host(mode, p, t, ops)
            assert (text, int(rec["code"])) == X.cs_of(ops, p, t, mode), name
            rows.append((text, int(rec["len"]), int(rec["code"])))
        want[mode] = rows
    return cl, seqs, pairs, recs, arena, want


def check_list(engine, cases):
    cl, seqs, pairs, recs, arena, want = cases
    engine.set_sequences(seqs)
    for mode in X.MODES:
        text, csout, total = engine.cs_cigars(mode, pairs, recs, arena)
        assert total == sum(w[1] for w in want[mode]) == len(text) and E.dense(csout)
        got = E.texts_of(text, csout)
        for k, c in enumerate(cl):
            assert (got[k], int(csout[k]["len"]), int(csout[k]["code"])) == want[mode][k], (mode, c[0])
        st = engine.cs_stats()
        assert st.pairs == len(cl) and st.text_bytes == total and st.kernel_ms > 0
        assert st.failed == sum(1 for w in want[mode] if w[2] in (X.BAD_OP, X.LENGTHS)) >= 6
        assert st.columns == sum(len(c[3]) for c in cl if c[4] == 0)


@pytest.mark.parametrize("workgroups", [0, 1, 2])
def test_cs_cigars_on_the_case_list(hip_lib, cases, workgroups):
    """workgroups 1 and 2: one wave takes record after record, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)
    try:
        check_list(e, cases)
    finally:
        e.close()


def test_cs_cigars_in_several_pieces(hip_lib, cases):
    """A small max_arena_bytes cuts the list into pieces, one launch each: the offsets run on across them."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=200000)
    try:
        assert len(cases[4]) > 10 * 200000
        check_list(e, cases)
    finally:
        e.close()


@pytest.mark.parametrize("mode", X.MODES)
def test_cs_cigars_all_of_the_text_or_none_across_pieces(hip_lib, cases, mode):
    """More than ten pieces and a buffer that the text outgrows at the last piece, halfway or at the first: csout and text_bytes
    are the fitting call's, and not one byte of the buffer is written."""
    from allwave_amd import ffi
    _, seqs, pairs, recs, arena, _ = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=200000)
    try:
        assert len(arena) > 10 * 200000
        e.set_sequences(seqs)
        full, cs0, total0 = e.cs_cigars(mode, pairs, recs, arena)
        assert len(full) == total0 > 2
        for cap in (total0 - 1, total0 // 2, 1):
            buf, csout, total = e.cs_cigars(mode, pairs, recs, arena, text_cap=cap)
            assert len(buf) == cap and (buf == 0xff).all() and csout.tobytes() == cs0.tobytes() and total == total0, cap
        buf, csout, total = e.cs_cigars(mode, pairs, recs, arena, text_cap=total0 + 9)
        assert bytes(buf[:total0]) == bytes(full) and (buf[total0:] == 0xff).all() and len(buf) == total0 + 9
        assert csout.tobytes() == cs0.tobytes() and total == total0
    finally:
        e.close()


@pytest.fixture(scope="module")
def alignment_engine(hip_lib):
    """An engine whose resident set is the 300 random alignments: sequence 2 k is alignment k's pattern, 2 k + 1 its text."""
    from allwave_amd import ffi
    al = X.random_alignments()
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    e.set_sequences([s for p, t, _ in al for s in (p, t)])
    yield e, al
    e.close()


def test_cs_cigars_slices_and_refusals(hip_lib, alignment_engine):
    from allwave_amd import ffi
    e, al = alignment_engine
    picks = X.random_slices([a[2] for a in al])
    recs, arena = K.pack_arena([al[i][2] for i, _ in picks], [(3 * k + 1) % 16 for k in range(len(picks))])
    pairs = np.array([(2 * i, 2 * i + 1, 0) for i, _ in picks], dtype=np.int32)
    slices = np.array([sl for _, sl in picks], dtype=np.int64)
    for mode in X.MODES:
        text, csout, total = e.cs_cigars(mode, pairs, recs, arena, slices=slices)
        want = [X.cs_of(al[i][2], al[i][0], al[i][1], mode, sl) for i, sl in picks]
        assert E.texts_of(text, csout) == [w[0] for w in want] and E.dense(csout) and total == sum(len(w[0]) for w in want)
        assert all(w[1] == X.OK for w in want) and (csout["code"] == X.OK).all()
    assert sum(1 for i, sl in picks if sl[0] == sl[1]) >= 20  # empty slices
    n_cut = sum(1 for i, (b, en, _, _) in picks if 0 < b < en < len(al[i][2]) and al[i][2][b - 1] == al[i][2][b] and al[i][2][en - 1] == al[i][2][en])
    assert n_cut >= 20  # slices that begin and end inside a run
    # skips that leave too little of a sequence: AWV_CST_LENGTHS, no text
    sl = slices.copy()
    sl[3] = (0, 0, 10 ** 9, 0)
    sl[4][3] = len(al[picks[4][0]][1]) + 1
    _, csout, _ = e.cs_cigars("long", pairs, recs, arena, slices=sl)
    assert [int(c) for c in csout["code"][3:5]] == [X.LENGTHS, X.LENGTHS] and E.dense(csout) and (csout["len"][3:5] == 0).all()

    def refused(*args, **kw):
        with pytest.raises(ffi.EngineError) as err:
            e.cs_cigars(*args, **kw)
        assert err.value.code == ffi.AWV_ERR_ARG

    for k, bad in ((0, (5, 4, 0, 0)), (1, (0, int(recs[1]["cigar_len"]) + 1, 0, 0)), (2, (0, 0, -1, 0)), (2, (0, 0, 0, -1))):
        sl = slices.copy()
        sl[k] = bad
        refused("short", pairs, recs, arena, slices=sl)
    for mode in (0, 3, -1):
        refused(mode, pairs, recs, arena)
    out = recs.copy()
    out[2]["cigar_off"] = len(arena)  # a completed record outside the arena
    out[2]["cigar_len"] = 1
    refused("short", pairs, out, arena)
    far = pairs.copy()
    far[5][0] = 2 * len(al)  # a sequence index outside the set
    refused("short", far, recs, arena)
    text, csout, total = e.cs_cigars("short", pairs[:0], recs[:0], b"")
    assert len(csout) == 0 and total == 0
    bare = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)  # no sequence set
    try:
        with pytest.raises(ffi.EngineError) as err:
            bare.cs_cigars("short", pairs, recs, arena)
        assert err.value.code == ffi.AWV_ERR_STATE
    finally:
        bare.close()


def test_cs_cigars_measuring_call(hip_lib, alignment_engine):
    """text_buf == NULL, and a text_cap that is too small: csout and text_bytes are filled, nothing is written."""
    e, al = alignment_engine
    al = al[:60]
    recs, arena = K.pack_arena([a[2] for a in al])
    pairs = np.array([(2 * i, 2 * i + 1, 0) for i in range(len(al))], dtype=np.int32)
    for mode in X.MODES:
        want = [X.cs_of(ops, p, t, mode)[0] for p, t, ops in al]
        full, cs0, total0 = e.cs_cigars(mode, pairs, recs, arena)
        assert E.texts_of(full, cs0) == want
        none, csout, total = e.cs_cigars(mode, pairs, recs, arena, want_text=False)
        assert none is None and total == total0 == sum(len(w) for w in want) and csout.tobytes() == cs0.tobytes()
        for cap in (total0 - 1, 1):
            buf, csout, total = e.cs_cigars(mode, pairs, recs, arena, text_cap=cap)
            assert total == total0 and csout.tobytes() == cs0.tobytes() and (buf == 0xff).all() and len(buf) == cap
        buf, csout, total = e.cs_cigars(mode, pairs, recs, arena, text_cap=total0 + 9)
        assert bytes(buf[:total0]) == bytes(full) and (buf[total0:] == 0xff).all()


def test_cs_ranges_on_both_strands(hip_lib):
    from allwave_amd import ffi
    seqs, ranges, seen = X.range_cases()
    recs, arena = K.pack_arena([ops for _, _, ops in seen])
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=3)
    try:
        e.set_sequences(seqs)
        assert sum(1 for r in ranges if r[2]) >= 15 and any(r[3] == r[4] for r in ranges)
        for mode in X.MODES:
            text, csout, total = e.cs_ranges(mode, ranges, recs, arena)
            want = [X.cs_of(ops, p, t, mode) for p, t, ops in seen]
            assert E.texts_of(text, csout) == [w[0] for w in want] and (csout["code"] == X.OK).all() and E.dense(csout)
            for (p, t, ops), got in zip(seen, E.texts_of(text, csout)):
                assert X.apply_cs(t, got) == (p, rle(ops))
        # one base cut off an interval that the string consumes to its end: AWV_CST_LENGTHS; an interval outside its sequence is refused
        k = next(i for i, (p, t, ops) in enumerate(seen) if len(t) > 0 and not ranges[i][2])
        cut = ranges.copy()
        cut[k][6] -= 1
        _, csout, _ = e.cs_ranges("short", cut, recs, arena)
        assert int(csout[k]["code"]) == X.LENGTHS and int(csout[k]["len"]) == 0
        cut[k][6] = len(seqs[cut[k][1]]) + 1
        with pytest.raises(ffi.EngineError) as err:
            e.cs_ranges("short", cut, recs, arena)
        assert err.value.code == ffi.AWV_ERR_ARG
    finally:
        e.close()


# ---- the cs align calls -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def repeat_set():
    return N.repeat_set()


def check_cs(seqs, pairs, res, cigars, cs, mode, clips=None):
    """Every cs text is cs_of on the op bytes that came back (the clip's slice with its skips, where there is one), the layout is
    dense, and apply_cs rebuilds the pattern and the cg:Z: text from the cs text and the target alone."""
    texts, csout = cs
    assert E.dense(csout)
    for k, (r, ops) in enumerate(zip(res, cigars)):
        p, t = seqs[pairs[k][0]], seqs[pairs[k][1]]
        if r["status"] != 0 or (clips is not None and clips[k]["code"] != K.OK):
            assert (texts[k], int(csout[k]["code"]), int(csout[k]["len"])) == (b"", X.SKIPPED, 0), k
            continue
        sl = None if clips is None else tuple(int(clips[k][f]) for f in ("col_beg", "col_end", "q_skip", "t_skip"))
        assert (texts[k], int(csout[k]["code"])) == X.cs_of(ops, p, t, mode, sl), k
        b, e, qs, ts = sl if sl else (0, len(ops), 0, 0)
        seg = ops[b:e]
        assert X.apply_cs(t[ts:], texts[k]) == (p[qs:qs + len(seg) - seg.count(b"I")], rle(seg)), k


@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT], ids=["2-piece", "edit"])
def test_align_pairs_cs(hip_lib, engine, repeat_set, scores, mode):
    from allwave_amd import ffi
    seqs, pairs, _ = repeat_set
    engine.set_sequences(seqs)
    res0, cig0 = engine.align_pairs(scores, pairs)
    assert (res0["status"] == 0).all()
    res, cig, cs = engine.align_pairs(scores, pairs, cs=mode)
    assert res.tobytes() == res0.tobytes() and cig == cig0
    check_cs(seqs, pairs, res, cig, cs, mode)
    st = engine.cs_stats()
    assert st.pairs == len(pairs) and st.failed == 0 and st.columns == int(res0["cigar_len"].sum()) and st.kernel_ms > 0
    assert st.text_bytes == sum(len(t) for t in cs[0]) > 0
    # a bound that puts some pairs above it: no text for them
    bounds = np.where(np.arange(len(pairs)) % 3 == 0, res0["penalty"] // 2, -1).astype(np.int32)
    resb, cigb = engine.align_pairs(scores, pairs, max_penalty=bounds)
    res, cig, cs = engine.align_pairs(scores, pairs, max_penalty=bounds, cs=mode)
    assert res.tobytes() == resb.tobytes() and cig == cigb and (res["status"] == ffi.AWV_ST_ABOVE_BOUND).sum() >= 3
    check_cs(seqs, pairs, res, cig, cs, mode)
    # normalize left, verify, clip and the run-length text, together: everything else is the call's without cs
    resn, textn, vn, cn, tn = engine.align_pairs(scores, pairs, normalize="left", verify=True, clip=1, encode=True)
    _, cign = engine.align_pairs(scores, pairs, normalize="left")
    res, text, vres, cres, tres, cs = engine.align_pairs(scores, pairs, normalize="left", verify=True, clip=1, encode=True, cs=mode)
    assert res.tobytes() == resn.tobytes() and text == textn and vres.tobytes() == vn.tobytes() and cres.tobytes() == cn.tobytes()
    assert tres.tobytes() == tn.tobytes() and (vres["code"] == 0).all()
    check_cs(seqs, pairs, res, cign, cs, mode, cres)
    for k in np.flatnonzero(cres["code"] == K.OK):  # the rebuilt CIGAR is the cg:Z: text
        assert X.apply_cs(seqs[pairs[k][1]][int(cres[k]["t_skip"]):], cs[0][k])[1].encode() == text[k]
    assert sum(1 for k in range(len(pairs)) if cn[k]["code"] == K.OK and cn[k]["col_end"] - cn[k]["col_beg"] < res0[k]["cigar_len"]) >= 3
    # without the run-length text the sink's first arena is the op bytes
    res, cig, cres, cs = engine.align_pairs(scores, pairs, normalize="left", clip=1, cs=mode)
    assert res.tobytes() == resn.tobytes() and cig == cign and cres.tobytes() == cn.tobytes()
    check_cs(seqs, pairs, res, cig, cs, mode, cres)


@pytest.mark.parametrize("mode", X.MODES)
def test_align_cs_ranges_batches_and_keep_on_device(hip_lib, mode):
    import random
    from allwave_amd import ffi
    seqs, pairs = K.flanked_set(n_pairs=14)
    rng = random.Random(83)
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=5)  # three batches: the first two go through the helper-thread sink
    try:
        e.set_sequences(seqs)
        res0, cig0, c0 = e.align_pairs(DEFAULT_2P, pairs, clip=1)
        res, cig, cres, cs = e.align_pairs(DEFAULT_2P, pairs, clip=1, cs=mode)
        assert res.tobytes() == res0.tobytes() and cig == cig0 and cres.tobytes() == c0.tobytes()
        for first in (0, 5, 10):  # every batch has a cs arena of its own
            assert E.dense(cs[1][first:first + 5])
        assert any(rev for _, _, rev in pairs)
        pats = [revcomp(seqs[q]) if rev else seqs[q] for q, _, rev in pairs]
        flat = [s for k, (q, t, rev) in enumerate(pairs) for s in (pats[k], seqs[t])]
        as_seen = np.array([(2 * k, 2 * k + 1, 0) for k in range(len(pairs))], dtype=np.int32)
        for first in (0, 5, 10):
            sl = slice(first, first + 5)
            check_cs(flat, as_seen[sl], res[sl], cig[sl], (cs[0][sl], cs[1][sl]), mode, cres[sl])
        res, text, tres, cs = e.align_pairs(DEFAULT_2P, pairs, encode=True, cs=mode)
        assert text == [rle(c).encode() for c in cig0] and e.cs_stats().pairs == len(pairs)
        for first in (0, 5, 10):
            sl = slice(first, first + 5)
            check_cs(flat, as_seen[sl], res[sl], cig0[sl], (cs[0][sl], cs[1][sl]), mode)
        ranges, seen = [], []
        for k, (q, t, rev) in enumerate(pairs):
            ql, tl = len(seqs[q]), len(seqs[t])
            r = (q, t, rev, rng.randint(0, ql // 4), rng.randint(3 * ql // 4, ql), rng.randint(0, tl // 4), rng.randint(3 * tl // 4, tl))
            ranges.append(r)
            seen += [revcomp(seqs[q][r[3]:r[4]]) if rev else seqs[q][r[3]:r[4]], seqs[t][r[5]:r[6]]]
        ranges.append((0, 1, 0, 5, 5, 7, 7))   # an empty CIGAR: empty text
        ranges.append((0, 1, 0, 5, 5, 7, 90))  # one run of 'I'
        seen += [b"", b"", b"", seqs[1][7:90]]
        as_seen = np.array([(2 * k, 2 * k + 1, 0) for k in range(len(ranges))], dtype=np.int32)
        resr, cigr = e.align_ranges(DEFAULT_2P, ranges)
        res, cig, cs = e.align_ranges(DEFAULT_2P, ranges, cs=mode)
        assert res.tobytes() == resr.tobytes() and cig == cigr
        cigs = [c if c is not None else b"" for c in cig]
        for first in range(0, len(ranges), 5):
            sl = slice(first, first + 5)
            check_cs(seen, as_seen[sl], res[sl], cigs[sl], (cs[0][sl], cs[1][sl]), mode)
        assert cs[0][-2] == b"" and cs[0][-1] == (b"-" + seqs[1][7:90].lower())
        resr, cigr, cr = e.align_ranges(EDIT, ranges, clip=2)
        res, cig, cres, cs = e.align_ranges(EDIT, ranges, clip=2, cs=mode)
        assert res.tobytes() == resr.tobytes() and cres.tobytes() == cr.tobytes() and cig == cigr
        cigs = [c if c is not None else b"" for c in cig]
        for first in range(0, len(ranges), 5):
            sl = slice(first, first + 5)
            check_cs(seen, as_seen[sl], res[sl], cigs[sl], (cs[0][sl], cs[1][sl]), mode, cres[sl])
        assert [int(c) for c in cr["code"][-2:]] == [K.EMPTY, K.EMPTY] and [int(c) for c in cs[1]["code"][-2:]] == [X.SKIPPED, X.SKIPPED]
        with pytest.raises(ValueError):
            e.align_pairs(DEFAULT_2P, pairs, cs=mode, split=(1, 10))
        with pytest.raises(ValueError):
            e.align_pairs(DEFAULT_2P, pairs, cs="medium")
    finally:
        e.close()
    keep = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_KEEP_ON_DEVICE)
    try:
        keep.set_sequences(seqs)
        plain, _ = keep.align_pairs(DEFAULT_2P, pairs)
        res, cig, cs = keep.align_pairs(DEFAULT_2P, pairs, cs=mode)  # the step runs, csout is filled, nothing is copied
        assert res.tobytes() == plain.tobytes() and all(c is None for c in cig) and all(t is None for t in cs[0]) and E.dense(cs[1])
        pats = [revcomp(seqs[q]) if rev else seqs[q] for q, _, rev in pairs]
        assert [int(n) for n in cs[1]["len"]] == [len(X.cs_of(c, pats[k], seqs[pairs[k][1]], mode)[0]) for k, c in enumerate(cig0)]
    finally:
        keep.close()


# ---- the host layer and the command-line tool ----------------------------------------------------------------------------------

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


def tag_of(line, by_id, mode):
    """The cs text of a PAF line, computed from the line's coordinates, its cg:Z: text and the sequences alone."""
    f = line.split("\t")
    q, t = by_id[f[0]], by_id[f[5]]
    pattern, text = q[int(f[2]):int(f[3])], t[int(f[7]):int(f[8])]
    if f[4] == "-":
        pattern = revcomp(pattern)
    cg = next(x for x in f[12:] if x.startswith("cg:Z:"))[5:]
    ops = b"".join({"=": b"M", "X": b"X", "I": b"D", "D": b"I"}[c] * int(n) for n, c in re.findall(r"(\d+)([=XID])", cg))
    got, code = X.cs_of(ops, pattern, text, mode)
    assert code == X.OK and X.apply_cs(text, got) == (pattern, cg)
    return got.decode()


def with_tags(lines, by_id, mode):
    return [ln + "\tcs:Z:" + tag_of(ln, by_id, mode) for ln in lines]


@pytest.mark.parametrize("mode", X.MODES)
def test_host_all_pairs_cs(hip_lib, host_lib, small_set, mode):
    host = host_lib
    ids, seqs = small_set
    by_id = dict(zip(ids, seqs))
    want = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa")
    assert len(want) == 90 and host.last_cs() == dict(pairs=0, failed=0, text_bytes=0, columns=0, kernel_ms=0.0)
    assert any(ln.split("\t")[4] == "-" for ln in want)
    tagged = with_tags(want, by_id, mode)
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", cs=mode)  # one slot: in list order
    lc = host.last_cs()
    assert got == tagged
    assert (lc["pairs"], lc["failed"], lc["text_bytes"]) == (90, 0, sum(len(g.rsplit("\tcs:Z:", 1)[1]) for g in got)) and lc["kernel_ms"] > 0
    assert sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", cs=mode, devices=[0, 0], min_batch_pairs=16)) == sorted(tagged)  # two slots
    assert host.last_cs()["text_bytes"] == lc["text_bytes"]
    assert host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", cs=mode, device_cigar=True) == tagged
    wantc = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left", verify=True, max_penalty=6000)
    gotc = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left", verify=True, max_penalty=6000,
                              device_cigar=True, cs=mode)
    assert gotc == with_tags(wantc, by_id, mode) and 5 <= len(wantc) < 90 and host.last_verify()["failures"] == []
    # the consumers that hand out alignment records ignore the setting; the counting consumer takes it
    assert sorted(host.iterate(ids, seqs, SCORES_2P, mode="par_collect", orientation="wfa", cs=mode)) == sorted(want)
    assert host.last_cs()["pairs"] == 0
    nb, nl, _, _ = host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="wfa", cs=mode)
    assert (nb, nl) == (sum(len(ln) + 1 for ln in tagged), 90) and host.last_cs()["text_bytes"] == lc["text_bytes"]


def test_host_align_ranges_cs(hip_lib, host_lib, small_set):
    import random
    host = host_lib
    ids, seqs = small_set
    by_id = dict(zip(ids, seqs))
    rng = random.Random(84)
    ranges = []
    for k in range(5):
        for rev in (0, 1):
            q, t = 2 * k, 2 * k + 1
            ql, tl = len(seqs[q]), len(seqs[t])
            ranges.append((q, t, rev, 0, ql, 0, tl))
            ranges.append((q, t, rev, rng.randint(0, ql // 3), rng.randint(2 * ql // 3, ql), rng.randint(0, tl // 3), rng.randint(2 * tl // 3, tl)))
    want = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    for mode in X.MODES:
        assert host.align_ranges(ids, seqs, ranges, SCORES_2P, cs=mode) == with_tags(want, by_id, mode)
        assert host.last_cs()["pairs"] == len(ranges)
    wantc = host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1)
    assert host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1, cs="short", device_cigar=True) == with_tags(wantc, by_id, "short")


def test_cli_cs(hip_lib, host_lib, small_set, tmp_path):
    import subprocess
    from allwave_amd import build
    ids, seqs = small_set
    by_id = dict(zip(ids, seqs))
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(out, *args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_text().splitlines(), r.stderr.splitlines()[-1]

    plain, summary0 = run("plain.paf", "-p", "none")
    for mode in X.MODES:
        got, summary = run("cs_%s.paf" % mode, "-p", "none", "--cs", mode)
        assert got == with_tags(plain, by_id, mode) and len(plain) == 90 and " cs " not in summary0
        m = re.search(r"cs (\d+) pairs, (\d+) failed, (\d+) text bytes, [0-9.]+ ms", summary)
        assert m and tuple(int(v) for v in m.groups()) == (90, 0, sum(len(g.rsplit("\tcs:Z:", 1)[1]) for g in got)), summary
    base, _ = run("clip.paf", "-p", "none", "--clip", "2", "--normalize", "left")
    got, summary = run("all.paf", "-p", "none", "--cs", "short", "--device-cigar", "--clip", "2", "--normalize", "left", "--verify")
    assert got == with_tags(base, by_id, "short") and 5 <= len(base) <= 90 and ", 0 failed" in summary and "encoded 90 pairs" in summary
    got, _ = run("two.paf", "-p", "none", "--cs", "long", "--devices", "0,0", "--forward-only")
    fwd, _ = run("fwd.paf", "-p", "none", "--forward-only")
    assert sorted(got) == sorted(with_tags(fwd, by_id, "long"))
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(plain[:40]) + "\n")
    base, _ = run("plain2.paf", "--align-paf", str(paf_in), "--normalize", "right")
    got, summary = run("cs2.paf", "--align-paf", str(paf_in), "--normalize", "right", "--cs", "long")
    assert got == with_tags(base, by_id, "long") and len(base) == 40 and "cs 40 pairs" in summary
