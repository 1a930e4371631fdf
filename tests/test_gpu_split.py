"""GPU tests of splitting into all good segments (csrc/split.hip): every device index entry and segment is compared, field for
field, with the host yardstick (awv_split_one_host) on the same op bytes -- on synthetic op strings through awv_split_cigars,
on the engine's own alignments through the splitting align calls, and through the host layer and the command-line tool."""
import random

import numpy as np
import pytest

import clip_cases as K
import split_cases as S
from util import DEFAULT_2P

pytestmark = pytest.mark.gpu

P1 = (0, 4, 6, 2)
UNIT = (0, 1, 1, 1)
SENTINEL = 0x5A


def yardstick(ffi, scores, a, min_score, recs, cigars):
    """[((code, count, column), [segment tuples])] of the host yardstick for records and their op strings."""
    out = []
    for r, ops in zip(recs, cigars):
        out.append(S.got(*ffi.split_one_host(scores, a, min_score, ops)) if r["status"] == 0 else ((K.SKIPPED, 0, -1), []))
    return out


def found(index, segs):
    return [S.got(index[i], segs[i]) for i in range(len(index))]


@pytest.fixture(scope="module")
def bare_engine(hip_lib):
    """An engine that never gets a sequence set: splitting reads none."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synthetic():
    """[(name, ops, residue of cigar_off modulo 16)]: every kernel string at a residue of its own, and the ones with the most
    structure at every residue."""
    rng = random.Random(91)
    base = S.kernel_strings(rng)
    out = [(name, ops, (3 * k + 1) % 16) for k, (name, ops) in enumerate(base)]
    for name, ops in base:
        if name in ("islands n=2049", "three-level recursion", "gap over the remainder's chunk boundary", "two equal-score segments over a chunk boundary",
                    "remainder of length 1 (left)"):
            out += [(name, ops, sh) for sh in range(16)]
    return out


def sentinel_slots(ffi, n):
    return np.frombuffer(bytes([SENTINEL]) * (max(n, 1) * ffi.CLIP_DTYPE.itemsize), dtype=ffi.CLIP_DTYPE).copy()


def check_cigars(ffi, engine, scores, a, min_score, strings, residues, status=None, lie=None):
    recs, arena = K.pack_arena(strings, residues, status)
    if lie is not None:
        recs["num_matches"] = lie
    need = [ffi.split_slots(a, min_score, len(ops)) if recs[k]["status"] == 0 else 0 for k, ops in enumerate(strings)]
    seg_first = np.concatenate(([0], np.cumsum(need))).astype(np.uint64)
    slots = sentinel_slots(ffi, int(seg_first[-1]))
    index, segs = engine.split_cigars(scores, a, min_score, recs, arena, seg_first=seg_first, slots=slots)
    got = found(index, segs)
    raw = slots.view(np.uint8).reshape(len(slots), -1)
    for k, ops in enumerate(strings):
        want = S.got(*ffi.split_one_host(scores, a, min_score, ops)) if recs[k]["status"] == 0 else ((K.SKIPPED, 0, -1), [])
        assert got[k] == want, (k, len(ops), residues[k], scores, a, min_score)
        lo, hi = int(seg_first[k]) + want[0][1], int(seg_first[k + 1])
        assert (raw[lo:hi] == SENTINEL).all(), (k, "a slot beyond count was written")
    return got


@pytest.mark.parametrize("scores,a,min_score", [(DEFAULT_2P, 1, 20), (UNIT, 1, 1), (P1, 2, 30)], ids=["2-piece", "unit-min1", "1-piece"])
def test_split_cigars_on_synthetic_strings(hip_lib, bare_engine, synthetic, scores, a, min_score):
    from allwave_amd import ffi
    names = [s[0] for s in synthetic]
    assert sorted(set(s[2] for s in synthetic)) == list(range(16))
    got = check_cigars(ffi, bare_engine, scores, a, min_score, [s[1] for s in synthetic], [s[2] for s in synthetic])
    st = bare_engine.split_stats()
    assert st.pairs == len(synthetic) and st.columns == sum(len(s[1]) for s in synthetic) and st.kernel_ms > 0
    assert st.segments == sum(g[0][1] for g in got) and st.empty == sum(1 for g in got if g[0][0] == K.EMPTY)
    assert st.columns_scanned >= st.columns
    by_name = {n: g for n, g in zip(names, got)}
    if scores == DEFAULT_2P:  # the cases are what their names say
        assert by_name["three-level recursion"][0][1] == 15
        two = by_name["two equal-score segments"]
        assert two[0][1] == 2 and two[1][0][2] == two[1][1][2] == 40
        assert sorted(set(g[1][1][3] % 16 for n, g in zip(names, got) if n.startswith("col_beg = "))) == list(range(16))
        sides = [g[1][1][3] - 1024 for n, g in zip(names, got) if n.startswith("col_beg at chunk boundary")]
        assert min(sides) < 0 < max(sides) and 0 in sides
        assert by_name["all X"][0] == (K.EMPTY, 0, -1) and by_name["all X over chunks"][0] == (K.EMPTY, 0, -1)
        assert by_name["gap over the remainder's chunk boundary"][0][1] == 2 and by_name["gap over the remainder's chunk boundary"][1][1][9] == 48
        assert by_name["long gap inside a right remainder"][0][1] == 3
    if min_score == 1:  # "M X M..." leaves [0, 2), whose clip [0, 1) leaves the remainder [1, 2)
        assert by_name["remainder of length 1 (left)"][0][1] == 2 and by_name["remainder of length 1 (left)"][1][0][3:5] == (0, 1)
        assert st.columns_scanned > st.columns


def test_split_cigars_lies_errors_and_mixed_batch(hip_lib, bare_engine):
    from allwave_amd import ffi
    rng = random.Random(92)
    strings, residues, status = [], [], []
    for sh in (0, 7, 15):
        for byte in (1023, 2047, 16):  # a bad byte in a later chunk, behind a good segment: still the clip's answer
            ops = bytearray(K.random_ops(rng, 2500, alphabet=b"MMMMXID"))
            ops[byte - sh] = ord("N")
            ops[byte - sh + 300] = ord("=")
            strings.append(bytes(ops))
            residues.append(sh)
            status.append(0)
    n_bad = len(strings)
    for k in range(40):  # SKIPPED, EMPTY and OK records side by side
        kind = k % 4
        strings.append([K.random_ops(rng, rng.randint(1, 1500), alphabet=b"MMMMMXID"), b"X" * rng.randint(1, 1200), b"",
                        K.random_ops(rng, rng.randint(1, 1500))][kind])
        residues.append(rng.randrange(16))
        status.append(rng.choice([1, 2, 3, 4]) if kind == 3 else 0)
    # records that misstate num_matches (0, and far more than the string holds): the slot rule goes by cigar_len
    for lie in (0, 2 ** 31 - 1):
        got = check_cigars(ffi, bare_engine, DEFAULT_2P, 2, 9, strings, residues, status, lie=lie)
        assert all(g[0][0] == K.BAD_OP and g[0][1] == 0 and g[0][2] >= 0 for g in got[:n_bad])
        codes = [g[0][0] for g in got[n_bad:]]
        assert codes.count(K.SKIPPED) == 10 and codes.count(K.EMPTY) >= 20 and codes.count(K.OK) >= 5
    st = bare_engine.split_stats()
    assert st.pairs == len(strings) and st.empty == codes.count(K.EMPTY)
    recs, arena = K.pack_arena(strings[n_bad:n_bad + 3], residues[n_bad:n_bad + 3])
    # a completed record whose op bytes lie outside the arena
    bad = recs.copy()
    bad[1]["cigar_len"] = len(arena)
    with pytest.raises(ffi.EngineError) as err:
        bare_engine.split_cigars(DEFAULT_2P, 1, 10 ** 9, bad, arena)
    assert err.value.code == ffi.AWV_ERR_ARG
    # an undersized seg_first: refused before any launch -- nothing is written and the last call's stats stay
    need = [ffi.split_slots(1, 5, int(r["cigar_len"])) for r in recs]
    seg_first = np.concatenate(([0], np.cumsum(need))).astype(np.uint64)
    slots = sentinel_slots(ffi, int(seg_first[-1]))
    short = seg_first.copy()
    short[1] -= 1  # (record 0 loses a slot to record 1)
    with pytest.raises(ffi.EngineError) as err:
        bare_engine.split_cigars(DEFAULT_2P, 1, 5, recs, arena, seg_first=short, slots=slots)
    assert err.value.code == ffi.AWV_ERR_ARG and (slots.view(np.uint8) == SENTINEL).all()
    assert bare_engine.split_stats().pairs == len(strings)
    descending = seg_first.copy()
    descending[2] = descending[1] - 1
    with pytest.raises(ffi.EngineError) as err:
        bare_engine.split_cigars(DEFAULT_2P, 1, 5, recs, arena, seg_first=descending, slots=slots)
    assert err.value.code == ffi.AWV_ERR_ARG
    for a, min_score in ((0, 5), (32768, 5), (1, 0), (1, -7)):
        with pytest.raises(ffi.EngineError) as err:
            bare_engine.split_cigars(DEFAULT_2P, a, min_score, recs, arena, seg_first=seg_first, slots=slots)
        assert err.value.code == ffi.AWV_ERR_ARG
    index, segs = bare_engine.split_cigars(DEFAULT_2P, 1, 5, recs, arena, seg_first=seg_first, slots=slots)
    assert found(index, segs) == yardstick(ffi, DEFAULT_2P, 1, 5, recs, strings[n_bad:n_bad + 3])
    index, segs = bare_engine.split_cigars(DEFAULT_2P, 1, 5, recs[:0], b"")
    assert len(index) == 0 and segs == []


def test_split_cigars_in_several_pieces(hip_lib, synthetic):
    """A small max_arena_bytes: the arena goes up in several pieces, one launch each, into one slot layout."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=8192)
    try:
        part = synthetic[::5]
        got = check_cigars(ffi, e, DEFAULT_2P, 1, 20, [s[1] for s in part], [s[2] for s in part])
        st = e.split_stats()
        assert st.pairs == len(part) and st.columns == sum(len(s[1]) for s in part) and st.segments == sum(g[0][1] for g in got)
    finally:
        e.close()


# ---- the splitting align calls ----------------------------------------------------------------------------------------------

A, MIN_SCORE = 1, 30


@pytest.fixture(scope="module")
def islands():
    return S.island_set()


@pytest.fixture(scope="module")
def plain(hip_lib, islands):
    """The unsplit call's records, op strings and verify results on the island set, and the yardstick's split of them: once."""
    from allwave_amd import ffi
    seqs, pairs = islands
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        res0, cig0, v0 = e.align_pairs(DEFAULT_2P, pairs, verify=True)
        clips = e.clip_cigars(DEFAULT_2P, A, *K.pack_arena(cig0))
    finally:
        e.close()
    assert (res0["status"] == 0).all() and (v0["code"] == 0).all()
    return res0, cig0, v0, yardstick(ffi, DEFAULT_2P, A, MIN_SCORE, res0, cig0), clips


def test_align_pairs_split(hip_lib, engine, islands, plain):
    from allwave_amd import ffi
    seqs, pairs = islands
    res0, cig0, v0, want, clips = plain
    engine.set_sequences(seqs)
    # the layout helper's arithmetic
    seg_first = engine.split_layout(pairs, A, MIN_SCORE)
    need = [ffi.split_slots(A, MIN_SCORE, min(len(seqs[q]), len(seqs[t]))) for q, t, _ in pairs]
    assert seg_first.tolist() == [0] + np.cumsum(need).tolist()
    seen = []

    def hook(first, n, sp):
        index, sf, slots = sp
        seen.append((first, n, [S.got(index[i], slots[int(sf[i]):int(sf[i]) + int(index["count"][i])]) for i in range(first, first + n)]))

    res, cigs, vres, (index, segs) = engine.align_pairs(DEFAULT_2P, pairs, verify=True, split=(A, MIN_SCORE), _sink_hook=hook)
    assert res.tobytes() == res0.tobytes() and cigs == cig0 and vres.tobytes() == v0.tobytes()
    assert found(index, segs) == want
    assert sum(n for _, n, _ in seen) == len(pairs)
    for first, n, got in seen:  # iout / sout are filled before the batch's sink call
        assert got == want[first:first + n]
    st = engine.split_stats()
    assert st.pairs == len(pairs) and st.columns == int(res0["cigar_len"].sum()) and st.segments == sum(w[0][1] for w in want)
    # the set is what the issue asks for: most pairs break into several segments
    assert sum(1 for w in want if w[0][1] >= 2) >= 8 and max(w[0][1] for w in want) >= 3
    # a clip that reaches min_score is its pair's top-scoring segment
    for w, cl in zip(want, clips):
        if cl["code"] == K.OK and cl["score"] >= MIN_SCORE:
            assert K.as_tuple(cl) in w[1] and int(cl["score"]) == max(s[2] for s in w[1])
        else:
            assert w[0][1] == 0
    # without verify the split comes third
    res2, cigs2, (index2, segs2) = engine.align_pairs(DEFAULT_2P, pairs, split=(A, MIN_SCORE))
    assert res2.tobytes() == res0.tobytes() and cigs2 == cig0 and found(index2, segs2) == want
    with pytest.raises(ValueError):
        engine.align_pairs(DEFAULT_2P, pairs, split=(A, MIN_SCORE), clip=1)


def test_align_pairs_split_refuses_a_short_layout(hip_lib, islands):
    """The C call itself: a record with fewer slots than awv_split_slots(a, min_score, min(plen, tlen)) is AWV_ERR_ARG before
    anything is launched."""
    import ctypes as C
    from allwave_amd import ffi
    seqs, pairs = islands
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        parr = e._pair_array(pairs[:4])
        seg_first = e.split_layout(parr, A, MIN_SCORE)
        seg_first[3:] -= 1
        index = np.zeros(4, dtype=ffi.SPLIT_INDEX_DTYPE)
        slots = sentinel_slots(ffi, int(seg_first[-1]) + 1)
        res = np.zeros(4, dtype=ffi.RESULT_DTYPE)
        pen = ffi.Penalties.from_scores(DEFAULT_2P)
        e.align_pairs(DEFAULT_2P, pairs[:1])
        before = e.stats().launches
        rc = hip_lib.awv_align_pairs_split(e._h, C.byref(pen), parr.ctypes.data, 4, None, A, MIN_SCORE, res.ctypes.data, None, seg_first.ctypes.data,
                                           index.ctypes.data, slots.ctypes.data, ffi.SINK_FN(), None)
        assert rc == ffi.AWV_ERR_ARG and b"slots" in hip_lib.awv_last_error()
        assert e.stats().launches == before and (slots.view(np.uint8) == SENTINEL).all() and not res["cigar_len"].any()
    finally:
        e.close()


def test_align_ranges_split(hip_lib, engine, islands):
    from allwave_amd import ffi
    seqs, pairs = islands
    rng = random.Random(93)
    ranges = []
    for q, t, rev in pairs[:8]:
        ql, tl = len(seqs[q]), len(seqs[t])
        ranges.append((q, t, rev, 0, ql, 0, tl))
        ranges.append((q, t, rev, rng.randint(0, ql // 5), rng.randint(4 * ql // 5, ql), rng.randint(0, tl // 5), rng.randint(4 * tl // 5, tl)))
    ranges.append((0, 1, 0, 5, 5, 7, 7))   # two empty intervals: an empty CIGAR, no slot, no segment
    ranges.append((0, 1, 0, 5, 5, 7, 90))  # one run of 'I'
    engine.set_sequences(seqs)
    rarr = engine._range_array(ranges)
    seg_first = engine.split_layout(rarr, A, MIN_SCORE)
    need = [ffi.split_slots(A, MIN_SCORE, min(r[4] - r[3], r[6] - r[5])) for r in ranges]
    assert seg_first.tolist() == [0] + np.cumsum(need).tolist() and need[-1] == need[-2] == 0
    res0, cig0 = engine.align_ranges(DEFAULT_2P, ranges)
    res, cigs, (index, segs) = engine.align_ranges(DEFAULT_2P, ranges, split=(A, MIN_SCORE))
    assert res.tobytes() == res0.tobytes() and cigs == cig0
    want = yardstick(ffi, DEFAULT_2P, A, MIN_SCORE, res0, cig0)
    assert found(index, segs) == want and want[-1][0] == (K.EMPTY, 0, -1) and want[-2][0] == (K.EMPTY, 0, -1)
    assert sum(1 for w in want if w[0][1] >= 2) >= 8
    with pytest.raises(ffi.EngineError) as err:
        engine.split_layout(engine._range_array([(0, 1, 0, 5, 4, 7, 7)]), A, MIN_SCORE)
    assert err.value.code == ffi.AWV_ERR_ARG


def test_split_under_bounds_batches_and_keep_on_device(hip_lib, islands, plain):
    """Bounds: an abandoned pair comes back SKIPPED.  Several batches: every batch's segments are there at its sink call, in
    the call's one layout.  AWV_F_KEEP_ON_DEVICE: the split runs though no CIGAR comes back."""
    from allwave_amd import ffi
    seqs, pairs = islands
    res0, cig0, v0, want, _ = plain
    base = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=5)
    try:
        base.set_sequences(seqs)
        bounds = np.where(np.arange(len(pairs)) % 3 == 0, res0["penalty"] // 2, -1).astype(np.int32)
        resb, cigb = base.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds)
        seen = []

        def hook(first, n, sp):
            index, sf, slots = sp
            seen.append((first, n, [S.got(index[i], slots[int(sf[i]):int(sf[i]) + int(index["count"][i])]) for i in range(first, first + n)]))

        res, cigs, vres, (index, segs) = base.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds, verify=True, split=(A, MIN_SCORE), _sink_hook=hook)
        assert res.tobytes() == resb.tobytes() and cigs == cigb
        above = res["status"] == ffi.AWV_ST_ABOVE_BOUND
        assert above.sum() == 4 and (res["status"][~above] == 0).all() and (vres["code"][~above] == 0).all()
        got = found(index, segs)
        for k in range(len(pairs)):
            assert got[k] == (((K.SKIPPED, 0, -1), []) if above[k] else want[k]), k
        assert [s[:2] for s in seen] == [(0, 5), (5, 5), (10, 2)]
        for first, n, g in seen:
            assert g == got[first:first + n]
        assert base.split_stats().pairs == len(pairs)
    finally:
        base.close()
    keep = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_KEEP_ON_DEVICE)
    try:
        keep.set_sequences(seqs)
        res, cigs, (index, segs) = keep.align_pairs(DEFAULT_2P, pairs, split=(A, MIN_SCORE))
        assert all(c is None for c in cigs) and found(index, segs) == want
        assert (res["cigar_len"] == res0["cigar_len"]).all() and (res["penalty"] == res0["penalty"]).all()
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
def small_set(islands):
    """The first three pairs of the island set (one of them with a reverse-complemented query), all against all."""
    seqs, _ = islands
    return ["s%d" % i for i in range(6)], seqs[:6]


@pytest.mark.parametrize("orientation", ["wfa", "mash"])
def test_host_all_pairs_split(hip_lib, host_lib, small_set, orientation):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    full = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation)
    assert len(full) == 30 and host.last_split() == dict(pairs=0, segments=0, empty=0, kernel_ms=0.0)
    assert {ln.split("\t")[4] for ln in full} == {"+", "-"}
    per_line = [S.segment_lines(ffi, DEFAULT_2P, A, MIN_SCORE, ln) for ln in full]
    want = [w for lines in per_line for w in lines]
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, split=A, split_min_score=MIN_SCORE, verify=True)
    assert got == want  # (pair order, column order within a pair; a pair without a segment gives no line)
    ls = host.last_split()
    assert (ls["pairs"], ls["segments"], ls["empty"]) == (30, len(want), sum(1 for lines in per_line if not lines)) and ls["kernel_ms"] > 0
    assert max(len(lines) for lines in per_line) >= 2 and ls["empty"] > 0 and {ln.split("\t")[4] for ln in got} == {"+", "-"}
    assert host.last_verify()["pairs"] == 30 and host.last_verify()["failures"] == []  # (the full alignments are what is verified)
    # every segment's line is the global alignment of its interval pair
    rep = host.check_paf(ids, seqs, "\n".join(got) + "\n", SCORES_2P, partial=True)
    assert rep["failures"] == [] and rep["checked"] == len(got)
    assert sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, split=A, split_min_score=MIN_SCORE, devices=[0, 0],
                                     min_batch_pairs=8)) == sorted(want)
    assert host.last_split()["segments"] == len(want)
    for mode in ("for_each", "next", "par_for_each", "par_collect"):
        lines = host.iterate(ids, seqs, SCORES_2P, mode=mode, orientation=orientation, split=A, split_min_score=MIN_SCORE, chunk=7)
        assert sorted(lines) == sorted(want), mode
        if mode in ("for_each", "next", "par_collect"):
            assert lines == want, mode
    _, n_lines = host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation=orientation, split=A, split_min_score=MIN_SCORE)[:2]
    assert n_lines == len(want)
    for kw in (dict(split=A), dict(split_min_score=5), dict(split=A, split_min_score=0), dict(split=0, split_min_score=5),
               dict(split=A, split_min_score=5, clip=1)):
        with pytest.raises(ValueError):
            host.all_pairs_paf(ids, seqs, SCORES_2P, **kw)


def test_host_align_ranges_split(hip_lib, host_lib, small_set):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    rng = random.Random(94)
    ranges = []
    for k in range(3):
        for rev in (0, 1):  # both strands of every related pair (one of them the wrong one), and sub-intervals
            q, t = 2 * k, 2 * k + 1
            ql, tl = len(seqs[q]), len(seqs[t])
            ranges.append((q, t, rev, 0, ql, 0, tl))
            ranges.append((q, t, rev, rng.randint(0, ql // 5), rng.randint(4 * ql // 5, ql), rng.randint(0, tl // 5), rng.randint(4 * tl // 5, tl)))
    full = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    per_line = [S.segment_lines(ffi, DEFAULT_2P, A, MIN_SCORE, ln) for ln in full]
    want = [w for lines in per_line for w in lines]
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, split=A, split_min_score=MIN_SCORE, verify=True)
    assert got == want and host.last_split()["pairs"] == len(ranges) and host.last_split()["segments"] == len(want)
    assert sum(1 for lines in per_line if len(lines) >= 2) >= 2
    assert any(ln.split("\t")[4] == "-" and ln.split("\t")[2] != "0" for ln in got)
    rep = host.check_paf(ids, seqs, "\n".join(got) + "\n", SCORES_2P, partial=True)
    assert rep["failures"] == [] and rep["checked"] == len(got)
    assert host.align_ranges(ids, seqs, ranges, SCORES_2P, split=A, split_min_score=MIN_SCORE, devices=[0, 0]) == want


def test_cli_split(hip_lib, host_lib, small_set, tmp_path):
    import re
    import subprocess
    from allwave_amd import build
    host = host_lib
    ids, seqs = small_set
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(*args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines(), r.stderr.splitlines()[-1]

    want = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="mash", split=A, split_min_score=MIN_SCORE)
    ls = host.last_split()
    got, summary = run("-p", "none", "--split", str(A), "--split-min-score", str(MIN_SCORE), "--verify")
    assert got == want and len(got) == ls["segments"] > 30 - ls["empty"]
    m = re.search(r"split (\d+) pairs into (\d+) segments, (\d+) without a segment, [0-9.]+ ms", summary)
    assert m and tuple(int(v) for v in m.groups()) == (30, ls["segments"], ls["empty"]), summary
    # the split PAF passes the checker: every line is the global alignment of its interval pair
    out = tmp_path / "split.paf"
    out.write_text("\n".join(got) + "\n")
    c = subprocess.run([build.CLI_BIN, "-i", str(fa), "--check-paf", str(out), "-s", SCORES_2P, "--partial"], capture_output=True, text=True, timeout=120)
    assert c.returncode == 0 and c.stdout == "", (c.stdout, c.stderr)
    # --align-paf: the unsplit run's lines as the mapping; the island mappings give several lines each, in input order
    full, _ = run("-p", "none")
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(full) + "\n")
    from allwave_amd import ffi
    per_line = [S.segment_lines(ffi, DEFAULT_2P, A, MIN_SCORE, ln) for ln in full]
    got, summary = run("--align-paf", str(paf_in), "--split", str(A), "--split-min-score", str(MIN_SCORE))
    assert got == [w for lines in per_line for w in lines]
    related = [k for k, ln in enumerate(full) if (int(ln.split("\t")[0][1:]) ^ 1) == int(ln.split("\t")[5][1:])]
    assert len(related) == 6 and sum(1 for k in related if len(per_line[k]) >= 2) >= 3
    assert "split 30 pairs into %d segments, %d without a segment" % (len(got), sum(1 for lines in per_line if not lines)) in summary
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--split", "1", "--split-min-score", "30", "--clip", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "--clip" in r.stderr
