"""GPU tests of the per-base depth accumulated on the device (csrc/coverage.hip): the two tracks an engine reads back are compared,
entry for entry, with the Python restatement (coverage_cases.coverage_of) of the same op bytes -- on the case list through
awv_coverage_cigars / awv_coverage_ranges, under contention, and on the engine's own alignments through the aligning calls.
All comparisons are exact equality of uint32 arrays."""
import numpy as np
import pytest

import clip_cases as K
import coverage_cases as V
import split_cases as S
import util
from verify_cases import revcomp

pytestmark = pytest.mark.gpu

SCORES = util.DEFAULT_2P


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list packed into one arena, with what every role mask makes of it (computed once)."""
    cl = V.case_list()
    recs, arena = K.pack_arena([c[4] for c in cl], [c[7] for c in cl], [c[6] for c in cl])
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == [0, 1, 15]
    pairs = np.array([(c[1], c[2], c[3]) for c in cl], dtype=np.int32)
    slices = np.array([c[5] if c[5] is not None else (0, len(c[4]), 0, 0) for c in cl], dtype=np.int64)
    items = V.expected_items(cl)
    assert {i[0] for i in items} == {V.OK, V.SKIPPED, V.BAD_OP, V.LENGTHS}
    tracks = {roles: V.expected_tracks(cl, roles) for roles in V.ROLES}
    return cl, V.resident_set(), pairs, recs, arena, slices, items, tracks


def read(engine):
    offsets, aligned, matched = engine.coverage_read()
    assert aligned.dtype == matched.dtype == np.uint32 and len(aligned) == len(matched) == int(offsets[-1])
    return aligned, matched


@pytest.mark.parametrize("workgroups", [1, 2, 0])
@pytest.mark.parametrize("roles", V.ROLES)
def test_coverage_cigars_on_the_case_list(hip_lib, cases, roles, workgroups):
    """workgroups 1 and 2: one wave takes item after item, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, tracks = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)
    try:
        e.set_sequences(seqs)
        e.coverage_begin(V.ROLE_NAMES[roles])
        got = e.coverage_cigars(pairs, recs, arena, slices=slices)
        for k, c in enumerate(cl):
            assert tuple(int(got[k][f]) for f in ("code", "aligned_cols", "matched_cols", "boundaries")) == items[k], c[0]
        aligned, matched = read(e)
        want = tracks[roles]
        assert np.array_equal(aligned, want.aligned) and np.array_equal(matched, want.matched)
        assert int(aligned.max()) > 20 and (matched <= aligned).all()
        st = e.coverage_stats()
        assert st.items == len(cl) and st.reads == 1 and st.kernel_ms > 0
        assert st.failed == sum(1 for i in items if i[0] in (V.BAD_OP, V.LENGTHS)) >= 8
        assert st.columns == sum(len(V.case_item(c)[0]) for c in cl if c[6] == 0)
        assert st.boundaries == sum(i[3] for i in items) * bin(roles).count("1")
    finally:
        e.close()


def test_coverage_cigars_in_pieces_and_state_errors(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, items, tracks = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=4096)

    def refused(code, fn, *args, **kw):
        with pytest.raises(ffi.EngineError) as err:
            fn(*args, **kw)
        assert err.value.code == code

    try:
        refused(ffi.AWV_ERR_STATE, e.coverage_begin, "both")  # no sequence set
        e.set_sequences(seqs)
        assert e.coverage_stats().items == 0
        refused(ffi.AWV_ERR_STATE, e.coverage_cigars, pairs, recs, arena)
        refused(ffi.AWV_ERR_STATE, e.coverage_read)
        refused(ffi.AWV_ERR_ARG, e.coverage_begin, 4)
        e.coverage_begin("both")
        assert len(arena) > 10 * 4096  # more than ten pieces
        got = e.coverage_cigars(pairs, recs, arena, slices=slices)
        assert [int(c) for c in got["code"]] == [i[0] for i in items]
        assert tracks[V.BOTH].equals(*read(e))
        total = sum(V.SET_LENS)
        buf = np.zeros(total + 1, dtype=np.uint32)
        for n in (total - 1, total + 1, 0):
            assert ffi.load().awv_engine_coverage_read(e._h, buf.ctypes.data, buf.ctypes.data, n) == ffi.AWV_ERR_ARG
        assert ffi.load().awv_engine_coverage_read(e._h, None, buf.ctypes.data, total) == ffi.AWV_OK  # either pointer may be null
        assert np.array_equal(buf[:total], tracks[V.BOTH].matched)
        # refused before anything is added: an index, an arena, a slice
        bad = pairs.copy()
        bad[5][1] = len(seqs)
        refused(ffi.AWV_ERR_ARG, e.coverage_cigars, bad, recs, arena, slices=slices)
        refused(ffi.AWV_ERR_ARG, e.coverage_cigars, pairs, recs, arena[:len(arena) // 2], slices=slices)
        sl = slices.copy()
        sl[-1] = (0, 0, -1, 0)
        refused(ffi.AWV_ERR_ARG, e.coverage_cigars, pairs, recs, arena, slices=sl)
        assert tracks[V.BOTH].equals(*read(e))
        # a begin starts from zero; roles 0 and a new set end coverage
        e.coverage_begin("target")
        assert not read(e)[0].any() and e.coverage_stats().items == 0
        e.coverage_begin(None)
        refused(ffi.AWV_ERR_STATE, e.coverage_read)
        e.coverage_begin("query")
        e.set_sequences(seqs)
        refused(ffi.AWV_ERR_STATE, e.coverage_cigars, pairs, recs, arena)
    finally:
        e.close()


def test_coverage_ranges_on_both_strands(hip_lib):
    from allwave_amd import ffi
    import cs_cases as X
    seqs, ranges, seen = X.range_cases()
    lens = [len(s) for s in seqs]
    recs, arena = K.pack_arena([ops for _, _, ops in seen])
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        e.coverage_begin("both")
        got = e.coverage_ranges(ranges, recs, arena)
        want = V.Tracks(lens)
        for r, (_, _, ops) in zip(ranges, seen):
            q, t, strand, span = V.span_of_range(r, lens)
            assert want.add(q, t, ops, strand, V.BOTH, span=span) == V.OK
        assert (got["code"] == V.OK).all() and want.equals(*read(e))
        assert sum(1 for r in ranges if r[2]) >= 10
    finally:
        e.close()


def test_contention_and_reading_twice(hip_lib):
    """300 copies of one record on one pair, then a mixed list that shares one target: every copy adds the same boundary slots."""
    from allwave_amd import ffi
    seqs = V.resident_set()
    ops = b"M" * 700 + b"X" * 3 + b"I" * 5 + b"M" * 400 + b"D" * 9 + b"MX" * 40 + b"M" * 900
    recs, arena = K.pack_arena([ops], [5])
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        e.coverage_begin("both")
        got = e.coverage_cigars(np.array([(4, 5, 1)] * 300, dtype=np.int32), np.repeat(recs, 300), arena)
        assert (got["code"] == V.OK).all()
        one = V.Tracks(V.SET_LENS)
        assert one.add(4, 5, ops, "-", V.BOTH) == V.OK
        aligned, matched = read(e)
        assert np.array_equal(aligned, one.aligned * np.uint32(300)) and np.array_equal(matched, one.matched * np.uint32(300))
        # more: a list whose items all share target 5, on both strands, queries of every length
        mixed = [(q, 5, k % 2, b"D" * (k % 4) + b"M" * (V.SET_LENS[q] - 8 - k % 4) + b"XMX" + b"I" * (k % 3)) for k, q in enumerate([0, 1, 2, 3, 4, 5] * 25)]
        recs2, arena2 = K.pack_arena([m[3] for m in mixed])
        got = e.coverage_cigars(np.array([m[:3] for m in mixed], dtype=np.int32), recs2, arena2)
        assert (got["code"] == V.OK).all()
        want = V.Tracks(V.SET_LENS)  # the second read is the sum: the single record 300 times and the mixed list once
        want.add(4, 5, ops, "-", V.BOTH, times=300)
        for q, t, rev, o in mixed:
            assert want.add(q, t, o, "-" if rev else "+", V.BOTH) == V.OK
        assert want.equals(*read(e))
        assert e.coverage_stats().reads == 2 and e.coverage_stats().items == 450
    finally:
        e.close()


# ---- the aligning calls ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family():
    """8 sequences of about 600 bp, mutated copies of one; the last four are stored as reverse complements.  All 56 ordered
    pairs, q_revcomp where exactly one of the two is stored reversed."""
    import random
    rng = random.Random(520)
    root = util.rand_seq(rng, 600)
    seqs = [util.mutate(root, 0.04, rng) for _ in range(8)]
    seqs = seqs[:4] + [revcomp(s) for s in seqs[4:]]
    pairs = np.array([(q, t, int((q >= 4) != (t >= 4))) for q in range(8) for t in range(8) if q != t], dtype=np.int32)
    return seqs, pairs


def tracks_of(seqs, pairs, res, cigars, roles, slices=None, spans=None):
    """The restatement applied to the records and op bytes an aligning call returned.  slices: per pair a list of CLIP_DTYPE-like
    records that contribute (None: the whole string)."""
    lens = [len(s) for s in seqs]
    tr = V.Tracks(lens)
    n = 0
    for i, p in enumerate(pairs):
        if int(res[i]["status"]) != 0:
            continue
        q, t, rev = int(p[0]), int(p[1]), int(p[2])
        span = None if spans is None else spans[i]
        for sl in ([None] if slices is None else slices[i]):
            ops, skips = (cigars[i], (0, 0)) if sl is None else (cigars[i][int(sl["col_beg"]):int(sl["col_end"])], (int(sl["q_skip"]), int(sl["t_skip"])))
            assert tr.add(q, t, ops, "-" if rev else "+", roles, span=span, skips=skips) == V.OK
            n += 1
    return tr, n


@pytest.mark.parametrize("roles", V.ROLES)
def test_align_pairs_accumulates_every_batch(hip_lib, family, roles):
    from allwave_amd import ffi
    seqs, pairs = family
    got = []
    for max_batch in (0, 16):
        e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=max_batch)
        try:
            e.set_sequences(seqs)
            plain, plain_cigars = e.align_pairs(SCORES, pairs)
            e.coverage_begin(V.ROLE_NAMES[roles])
            res, cigars = e.align_pairs(SCORES, pairs)
            assert res.tobytes() == plain.tobytes() and cigars == plain_cigars  # nothing else changes
            want, n = tracks_of(seqs, pairs, res, cigars, roles)
            assert n == 56 and want.equals(*read(e))
            st = e.coverage_stats()
            assert st.items == 56 and st.failed == 0 and st.columns == sum(len(c) for c in cigars)
            e.score_pairs(SCORES, pairs)  # a score-only call adds nothing
            assert want.equals(*read(e))
            got.append(read(e))
        finally:
            e.close()
    assert len(pairs) > 3 * 16  # four batches
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    if roles == V.BOTH:  # every base of every sequence is aligned in all 14 alignments it takes part in, gaps aside
        assert int(got[0][0].max()) == 14 and int(np.median(got[0][0])) >= 13


def test_align_pairs_normalized_bounded_and_failing(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        e.coverage_begin("both")
        res, cigars = e.align_pairs(SCORES, pairs, normalize="left")
        plain = e.align_pairs(SCORES, pairs)[1]
        assert sum(1 for a, b in zip(cigars, plain) if a != b) >= 3  # gap runs moved: they count where they end up
        want, _ = tracks_of(seqs, pairs, res, cigars, V.BOTH)
        both, _ = tracks_of(seqs, pairs, res, plain, V.BOTH)
        want.aligned += both.aligned
        want.matched += both.matched
        assert want.equals(*read(e))
        # pairs above their bound contribute nothing
        e.coverage_begin("both")
        bounds = np.where(np.arange(len(pairs)) % 3 == 0, 5, -1).astype(np.int32)
        res, cigars = e.align_pairs(SCORES, pairs, max_penalty=bounds)
        n_above = int((res["status"] == ffi.AWV_ST_ABOVE_BOUND).sum())
        assert n_above >= 10 and int((res["status"] == 0).sum()) == len(pairs) - n_above
        want, n = tracks_of(seqs, pairs, res, cigars, V.BOTH)
        assert n == len(pairs) - n_above and want.equals(*read(e)) and e.coverage_stats().items == n
    finally:
        e.close()
    # a pair that fails (rows too narrow, no re-run) contributes nothing
    import random
    rng = random.Random(521)
    a = util.rand_seq(rng, 6000)
    wide = [a, util.mutate(a, 0.08, rng), util.mutate(a, 0.01, rng)]
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_NO_RERUN, first_row_cols=2048)
    try:
        e.set_sequences(wide)
        e.coverage_begin("both")
        p = np.array([(i, j, 0) for i in range(3) for j in range(3) if i != j], dtype=np.int32)
        res, cigars = e.align_pairs(SCORES, p)
        failed = res["status"] != 0
        assert failed.any() and not failed.all() and (res["status"][failed] == ffi.AWV_ST_CAPACITY).all()
        want, n = tracks_of(wide, p, res, cigars, V.BOTH)
        assert n == int((~failed).sum()) and want.equals(*read(e)) and e.coverage_stats().items == n
    finally:
        e.close()


def test_align_pairs_clipped_with_a_threshold(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    a = 2
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=20)
    try:
        e.set_sequences(seqs)
        _, _, clips = e.align_pairs(SCORES, pairs, clip=a)
        threshold = int(np.median(clips["score"])) + 1
        e.coverage_begin("both", clip_min_score=threshold)
        res, cigars, clips = e.align_pairs(SCORES, pairs, clip=a)
        keep = [[c] if int(c["code"]) == ffi.AWV_CL_OK and int(c["score"]) >= threshold else [] for c in clips]
        n_kept = sum(len(k) for k in keep)
        assert 0 < n_kept < len(pairs)  # the threshold drops some pairs, not all
        want, n = tracks_of(seqs, pairs, res, cigars, V.BOTH, slices=keep)
        assert n == n_kept and want.equals(*read(e)) and e.coverage_stats().items == n_kept
    finally:
        e.close()


def test_align_pairs_split_adds_every_segment(hip_lib):
    from allwave_amd import ffi
    seqs, pairs = S.island_set()
    a, min_score = 1, 100
    for roles in (V.BOTH, V.QUERY):
        e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=5)
        try:
            e.set_sequences(seqs)
            e.coverage_begin(V.ROLE_NAMES[roles])
            res, cigars, (index, segs) = e.align_pairs(SCORES, pairs, split=(a, min_score))
            assert sum(1 for s in segs if len(s) >= 2) >= 6  # islands: several segments per pair
            want, n = tracks_of(seqs, pairs, res, cigars, roles, slices=segs)
            assert n == sum(len(s) for s in segs) > len(pairs) and want.equals(*read(e)) and e.coverage_stats().items == n
        finally:
            e.close()


def test_align_ranges_on_both_strands(hip_lib, family):
    from allwave_amd import ffi
    seqs, pairs = family
    lens = [len(s) for s in seqs]
    ranges = np.array([(q, t, rev, 40 + 7 * k, lens[q] - 30 - k, 25 + 3 * k, lens[t] - 50 + k) for k, (q, t, rev) in enumerate(pairs[::3])], dtype=np.int32)
    # a forward interval [b, e) of a reversed query pairs with the target's mirrored interval
    for r in ranges:
        if r[2]:
            r[5], r[6] = max(lens[r[1]] - (r[4] + 10), 0), lens[r[1]] - r[3]
    assert sum(1 for r in ranges if r[2]) >= 5
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=7)
    try:
        e.set_sequences(seqs)
        e.coverage_begin("both")
        res, cigars = e.align_ranges(SCORES, ranges)
        assert (res["status"] == 0).all()
        spans = [V.span_of_range(r, lens)[3] for r in ranges]
        want, n = tracks_of(seqs, ranges, res, cigars, V.BOTH, spans=spans)
        assert n == len(ranges) and want.equals(*read(e))
        assert int(res["num_matches"].sum()) > int(res["cigar_len"].sum()) // 2  # the mirrored intervals are homologous
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


def equal_tracks(cov, want):
    return cov["offsets"].tolist() == want.offsets.tolist() and want.equals(cov["aligned"], cov["matched"])


@pytest.mark.parametrize("roles", V.ROLES)
def test_host_all_pairs_coverage(hip_lib, host_lib, small_set, roles):
    host = host_lib
    ids, seqs = small_set
    lens = [len(s) for s in seqs]
    name = V.ROLE_NAMES[roles]
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa")
    assert host.last_coverage()["offsets"] is None and len(plain) == 90 and any(ln.split("\t")[4] == "-" for ln in plain)
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", coverage=name)  # (WFA orientation's own alignments do not count)
    cov = host.last_coverage()
    assert got == plain
    want = V.coverage_from_paf(got, ids, lens, roles)
    assert equal_tracks(cov, want) and int(cov["aligned"].max()) >= 5
    assert (cov["items"], cov["failed"], cov["reads"]) == (90, 0, 1) and cov["boundaries"] > 0 and cov["kernel_ms"] > 0
    # two slots on one device: the slots' arrays add up to the one-slot result exactly
    two = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", coverage=name, devices=[0, 0], min_batch_pairs=16)
    cov2 = host.last_coverage()
    assert sorted(two) == sorted(plain) and equal_tracks(cov2, want) and (cov2["items"], cov2["reads"]) == (90, 2)
    # the clip's slices, and only those that reach the least score
    clipped = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left", coverage=name)
    covc = host.last_coverage()
    assert clipped == host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30, normalize="left")
    assert 5 <= len(clipped) < 90 and covc["items"] == len(clipped)
    assert equal_tracks(covc, V.coverage_from_paf(clipped, ids, lens, roles))
    if roles == V.BOTH:  # every other consumer accumulates too: the records' iterator since the list's start, the counting one, the text ones
        for kw in (dict(mode="for_each"), dict(mode="next", chunk=25), dict(mode="par_collect")):
            assert sorted(host.iterate(ids, seqs, SCORES_2P, orientation="wfa", coverage=name, **kw)) == sorted(plain)
            assert equal_tracks(host.last_coverage(), want), kw
        host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="wfa", coverage=name)
        assert equal_tracks(host.last_coverage(), want)
        assert host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", coverage=name, cs="short", device_cigar=True, verify=True)[0].startswith(plain[0])
        assert equal_tracks(host.last_coverage(), want)
        segs = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", split=2, split_min_score=60, coverage=name)
        assert len(segs) >= 5 and equal_tracks(host.last_coverage(), V.coverage_from_paf(segs, ids, lens, roles))


def test_host_align_ranges_coverage(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs = small_set
    lens = [len(s) for s in seqs]
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30)
    ranges = []
    for ln in plain:  # the clips of a first run, as interval pairs on both strands
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    assert sum(r[2] for r in ranges) >= 2
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, coverage="both")
    cov = host.last_coverage()
    assert len(got) == len(ranges) and equal_tracks(cov, V.coverage_from_paf(got, ids, lens, V.BOTH)) and cov["items"] == len(ranges)


def test_cli_coverage(hip_lib, host_lib, small_set, tmp_path):
    import re
    import subprocess
    from allwave_amd import build
    ids, seqs = small_set
    lens = [len(s) for s in seqs]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(out, *args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_bytes(), r.stderr.splitlines()[-1]

    plain, summary0 = run("plain.paf", "-p", "none")
    assert " coverage " not in summary0
    for roles in V.ROLES:
        cov = tmp_path / ("cov_%d.tsv" % roles)
        got, summary = run("cov_%d.paf" % roles, "-p", "none", "--coverage", str(cov), *(() if roles == V.BOTH else ("--coverage-of", V.ROLE_NAMES[roles])))
        assert got == plain  # byte for byte
        want = V.coverage_from_paf(got.decode().splitlines(), ids, lens, roles)
        lines = cov.read_text().splitlines()
        assert lines == V.format_tracks(ids, want) and len(lines) > 10 * len(ids)
        m = re.search(r"coverage (\d+) items, (\d+) boundaries, [0-9.]+ ms", summary)
        assert m and int(m.group(1)) == 90 and int(m.group(2)) > 0, summary
    # every sequence end to end, in input order, zeros included
    by_name = {}
    for ln in lines:
        f = ln.split("\t")
        by_name.setdefault(f[0], []).append((int(f[1]), int(f[2])))
    assert list(by_name) == ids
    for name, n in zip(ids, lens):
        iv = by_name[name]
        assert iv[0][0] == 0 and iv[-1][1] == n and all(a[1] == b[0] for a, b in zip(iv, iv[1:]))
    # with --align-paf, --clip and two slots
    paf_in = tmp_path / "map.paf"
    paf_in.write_bytes(b"\n".join(plain.splitlines()[:40]) + b"\n")
    cov = tmp_path / "cov_ranges.tsv"
    base, _ = run("ranges.paf", "--align-paf", str(paf_in), "--clip", "2")
    got, summary = run("ranges_cov.paf", "--align-paf", str(paf_in), "--clip", "2", "--coverage", str(cov), "--devices", "0,0")
    assert sorted(got.splitlines()) == sorted(base.splitlines())
    assert cov.read_text().splitlines() == V.format_tracks(ids, V.coverage_from_paf(got.decode().splitlines(), ids, lens, V.BOTH))
