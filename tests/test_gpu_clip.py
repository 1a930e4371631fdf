"""GPU tests of clipping to the best-scoring segment (csrc/clip.hip): every device record is compared, field for field, with
the host yardstick (awv_clip_one_host) on the same op bytes -- on synthetic op strings through awv_clip_cigars, on the
engine's own alignments through the clipped align calls, and through the host layer and the command-line tool."""
import random

import numpy as np
import pytest

import clip_cases as K
from util import DEFAULT_2P, mutate, rand_seq

pytestmark = pytest.mark.gpu

P1 = (0, 4, 6, 2)
UNIT = (0, 1, 1, 1)


def yardstick(ffi, scores, a, recs, cigars):
    """[record tuple] of the host yardstick for an engine call's records and op strings."""
    out = []
    for r, ops in zip(recs, cigars):
        out.append(K.as_tuple(ffi.clip_one_host(scores, a, ops)) if r["status"] == 0 else (K.SKIPPED,) + (0,) * 12)
    return out


def tuples(cres):
    return [K.as_tuple(c) for c in cres]


@pytest.fixture(scope="module")
def bare_engine(hip_lib):
    """An engine that never gets a sequence set: clipping reads none."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def synthetic():
    """[(name, ops, residue of cigar_off modulo 16)]: the boundary strings for every residue, and the lengths at residues of
    their own."""
    rng = random.Random(77)
    out = []
    for sh in range(16):
        out += [(name, ops, sh) for name, ops in K.boundary_strings(sh)]
    out += [(name, ops, (5 * k + 3) % 16) for k, (name, ops) in enumerate(K.length_strings(rng))]
    return out


def check_cigars(ffi, engine, scores, a, strings, residues, status=None):
    recs, arena = K.pack_arena(strings, residues, status)
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == sorted(set(r % 16 for r in residues))
    got = tuples(engine.clip_cigars(scores, a, recs, arena))
    for k, ops in enumerate(strings):
        want = K.as_tuple(ffi.clip_one_host(scores, a, ops)) if recs[k]["status"] == 0 else (K.SKIPPED,) + (0,) * 12
        assert got[k] == want, (k, len(ops), residues[k], scores, a)
    return got


@pytest.mark.parametrize("scores,a", [(DEFAULT_2P, 1), (UNIT, 1), (P1, 2)], ids=["2-piece", "unit", "1-piece"])
def test_clip_cigars_on_synthetic_strings(hip_lib, bare_engine, synthetic, scores, a):
    from allwave_amd import ffi
    names = [s[0] for s in synthetic]
    got = check_cigars(ffi, bare_engine, scores, a, [s[1] for s in synthetic], [s[2] for s in synthetic])
    st = bare_engine.clip_stats()
    assert st.pairs == len(synthetic) and st.columns == sum(len(s[1]) for s in synthetic) and st.kernel_ms > 0
    assert st.empty == sum(1 for g in got if g[0] == K.EMPTY)
    if scores == UNIT:  # the cases are what their names say (a = x = 1), for every residue
        for sh in range(16):
            k = next(i for i, s in enumerate(synthetic) if s[0] == "minimum tied between two chunks" and s[2] == sh)
            first_min = 1024 - 40 - sh  # the columns before the first M
            assert got[k][2:5] == (200, first_min + 100, first_min + 300), sh
            k = next(i for i, s in enumerate(synthetic) if s[0] == "best tied between two chunks" and s[2] == sh)
            assert got[k][3:5] == (0, 1024 - 30 - sh) and got[k][2] == 1024 - 30 - sh, sh
            k = next(i for i, s in enumerate(synthetic) if s[0] == "segment over three chunks" and s[2] == sh)
            assert got[k][3] < 1024 - sh and got[k][4] > 2 * 1024 - sh, sh
    assert names.count("all-gap chunk") == 16


def test_clip_cigars_bad_bytes_and_mixed_batch(hip_lib, bare_engine):
    from allwave_amd import ffi
    rng = random.Random(78)
    strings, residues, status = [], [], []
    for sh in (0, 1, 7, 15):
        for byte in (1023, 1008, 2047, 16, 0):  # the last lane of a chunk (its last and its first byte), of the second chunk; early
            ops = bytearray(K.random_ops(rng, 2500, alphabet=b"MMMMXID"))
            col = byte - sh
            if col < 0:
                continue
            ops[col] = ord("N")
            ops[col + 300] = ord("=")  # (a later bad byte does not matter)
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
    got = check_cigars(ffi, bare_engine, DEFAULT_2P, 2, strings, residues, status)
    assert all(g[0] == K.BAD_OP for g in got[:n_bad])
    codes = [g[0] for g in got[n_bad:]]
    assert codes.count(K.SKIPPED) == 10 and codes.count(K.EMPTY) >= 20 and codes.count(K.OK) >= 5
    st = bare_engine.clip_stats()
    assert st.pairs == len(strings) and st.empty == codes.count(K.EMPTY)
    # a completed record whose op bytes lie outside the arena is refused before anything is read
    recs, arena = K.pack_arena(strings[:3], residues[:3])
    recs[1]["cigar_len"] = len(arena)
    with pytest.raises(ffi.EngineError) as err:
        bare_engine.clip_cigars(DEFAULT_2P, 1, recs, arena)
    assert err.value.code == ffi.AWV_ERR_ARG
    for a in (0, 32768):
        with pytest.raises(ffi.EngineError) as err:
            bare_engine.clip_cigars(DEFAULT_2P, a, recs[:1], arena)
        assert err.value.code == ffi.AWV_ERR_ARG
    assert len(bare_engine.clip_cigars(DEFAULT_2P, 1, recs[:0], b"")) == 0
    # a call that succeeds on an engine without a sequence set leaves the thread's last error alone
    assert b"match_bonus" in hip_lib.awv_last_error()
    recs, arena = K.pack_arena(strings[n_bad:n_bad + 3], residues[n_bad:n_bad + 3])
    bare_engine.clip_cigars(DEFAULT_2P, 1, recs, arena)
    assert b"match_bonus" in hip_lib.awv_last_error() and b"sequence set" not in hip_lib.awv_last_error()


def test_clip_cigars_in_several_pieces(hip_lib, synthetic):
    """A small max_arena_bytes: the arena goes up in several pieces, one launch each."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=8192)
    try:
        part = synthetic[::7]
        check_cigars(ffi, e, DEFAULT_2P, 1, [s[1] for s in part], [s[2] for s in part])
        st = e.clip_stats()
        assert st.pairs == len(part) and st.columns == sum(len(s[1]) for s in part)
    finally:
        e.close()


# ---- the clipped align calls ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def flanked():
    return K.flanked_set()


_PLAIN = {}


def plain_run(engine, flanked, scores):
    """The unclipped call's records, op strings and verify results, once per engine flavour and penalty set."""
    key = (id(engine), scores)
    if key not in _PLAIN:
        seqs, pairs = flanked
        engine.set_sequences(seqs)
        _PLAIN[key] = engine.align_pairs(scores, pairs, verify=True)
    return _PLAIN[key]


@pytest.mark.parametrize("scores,a", [(DEFAULT_2P, 2), (P1, 1)], ids=["2-piece", "1-piece"])
def test_align_pairs_clipped(hip_lib, engine, flanked, scores, a):
    from allwave_amd import ffi
    seqs, pairs = flanked
    res0, cig0, v0 = plain_run(engine, flanked, scores)
    assert (res0["status"] == 0).all() and (v0["code"] == 0).all() and set(pairs[:, 2]) == {0, 1}
    engine.set_sequences(seqs)
    seen = []
    res, cigs, vres, cres = engine.align_pairs(scores, pairs, verify=True, clip=a,
                                               _sink_hook=lambda first, n, c: seen.append((first, n, c[first:first + n].copy())))
    assert res.tobytes() == res0.tobytes() and cigs == cig0 and vres.tobytes() == v0.tobytes()
    want = yardstick(ffi, scores, a, res0, cig0)
    assert tuples(cres) == want
    assert sum(n for _, n, _ in seen) == len(pairs)
    for first, n, c in seen:  # cout is filled before the batch's sink call
        assert tuples(c) == want[first:first + n]
    st = engine.clip_stats()
    assert st.pairs == len(pairs) and st.columns == int(res0["cigar_len"].sum()) and st.empty == sum(1 for w in want if w[0] == K.EMPTY)
    # the set is what the issue asks for: clips that drop flanks, and pairs without a shared core
    n_trimmed = sum(1 for w, r in zip(want, res0) if w[0] == K.OK and (w[3] > 0 or w[4] < r["cigar_len"]))
    assert n_trimmed >= 12
    # without verify the clip array comes third
    res2, cigs2, cres2 = engine.align_pairs(scores, pairs, clip=a)
    assert res2.tobytes() == res0.tobytes() and cigs2 == cig0 and tuples(cres2) == want


def test_align_ranges_clipped(hip_lib, engine, flanked):
    from allwave_amd import ffi
    seqs, pairs = flanked
    rng = random.Random(79)
    ranges = []
    for q, t, rev in pairs[:24]:
        ql, tl = len(seqs[q]), len(seqs[t])
        qb, tb = rng.randint(0, ql // 4), rng.randint(0, tl // 4)
        ranges.append((q, t, rev, qb, rng.randint(3 * ql // 4, ql), tb, rng.randint(3 * tl // 4, tl)))
    ranges.append((0, 1, 0, 5, 5, 7, 7))  # two empty intervals: an empty CIGAR, an empty clip
    ranges.append((0, 1, 0, 5, 5, 7, 90))  # one run of 'I'
    engine.set_sequences(seqs)
    res0, cig0 = engine.align_ranges(DEFAULT_2P, ranges)
    res, cigs, cres = engine.align_ranges(DEFAULT_2P, ranges, clip=3)
    assert res.tobytes() == res0.tobytes() and cigs == cig0
    want = yardstick(ffi, DEFAULT_2P, 3, res0, cig0)
    assert tuples(cres) == want and want[-1][0] == K.EMPTY and want[-2][0] == K.EMPTY
    assert sum(1 for w in want if w[0] == K.OK) >= 15


def test_clipped_under_bounds_batches_and_keep_on_device(hip_lib, flanked):
    """Bounds: an abandoned pair clips as SKIPPED.  Several batches: every batch's clips are there at its sink call.
    AWV_F_KEEP_ON_DEVICE: the clip runs though no CIGAR comes back."""
    from allwave_amd import ffi
    seqs, pairs = flanked
    base = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=16)
    try:
        base.set_sequences(seqs)
        res0, cig0 = base.align_pairs(DEFAULT_2P, pairs)
        want = yardstick(ffi, DEFAULT_2P, 1, res0, cig0)
        bounds = np.where(np.arange(len(pairs)) % 3 == 0, res0["penalty"] // 2, -1).astype(np.int32)
        resb, cigb = base.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds)
        seen = []
        res, cigs, cres = base.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds, clip=1,
                                           _sink_hook=lambda first, n, c: seen.append((first, n, c[first:first + n].copy())))
        assert res.tobytes() == resb.tobytes() and cigs == cigb
        above = res["status"] == ffi.AWV_ST_ABOVE_BOUND
        assert above.sum() >= 10 and (res["status"][~above] == 0).all()
        got = tuples(cres)
        for k in range(len(pairs)):
            assert got[k] == ((K.SKIPPED,) + (0,) * 12 if above[k] else want[k]), k
        assert len(seen) == 3 and [s[:2] for s in seen] == [(0, 16), (16, 16), (32, 8)]
        for first, n, c in seen:
            assert tuples(c) == got[first:first + n]
        assert base.clip_stats().pairs == len(pairs)
    finally:
        base.close()
    keep = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_KEEP_ON_DEVICE)
    try:
        keep.set_sequences(seqs)
        plain, _ = keep.align_pairs(DEFAULT_2P, pairs)  # (one batch here: the arena offsets are not the three batches')
        res, cigs, cres = keep.align_pairs(DEFAULT_2P, pairs, clip=1)
        assert res.tobytes() == plain.tobytes() and all(c is None for c in cigs) and tuples(cres) == want
        assert (res["cigar_len"] == res0["cigar_len"]).all() and (res["penalty"] == res0["penalty"]).all()
    finally:
        keep.close()


def test_rerun_pairs_are_clipped(hip_lib):
    """first_row_cols small enough that pairs come back AWV_ST_CAPACITY from the first attempt and are re-run wider: their
    op strings are clipped like the others'."""
    from allwave_amd import ffi
    rng = random.Random(4242)
    a = rand_seq(rng, 6000)
    seqs = [a, rand_seq(rng, 400) + mutate(a, 0.08, rng) + rand_seq(rng, 300), mutate(a, 0.01, rng), rand_seq(rng, 1500)]
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, first_row_cols=2048)
    try:
        e.set_sequences(seqs)
        res0, cig0 = e.align_pairs(DEFAULT_2P, pairs)
        assert e.stats().launches >= 2 and (res0["status"] == 0).all()
        res, cigs, vres, cres = e.align_pairs(DEFAULT_2P, pairs, verify=True, clip=2)
        assert e.stats().launches >= 2
        assert res.tobytes() == res0.tobytes() and cigs == cig0 and (vres["code"] == 0).all()
        assert tuples(cres) == yardstick(ffi, DEFAULT_2P, 2, res0, cig0)
    finally:
        e.close()


# ---- the host layer and the command-line tool ----------------------------------------------------------------------------------

SCORES_2P = "0,5,8,2,24,1"


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


@pytest.fixture(scope="module")
def small_set(flanked):
    """The first five pairs of the flanked set (two of them with a reverse-complemented query), all against all."""
    seqs, _ = flanked
    return ["s%d" % i for i in range(10)], seqs[:10]


def clipped_line(ffi, scores, a, line, min_score=1):
    """The line `line` of an unclipped run becomes under --clip a: (line or None, clip record).  From the yardstick clip of
    the line's own op string and the coordinate rule; columns 3-4 and 8-9 of `line` are the range that was aligned."""
    f = line.split("\t")
    ops = K.V.expand_cg(f[-1][5:])
    cl = ffi.clip_one_host(scores, a, ops)
    if cl["code"] != K.OK or cl["score"] < min_score:
        return None, cl
    qs, qe, ts, te = K.clipped_paf_fields(cl, int(f[1]), int(f[6]), int(f[2]), int(f[3]), int(f[7]), f[4] == "-")
    nm, nx = int(cl["num_matches"]), int(cl["num_mismatches"])
    seg = ops[int(cl["col_beg"]):int(cl["col_end"])]
    from util import rle
    out = f[:2] + [str(qs), str(qe), f[4]] + f[5:7] + [str(ts), str(te), str(nm), str(max(qe - qs, te - ts)), "60", "gi:f:%.6f" % (nm / (nm + nx)),
                                                        "cg:Z:" + rle(seg)]
    return "\t".join(out), cl


@pytest.mark.parametrize("orientation", ["wfa", "mash"])
def test_host_all_pairs_clipped(hip_lib, host_lib, small_set, orientation):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    a = 2
    full = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation)
    assert len(full) == 90 and host.last_clip() == dict(pairs=0, empty=0, below_min_score=0, kernel_ms=0.0)
    assert {ln.split("\t")[4] for ln in full} == {"+", "-"}
    for min_score in (None, 150):
        got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, clip=a, clip_min_score=min_score, verify=True)
        lc, want, n_empty, n_below = host.last_clip(), [], 0, 0
        for ln in full:
            w, cl = clipped_line(ffi, DEFAULT_2P, a, ln, min_score or 1)
            if w is None:
                n_empty += cl["code"] != K.OK
                n_below += cl["code"] == K.OK
            else:
                want.append(w)
        assert got == want  # (the dropped pairs are exactly the empty and the below-min-score ones)
        assert (lc["pairs"], lc["empty"], lc["below_min_score"]) == (90, n_empty, n_below) and lc["kernel_ms"] > 0
        assert host.last_verify()["pairs"] == 90 and host.last_verify()["failures"] == []  # (the full alignments are what is verified)
        if min_score:
            assert 5 <= len(want) < 90 and n_below > 0
        else:
            assert sum(1 for g, f in zip(got, full) if g != f) >= 30 and {ln.split("\t")[4] for ln in got} == {"+", "-"}
            # the coordinate convention is the one the checker reads: every clipped line is the global alignment of its interval pair
            rep = host.check_paf(ids, seqs, "\n".join(got) + "\n", SCORES_2P, partial=True)
            assert rep["failures"] == [] and rep["checked"] == len(got)
            assert sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, clip=a, devices=[0, 0], min_batch_pairs=16)) == sorted(want)
    # every consumer of the pair list hands out the clipped alignments
    for mode in ("for_each", "next", "par_for_each", "par_collect"):
        lines = host.iterate(ids, seqs, SCORES_2P, mode=mode, orientation=orientation, clip=a, chunk=32)
        assert sorted(lines) == sorted(want0 for want0 in (clipped_line(ffi, DEFAULT_2P, a, ln)[0] for ln in full) if want0), mode


def test_host_align_ranges_clipped(hip_lib, host_lib, small_set):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    rng = random.Random(80)
    ranges = []
    for k in range(5):
        for rev in (0, 1):  # both strands of every related pair (one of them the wrong one), and sub-intervals
            q, t = 2 * k, 2 * k + 1
            ql, tl = len(seqs[q]), len(seqs[t])
            ranges.append((q, t, rev, 0, ql, 0, tl))
            ranges.append((q, t, rev, rng.randint(0, ql // 3), rng.randint(2 * ql // 3, ql), rng.randint(0, tl // 3), rng.randint(2 * tl // 3, tl)))
    # a refused clip argument leaves no bound behind for the thread's next call: every argument is checked before any is set
    with pytest.raises(ValueError):
        host.align_ranges(ids, seqs, ranges, SCORES_2P, max_penalty=0, clip=0)
    full = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    assert len(full) == len(ranges) and host.last_bounds()["pairs"] == 0
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1, verify=True)
    want = [w for w in (clipped_line(ffi, DEFAULT_2P, 1, ln)[0] for ln in full) if w]
    assert got == want and len(want) >= 10 and host.last_clip()["pairs"] == len(ranges)
    assert any(ln.split("\t")[4] == "-" and ln.split("\t")[2] != "0" for ln in got)
    rep = host.check_paf(ids, seqs, "\n".join(got) + "\n", SCORES_2P, partial=True)
    assert rep["failures"] == [] and rep["checked"] == len(got)
    assert host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1, devices=[0, 0]) == want


def test_cli_clip(hip_lib, host_lib, small_set, tmp_path):
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

    want = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="mash", clip=1, clip_min_score=40)
    lc = host.last_clip()
    got, summary = run("-p", "none", "--clip", "1", "--clip-min-score", "40")
    assert got == want
    m = re.search(r"clipped (\d+) pairs, (\d+) empty, (\d+) below min score, [0-9.]+ ms", summary)
    assert m and tuple(int(v) for v in m.groups()) == (90, lc["empty"], lc["below_min_score"]) and lc["below_min_score"] > 0, summary
    assert len(got) == 90 - lc["empty"] - lc["below_min_score"]
    # --align-paf: the unclipped run's lines as the mapping
    full, _ = run("-p", "none")
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(full[:40]) + "\n")
    ranges = []
    for ln in full[:40]:
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    got, summary = run("--align-paf", str(paf_in), "--clip", "1")
    assert got == host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1)
    assert "clipped 40 pairs, %d empty, 0 below min score" % host.last_clip()["empty"] in summary
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--clip", "1", "--score-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "--score-only" in r.stderr
