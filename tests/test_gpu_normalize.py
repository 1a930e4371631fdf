"""GPU tests of gap-run normalization (csrc/normalize.hip): the device's op bytes and awv_norm_result records are compared,
byte for byte, with the host yardstick (awv_normalize_one_host) -- on caller-supplied strings through awv_normalize_cigars /
awv_normalize_ranges, on the engine's own alignments of repeat-rich pairs under awv_engine_set_normalize, composed with the
check, the clip, the split and the bounds, and through the host layer and the command-line tool."""
import random
import re
import subprocess

import numpy as np
import pytest

import clip_cases as K
import normalize_cases as N
import verify_cases as V
from util import DEFAULT_2P, rle

pytestmark = pytest.mark.gpu

SKIPPED_REC = (N.SKIPPED, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def cases():
    return N.device_cases()


def pack(strings, seed):
    """clip_cases.pack_arena with residues modulo 16 that cover all sixteen."""
    rng = random.Random(seed)
    residues = [(k if k < 32 else rng.randrange(16)) % 16 for k in range(len(strings))]
    return K.pack_arena(strings, residues)


def want_for(ffi, direction, seen):
    out = []
    for p, t, ops in seen:
        got, rec = ffi.normalize_one_host(direction, p, t, ops)
        out.append((got, N.as_tuple(rec)))
    return out


def check_supplied(ffi, e, direction, call, first, seen, seed):
    recs, arena = pack([s[2] for s in seen], seed)
    out, nres = call(direction, first, recs, arena)
    want = want_for(ffi, direction, seen)
    for k, r in enumerate(recs):
        off, n = int(r["cigar_off"]), int(r["cigar_len"])
        assert out[off:off + n].tobytes() == want[k][0], (direction, k, n, off % 16)
        assert N.as_tuple(nres[k]) == want[k][1], (direction, k)
    # nothing outside the strings is touched
    mask = np.ones(len(arena), dtype=bool)
    for r in recs:
        mask[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])] = False
    assert (out[mask] == np.frombuffer(arena, dtype=np.uint8)[mask]).all()
    st = e.normalize_stats()
    assert st.pairs == len(seen) and st.columns == sum(len(s[2]) for s in seen) and st.kernel_ms > 0
    assert st.runs == sum(len(N.gap_runs(s[2])) for s in seen)
    assert st.runs_moved == sum(w[1][1] for w in want) and st.columns_moved == sum(w[1][2] for w in want)
    assert st.records_moved == sum(1 for w in want if w[1][1] > 0) > 0
    return want


@pytest.mark.parametrize("direction", ["left", "right"])
@pytest.mark.parametrize("workgroups,max_arena", [(0, 0), (1, 0), (2, 4096)], ids=["default", "one-workgroup", "two-workgroups-pieces"])
def test_normalize_cigars_and_ranges(hip_lib, cases, direction, workgroups, max_arena):
    """The traps, random scripts (N, lower case), long scripts and q_revcomp pairs, as pairs and as ranges: one and two
    workgroups take record after record, and a small max_arena_bytes sends the arena up and back in several pieces."""
    from allwave_amd import ffi
    seqs, pairs, ranges, seen_p, seen_r = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups, max_arena_bytes=max_arena)
    try:
        e.set_sequences(seqs)
        check_supplied(ffi, e, direction, e.normalize_cigars, pairs, seen_p, 5)
        check_supplied(ffi, e, direction, e.normalize_ranges, ranges, seen_r, 6)
    finally:
        e.close()


def test_refusals_skips_and_argument_errors(hip_lib):
    from allwave_amd import ffi
    ref = N.refusals()
    good = [c for c in N.traps() if c[1] == "left"][:6]
    seqs, pairs, strings, status = [], [], [], []
    for k, (p, t, ops) in enumerate([(r[1], r[2], r[3]) for r in ref] + [(g[2], g[3], g[4]) for g in good] * 2):
        seqs += [p if p else b"", t if t else b""]
        pairs.append((2 * k, 2 * k + 1, 0))
        strings.append(ops)
        status.append(0 if k < len(ref) + len(good) else (1, 2, 3, 4, 1, 2)[k - len(ref) - len(good)])
    recs, arena = K.pack_arena(strings, None, status)
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=2)
    try:
        with pytest.raises(ffi.EngineError) as err:  # no sequence set yet
            e.normalize_cigars("left", pairs, recs, arena)
        assert err.value.code == ffi.AWV_ERR_STATE
        e.set_sequences(seqs)
        out, nres = e.normalize_cigars("left", pairs, recs, arena)
        for k, r in enumerate(recs):
            ops = strings[k]
            got = out[int(r["cigar_off"]):int(r["cigar_off"]) + len(ops)].tobytes()
            if k < len(ref):
                assert got == ops and N.as_tuple(nres[k]) == (ref[k][4], 0, ref[k][5], 0, 0), ref[k][0]
            elif status[k] == 0:
                assert got == good[k - len(ref)][5] and int(nres[k]["code"]) == N.OK
            else:
                assert got == ops and N.as_tuple(nres[k]) == SKIPPED_REC
        assert e.normalize_stats().pairs == len(strings)
        # a completed record whose op bytes lie outside the arena, a bad index, a bad direction: refused before any launch
        bad = recs.copy()
        bad[1]["cigar_len"] = len(arena)
        for args in (("left", pairs, bad, arena), ("left", [(0, len(seqs), 0)] + pairs[1:], recs, arena)):
            with pytest.raises(ffi.EngineError) as err:
                e.normalize_cigars(*args)
            assert err.value.code == ffi.AWV_ERR_ARG
        assert hip_lib.awv_normalize_cigars(e._h, 0, np.zeros(1, dtype=ffi.PAIR_DTYPE).ctypes.data, 0, None, None, 0, None) == ffi.AWV_ERR_ARG
        assert hip_lib.awv_engine_set_normalize(e._h, 3) == ffi.AWV_ERR_ARG
        out, nres = e.normalize_cigars("right", pairs[:0], recs[:0], b"")
        assert len(nres) == 0 and e.normalize_stats().pairs == 0
    finally:
        e.close()


def test_linear_work_on_a_homopolymer(hip_lib):
    """30 kbp of one base with more than 300 gap runs, each free to move thousands of columns: the device's bytes are the
    yardstick's, in both directions, and the kernel's time stays far from what quadratic work would take."""
    from allwave_amd import ffi
    p, t, ops = N.homopolymer_case()
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences([p, t])
        recs, arena = K.pack_arena([ops], [3])
        for direction in ("left", "right"):
            out, nres = e.normalize_cigars(direction, [(0, 1, 0)], recs, arena)
            want, rec = ffi.normalize_one_host(direction, p, t, ops)
            assert out[int(recs[0]["cigar_off"]):][:len(ops)].tobytes() == want
            assert N.as_tuple(nres[0]) == N.as_tuple(rec) and int(rec["runs_moved"]) >= 300
            st = e.normalize_stats()
            print("homopolymer %s: %d runs moved, %d columns moved, %.3f ms" % (direction, st.runs_moved, st.columns_moved, st.kernel_ms))
            assert st.kernel_ms < 1000.0
    finally:
        e.close()


# ---- the aligning calls -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def repeat_set():
    return N.repeat_set()


_PLAIN = {}


def plain_run(engine, repeat_set, scores):
    """The unnormalized call's records and op strings, once per engine flavour and penalty set."""
    key = (id(engine), scores)
    if key not in _PLAIN:
        seqs, pairs, _ = repeat_set
        engine.set_sequences(seqs)
        _PLAIN[key] = engine.align_pairs(scores, pairs)
    return _PLAIN[key]


def normalized(ffi, direction, seqs, pairs, res, cigs):
    out = []
    for (q, t, rev), r, ops in zip(pairs, res, cigs):
        if r["status"] != 0:
            out.append((None, SKIPPED_REC))
            continue
        p = V.revcomp(seqs[q]) if rev else seqs[q]
        got, rec = ffi.normalize_one_host(direction, p, seqs[t], ops)
        out.append((got, N.as_tuple(rec)))
    return out


@pytest.mark.parametrize("scores", N.ALIGN_SCORES, ids=["2-piece", "1-piece"])
def test_align_pairs_normalized(hip_lib, engine, repeat_set, scores):
    from allwave_amd import ffi
    seqs, pairs, names = repeat_set
    res0, cig0 = plain_run(engine, repeat_set, scores)
    assert (res0["status"] == 0).all()
    want = normalized(ffi, "left", seqs, pairs, res0, cig0)
    engine.set_sequences(seqs)
    res, cigs, vres = engine.align_pairs(scores, pairs, verify=True, normalize="left")
    assert res.tobytes() == res0.tobytes()
    assert cigs == [w[0] for w in want]
    assert (vres["code"] == ffi.AWV_VF_OK).all()
    st = engine.normalize_stats()
    assert st.pairs == len(pairs) and st.runs_moved == sum(w[1][1] for w in want) > 0 and st.columns == int(res0["cigar_len"].sum())
    assert st.columns_moved == sum(w[1][2] for w in want) and st.kernel_ms > 0
    for name in N.GENERATORS:  # every class has a pair whose bytes moved
        assert any(w[0] != c for w, c, nm in zip(want, cig0, names) if nm == name), name
    # right, without the check
    res_r, cigs_r = engine.align_pairs(scores, pairs, normalize="right")
    assert res_r.tobytes() == res0.tobytes() and cigs_r == [w[0] for w in normalized(ffi, "right", seqs, pairs, res0, cig0)]
    # the mode does not outlive the call: off again, byte-identical to the first unnormalized call
    res2, cigs2 = engine.align_pairs(scores, pairs)
    assert res2.tobytes() == res0.tobytes() and cigs2 == cig0
    # score-only and orientation calls ignore a mode that is set
    engine.set_normalize("left")
    try:
        sc = engine.score_pairs(scores, pairs)
        assert (sc["penalty"] == res0["penalty"]).all()
        res3, cigs3 = engine.align_pairs(scores, pairs)  # (the engine's own mode is read by a plain call)
        assert cigs3 == [w[0] for w in want] and res3.tobytes() == res0.tobytes()
    finally:
        engine.set_normalize(None)


def test_align_ranges_and_align_one_normalized(hip_lib, engine, repeat_set):
    from allwave_amd import ffi
    seqs, pairs, _ = repeat_set
    rng = random.Random(94)
    ranges, subs = [], []
    for q, t, _ in pairs:
        ql, tl = len(seqs[q]), len(seqs[t])
        qb, tb = rng.randint(0, ql // 5), rng.randint(0, tl // 5)
        qe, te = rng.randint(4 * ql // 5, ql), rng.randint(4 * tl // 5, tl)
        ranges.append((q, t, 0, qb, qe, tb, te))
        subs.append((seqs[q][qb:qe], seqs[t][tb:te]))
    engine.set_sequences(seqs)
    res0, cig0 = engine.align_ranges(DEFAULT_2P, ranges)
    res, cigs, vres = engine.align_ranges(DEFAULT_2P, ranges, verify=True, normalize="left")
    assert res.tobytes() == res0.tobytes() and (vres["code"] == ffi.AWV_VF_OK).all()
    want = [ffi.normalize_one_host("left", p, t, ops)[0] for (p, t), ops in zip(subs, cig0)]
    assert cigs == want and sum(1 for w, c in zip(want, cig0) if w != c) >= 5
    # awv_align_one reads the mode too, over its own temporary sequences
    p, t = subs[next(k for k, (w, c) in enumerate(zip(want, cig0)) if w != c)]
    r0, ops0 = engine.align_one(DEFAULT_2P, p, t)
    engine.set_normalize("left")
    try:
        r1, ops1 = engine.align_one(DEFAULT_2P, p, t)
    finally:
        engine.set_normalize(None)
    assert r1.tobytes() == r0.tobytes() and ops1 == ffi.normalize_one_host("left", p, t, ops0)[0] and ops1 != ops0


def test_composition_with_clip_split_and_bounds(hip_lib, repeat_set):
    """The clip and the split describe the normalized string; a pair above its bound is skipped and untouched; several
    batches and AWV_F_KEEP_ON_DEVICE normalize too."""
    from allwave_amd import ffi
    seqs, pairs, _ = repeat_set
    scores = DEFAULT_2P
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=4)
    try:
        e.set_sequences(seqs)
        res0, cig0 = e.align_pairs(scores, pairs)
        want = normalized(ffi, "left", seqs, pairs, res0, cig0)
        a = 2
        res, cigs, cres = e.align_pairs(scores, pairs, clip=a, normalize="left")
        assert res.tobytes() == res0.tobytes() and cigs == [w[0] for w in want]
        assert [K.as_tuple(c) for c in cres] == [K.as_tuple(ffi.clip_one_host(scores, a, w[0])) for w in want]
        assert e.normalize_stats().pairs == len(pairs)
        res, cigs, (index, segs) = e.align_pairs(scores, pairs, split=(a, 40), normalize="left")
        assert cigs == [w[0] for w in want]
        for k, w in enumerate(want):
            idx, sg = ffi.split_one_host(scores, a, 40, w[0])
            assert int(index[k]["code"]) == int(idx["code"]) and [K.as_tuple(s) for s in segs[k]] == [K.as_tuple(s) for s in sg], k
        bounds = np.where(np.arange(len(pairs)) % 3 == 0, res0["penalty"] // 2, -1).astype(np.int32)
        resb, cigb = e.align_pairs(scores, pairs, max_penalty=bounds)
        res, cigs, vres = e.align_pairs(scores, pairs, max_penalty=bounds, verify=True, normalize="left")
        above = res["status"] == ffi.AWV_ST_ABOVE_BOUND
        assert res.tobytes() == resb.tobytes() and above.sum() >= 3
        for k in range(len(pairs)):
            assert cigs[k] == (None if above[k] else want[k][0]), k
        assert (vres["code"][above] == ffi.AWV_VF_SKIPPED).all() and (vres["code"][~above] == ffi.AWV_VF_OK).all()
        st = e.normalize_stats()
        assert st.pairs == len(pairs) and st.runs_moved == sum(w[1][1] for k, w in enumerate(want) if not above[k])
    finally:
        e.close()
    keep = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_KEEP_ON_DEVICE)
    try:
        keep.set_sequences(seqs)
        res, cigs, cres = keep.align_pairs(scores, pairs, clip=a, normalize="left")
        assert all(c is None for c in cigs) and [K.as_tuple(c) for c in cres] == [K.as_tuple(ffi.clip_one_host(scores, a, w[0])) for w in want]
        assert keep.normalize_stats().runs_moved == sum(w[1][1] for w in want)
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
def small_set(hip_lib, repeat_set):
    """Three pairs of the repeat set, all against all: of the tandem, copy-number and microsatellite classes the first pair
    whose alignment left-normalization changes (short sequences never leave the base case, whose backtrace already places
    gaps leftmost: it is the breakpoints of longer ones that strand a gap mid-repeat).  The first pair's text is stored
    reverse-complemented, so both strands are among the lines."""
    from allwave_amd import ffi
    seqs, pairs, names = repeat_set
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        res, cigs = e.align_pairs(DEFAULT_2P, pairs)
    finally:
        e.close()
    out = []
    for name in ("tandem", "cnv", "microsatellite"):
        k = next(k for k in range(len(pairs)) if names[k] == name and
                 ffi.normalize_one_host("left", seqs[2 * k], seqs[2 * k + 1], cigs[k])[0] != cigs[k])
        out += [seqs[2 * k], seqs[2 * k + 1]]
    out[1] = V.revcomp(out[1])
    return ["s%d" % i for i in range(len(out))], out


def normalized_line(ffi, ids, seqs, direction, line):
    """The PAF line `line` of an unnormalized run as normalization leaves it: cg:Z: replaced by the run-length form of the
    yardstick's bytes over the line's own intervals."""
    f = line.split("\t")
    q, t = seqs[ids.index(f[0])], seqs[ids.index(f[5])]
    p = q[int(f[2]):int(f[3])]
    if f[4] == "-":
        p = V.revcomp(p)
    ops = V.expand_cg(f[-1][5:])
    got, rec = ffi.normalize_one_host(direction, p, t[int(f[7]):int(f[8])], ops)
    assert int(rec["code"]) == N.OK, line[:80]
    return "\t".join(f[:-1] + ["cg:Z:" + rle(got)]), int(rec["runs_moved"])


def solo_ranges(seqs):
    """The set's second and third pair as whole-sequence ranges, one direction each: aligned on their own (no swapped twin
    in the list to share breakpoints with), these are the alignments the fixture chose for moving under "left"."""
    return [(2, 3, 0, 0, len(seqs[2]), 0, len(seqs[3])), (4, 5, 0, 0, len(seqs[4]), 0, len(seqs[5]))]


@pytest.mark.parametrize("orientation", ["wfa", "mash"])
def test_host_all_pairs_normalized(hip_lib, host_lib, small_set, orientation):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    full = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation)
    assert host.last_normalize()["pairs"] == 0 and {ln.split("\t")[4] for ln in full} == {"+", "-"}
    wants, total = {}, {}
    for direction in ("left", "right"):
        want, moved = zip(*(normalized_line(ffi, ids, seqs, direction, ln) for ln in full))
        got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, normalize=direction, verify=True)
        assert got == list(want)
        ln_ = host.last_normalize()
        print("host all-pairs, %s, normalize %s: %d of %d lines change, %d runs moved" %
              (orientation, direction, sum(1 for g, f in zip(got, full) if g != f), len(full), sum(moved)))
        assert ln_["pairs"] == len(full) and ln_["runs_moved"] == sum(moved) and ln_["kernel_ms"] > 0
        assert host.last_verify()["pairs"] == len(full) and host.last_verify()["failures"] == []
        rep = host.check_paf(ids, seqs, "\n".join(got) + "\n", SCORES_2P)
        assert rep["failures"] == [] and rep["checked"] == len(got)
        wants[direction], total[direction] = list(want), sum(moved)
    # (an entry and its swapped twin share their breakpoints, and a base case's backtrace leaves gaps leftmost: which
    # direction moves more is the data's; that something moves is required)
    best = max(total, key=total.get)
    assert total[best] > 0 and sum(1 for w, f in zip(wants[best], full) if w != f) >= 2
    want = wants[best]
    assert sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, normalize=best, devices=[0, 0], min_batch_pairs=8)) == sorted(want)
    assert host.last_normalize()["pairs"] == len(full) and host.last_normalize()["runs_moved"] == total[best]
    for mode in ("for_each", "next", "par_for_each", "par_collect"):
        lines = host.iterate(ids, seqs, SCORES_2P, mode=mode, orientation=orientation, normalize=best, chunk=8)
        assert sorted(lines) == sorted(want), mode
    # the mode does not outlive its call: the engines the host layer keeps are off again
    assert host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation) == full


def test_host_align_ranges_normalized(hip_lib, host_lib, small_set):
    from allwave_amd import ffi
    host = host_lib
    ids, seqs = small_set
    ranges = solo_ranges(seqs) + [(0, 1, 1, 10, len(seqs[0]) - 7, 5, len(seqs[1]) - 12), (3, 2, 0, 20, len(seqs[3]), 0, len(seqs[2]) - 20)]
    full = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    assert host.last_normalize()["pairs"] == 0
    changed = [False] * len(ranges)
    for direction in ("left", "right"):
        want, moved = zip(*(normalized_line(ffi, ids, seqs, direction, ln) for ln in full))
        got = host.align_ranges(ids, seqs, ranges, SCORES_2P, normalize=direction, verify=True)
        assert got == list(want)
        assert host.last_normalize()["pairs"] == len(ranges) and host.last_normalize()["runs_moved"] == sum(moved)
        assert host.last_verify()["failures"] == []
        assert host.align_ranges(ids, seqs, ranges, SCORES_2P, normalize=direction, devices=[0, 0]) == list(want)
        changed = [c or g != f for c, g, f in zip(changed, got, full)]
    assert changed[0] and changed[1]  # (a copy-number gap and a microsatellite gap lie in repeats: one of the two directions moves them)
    # composed with the clip: the clip of the normalized string
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, normalize="left", clip=2)
    norm = host.align_ranges(ids, seqs, ranges, SCORES_2P, normalize="left")
    for g, n_line in zip(got, norm):  # (every range here keeps a clip: line for line)
        fg, fn = g.split("\t"), n_line.split("\t")
        ops = V.expand_cg(fn[-1][5:])
        cl = ffi.clip_one_host(DEFAULT_2P, 2, ops)
        assert int(cl["code"]) == K.OK and fg[-1] == "cg:Z:" + rle(ops[int(cl["col_beg"]):int(cl["col_end"])])
    assert len(got) == len(norm) == len(ranges)


def test_cli_normalize(hip_lib, host_lib, small_set, tmp_path):
    from allwave_amd import build, ffi
    host = host_lib
    ids, seqs = small_set
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(*args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines(), r.stderr.splitlines()[-1]

    for direction in ("left", "right"):
        want = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="mash", normalize=direction)
        ln_ = host.last_normalize()
        got, summary = run("-p", "none", "--normalize", direction, "--verify")
        assert got == want
        m = re.search(r"normalized (\d+) pairs, (\d+) runs moved, [0-9.]+ ms", summary)
        assert m and tuple(int(v) for v in m.groups()) == (len(want), ln_["runs_moved"]), summary
        assert "verified %d pairs, 0 failed" % len(want) in summary
    # composed with --clip and --devices: the clip of the normalized string
    got_c, summary = run("-p", "none", "--normalize", "right", "--clip", "2", "--devices", "0,0")
    assert sorted(got_c) == sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="mash", normalize="right", clip=2))
    assert "normalized %d pairs" % len(want) in summary and "clipped %d pairs" % len(want) in summary
    # --align-paf: mapping lines that name the solo ranges and some of the unnormalized run's lines
    full, _ = run("-p", "none")
    ranges = solo_ranges(seqs)
    lines = ["\t".join(str(v) for v in (ids[q], len(seqs[q]), qb, qe, "-" if rev else "+", ids[t], len(seqs[t]), tb, te, 0, 0, 255))
             for q, t, rev, qb, qe, tb, te in ranges] + full[:10]
    for ln in full[:10]:
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(lines) + "\n")
    plain = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    total = 0
    for direction in ("left", "right"):
        got, summary = run("--align-paf", str(paf_in), "--normalize", direction)
        assert got == host.align_ranges(ids, seqs, ranges, SCORES_2P, normalize=direction)
        moved = host.last_normalize()["runs_moved"]
        assert got == [normalized_line(ffi, ids, seqs, direction, ln)[0] for ln in plain]
        assert "normalized 12 pairs, %d runs moved" % moved in summary
        total += moved
    assert total >= 2
