"""GPU tests of the run-length CIGAR text made on the device (csrc/encode.hip): every text and every awv_cigar_text is compared,
byte for byte, with the host yardstick (awv_encode_one_host) or with the Python restatement (util.rle) of the same op bytes --
on the case list through awv_encode_cigars, on the engine's own alignments through the encoded align calls, and through the
host layer and the command-line tool.  All comparisons are exact."""
import random
import re
import subprocess

import numpy as np
import pytest

import clip_cases as K
import encode_cases as E
import normalize_cases as N
from util import DEFAULT_2P, EDIT, rle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list packed into one arena, with the yardstick's text and record for every case (computed once)."""
    from allwave_amd import ffi
    cl = E.case_list()
    recs, arena = E.pack(cl)
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == list(range(16))
    want = []
    for _, ops, status in cl:
        text, rec = ffi.encode_one_host(ops if status == 0 else b"")
        want.append((text, int(rec["len"]), int(rec["runs"])))
    return cl, recs, arena, want


def check_list(engine, cases):
    cl, recs, arena, want = cases
    text, tout, total = engine.encode_cigars(recs, arena)
    assert total == sum(w[1] for w in want) == len(text) and E.dense(tout)
    got = E.texts_of(text, tout)
    for k, (name, _, _) in enumerate(cl):
        assert (got[k], int(tout[k]["len"]), int(tout[k]["runs"])) == want[k], name
    st = engine.encode_stats()
    assert st.pairs == len(cl) and st.text_bytes == total and st.kernel_ms > 0
    assert st.runs == sum(w[2] for w in want) and st.columns == sum(len(c[1]) for c in cl if c[2] == 0)


@pytest.mark.parametrize("workgroups", [0, 1, 2])
def test_encode_cigars_on_the_case_list(hip_lib, cases, workgroups):
    """workgroups 1 and 2: one wave takes record after record, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)  # (never gets a sequence set: the text reads none)
    try:
        check_list(e, cases)
    finally:
        e.close()


def test_encode_cigars_in_several_pieces(hip_lib, cases):
    """A small max_arena_bytes cuts the list into pieces, one launch each: the offsets run on across them."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=200000)
    try:
        assert len(cases[2]) > 10 * 200000
        check_list(e, cases)
    finally:
        e.close()


def test_encode_cigars_all_of_the_text_or_none_across_pieces(hip_lib, cases):
    """More than ten pieces and a buffer that the text outgrows at the last piece, halfway or at the first: tout and text_bytes are
    the fitting call's, and not one byte of the buffer is written."""
    from allwave_amd import ffi
    _, recs, arena, _ = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=200000)
    try:
        assert len(arena) > 10 * 200000
        full, tout0, total0 = e.encode_cigars(recs, arena)
        assert len(full) == total0 > 2
        for cap in (total0 - 1, total0 // 2, 1):
            buf, tout, total = e.encode_cigars(recs, arena, text_cap=cap)
            assert len(buf) == cap and (buf == 0xff).all() and tout.tobytes() == tout0.tobytes() and total == total0, cap
        buf, tout, total = e.encode_cigars(recs, arena, text_cap=total0 + 9)
        assert bytes(buf[:total0]) == bytes(full) and (buf[total0:] == 0xff).all() and len(buf) == total0 + 9
        assert tout.tobytes() == tout0.tobytes() and total == total0
    finally:
        e.close()


@pytest.fixture(scope="module")
def bare_engine(hip_lib):
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    yield e
    e.close()


def test_encode_cigars_slices(hip_lib, bare_engine):
    from allwave_amd import ffi
    strings = [s for s in [c[1] for c in E.case_list()] + E.random_strings() if 0 < len(s) <= 5000]
    picks = E.random_slices(strings)
    recs, arena = K.pack_arena([strings[i] for i, _, _ in picks], [(3 * k + 1) % 16 for k in range(len(picks))])
    slices = np.array([(b, e) for _, b, e in picks], dtype=np.uint32)
    text, tout, total = bare_engine.encode_cigars(recs, arena, slices=slices)
    want = [rle(strings[i][b:e]).encode() for i, b, e in picks]
    assert E.texts_of(text, tout) == want and E.dense(tout) and total == sum(len(w) for w in want)
    assert [int(t["runs"]) for t in tout] == [sum(1 for c in w if not 48 <= c <= 57) for w in want]
    assert sum(1 for w in want if not w) >= 20  # empty slices
    n_cut = sum(1 for i, b, e in picks if 0 < b < e < len(strings[i]) and strings[i][b - 1] == strings[i][b] and strings[i][e - 1] == strings[i][e])
    assert n_cut >= 20  # slices cut inside a run at both ends
    for k, bad in ((0, (5, 4)), (1, (0, int(recs[1]["cigar_len"]) + 1))):  # col_beg > col_end; col_end > cigar_len
        sl = slices.copy()
        sl[k] = bad
        with pytest.raises(ffi.EngineError) as err:
            bare_engine.encode_cigars(recs, arena, slices=sl)
        assert err.value.code == ffi.AWV_ERR_ARG
    out = recs.copy()
    out[2]["cigar_off"] = len(arena)  # a completed record outside the arena
    out[2]["cigar_len"] = 1
    with pytest.raises(ffi.EngineError) as err:
        bare_engine.encode_cigars(out, arena)
    assert err.value.code == ffi.AWV_ERR_ARG
    text, tout, total = bare_engine.encode_cigars(recs[:0], b"")
    assert len(tout) == 0 and total == 0


def test_encode_cigars_measuring_call(hip_lib, bare_engine):
    """text_buf == NULL, and a text_cap that is too small: tout and text_bytes are filled, nothing is written."""
    strings = E.random_strings()[:60]
    recs, arena = K.pack_arena(strings)
    want = [rle(s).encode() for s in strings]
    full, tout0, total0 = bare_engine.encode_cigars(recs, arena)
    assert E.texts_of(full, tout0) == want
    none, tout, total = bare_engine.encode_cigars(recs, arena, want_text=False)
    assert none is None and total == total0 == sum(len(w) for w in want) and tout.tobytes() == tout0.tobytes()
    for cap in (total0 - 1, 1):
        buf, tout, total = bare_engine.encode_cigars(recs, arena, text_cap=cap)
        assert total == total0 and tout.tobytes() == tout0.tobytes() and (buf == 0xff).all() and len(buf) == cap
    buf, tout, total = bare_engine.encode_cigars(recs, arena, text_cap=total0 + 9)
    assert bytes(buf[:total0]) == bytes(full) and (buf[total0:] == 0xff).all()


# ---- the encoded align calls ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def repeat_set():
    return N.repeat_set()


def texts_want(res, cigars, clips=None):
    out = []
    for k, (r, ops) in enumerate(zip(res, cigars)):
        if r["status"] != 0:
            out.append(b"")
        elif clips is not None:
            out.append(rle(ops[int(clips[k]["col_beg"]):int(clips[k]["col_end"])]).encode() if clips[k]["code"] == K.OK else b"")
        else:
            out.append(rle(ops).encode())
    return out


@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT], ids=["2-piece", "edit"])
def test_align_pairs_encoded(hip_lib, engine, repeat_set, scores):
    from allwave_amd import ffi
    seqs, pairs, _ = repeat_set
    engine.set_sequences(seqs)
    res0, cig0 = engine.align_pairs(scores, pairs)
    assert (res0["status"] == 0).all()
    res, texts, tout = engine.align_pairs(scores, pairs, encode=True)
    assert res.tobytes() == res0.tobytes() and texts == texts_want(res0, cig0) and E.dense(tout)
    st = engine.encode_stats()
    assert st.pairs == len(pairs) and st.columns == int(res0["cigar_len"].sum()) and st.text_bytes == sum(len(t) for t in texts)
    assert st.runs == int(tout["runs"].sum()) and st.kernel_ms > 0
    # a bound that puts some pairs above it: no text for them
    bounds = np.where(np.arange(len(pairs)) % 3 == 0, res0["penalty"] // 2, -1).astype(np.int32)
    resb, cigb = engine.align_pairs(scores, pairs, max_penalty=bounds)
    res, texts, tout = engine.align_pairs(scores, pairs, max_penalty=bounds, encode=True)
    above = res["status"] == ffi.AWV_ST_ABOVE_BOUND
    assert res.tobytes() == resb.tobytes() and above.sum() >= 3 and texts == texts_want(resb, cigb) and E.dense(tout)
    assert all(texts[k] == b"" and tout[k]["runs"] == 0 for k in np.flatnonzero(above))
    # normalize, verify, clip
    resn, cign = engine.align_pairs(scores, pairs, normalize="left")
    res, texts, tout = engine.align_pairs(scores, pairs, normalize="left", encode=True)
    assert res.tobytes() == resn.tobytes() and texts == texts_want(resn, cign) and engine.normalize_stats().pairs == len(pairs)
    _, _, v0 = engine.align_pairs(scores, pairs, verify=True)
    res, texts, vres, tout = engine.align_pairs(scores, pairs, verify=True, encode=True)
    assert res.tobytes() == res0.tobytes() and vres.tobytes() == v0.tobytes() and (vres["code"] == 0).all() and texts == texts_want(res0, cig0)
    _, _, c0 = engine.align_pairs(scores, pairs, clip=1)
    res, texts, cres, tout = engine.align_pairs(scores, pairs, clip=1, encode=True)
    assert res.tobytes() == res0.tobytes() and cres.tobytes() == c0.tobytes() and texts == texts_want(res0, cig0, c0) and E.dense(tout)
    assert sum(1 for k in range(len(pairs)) if c0[k]["code"] == K.OK and c0[k]["col_end"] - c0[k]["col_beg"] < res0[k]["cigar_len"]) >= 3


def test_align_encoded_empty_clip_ranges_batches_and_keep_on_device(hip_lib):
    from allwave_amd import ffi
    seqs, pairs = K.flanked_set(n_pairs=14)
    rng = random.Random(81)
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=5)  # three batches: the first two go through the helper-thread sink
    try:
        e.set_sequences(seqs)
        res0, cig0, c0 = e.align_pairs(DEFAULT_2P, pairs, clip=1)
        res, texts, cres, tout = e.align_pairs(DEFAULT_2P, pairs, clip=1, encode=True)
        assert res.tobytes() == res0.tobytes() and cres.tobytes() == c0.tobytes() and texts == texts_want(res0, cig0, c0)
        for first in (0, 5, 10):  # every batch has a text arena of its own
            assert E.dense(tout[first:first + 5])
        res, texts, tout = e.align_pairs(DEFAULT_2P, pairs, encode=True)
        assert texts == texts_want(res0, cig0) and e.encode_stats().pairs == len(pairs)
        ranges = []
        for q, t, rev in pairs:
            ql, tl = len(seqs[q]), len(seqs[t])
            ranges.append((q, t, rev, rng.randint(0, ql // 4), rng.randint(3 * ql // 4, ql), rng.randint(0, tl // 4), rng.randint(3 * tl // 4, tl)))
        ranges.append((0, 1, 0, 5, 5, 7, 7))   # an empty CIGAR: empty text
        ranges.append((0, 1, 0, 5, 5, 7, 90))  # one run of 'I'
        resr, cigr = e.align_ranges(DEFAULT_2P, ranges)
        res, texts, tout = e.align_ranges(DEFAULT_2P, ranges, encode=True)
        assert res.tobytes() == resr.tobytes() and texts == texts_want(resr, cigr) and texts[-2:] == [b"", b"83D"]
        resr, cigr, cr = e.align_ranges(EDIT, ranges, clip=2)
        res, texts, cres, tout = e.align_ranges(EDIT, ranges, clip=2, encode=True)
        assert res.tobytes() == resr.tobytes() and cres.tobytes() == cr.tobytes() and texts == texts_want(resr, cigr, cr)
        assert [int(c) for c in cr["code"][-2:]] == [K.EMPTY, K.EMPTY] and texts[-2:] == [b"", b""]  # an empty clip: empty text
        with pytest.raises(ValueError):
            e.align_pairs(DEFAULT_2P, pairs, encode=True, split=(1, 10))
    finally:
        e.close()
    keep = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE | ffi.AWV_F_KEEP_ON_DEVICE)
    try:
        keep.set_sequences(seqs)
        plain, _ = keep.align_pairs(DEFAULT_2P, pairs)
        res, texts, tout = keep.align_pairs(DEFAULT_2P, pairs, encode=True)  # the step runs, tout is filled, no text is copied
        assert res.tobytes() == plain.tobytes() and all(t is None for t in texts) and E.dense(tout)
        assert [int(n) for n in tout["len"]] == [len(rle(c)) for c in cig0]
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


def sum_over_lines(lines):
    """(pairs, runs, text bytes, columns) of the cg:Z: strings of PAF lines."""
    cgs = [ln.split("\t")[-1][5:] for ln in lines]
    return (len(lines), sum(len(re.findall(r"[=XID]", cg)) for cg in cgs), sum(len(cg) for cg in cgs),
            sum(int(n) for cg in cgs for n in re.findall(r"\d+", cg)))


@pytest.mark.parametrize("orientation", ["forward", "mash", "wfa"])
def test_host_all_pairs_device_cigar(hip_lib, host_lib, small_set, orientation):
    host = host_lib
    ids, seqs = small_set
    want = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation)
    assert len(want) == 90 and host.last_encode() == dict(pairs=0, runs=0, text_bytes=0, columns=0, kernel_ms=0.0)
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, device_cigar=True)
    le = host.last_encode()
    assert got == want
    assert (le["pairs"], le["runs"], le["text_bytes"], le["columns"]) == sum_over_lines(want) and le["kernel_ms"] > 0
    assert sorted(host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, device_cigar=True, devices=[0, 0], min_batch_pairs=16)) == sorted(want)
    assert host.last_encode()["text_bytes"] == le["text_bytes"]
    wantc = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, clip=2, clip_min_score=30, normalize="left", verify=True)
    gotc = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation=orientation, clip=2, clip_min_score=30, normalize="left", verify=True, device_cigar=True)
    assert gotc == wantc and 5 <= len(wantc) < 90 and host.last_encode()["pairs"] == 90 and host.last_verify()["failures"] == []
    if orientation == "forward":  # the consumers that hand out op bytes ignore the setting; the counting consumer takes it
        assert sorted(host.iterate(ids, seqs, SCORES_2P, mode="par_collect", orientation="forward", device_cigar=True)) == sorted(want)
        assert host.last_encode()["pairs"] == 0
        nb, nl, _, _ = host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="forward", device_cigar=True)
        assert (nb, nl) == (sum(len(ln) + 1 for ln in want), 90) and host.last_encode()["text_bytes"] == le["text_bytes"]


def test_host_align_ranges_device_cigar(hip_lib, host_lib, small_set):
    host = host_lib
    ids, seqs = small_set
    rng = random.Random(82)
    ranges = []
    for k in range(5):
        for rev in (0, 1):
            q, t = 2 * k, 2 * k + 1
            ql, tl = len(seqs[q]), len(seqs[t])
            ranges.append((q, t, rev, 0, ql, 0, tl))
            ranges.append((q, t, rev, rng.randint(0, ql // 3), rng.randint(2 * ql // 3, ql), rng.randint(0, tl // 3), rng.randint(2 * tl // 3, tl)))
    want = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, device_cigar=True)
    assert got == want and len(want) == len(ranges)
    assert tuple(host.last_encode()[k] for k in ("pairs", "runs", "text_bytes", "columns")) == sum_over_lines(want)
    assert host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1, device_cigar=True) == host.align_ranges(ids, seqs, ranges, SCORES_2P, clip=1)


def test_cli_device_cigar(hip_lib, host_lib, small_set, tmp_path):
    from allwave_amd import build
    ids, seqs = small_set
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(out, *args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_bytes(), r.stderr.splitlines()[-1]

    plain, summary0 = run("plain.paf", "-p", "none")
    enc, summary = run("enc.paf", "-p", "none", "--device-cigar")
    assert enc == plain and len(plain.splitlines()) == 90 and "encoded" not in summary0
    m = re.search(r"encoded (\d+) pairs, (\d+) runs, (\d+) text bytes, [0-9.]+ ms", summary)
    assert m and tuple(int(v) for v in m.groups()) == sum_over_lines(plain.decode().splitlines())[:3], summary
    paf_in = tmp_path / "map.paf"
    paf_in.write_bytes(b"\n".join(plain.splitlines()[:40]) + b"\n")
    plain, _ = run("plain2.paf", "--align-paf", str(paf_in), "--normalize", "right")
    enc, summary = run("enc2.paf", "--align-paf", str(paf_in), "--normalize", "right", "--device-cigar")
    assert enc == plain and len(plain.splitlines()) == 40 and "encoded 40 pairs" in summary
