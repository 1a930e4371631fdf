"""GPU tests of the target-anchored multiple alignments built on the device (csrc/msa.hip): items, targets and the arena of blocks
are compared, byte for byte, with the Python restatement (msa_cases.msa_of) of the same op bytes -- on the case list through
awv_msa_cigars / awv_msa_ranges, and on the engine's own alignments through the host calls and the command-line tool, where the
items are rebuilt from the run's own PAF lines.  All comparisons are exact equality."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import clip_cases as K
import msa_cases as M
import util
from verify_cases import revcomp

pytestmark = pytest.mark.gpu

SCORES = util.DEFAULT_2P


@pytest.fixture(scope="module")
def cases(hip_lib):
    """The case list packed into one arena at its residues, with what msa_of makes of it (computed once)."""
    cl = M.case_list()
    recs, arena = K.pack_arena([c[4] for c in cl], [c[7] for c in cl], [c[6] for c in cl])
    assert sorted(set(int(o) % 16 for o in recs["cigar_off"])) == [0, 1, 15]
    pairs = np.array([(c[1], c[2], c[3]) for c in cl], dtype=np.int32)
    slices = np.array([c[5] if c[5] is not None else (0, len(c[4]), 0, 0) for c in cl], dtype=np.int64)
    seqs = M.resident_set()
    return cl, seqs, pairs, recs, arena, slices, M.msa_of(seqs, list(M.TARGETS), M.case_items(cl))


def check(got, want, n_items):
    items, tgts, buf, size = got
    assert [M.fields(i, M.ITEM_FIELDS) for i in items] == want["items"]
    assert [M.fields(t, M.TARGET_FIELDS) for t in tgts] == want["targets"]
    assert size == want["bytes"]
    if buf is not None:
        assert buf.dtype == np.uint8 and np.array_equal(buf, M.arena_of(want["blocks"]))


def check_stats(st, want, n_items, emitted=True):
    assert (st.items, st.failed, st.columns, st.runs, st.bases, st.bytes) == (n_items, want["failed"], want["columns"], want["runs"], want["bases"], want["bytes"])
    assert st.width_ms > 0 and st.scan_ms > 0 and (st.emit_ms > 0) == emitted


@pytest.mark.parametrize("workgroups", [1, 2, 0])
def test_msa_cigars_on_the_case_list(hip_lib, cases, workgroups):
    """workgroups 1 and 2: one wave takes item after item, so what it carries from chunk to chunk must start afresh."""
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, want = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, workgroups=workgroups)
    try:
        e.set_sequences(seqs)
        assert e.msa_stats().items == 0
        got = e.msa_cigars(pairs, recs, arena, M.TARGETS, slices=slices)
        check(got, want, len(cl))
        check_stats(e.msa_stats(), want, len(cl))
        # the measuring call returns the sizes and writes nothing; too small a buffer stays as it was
        items, tgts, buf, size = e.msa_cigars(pairs, recs, arena, M.TARGETS, slices=slices, want_blocks=False)
        assert buf is None
        check((items, tgts, None, size), want, len(cl))
        check_stats(e.msa_stats(), want, len(cl), emitted=False)
        items, tgts, buf, size = e.msa_cigars(pairs, recs, arena, M.TARGETS, slices=slices, cap=want["bytes"] - 1)
        assert size == want["bytes"] and (buf == 0xff).all()
        check((items, tgts, None, size), want, len(cl))
        # another order of the targets moves the blocks and changes nothing in them
        order = list(reversed(M.TARGETS))
        got = e.msa_cigars(pairs, recs, arena, order, slices=slices)
        w2 = M.msa_of(seqs, order, M.case_items(cl))
        check(got, w2, len(cl))
        for j, s in enumerate(order):
            assert np.array_equal(w2["blocks"][j], want["blocks"][M.TARGETS.index(s)])
    finally:
        e.close()


def test_msa_cigars_in_pieces(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, want = cases
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_arena_bytes=4096)
    try:
        e.set_sequences(seqs)
        assert sum(len(c[4]) for c in cl if c[6] == 0) >= 3 * 4096  # three pieces or more, for the widths and again for the rows
        check(e.msa_cigars(pairs, recs, arena, M.TARGETS, slices=slices), want, len(cl))
        check_stats(e.msa_stats(), want, len(cl))
        # no targets, no items
        items, tgts, buf, size = e.msa_cigars(pairs, recs, arena, [], slices=slices)
        assert size == 0 and len(tgts) == 0 and all(int(i["code"]) == M.NOT_CHOSEN and int(i["target"]) == -1 for i in items)
        items, tgts, buf, size = e.msa_cigars(pairs[:0], recs[:0], arena, [12, 0])
        assert [M.fields(t, M.TARGET_FIELDS) for t in tgts] == [(12, 1, 33, 0), (0, 1, 10, 33)] and size == 43
        assert bytes(buf) == seqs[12].upper() + seqs[0].upper()
    finally:
        e.close()


def test_msa_ranges(hip_lib):
    """Rectangles inside longer sequences, forward and q_revcomp, with and without slices."""
    from allwave_amd import ffi
    rng = random.Random(731)
    seqs = [util.rand_seq(rng, n, b"ACGTacgtN") for n in (400, 350, 90, 1500)]
    ranges, strings, items, slices = [], [], [], []
    for k, (q, t, rev, qb, tb, spec) in enumerate(((1, 0, 0, 7, 11, "40M3D20M2I30M"), (2, 0, 1, 5, 30, "2D30M5D20M1D"), (3, 0, 0, 100, 0, "300M40D60M"),
                                                   (1, 3, 1, 0, 200, "100M1000I100M7D50M"), (2, 3, 0, 1, 1499, "1M80D"), (0, 1, 0, 0, 0, "10M"))):
        ops = M.expand(spec)
        nq, nt = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        ranges.append((q, t, rev, qb, qb + nq, tb, tb + nt))
        qlen = len(seqs[q])
        span = (qlen - qb - nq, qlen - qb, tb, tb + nt) if rev else (qb, qb + nq, tb, tb + nt)
        sl = None
        if k in (0, 3):
            b, e_ = 25, len(ops) - 30
            sl = (b, e_, b - ops[:b].count(b"I"), b - ops[:b].count(b"D"))
        strings.append(ops)
        slices.append(sl if sl is not None else (0, len(ops), 0, 0))
        items.append((q, t, rev, ops, span, sl, 0))
    recs, arena = K.pack_arena(strings)
    want = M.msa_of(seqs, [3, 0], items)
    assert want["items"][-1][0] == M.NOT_CHOSEN and all(i[0] == M.OK for i in want["items"][:-1])
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        check(e.msa_ranges(np.array(ranges, dtype=np.int32), recs, arena, [3, 0], slices=np.array(slices, dtype=np.int64)), want, len(items))
    finally:
        e.close()


def test_msa_refusals(hip_lib, cases):
    from allwave_amd import ffi
    cl, seqs, pairs, recs, arena, slices, want = cases

    def refused(code, fn, *args, **kw):
        with pytest.raises(ffi.EngineError) as err:
            fn(*args, **kw)
        assert err.value.code == code

    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        refused(ffi.AWV_ERR_STATE, e.msa_cigars, pairs, recs, arena, [0])  # no sequence set
        e.set_sequences(seqs)
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, recs, arena, [0, len(seqs)], slices=slices)  # a target outside the set
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, recs, arena, [0, -1], slices=slices)
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, recs, arena, [1, 0, 1], slices=slices)  # a repeated target
        bad = pairs.copy()
        bad[3][0] = len(seqs)
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, bad, recs, arena, [0], slices=slices)  # what awv_cs_cigars refuses
        out = recs.copy()
        out[2]["cigar_off"] = len(arena)
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, out, arena, [0], slices=slices)
        sl = slices.copy()
        sl[0][1] = len(cl[0][4]) + 1
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, recs, arena, [0], slices=sl)
        sl = slices.copy()
        sl[0][2] = -1
        refused(ffi.AWV_ERR_ARG, e.msa_cigars, pairs, recs, arena, [0], slices=sl)
        refused(ffi.AWV_ERR_ARG, e.msa_ranges, np.array([(0, 1, 0, 0, 11, 0, 5)], dtype=np.int32), recs[:1], arena, [1])
        check(e.msa_cigars(pairs, recs, arena, M.TARGETS, slices=slices), want, len(cl))  # and the engine goes on
    finally:
        e.close()


# ---- end to end: the host calls and the command-line tool --------------------------------------------------------------------

SCORES_2P = "0,5,8,2,24,1"
E2E_TARGETS = [0, 7, 4]


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


@pytest.fixture(scope="module")
def family():
    return M.diverged_family()


def same_blocks(got, want):
    assert sorted(got) == sorted(want)
    for t in want:
        assert got[t][0] == want[t][0], t
        assert got[t][1].dtype == np.uint8 and np.array_equal(got[t][1], want[t][1]), t
    return True


@pytest.mark.parametrize("variant", ["plain", "normalized", "clipped"])
def test_host_all_pairs_msa(hip_lib, host_lib, family, variant):
    host = host_lib
    ids, seqs = family
    kw = dict(plain={}, normalized=dict(normalize="left"), clipped=dict(clip=2, clip_min_score=30))[variant]
    plain = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", **kw)
    assert host.last_msa() == {} and len(plain) >= 20
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", msa_targets=[0, "s7", 4], **kw)
    assert got == plain  # byte for byte
    blocks = host.last_msa()
    want = M.blocks_from_paf(got, ids, seqs, E2E_TARGETS)
    assert same_blocks(blocks, want) and list(blocks) == E2E_TARGETS
    assert all(b.shape[1] >= len(seqs[t]) for t, (_, b) in blocks.items()) and any(b.shape[1] > len(seqs[t]) for t, (_, b) in blocks.items())
    # (a family has four members and s4 is reverse-complemented: forward clips keep 0's three relatives, 7's two others, none of 4's)
    assert sum(b.shape[0] for _, b in blocks.values()) >= 4 + 3 + 1
    st = host.last_msa_stats()
    assert st.items == sum(b.shape[0] - 1 for _, b in blocks.values()) and st.failed == 0 and st.bytes == sum(b.size for _, b in blocks.values())
    assert st.width_ms > 0 and st.scan_ms > 0 and st.emit_ms > 0
    if variant == "plain":
        # two slots on one device give the one-engine blocks exactly
        two = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", msa_targets=[0, "s7", 4], devices=[0, 0], min_batch_pairs=16)
        assert sorted(two) == sorted(plain) and same_blocks(host.last_msa(), want)
        # WFA orientation finds the reverse-complemented member
        wfa = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", msa_targets="all")
        all_blocks = host.last_msa()
        assert wfa == host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa") and any(ln.split("\t")[4] == "-" for ln in wfa)
        assert same_blocks(all_blocks, M.blocks_from_paf(wfa, ids, seqs, list(range(len(ids)))))
        assert any(nm.endswith("-") for nm in all_blocks[1][0][1:])
        # the other consumers keep the same items
        for kw2 in (dict(mode="for_each"), dict(mode="next", chunk=25), dict(mode="par_collect")):
            assert sorted(host.iterate(ids, seqs, SCORES_2P, orientation="forward", msa_targets=E2E_TARGETS, **kw2)) == sorted(plain)
            assert same_blocks(host.last_msa(), want), kw2
        host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation="forward", msa_targets=E2E_TARGETS)
        assert same_blocks(host.last_msa(), want)
        # beside the other passes: the check, the cs text, the depth, the allele table and a lifted region
        both = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", verify=True, cs="short", coverage="both", variants=True,
                                  liftover=[(0, 10, 60)], msa_targets=E2E_TARGETS)
        assert [ln.split("\tcs:Z:")[0] for ln in both] == plain and same_blocks(host.last_msa(), want)
        segs = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", split=2, split_min_score=60, msa_targets=E2E_TARGETS)
        assert len(segs) >= 40 and same_blocks(host.last_msa(), M.blocks_from_paf(segs, ids, seqs, E2E_TARGETS))
        # the bound: the alignments are delivered, then the call fails and names the bound and the size needed
        with pytest.raises(host.HostError) as err:
            host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", msa_targets=E2E_TARGETS, msa_max_bytes=1000)
        assert "msa_max_bytes = 1000" in str(err.value) and re.search(r"need \d+ bytes", str(err.value))
        for bad in (dict(msa_targets=[0, 0]), dict(msa_targets=[len(ids)]), dict(msa_targets=["nobody"]), dict(msa_targets=[0], device_cigar=True),
                    dict(msa_targets=[0], msa_max_bytes=0), dict(msa_max_bytes=5)):
            with pytest.raises(ValueError):
                host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward", **bad)
        assert host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="forward") == plain and host.last_msa() == {}


def test_host_align_ranges_msa(hip_lib, host_lib, family):
    host = host_lib
    ids, seqs = family
    first = host.all_pairs_paf(ids, seqs, SCORES_2P, orientation="wfa", clip=2, clip_min_score=30)
    ranges = []
    for ln in first:  # the clips of a first run, as interval pairs on both strands
        f = ln.split("\t")
        ranges.append((ids.index(f[0]), ids.index(f[5]), int(f[4] == "-"), int(f[2]), int(f[3]), int(f[7]), int(f[8])))
    assert sum(r[2] for r in ranges) >= 2
    plain = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    got = host.align_ranges(ids, seqs, ranges, SCORES_2P, msa_targets=[4, 1])
    assert got == plain and same_blocks(host.last_msa(), M.blocks_from_paf(got, ids, seqs, [4, 1]))


def parse_fasta(path):
    names, rows = [], []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            names.append(ln[1:].decode())
        elif ln:
            rows.append(np.frombuffer(ln, dtype=np.uint8))
    return names, np.stack(rows)


def test_cli_msa(hip_lib, host_lib, family, tmp_path):
    from allwave_amd import build
    ids, seqs = family
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(out, *args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P, "-o", str(tmp_path / out)] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return (tmp_path / out).read_bytes(), r.stderr.splitlines()[-1]

    plain, summary0 = run("plain.paf", "-p", "none")
    assert " msa " not in summary0
    got, summary = run("msa.paf", "-p", "none", "--msa", str(tmp_path / "aln_{}.fa"), "--msa-target", "s7", "--msa-target", "s2")
    assert got == plain  # byte for byte
    want = M.blocks_from_paf(got.decode().splitlines(), ids, seqs, [7, 2])
    rows = 0
    for t in (7, 2):
        names, block = parse_fasta(tmp_path / ("aln_%d.fa" % t))
        assert names == want[t][0] and np.array_equal(block, want[t][1]) and names[0] == ids[t] and re.fullmatch(r"s\d+/\d+-\d+[+-]", names[1])
        rows += len(names)
    assert not os.path.exists(tmp_path / "aln_0.fa")
    m = re.search(r"msa (\d+) targets, (\d+) rows, (\d+) bytes, [0-9.]+ ms", summary)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (2, rows, sum(want[t][1].size for t in want)), summary
    # one target needs no {}; with --align-paf, --clip and two slots
    paf_in = tmp_path / "map.paf"
    paf_in.write_bytes(b"\n".join(plain.splitlines()[:60]) + b"\n")
    base, _ = run("ranges.paf", "--align-paf", str(paf_in), "--clip", "2")
    got, summary = run("ranges_msa.paf", "--align-paf", str(paf_in), "--clip", "2", "--msa", str(tmp_path / "one.fa"), "--msa-target", "s1", "--devices", "0,0")
    assert sorted(got.splitlines()) == sorted(base.splitlines())
    names, block = parse_fasta(tmp_path / "one.fa")
    w1 = M.blocks_from_paf(got.decode().splitlines(), ids, seqs, [1])[1]
    assert names == w1[0] and np.array_equal(block, w1[1]) and len(names) >= 2
