"""GPU tests of what a persistent wave carries from one record to the next in the ninth and tenth record passes,
lift.hip and msa.hip, and of the launch-grid loops of msa.hip's scan and target kernels.  Every list of tests/reuse_cases.py --
record k + 1 a trap for the state record k leaves; tests/test_reuse_lift_msa_cpu.py shows that a leaked carry changes the
answer -- goes through awv_lift_cigars (reuse_cases.lift_queries: every third record without a query, two records with 200)
and through awv_msa_cigars in two layouts (every record its own target; all records on three shared targets) with workgroups =
1, 2 and 0 and with one wave over several pieces of the arena: every field of every lift result against lift_one_host, items,
targets, size and the arena of blocks byte for byte against msa_cases.msa_of, and each pass's stats.  Then range records that
alternate with whole forward ones, 12,288 short records through the default grid (more targets than the scan and target
kernels have workgroups), an engine that lifts its own alignments at two workgroups, and a small set whose targets put 'D'
runs on the tile edges of the scan and behind the first trip of the target kernel.  All comparisons are exact equality.

What each list traps here: main-D / pass-D, gap_tail -> gap_head: msa's run0 and, from the query side, lift's last_a; main-I /
pass-I, the same pair: last_a from the target side; all_gaps -> plain on a 16-byte boundary: msa's prev_d (stats.runs); any
two records: cq / ct and the four op counts; the records with 200 queries: the probe cursors and the step of 64; zero: SKIPPED
and column-free records behind walked ones."""
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import reuse_cases as RC
import split_cases as S
from test_gpu_reuse import engines, same_bytes, scan_engines  # noqa: F401  (engines: the module's fixture)
from test_gpu_reuse_passes import want
from util import DEFAULT_2P

pytestmark = pytest.mark.gpu

MSA_STATS = ("items", "failed", "columns", "runs", "bases", "bytes")
LAYOUTS = {"own-targets": False, "shared-targets": True}


@pytest.fixture(autouse=True)
def wall_time(request):
    """Each test's wall time, printed behind it (run with -s or -rA to see it)."""
    t0 = time.time()
    yield
    print("%s: %.1f s" % (request.node.name, time.time() - t0))


def inputs(name):
    return want(("lift-msa inputs", name), lambda: RC.lift_msa_inputs(RC.all_lists()[name]))


def lift_stats_tuple(st):
    return (st.records, st.columns, st.queries, st.ok, st.skipped, st.bad_op, st.lengths, st.unaligned, st.outside)


def same_lifts(got, wanted, queries, recs, where):
    """Two LIFT_DTYPE arrays byte for byte; a difference is reported with the query, its record and the record walked before it."""
    if got.tobytes() == wanted.tobytes():
        return
    assert len(got) == len(wanted), (where, len(got), len(wanted))
    ks = sorted({q[0] for q in queries})
    bad = [j for j in range(len(wanted)) if got[j].tobytes() != wanted[j].tobytes()]
    j = bad[0]
    k = queries[j][0]
    before = ks[ks.index(k) - 1] if ks.index(k) else None
    assert False, (where, "query %d %r differs (%d in all): record %d of %d" % (j, queries[j], len(bad), k, len(recs)), recs[k].kind, len(recs[k].ops),
                   "behind record %r" % before, None if before is None else recs[before].kind, got[j], wanted[j])


def check_lift(ffi, e, call, recs, queries, ref, where):
    before = lift_stats_tuple(e.lift_stats())
    got = call(queries)
    same_lifts(got, ref, queries, recs, where)
    delta = tuple(x - y for x, y in zip(lift_stats_tuple(e.lift_stats()), before))
    codes = tuple(int((ref["code"] == c).sum()) for c in range(6))
    assert delta == RC.lift_walked(recs, queries) + (len(queries),) + codes, (where, delta)


def same_blocks(got, ref, recs, where):
    """The arena of blocks byte for byte; a difference is reported with the record whose row it falls in and the one before it."""
    wanted = ref["arena"]
    assert got.dtype == np.uint8 and len(got) == len(wanted), (where, "the arena has %d bytes, not %d" % (len(got), len(wanted)))
    if np.array_equal(got, wanted):
        return
    at = int(np.flatnonzero(got != wanted)[0])
    j = max(j for j, t in enumerate(ref["targets"]) if t[3] <= at)
    row = (at - ref["targets"][j][3]) // ref["targets"][j][2]
    if row == 0:
        assert False, (where, "row 0 of target %d differs at byte %d" % (j, at), int(got[at]), int(wanted[at]))
    i = next(i for i, it in enumerate(ref["items"]) if it[0] == 0 and it[1] == j and it[2] == row)
    assert False, (where, "the row of record %d of %d differs at byte %d (%d bytes in all)" % (i, len(recs), at, int((got != wanted).sum())), recs[i].kind,
                   len(recs[i].ops), "behind", recs[i - 1].kind if i else None, bytes(got[at:at + 24]), bytes(wanted[at:at + 24]))


def check_msa(ffi, e, call, recs, ref, where):
    items, tgts, buf, size = call(True)
    same_bytes(items, ref["item_array"], recs, where)
    assert tgts.tobytes() == ref["target_array"].tobytes(), (where, "the targets differ", [j for j in range(len(tgts)) if tgts[j].tobytes() != ref["target_array"][j].tobytes()][:4])
    assert size == ref["bytes"], (where, size, ref["bytes"])
    same_blocks(buf, ref, recs, where)
    st = e.msa_stats()
    wanted = (len(recs), ref["failed"], ref["columns"], ref["runs"], ref["bases"], ref["bytes"])
    assert tuple(getattr(st, f) for f in MSA_STATS) == wanted, (where, [(f, getattr(st, f), w) for f, w in zip(MSA_STATS, wanted) if getattr(st, f) != w])
    # the measuring call: the same items and sizes, and no buffer to write to
    items, tgts, buf, size = call(False)
    assert buf is None and size == ref["bytes"] and tgts.tobytes() == ref["target_array"].tobytes(), where
    same_bytes(items, ref["item_array"], recs, (where, "measuring"))
    assert tuple(getattr(e.msa_stats(), f) for f in MSA_STATS) == wanted and e.msa_stats().emit_ms == 0, where


# ---- the trap lists ---------------------------------------------------------------------------------------------------------------

def test_lift_waves_take_record_after_record(engines):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, results, arena = inputs(name)
        queries = want(("lift queries", name), lambda: RC.lift_queries(recs, seqs, name))
        ref = want(("lift", name), lambda: RC.lift_want(ffi, recs, queries, seqs))
        if name != "zero":
            assert 2 * int((ref["code"] == ffi.AWV_LF_OK).sum()) > len(queries) and int((ref["code"] == ffi.AWV_LF_UNALIGNED).sum()) >= 100, name
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            check_lift(ffi, e, lambda q: e.lift_cigars(pairs, results, arena, q), recs, queries, ref, (name, ename))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_msa_waves_take_record_after_record(engines, layout):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, _, results, arena = inputs(name)
        set_, pairs, targets = want(("msa layout", name, layout), lambda: RC.msa_layout(recs, seqs, LAYOUTS[layout], name))
        ref = want(("msa", name, layout), lambda: RC.msa_want(set_, targets, RC.msa_items(recs, pairs)))
        if name != "zero":
            assert 2 * int((ref["item_array"]["code"] == ffi.AWV_MS_OK).sum()) > len(recs) and ref["runs"] >= 500, name
        for ename, e in scan_engines(engines):
            e.set_sequences(set_)
            check_msa(ffi, e, lambda blocks: e.msa_cigars(pairs, results, arena, targets, want_blocks=blocks), recs, ref, (name, layout, ename))


def test_lift_and_msa_range_records_then_whole_forward_sequences(engines):
    """lift and msa on intervals that begin off the dword grid, on both strands, alternating with forward records on whole sequences
    (reuse_cases.verify_ranges_list), every odd sequence a target."""
    from allwave_amd import ffi
    recs, begs = RC.verify_ranges_list()
    seqs, ranges, claimed, arena = RC.verify_range_inputs(recs, begs, DEFAULT_2P, random.Random("reuse/ranges"))
    geometry = RC.range_geometry(seqs, ranges)
    queries = RC.lift_queries(recs, seqs, "ranges", geometry)
    lifted = RC.lift_want(ffi, recs, queries, seqs, geometry)
    targets = list(range(1, len(seqs), 2))
    msa = RC.msa_want(seqs, targets, RC.msa_items(recs, ranges, geometry))
    assert set(int(c) for c in lifted["code"]) <= {ffi.AWV_LF_OK, ffi.AWV_LF_UNALIGNED, ffi.AWV_LF_OUTSIDE} and int((lifted["code"] == ffi.AWV_LF_OK).sum()) > len(queries) // 2
    assert (msa["item_array"]["code"] == ffi.AWV_MS_OK).all() and msa["runs"] > 20
    for ename, e in scan_engines(engines):
        e.set_sequences(seqs)
        check_lift(ffi, e, lambda q: e.lift_ranges(ranges, claimed, arena, q), recs, queries, lifted, ("ranges", ename))
        check_msa(ffi, e, lambda blocks: e.msa_ranges(ranges, claimed, arena, targets, want_blocks=blocks), recs, msa, ("ranges", ename))


def test_default_grid_takes_several_lift_and_msa_records_per_wave(hip_lib):
    """Nothing set: what production runs.  The 12,288 short records of reuse_cases.default_path_records -- at 16 waves per CU every
    wave takes more than one -- with two queries a record, and with all 12,288 odd sequences as targets: more targets than the
    scan kernel has workgroups (2 per CU) and than the target kernel has rows of workgroups (1,024), so both walk on by their
    grid's size."""
    from allwave_amd import ffi
    n = 12288
    child = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)  # (as tests/test_gpu_reuse.py: torch in a process of its own)
    assert child.returncode == 0, child.stderr.decode(errors="replace")[-2000:]
    cus = int(child.stdout.split()[-1])
    assert 2 * 16 * cus <= n  # a device with more CUs would turn this into a run without reuse
    recs = RC.default_path_records(n)
    seqs, pairs, results, arena = RC.lift_msa_inputs(recs)
    rng = random.Random("reuse/lift/default")
    queries = []
    for k, r in enumerate(recs):  # the whole target, and a random interval of the query (a sequence without a base: none)
        if seqs[2 * k + 1]:
            queries.append((k, RC.FROM_TARGET, 0, len(seqs[2 * k + 1])))
        if seqs[2 * k]:
            b = rng.randrange(len(seqs[2 * k]))
            queries.append((k, RC.FROM_QUERY, b, rng.randint(b + 1, len(seqs[2 * k]))))
    assert len({q[0] for q in queries}) >= 2 * 16 * cus
    lifted = RC.lift_want(ffi, recs, queries, seqs)
    targets = list(range(1, 2 * n, 2))
    nt = len(targets)
    assert nt > 1024 and nt > 2 * cus  # awv_msa_target_kernel's j += gridDim.y and awv_msa_scan_kernel's j += gridDim.x are entered
    msa = RC.msa_want(seqs, targets, RC.msa_items(recs, pairs))
    e = ffi.Engine()
    try:
        e.set_sequences(seqs)
        check_lift(ffi, e, lambda q: e.lift_cigars(pairs, results, arena, q), recs, queries, lifted, "lift")
        check_msa(ffi, e, lambda blocks: e.msa_cigars(pairs, results, arena, targets, want_blocks=blocks), recs, msa, "msa")
    finally:
        e.close()


def test_lifting_engine_with_two_workgroups(engines):
    """The island set, aligned by an engine that lifts regions through its own alignments at workgroups = 2: the table is the
    default engine's, byte for byte."""
    seqs, pairs = S.island_set()
    regions = [(s, b, b + 150) for s in range(len(seqs)) for b in (50, 400, 900, 1500) if b + 150 <= len(seqs[s])]
    out = []
    for e in (engines("NO_ARENA_PROBE"), engines("NO_ARENA_PROBE", workgroups=2)):
        e.set_sequences(seqs)
        e.lift_begin(regions, "both")
        res, cigs = e.align_pairs(DEFAULT_2P, pairs)
        table = e.lift_read()
        st = e.lift_stats()
        assert (res["status"] == 0).all() and len(table) > 20 and st.ok == len(table) and st.records >= len(pairs)
        out.append((res.tobytes(), cigs, table.tobytes()))
        e.lift_begin(None, None)
    assert out[0] == out[1]


# ---- msa.hip's launch geometry -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("workgroups", [1, 0])
def test_msa_runs_on_tile_edges_and_behind_the_first_trip(engines, workgroups):
    """reuse_cases.geometry_set through awv_msa_ranges: targets of 1,023, 1,024, 2,047, 2,048 and 16,500 bases with 'D' runs of two
    or three widths at slots 0, 1,023, 1,024, 2,047, 2,048, 16,383, 16,384, len - 1 and len -- on both sides of every tile edge
    of awv_msa_scan_kernel, and in the part of the long target that awv_msa_target_kernel reaches in its second trip."""
    from allwave_amd import ffi
    import clip_cases as K
    import msa_cases as M
    seqs, ranges, strings, items, targets = RC.geometry_set()
    results, arena = K.pack_arena(strings)
    ref = want("msa geometry", lambda: RC.msa_want(seqs, targets, items))
    e = engines("NO_ARENA_PROBE", workgroups=workgroups) if workgroups else engines("NO_ARENA_PROBE")
    e.set_sequences(seqs)
    got_items, tgts, buf, size = e.msa_ranges(ranges, results, arena, targets)
    for j, t in enumerate(targets):
        assert int(tgts[j]["width"]) == len(seqs[t]) + sum(ref["ins"][j]), (workgroups, t)
        off, rows, width = int(tgts[j]["off"]), int(tgts[j]["rows"]), int(tgts[j]["width"])
        assert (rows, width, off) == ref["targets"][j][1:] and size == ref["bytes"]
        block = buf[off:off + rows * width].reshape(rows, width)
        row0 = ref["blocks"][j][0]
        if not np.array_equal(block[0], row0):
            at = int(np.flatnonzero(block[0] != row0)[0])
            assert False, (workgroups, "row 0 of the target of %d bases differs at column %d of %d" % (len(seqs[t]), at, width), bytes(block[0][at:at + 16]), bytes(row0[at:at + 16]))
    for i, it in enumerate(ref["items"]):
        assert M.fields(got_items[i], M.ITEM_FIELDS) == it, (workgroups, i, "the run of %d at slot %d of target %d" % (items[i][3].count(b"D"), items[i][4][2] + items[i][3].index(b"D"), items[i][1]))
        j, row = it[1], it[2]
        off, width = ref["targets"][j][3], ref["targets"][j][2]
        assert np.array_equal(buf[off + row * width:off + (row + 1) * width], ref["blocks"][j][row]), (workgroups, i)
    assert tgts.tobytes() == ref["target_array"].tobytes() and np.array_equal(buf, ref["arena"])
    st = e.msa_stats()
    assert tuple(getattr(st, f) for f in MSA_STATS) == (len(items), 0, ref["columns"], ref["runs"], ref["bases"], ref["bytes"])
