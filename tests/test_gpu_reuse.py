"""GPU tests of what a persistent workgroup carries from one item to the next.  Every kernel here that does
per-record or per-pair work takes its items from a cursor, one after the other in the same registers, LDS region, DFS stack,
event arena and history slot.  The lists of tests/reuse_cases.py are processed in list order at one workgroup, and item
k + 1 is a trap for the state item k leaves (tests/test_reuse_cpu.py shows, from the references alone, that a leaked carry
changes the answer).  The scan kernels (verify.hip, clip.hip, split.hip) run with workgroups = 1, 2 and 0 against the host
yardsticks, every field of every result, and their output arrays must be byte-identical; the align kernels run in four
pinned flavours with one slot, two slots and the default, against the CPU oracle, every record field and every op byte."""
import random
import subprocess
import sys

import numpy as np
import pytest

import bounded_cases as BC
import clip_cases as K
import penalty_space as PS
import reuse_cases as RC
import split_cases as S
import twin_cases as TC
from util import DEFAULT_2P, EDIT

pytestmark = pytest.mark.gpu

P1 = (0, 4, 6, 2)
UNIT = (0, 1, 1, 1)
SCAN_SETS = {"2-piece": DEFAULT_2P, "1-piece": P1, "unit": UNIT}
SENTINEL = 0x5A
SCRATCH_CAP = 6 << 30       # as tests/test_gpu_penalties.py
RING256 = PS.BY_NAME["ring256_2p_chain3"]


@pytest.fixture(scope="module")
def engines(hip_lib):
    """Engines by (flag names, other awv_engine_config fields), made on first use and closed with the module."""
    from allwave_amd import ffi
    made = {}

    def get(*names, **cfg):
        key = (names, tuple(sorted(cfg.items())))
        if key not in made:
            flags = 0
            for n in names:
                flags |= getattr(ffi, "AWV_F_" + n)
            made[key] = ffi.Engine(flags=flags, **cfg)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def scan_engines(engines):
    """[(name, engine)]: one wave, two waves, the default grid, and one wave through several pieces of the arena."""
    return [("workgroups=1", engines("NO_ARENA_PROBE", workgroups=1)), ("workgroups=2", engines("NO_ARENA_PROBE", workgroups=2)),
            ("workgroups=0", engines("NO_ARENA_PROBE")), ("workgroups=1, pieces", engines("NO_ARENA_PROBE", workgroups=1, max_arena_bytes=8192))]


def same_bytes(got, want, recs, where):
    """Two result arrays byte for byte; a difference is reported with the record it falls on and the one before it."""
    if got.tobytes() == want.tobytes():
        return
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    i = bad[0]
    assert False, (where, "record %d of %d differs (%d in all)" % (i, len(want), len(bad)), recs[i].kind, len(recs[i].ops),
                   "behind", recs[i - 1].kind if i else None, got[i], want[i])


# ---- the scan kernels ---------------------------------------------------------------------------------------------------------

def _verify_want(ffi, scores, recs, seqs, pairs, claimed, arena):
    want = np.zeros(len(recs), dtype=ffi.VERIFY_DTYPE)
    for k, r in enumerate(recs):
        want[k] = ffi.verify_one_host(scores, r.pattern, r.text, r.ops, claimed[k])
    return want


@pytest.mark.parametrize("scores", list(SCAN_SETS.values()), ids=list(SCAN_SETS))
def test_verify_waves_take_record_after_record(engines, scores):
    from allwave_amd import ffi
    lists = dict(RC.scan_lists())
    for name, recs in lists.items():
        seqs, pairs, claimed, arena = RC.verify_inputs(recs, scores)
        want = _verify_want(ffi, scores, recs, seqs, pairs, claimed, arena)
        if name != "zero":
            assert sum(1 for c in want["code"] if c == ffi.AWV_VF_OK) > len(recs) // 2 and len(set(want["code"])) >= 6, name
        columns = sum(min(len(r.ops), len(r.pattern) + len(r.text) + 1) for r in recs if r.status == 0)
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            got = e.verify_cigars(scores, pairs, claimed, arena)
            same_bytes(got, want, recs, (name, ename))
            st = e.verify_stats()
            assert (st.pairs, st.columns) == (len(recs), columns), (name, ename, st.pairs, st.columns)
            assert st.failed == sum(1 for c in want["code"] if c not in (ffi.AWV_VF_OK, ffi.AWV_VF_SKIPPED)), (name, ename)
    # ranges: intervals that begin off the dword grid, on both strands, then whole forward sequences
    recs, begs = RC.verify_ranges_list()
    seqs, ranges, claimed, arena = RC.verify_range_inputs(recs, begs, scores, random.Random("reuse/ranges"))
    want = _verify_want(ffi, scores, recs, seqs, ranges, claimed, arena)
    assert (want["code"] == ffi.AWV_VF_OK).all()
    for ename, e in scan_engines(engines):
        e.set_sequences(seqs)
        same_bytes(e.verify_ranges(scores, ranges, claimed, arena), want, recs, ("ranges", ename))


@pytest.mark.parametrize("a", [1, 2])
@pytest.mark.parametrize("scores", list(SCAN_SETS.values()), ids=list(SCAN_SETS))
def test_clip_waves_take_record_after_record(engines, scores, a):
    from allwave_amd import ffi
    for name, recs in RC.scan_lists().items():
        claimed, arena = RC.pack_back_to_back(recs)
        want = np.zeros(len(recs), dtype=ffi.CLIP_DTYPE)
        for k, r in enumerate(recs):
            if r.status == 0:
                want[k] = ffi.clip_one_host(scores, a, r.ops)
            else:
                want[k]["code"] = K.SKIPPED
        for ename, e in scan_engines(engines):
            got = e.clip_cigars(scores, a, claimed, arena)
            same_bytes(got, want, recs, (name, ename, a))
            st = e.clip_stats()
            assert (st.pairs, st.columns) == (len(recs), sum(len(r.ops) for r in recs if r.status == 0)), (name, ename)
            assert st.empty == sum(1 for c in want["code"] if c == K.EMPTY), (name, ename)


@pytest.mark.parametrize("min_score", [1, 20])
@pytest.mark.parametrize("a", [1, 2])
@pytest.mark.parametrize("scores", list(SCAN_SETS.values()), ids=list(SCAN_SETS))
def test_split_waves_take_record_after_record(engines, scores, a, min_score):
    """Index entries and the whole slot region, byte for byte: the yardstick's segments in their places and the caller's
    sentinel in every slot beyond a record's count."""
    from allwave_amd import ffi
    for name, recs in RC.scan_lists().items():
        claimed, arena = RC.pack_back_to_back(recs)
        need = [ffi.split_slots(a, min_score, len(r.ops)) if r.status == 0 else 0 for r in recs]
        seg_first = np.concatenate(([0], np.cumsum(need))).astype(np.uint64)
        blank = np.frombuffer(bytes([SENTINEL]) * (max(int(seg_first[-1]), 1) * ffi.CLIP_DTYPE.itemsize), dtype=ffi.CLIP_DTYPE)
        want_slots = blank.copy()
        want = np.zeros(len(recs), dtype=ffi.SPLIT_INDEX_DTYPE)
        for k, r in enumerate(recs):
            if r.status == 0:
                ix, segs = ffi.split_one_host(scores, a, min_score, r.ops)
                want[k] = ix
                assert int(ix["count"]) == len(segs) <= need[k]
                want_slots[int(seg_first[k]):int(seg_first[k]) + len(segs)] = segs
            else:
                want[k] = (K.SKIPPED, 0, -1)
        if name != "zero" and (scores, a, min_score) == (DEFAULT_2P, 1, 20):
            assert sorted(set(want["count"]))[-1] == 15 and (want["count"] == 1).sum() >= 2
        for ename, e in scan_engines(engines):
            slots = blank.copy()
            index, _ = e.split_cigars(scores, a, min_score, claimed, arena, seg_first=seg_first, slots=slots)
            same_bytes(index, want, recs, (name, ename, a, min_score))
            if slots.tobytes() != want_slots.tobytes():
                k = next(k for k in range(len(recs)) if slots[int(seg_first[k]):int(seg_first[k + 1])].tobytes() !=
                         want_slots[int(seg_first[k]):int(seg_first[k + 1])].tobytes())
                assert False, (name, ename, a, min_score, "the slots of record %d differ" % k, recs[k].kind, len(recs[k].ops))
            st = e.split_stats()
            assert (st.pairs, st.columns) == (len(recs), sum(len(r.ops) for r in recs if r.status == 0)), (name, ename)
            assert st.segments == int(want["count"].sum()) and st.empty == int((want["code"] == K.EMPTY).sum()), (name, ename)
            assert st.columns_scanned >= st.columns


def test_aligning_calls_with_two_workgroups(engines):
    """awv_align_pairs_verified / _clipped / _split on the island set with workgroups = 2: records, op bytes, verify, clip and
    split results are the default engine's, byte for byte."""
    seqs, pairs = S.island_set()
    a, min_score = 1, 30
    out = []
    for e in (engines("NO_ARENA_PROBE"), engines("NO_ARENA_PROBE", workgroups=2)):
        e.set_sequences(seqs)
        res, cigs, vres, cres = e.align_pairs(DEFAULT_2P, pairs, verify=True, clip=a)
        res2, cigs2, (index, segs) = e.align_pairs(DEFAULT_2P, pairs, split=(a, min_score))
        assert (res["status"] == 0).all() and (vres["code"] == 0).all() and e.verify_stats().pairs == e.clip_stats().pairs == len(pairs)
        out.append((res.tobytes(), cigs, vres.tobytes(), cres.tobytes(), res2.tobytes(), cigs2, index.tobytes(), [s.tobytes() for s in segs]))
        assert int(index["count"].sum()) > len(pairs)
    assert out[0] == out[1]


def test_default_grid_takes_several_records_per_wave(hip_lib):
    """Nothing set: what production runs.  12,288 records of 1 .. 64 columns, the kinds of the lists in rotation, through
    each of the three kernels against its yardstick -- at 16 waves per CU every wave takes more than one."""
    from allwave_amd import ffi
    n = 12288
    # the CU count as torch reports it, from a process of its own: in this one the engine's HIP runtime is loaded already,
    # and torch's does not find the device beside it (bench.py imports torch first for the same reason)
    child = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert child.returncode == 0, child.stderr.decode(errors="replace")[-2000:]
    assert 2 * 16 * int(child.stdout.split()[-1]) <= n  # a device with more CUs would turn this into a run without reuse
    recs = RC.default_path_records(n)
    seqs, pairs, claimed, arena = RC.verify_inputs(recs, DEFAULT_2P)
    e = ffi.Engine()
    try:
        e.set_sequences(seqs)
        same_bytes(e.verify_cigars(DEFAULT_2P, pairs, claimed, arena), _verify_want(ffi, DEFAULT_2P, recs, seqs, pairs, claimed, arena), recs, "verify")
        a, min_score = 2, 3
        want = np.zeros(n, dtype=ffi.CLIP_DTYPE)
        index = np.zeros(n, dtype=ffi.SPLIT_INDEX_DTYPE)
        segs = []
        for k, r in enumerate(recs):
            if r.status == 0:
                want[k] = ffi.clip_one_host(DEFAULT_2P, a, r.ops)
                ix, sg = ffi.split_one_host(DEFAULT_2P, a, min_score, r.ops)
                index[k] = ix
                segs.append(sg.tobytes())
            else:
                want[k]["code"] = K.SKIPPED
                index[k] = (K.SKIPPED, 0, -1)
                segs.append(b"")
        same_bytes(e.clip_cigars(DEFAULT_2P, a, claimed, arena), want, recs, "clip")
        got_index, got_segs = e.split_cigars(DEFAULT_2P, a, min_score, claimed, arena)
        same_bytes(got_index, index, recs, "split")
        assert [s.tobytes() for s in got_segs] == segs
        assert len(set(want["code"])) == 4 and int(index["count"].max()) >= 2
    finally:
        e.close()


def test_record_passes_share_their_checks(engines):
    """What every record pass checks before anything goes up, through each pass's own entry point: three
    20-column records back to back, the arena handed over one byte short of the last one.  The eight caller-supplied passes."""
    from allwave_amd import ffi
    e = engines("NO_ARENA_PROBE")
    seq = b"ACGTTGCAAC" * 2
    e.set_sequences([seq] * 2)
    pairs = [(0, 1, 0)] * 3
    recs = np.zeros(3, dtype=ffi.RESULT_DTYPE)
    recs["cigar_len"] = 20
    recs["cigar_off"] = [0, 20, 40]
    arena = b"M" * 59  # record 2 ends at byte 60
    NO_RUN = -1

    class ItemStats:
        """The stats of coverage and variants, which count since their begin and call a record an item: `pairs` is `items`; not
        among the fields that an empty call leaves zero: what begin itself sets."""
        def __init__(self, st, set_by_begin=()):
            self.st, self.pairs = st, st.items
            self._fields_ = [f for f in st._fields_ if f[0] not in set_by_begin]

        def __getattr__(self, f):
            return getattr(self.st, f)

    def coverage(r, n):  # (a begin of its own: the stats count from there)
        e.coverage_begin("both")
        return e.coverage_cigars(pairs[:n], r, arena)["code"]

    def variants(r, n):
        e.variants_begin()
        return e.variants_cigars(pairs[:n], r, arena)[0]["code"]

    passes = {
        "verify_cigars": (lambda r, n=3: e.verify_cigars(DEFAULT_2P, pairs[:n], r, arena)["code"], e.verify_stats, ffi.AWV_VF_SKIPPED),
        "clip_cigars": (lambda r, n=3: e.clip_cigars(DEFAULT_2P, 1, r, arena)["code"], e.clip_stats, ffi.AWV_CL_SKIPPED),
        "split_cigars": (lambda r, n=3: e.split_cigars(DEFAULT_2P, 1, 1, r, arena)[0]["code"], e.split_stats, ffi.AWV_CL_SKIPPED),
        "normalize_cigars": (lambda r, n=3: e.normalize_cigars("left", pairs[:n], r, arena)[1]["code"], e.normalize_stats, ffi.AWV_NM_SKIPPED),
        # (a text has no code: a record that was put off has no run, a completed one of 20 'M' columns has one)
        "encode_cigars": (lambda r, n=3: np.where(e.encode_cigars(r, arena)[1]["runs"] == 0, NO_RUN, 0), e.encode_stats, NO_RUN),
        "cs_cigars": (lambda r, n=3: e.cs_cigars("short", pairs[:n], r, arena)[1]["code"], e.cs_stats, ffi.AWV_CST_SKIPPED),
        "coverage_cigars": (lambda r, n=3: coverage(r, n), lambda: ItemStats(e.coverage_stats()), ffi.AWV_CV_SKIPPED),
        "variants_cigars": (lambda r, n=3: variants(r, n), lambda: ItemStats(e.variants_stats(), ("capacity_rows",)), ffi.AWV_VR_SKIPPED),
    }
    for name, (call, stats, skipped) in passes.items():
        with pytest.raises(ffi.EngineError) as err:
            call(recs)
        msg = ffi.load().awv_last_error().decode()
        assert err.value.code == ffi.AWV_ERR_ARG and msg.startswith(name + ":") and "outside the CIGAR arena" in msg, (name, err.value.code, msg)
        put_off = recs.copy()
        put_off["status"][2] = ffi.AWV_ST_CAPACITY
        codes = call(put_off)
        assert codes[2] == skipped and skipped not in codes[:2], (name, codes)
        assert stats().pairs == 3, name
        assert len(call(recs[:0], 0)) == 0, name
        st = stats()
        assert all(getattr(st, f) == 0 for f, _ in st._fields_), (name, [(f, getattr(st, f)) for f, _ in st._fields_])


# ---- the align kernels --------------------------------------------------------------------------------------------------------

FLAVOURS = {"one-wave": ("ONE_WAVE", "NO_TWIN"), "four-waves": ("FOUR_WAVES",), "one-wave-int32": ("ONE_WAVE", "FORCE_INT32"),
            "four-waves-int32": ("FOUR_WAVES", "FORCE_INT32")}
ALIGN_SETS = (DEFAULT_2P, P1, EDIT)


def trio(engines, flavour, **cfg):
    """The flavour's default engine and its two reduced ones, of one slot and of two: engine.hip divides `workgroups` by the
    waves of a workgroup."""
    names = FLAVOURS[flavour]
    waves = 4 if "FOUR_WAVES" in names else 1
    return [("default", engines(*names, **cfg)), ("one slot", engines(*names, workgroups=waves, **cfg)), ("two slots", engines(*names, workgroups=2 * waves, **cfg))]


def oracle_of(oracle, name, scores):
    seqs, pairs, kinds = RC.align_lists()[name]
    return seqs, pairs, kinds, TC.oracle_records(oracle, seqs, pairs, scores, key=("reuse", name))


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_align_workgroups_take_pair_after_pair(engines, oracle, flavour):
    """Every list on the flavour's three engines under three penalty sets, and list (a) + (h) under a ring-256 set: the
    oracle's records and op bytes, the same between the engines, the same base cases and searches -- only serialised."""
    runs = [(scores, name, {}) for scores in ALIGN_SETS for name in RC.align_lists()] + [(RING256, "deep", {"max_scratch_bytes": SCRATCH_CAP})]
    for scores, name, cfg in runs:
        seqs, pairs, kinds, want = oracle_of(oracle, name, scores)
        got, work = [], []
        for ename, e in trio(engines, flavour, **cfg):
            e.set_sequences(seqs)
            got.append(e.align_pairs(scores, pairs))
            st = e.stats()
            work.append((st.n_base, st.n_breakpoints))
            print("%s %s %s %s: %.2f ms, n_base %d n_breakpoints %d restarts %d windows[2] %d" %
                  (flavour, scores, name, ename, st.kernel_ms, st.n_base, st.n_breakpoints, st.restarts, st.windows[2]))
            TC.check_records(got[-1], want, seqs, pairs)
            assert st.pairs_completed == len(pairs)
            if scores == DEFAULT_2P and name.startswith("restart"):
                assert st.restarts > 0, (flavour, name, ename)
            if scores == DEFAULT_2P and name == "gaps":
                assert st.windows[2] > 0, (flavour, name, ename)
        TC.same_records(got[0], got[1])
        TC.same_records(got[0], got[2])
        assert work[0] == work[1] == work[2], (flavour, scores, name, work)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_slots_are_limited(hip_lib, oracle, flavour):
    """The arenas are sized per slot: fresh engines that ran the same list hold less scratch at one slot than at two, and
    less at two than by default."""
    from allwave_amd import ffi
    names = FLAVOURS[flavour]
    waves = 4 if "FOUR_WAVES" in names else 1
    flags = 0
    for n in names:
        flags |= getattr(ffi, "AWV_F_" + n)
    seqs, pairs, kinds, want = oracle_of(oracle, "deep", DEFAULT_2P)
    held = []
    for wg in (waves, 2 * waves, 0):
        e = ffi.Engine(flags=flags, workgroups=wg)
        try:
            e.set_sequences(seqs)
            TC.check_records(e.align_pairs(DEFAULT_2P, pairs), want, seqs, pairs)
            held.append(e.stats().scratch_bytes)
        finally:
            e.close()
    assert 0 < held[0] < held[1] < held[2], (flavour, held)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_one_slot_in_every_call_mode(engines, oracle, flavour):
    """The flavour's one-slot engine, every list: score-only, per-pair bounds that abandon every second or third pair
    mid-search, and the lists as ranges of longer resident sequences at every word phase on both strands."""
    from allwave_amd import ffi
    e = trio(engines, flavour)[1][1]
    first = 0
    for name in RC.align_lists():
        for scores in ALIGN_SETS:
            seqs, pairs, kinds, want = oracle_of(oracle, name, scores)
            e.set_sequences(seqs)
            TC.check_scores(e.score_pairs(scores, pairs), want, pairs)
            ref = e.align_pairs(scores, pairs)
            TC.check_records(ref, want, seqs, pairs)
            for every in (2, 3):
                bounds = RC.bounds_for(want, every)
                res, cigs = e.align_pairs(scores, pairs, max_penalty=bounds)
                sc = e.score_pairs(scores, pairs, max_penalty=bounds)
                BC.check_contract(ffi, bounds, res, cigs, sc, ref[0], ref[1], where=(flavour, name, scores, every))
                gone = res["status"] == ffi.AWV_ST_ABOVE_BOUND
                assert [bool(g) for g in gone] == [b >= 0 and pen > b for b, (pen, _) in zip(bounds, want)], (flavour, name, scores, every)
        for scores in (DEFAULT_2P, EDIT):
            seqs, pairs, kinds, want = oracle_of(oracle, name, scores)
            res_seqs, ranges = RC.as_ranges(seqs, pairs, first)
            e.set_sequences(res_seqs)
            res, cigs = e.align_ranges(scores, ranges)
            subs = [s for r in ranges.tolist() for s in (res_seqs[r[0]][r[3]:r[4]], res_seqs[r[1]][r[5]:r[6]])]
            TC.check_records((res, cigs), want, subs, [(2 * k, 2 * k + 1) for k in range(len(pairs))])
            TC.check_scores(e.score_ranges(scores, ranges), want, pairs)
        first += len(pairs)


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("flavour", ["one-wave", "one-wave-int32"])
def test_capacity_behind_and_before_other_pairs(engines, oracle, flavour, slots):
    """Rows capped at 2,048 columns on the twelve pairs of twin_cases.rerun_inputs: under AWV_F_NO_RERUN the divergent 6 kbp
    pairs end CAPACITY, and so do the six pairs of a 6 kbp sequence with the 1.5 kbp one -- they end on diagonal +-4,500, which
    a row of 2,048 columns cannot hold, whatever the kernel does.  The two 6 kbp pairs 1 % apart fit and are the oracle's: in
    dispatch order they run behind eight pairs that ended CAPACITY in the same workgroup and before two more.  Without the
    flag every pair is the oracle's, after a second launch."""
    from allwave_amd import ffi
    seqs, pairs, divergent = RC.capacity_list()
    divergent = [d or abs(len(seqs[q]) - len(seqs[t])) > 2048 for d, (q, t, _) in zip(divergent, pairs)]
    assert [k for k, d in enumerate(divergent) if not d] == [8, 9]
    want = TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key=("reuse", "capacity"))
    names = FLAVOURS[flavour]
    e = engines(*names, "NO_RERUN", workgroups=slots, first_row_cols=2048)
    e.set_sequences(seqs)
    res, cigs = e.align_pairs(DEFAULT_2P, pairs)
    print("%s, %d slot(s), NO_RERUN: statuses %s" % (flavour, slots, list(res["status"])))
    stayed = [k for k in range(len(pairs)) if not divergent[k]]
    assert [int(s) for s in res["status"]] == [ffi.AWV_ST_CAPACITY if d else 0 for d in divergent]
    TC.check_records((res[stayed], [cigs[k] for k in stayed]), [want[k] for k in stayed], seqs, [pairs[k] for k in stayed])
    e = engines(*names, workgroups=slots, first_row_cols=2048)
    e.set_sequences(seqs)
    got = e.align_pairs(DEFAULT_2P, pairs)
    TC.check_records(got, want, seqs, pairs)
    assert e.stats().launches >= 2
