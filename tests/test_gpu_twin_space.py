"""GPU tests (-m gpu) that carry twin units through the penalty space, the one-wave pins, the failure
branch and its re-run, workgroups that take unit after unit, degenerate score-only units, batch cuts, the engine's own
routing, the host layer and long reads.

Twin units exist only in the one-wave kernel with 16-bit rows, and a batch of at most WAVES_PER_SIMD * CUs pairs goes four
waves per pair, so nearly every case pins AWV_F_ONE_WAVE and lists each pair in both orders.  Every comparison is three-way
-- the twin path, the same engine configuration with AWV_F_NO_TWIN, the CPU oracle, every record field and every op byte
-- and every test asserts through Engine.twin_stats() that units were formed (or that none were where none may be): a run
in which the twin path silently formed no unit cannot pass.  Oracle results are computed once per (set, input).
"""
import os

import pytest

import penalty_space as PS
import twin_cases as TC
from util import DEFAULT_2P, rle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = os.path.join(ROOT, "tests", "golden", "pin")
LARGE_SB = 1100                 # as tests/test_gpu_penalties.py: sets above this get engines with capped scratch
SCRATCH_CAP = 6 << 30
NO_UNITS = (0, 0, 0, 0)
RERUN_COLS = 2048               # first_row_cols of the re-run cases: the divergent 6 kbp pairs outgrow such rows


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


def _cap(scores):
    return {"max_scratch_bytes": SCRATCH_CAP} if PS.derive(scores).sb > LARGE_SB else {}


def _penalty_oracle(oracle, name, unordered=None):
    """The oracle's records of penalty_inputs(name): all computed once, a shorter list being their first entries."""
    seqs, pairs = TC.penalty_inputs(name)
    want = TC.oracle_records(oracle, seqs, pairs, PS.BY_NAME[name], key=("twin-penalties", name))
    n = len(pairs) if unordered is None else 2 * unordered
    return seqs[:n], pairs[:n], want[:n]


_twelve_cache = {}


def _twelve(oracle):
    """twin_cases.twelve() and the oracle's record of each of its 133 directed pairs under the default scores."""
    if not _twelve_cache:
        seqs, pairs = TC.twelve()
        want = TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key="twelve")
        _twelve_cache["v"] = (seqs, pairs, dict(zip(pairs, want)))
    return _twelve_cache["v"]


# ---- 1. the penalty space, both orders

_SET_COUNTERS = {}


def _run_set(engines, oracle, name):
    """One accepted set on its both-order list: see test_penalty_space_in_both_orders.  Returns the twin counters of the
    run that shares at every level; each set is run once per session."""
    if name in _SET_COUNTERS:
        return _SET_COUNTERS[name]
    scores = PS.BY_NAME[name]
    seqs, pairs, want = _penalty_oracle(oracle, name)
    nunits = len(pairs) // 2        # 12, and 16 under the sets that need dearer pairs for a search below the top level
    assert nunits == (12 + TC.DEEP_EXTRA if name in TC.DEEP_SETS else 12)
    cap = _cap(scores)
    off = engines("ONE_WAVE", "NO_TWIN", **cap)
    off.set_sequences(seqs)
    plain = off.align_pairs(scores, pairs)
    assert off.twin_stats() == NO_UNITS, name
    plain_searches = off.stats().n_breakpoints
    TC.check_records(plain, want, seqs, pairs)
    plain_scores = off.score_pairs(scores, pairs)
    assert off.twin_stats() == NO_UNITS, name
    TC.check_scores(plain_scores, want, pairs)
    counters = None
    for depth in ("TWIN_TOP_ONLY", None):
        e = engines(*(("ONE_WAVE", depth) if depth else ("ONE_WAVE",)), **cap)
        e.set_sequences(seqs)
        got = e.align_pairs(scores, pairs)
        units, shared, solo, nonmirror = e.twin_stats()
        print("%s %s %s: units %d shared %d per-orientation %d non-mirror %d; searches %d, %d under AWV_F_NO_TWIN" %
              (name, scores, "top level only" if depth else "every level", units, shared, solo, nonmirror, e.stats().n_breakpoints, plain_searches))
        TC.same_records(got, plain)
        TC.check_records(got, want, seqs, pairs)
        assert units == nunits, (name, depth, units)
        if depth:
            assert 0 < shared <= nunits, (name, shared)     # at most the top-level search of each unit
        else:
            assert shared > nunits, (name, "no search below the top level ran shared", shared)
            counters = (units, shared, solo, nonmirror)
        st = e.stats()
        assert st.pairs_completed == len(pairs) and st.aligned_bp == sum(len(seqs[a]) for a, _ in pairs), name
        sc = e.score_pairs(scores, pairs)       # a score-only unit: one top-level search gives both entries their penalty
        assert e.twin_stats()[0] == nunits, (name, depth, e.twin_stats())
        TC.check_scores(sc, want, pairs)
        assert sc.tobytes() == plain_scores.tobytes(), name
    _SET_COUNTERS[name] = counters
    return counters


@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_penalty_space_in_both_orders(engines, oracle, name):
    """Every accepted set of tests/penalty_space.py on 12 unordered pairs listed in both orders (tests/test_twin_space_cpu.py
    shows from the oracle that the two orders break ties differently on 103 of the 372 pairs): rings up to 256, scopes up
    to 126 -- last-hit tables up to 630 entries, read back 64 per load --, equal, inverted and crossing pieces, and at ring
    256 no LDS left for the packed sequences, where the twin record is the last 32 bytes of the dynamic LDS.  Shared at
    every level, at the top level only and under AWV_F_NO_TWIN: records and bytes equal each other's and the oracle's, 12
    units in both twin runs and none in the plain one, more searches shared than there are units when every level shares;
    and the same lists score-only.  Under the five sets of twin_cases.DEEP_SETS no pair of the 12 costs enough for a search
    below the top level -- AWV_F_NO_TWIN runs 24 searches for the 24 entries --, so their lists carry four dearer pairs
    more: 16 units there."""
    _run_set(engines, oracle, name)


def test_some_shared_search_of_the_tie_rich_sets_is_not_a_mirror(engines, oracle):
    """Under the seven sets whose ties the two orders break differently on at least 7 of 12 pairs, some shared search must
    have found two breakpoints that are not mirror images (the four-way push): the one counter of awv_twin_stats that
    cannot be derived on the CPU."""
    counts = {name: _run_set(engines, oracle, name)[3] for name in TC.TIE_RICH}
    print("non-mirror shared searches: " + " ".join("%s:%d" % kv for kv in counts.items()))
    assert sum(counts.values()) > 0, counts


# ---- 2. the one-wave pins

PINS = ("SINGLE_STEP", "NO_CHAIN", "NO_DEEP", "NO_PACKED_SEQ")


@pytest.mark.parametrize("pin", PINS)
def test_one_wave_pins_form_units(engines, oracle, pin):
    """Each one-wave pin with AWV_F_ONE_WAVE over penalty_space.FLAVOUR_SETS, on the first 6 unordered pairs of part 1's
    lists in both orders: three-way equality and 6 units.  AWV_F_NO_PACKED_SEQ (every set) and the ring-256 sets (every
    pin) are the launches with lds_seq_bytes == 0: the twin record then lies at the very end of the dynamic LDS, which the
    kernel addresses as dyn_smem + lds_meta_bytes - 32 and the overlap search as lds.seq - 32."""
    on = engines("ONE_WAVE", pin, max_scratch_bytes=SCRATCH_CAP)
    off = engines("ONE_WAVE", pin, "NO_TWIN", max_scratch_bytes=SCRATCH_CAP)
    for name in PS.FLAVOUR_SETS:
        scores = PS.BY_NAME[name]
        seqs, pairs, want = _penalty_oracle(oracle, name, 6)
        off.set_sequences(seqs)
        plain = off.align_pairs(scores, pairs)
        assert off.twin_stats() == NO_UNITS, (pin, name)
        on.set_sequences(seqs)
        got = on.align_pairs(scores, pairs)
        ts = on.twin_stats()
        print("%s %s: units %d shared %d per-orientation %d non-mirror %d" % ((pin, name) + ts))
        TC.same_records(got, plain)
        TC.check_records(got, want, seqs, pairs)
        assert ts[0] == 6 and ts[1] >= 6, (pin, name, ts)


@pytest.mark.parametrize("variant", [("ONE_WAVE", "FORCE_INT32"), ("FOUR_WAVES",)], ids=["force_int32", "four_waves"])
def test_other_instantiations_form_no_unit(engines, oracle, variant):
    """32-bit rows and four waves per pair on part 2's lists: no unit, the oracle's bytes."""
    e = engines(*variant, max_scratch_bytes=SCRATCH_CAP)
    for name in PS.FLAVOUR_SETS:
        seqs, pairs, want = _penalty_oracle(oracle, name, 6)
        e.set_sequences(seqs)
        got = e.align_pairs(PS.BY_NAME[name], pairs)
        assert e.twin_stats() == NO_UNITS, (variant, name)
        TC.check_records(got, want, seqs, pairs)


# ---- 3. the failure branch and the re-run

def _rerun_oracle(oracle):
    seqs, pairs = TC.rerun_inputs()
    return seqs, pairs, TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key="rerun")


def test_unit_that_fails_is_rerun_and_paired_again(engines, oracle):
    """Rows capped at 2048 columns: the divergent 6 kbp pairs end CAPACITY inside their units -- the failure branch after the
    DFS, where one orientation keeps its non-OK record and the other is run again alone -- and the host pairs the CAPACITY
    entries again for the wider launch.  Six units form in the first launch and the counters sum over the call's launches,
    so a seventh unit proves that a re-run launch formed units.  Same launches, pairs and bases as under AWV_F_NO_TWIN."""
    seqs, pairs, want = _rerun_oracle(oracle)
    on = engines("ONE_WAVE", first_row_cols=RERUN_COLS)
    off = engines("ONE_WAVE", "NO_TWIN", first_row_cols=RERUN_COLS)
    off.set_sequences(seqs)
    plain = off.align_pairs(DEFAULT_2P, pairs)
    assert off.twin_stats() == NO_UNITS
    st_off = off.stats()
    on.set_sequences(seqs)
    got = on.align_pairs(DEFAULT_2P, pairs)
    ts = on.twin_stats()
    st_on = on.stats()
    print("re-run: launches %d (plain %d), units %d shared %d per-orientation %d non-mirror %d" % ((st_on.launches, st_off.launches) + ts))
    assert (got[0]["status"] == 0).all() and (plain[0]["status"] == 0).all()
    TC.same_records(got, plain)
    TC.check_records(got, want, seqs, pairs)
    assert st_on.launches >= 2 and st_off.launches >= 2 and st_on.launches == st_off.launches, (st_on.launches, st_off.launches)
    assert ts[0] >= 7, ts
    assert st_on.pairs_completed == st_off.pairs_completed == len(pairs)
    assert st_on.aligned_bp == st_off.aligned_bp == sum(len(seqs[a]) for a, _ in pairs)
    # score-only on the same engines
    plain_scores = off.score_pairs(DEFAULT_2P, pairs)
    assert off.twin_stats() == NO_UNITS
    sc = on.score_pairs(DEFAULT_2P, pairs)
    assert on.twin_stats()[0] >= 6, on.twin_stats()
    TC.check_scores(plain_scores, want, pairs)
    TC.check_scores(sc, want, pairs)
    assert sc.tobytes() == plain_scores.tobytes()


# ---- 4. unit after unit in one workgroup

def _pairing_oracle(oracle, scores):
    """PAIRING_LIST as (sequences, pairs) flattened so that check_records sees a q_revcomp entry's own query."""
    seqs, pairs = TC.pairing_sequences(), TC.PAIRING_LIST
    want = TC.oracle_records(oracle, seqs, pairs, scores, key="pairing")
    flat = [s for q, t, r in pairs for s in (TC.rc(seqs[q]) if r else seqs[q], seqs[t])]
    return seqs, pairs, want, flat, [(2 * i, 2 * i + 1) for i in range(len(pairs))]


def test_a_workgroup_takes_unit_after_unit(engines, oracle):
    """With workgroups = 3 (2 on the re-run list) every workgroup aligns about twenty units in turn, where every other twin
    test gives a workgroup at most one: what a unit leaves behind -- the second orientation's scalars, the twin record in
    LDS, the last-hit table, the mode bits of the stack -- must not reach the next one.  That is what this test is for.  On
    the 66 units and one single entry of `twelve`; on PAIRING_LIST, whose units include an empty sequence, identical
    sequences and lengths of at most 100 next to single entries; and with rows capped at 2048 columns, where a workgroup
    takes a fresh unit after one that ended CAPACITY."""
    seqs, pairs, by_pair = _twelve(oracle)
    want = [by_pair[p] for p in pairs]
    on, off = engines("ONE_WAVE", workgroups=3), engines("ONE_WAVE", "NO_TWIN", workgroups=3)
    for e in (off, on):
        e.set_sequences(seqs)
    plain, got = off.align_pairs(DEFAULT_2P, pairs), on.align_pairs(DEFAULT_2P, pairs)
    print("twelve, 3 workgroups: units %d shared %d per-orientation %d non-mirror %d" % on.twin_stats())
    assert off.twin_stats() == NO_UNITS and on.twin_stats()[0] == 66
    TC.same_records(got, plain)
    TC.check_records(got, want, seqs, pairs)
    assert on.stats().pairs_completed == 133

    seqs, pairs, want, flat, flat_pairs = _pairing_oracle(oracle, DEFAULT_2P)
    for e in (off, on):
        e.set_sequences(seqs)
    plain, got = off.align_pairs(DEFAULT_2P, pairs), on.align_pairs(DEFAULT_2P, pairs)
    print("pairing list, 3 workgroups: units %d shared %d per-orientation %d non-mirror %d" % on.twin_stats())
    assert off.twin_stats() == NO_UNITS and on.twin_stats()[0] == 8
    TC.same_records(got, plain)
    TC.check_records(got, want, flat, flat_pairs)
    assert on.stats().pairs_completed == len(pairs)

    seqs, pairs, want = _rerun_oracle(oracle)
    on = engines("ONE_WAVE", workgroups=2, first_row_cols=RERUN_COLS)
    off = engines("ONE_WAVE", "NO_TWIN", workgroups=2, first_row_cols=RERUN_COLS)
    for e in (off, on):
        e.set_sequences(seqs)
    plain, got = off.align_pairs(DEFAULT_2P, pairs), on.align_pairs(DEFAULT_2P, pairs)
    print("re-run list, 2 workgroups: launches %d, units %d shared %d per-orientation %d non-mirror %d" % ((on.stats().launches,) + on.twin_stats()))
    assert off.twin_stats() == NO_UNITS and on.twin_stats()[0] >= 7, on.twin_stats()
    TC.same_records(got, plain)
    TC.check_records(got, want, seqs, pairs)
    assert on.stats().launches == off.stats().launches >= 2


# ---- 5. degenerate score-only units

@pytest.mark.parametrize("scores", [DEFAULT_2P, (0, 4, 6, 2), (0, 7, 0, 3)], ids=str)
def test_score_only_units_on_degenerate_entries(engines, oracle, scores):
    """awv_score_pairs on PAIRING_LIST: units of an empty sequence, of identical sequences and of lengths of at most 100 --
    where a shared top task is split into an A and a B task instead of searched -- next to single, duplicate and
    q_revcomp entries.  The oracle's penalties (a q_revcomp entry's query reverse-complemented), AWV_F_NO_TWIN's bytes,
    8 units."""
    seqs, pairs, want, _, _ = _pairing_oracle(oracle, scores)
    on, off = engines("ONE_WAVE"), engines("ONE_WAVE", "NO_TWIN")
    off.set_sequences(seqs)
    plain = off.score_pairs(scores, pairs)
    assert off.twin_stats() == NO_UNITS
    on.set_sequences(seqs)
    got = on.score_pairs(scores, pairs)
    print("%s score-only pairing list: units %d shared %d per-orientation %d non-mirror %d" % ((scores,) + on.twin_stats()))
    assert on.twin_stats()[0] == 8, on.twin_stats()
    TC.check_scores(plain, want, pairs)
    TC.check_scores(got, want, pairs)
    assert got.tobytes() == plain.tobytes()


# ---- 6. batch cuts, the engine's own routing, the host, long reads

def _carve(lengths, pairs, max_arena):
    """engine.hip's batch carving under max_arena_bytes, restated: an entry takes (ql + tl + 7) & ~7 bytes of CIGAR arena and
    a batch ends before the entry that would pass the cap (a batch always takes one entry).  Returns each entry's batch."""
    batch, used, n, out = 0, 0, 0, []
    for q, t in pairs:
        need = (lengths[q] + lengths[t] + 7) & ~7
        if n > 0 and used + need > max_arena:
            batch, used, n = batch + 1, 0, 0
        out.append(batch)
        used += need
        n += 1
    return out


def test_batch_cuts_separate_some_twins(engines, oracle):
    """The 66 unordered pairs of `twelve`, each followed by its twin, cut into batches of 7 entries and into batches of
    about five entries' CIGAR arena: a twin on the far side of a cut stays single (twins never cross a launch), so the
    units are exactly the pairs no cut separates; bytes equal the unbatched call's, AWV_F_NO_TWIN's and the oracle's."""
    seqs, _, by_pair = _twelve(oracle)
    seqs = seqs[:12]
    pairs = TC.interleaved(12)
    want = [by_pair[p] for p in pairs]
    whole, off = engines("ONE_WAVE"), engines("ONE_WAVE", "NO_TWIN")
    for e in (whole, off):
        e.set_sequences(seqs)
    ref, plain = whole.align_pairs(DEFAULT_2P, pairs), off.align_pairs(DEFAULT_2P, pairs)
    assert whole.twin_stats()[0] == 66 and whole.stats().launches == 1 and off.twin_stats() == NO_UNITS
    TC.same_records(ref, plain)
    TC.check_records(ref, want, seqs, pairs)

    by7 = engines("ONE_WAVE", max_batch_pairs=7)
    by7.set_sequences(seqs)
    got = by7.align_pairs(DEFAULT_2P, pairs)
    expect = sum((2 * k) // 7 == (2 * k + 1) // 7 for k in range(66))
    print("batches of 7: launches %d, units %d (expected %d) shared %d per-orientation %d non-mirror %d" %
          ((by7.stats().launches, by7.twin_stats()[0], expect) + by7.twin_stats()[1:]))
    assert by7.stats().launches == 19 and 0 < expect < 66
    assert by7.twin_stats()[0] == expect
    assert got[1] == ref[1]
    for name in got[0].dtype.names:
        if name != "cigar_off":   # (an offset into its own batch's arena)
            assert (got[0][name] == ref[0][name]).all(), name

    lengths = [len(s) for s in seqs]
    cap = 5 * (2 * max(lengths) + 8) * 7 // 10      # about five entries (the mean entry is ~0.7 of the largest)
    batch_of = _carve(lengths, pairs, cap)
    expect = sum(batch_of[2 * k] == batch_of[2 * k + 1] for k in range(66))
    arena = engines("ONE_WAVE", max_arena_bytes=cap)
    arena.set_sequences(seqs)
    got = arena.align_pairs(DEFAULT_2P, pairs)
    print("arena of %d bytes: launches %d (carved %d), units %d (expected %d) shared %d per-orientation %d non-mirror %d" %
          ((cap, arena.stats().launches, batch_of[-1] + 1, arena.twin_stats()[0], expect) + arena.twin_stats()[1:]))
    assert arena.stats().launches == batch_of[-1] + 1 >= 20 and 0 < expect < 66
    assert arena.twin_stats()[0] == expect
    assert got[1] == ref[1]
    for name in got[0].dtype.names:
        if name != "cigar_off":
            assert (got[0][name] == ref[0][name]).all(), name


def test_the_engines_own_routing_forms_units(engines, oracle):
    """Default flags: the 4,290 directed pairs of 66 sequences of 300-450 bases, 2-6 % from one base -- one batch above
    WAVES_PER_SIMD * CUs, and above 4 * WAVES_PER_SIMD * CUs should the engine call its costs skewed (they are even: the
    dearest pair costs under three times the median) -- go one wave per pair by the engine's own choice: 2,145 units, the
    bytes of AWV_F_NO_TWIN and of the oracle."""
    cus = _compute_units()
    if cus > 1072:
        pytest.skip("%d CUs: 4,290 pairs no longer exceed 4 * WAVES_PER_SIMD * CUs, the batch would go four waves per pair" % cus)
    seqs, pairs = TC.routing_inputs()
    assert len(pairs) == 4290
    want = TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key="routing")
    on, off = engines(), engines("NO_TWIN")
    off.set_sequences(seqs)
    plain = off.align_pairs(DEFAULT_2P, pairs)
    assert off.twin_stats() == NO_UNITS
    on.set_sequences(seqs)
    got = on.align_pairs(DEFAULT_2P, pairs)
    print("own routing: units %d shared %d per-orientation %d non-mirror %d" % on.twin_stats())
    assert on.twin_stats()[0] == 2145, on.twin_stats()
    TC.same_records(got, plain)
    TC.check_records(got, want, seqs, pairs)
    assert on.stats().launches == 1 and on.stats().pairs_completed == 4290


def _compute_units():
    """The CU count of device 0, from the HIP runtime the engine's library is linked against."""
    import ctypes as C
    from allwave_amd import ffi
    n = C.c_int(0)
    rc = ffi.load().hipDeviceGetAttribute(C.byref(n), 63, 0)   # hipDeviceAttributeMultiprocessorCount
    assert rc == 0 and n.value > 0, (rc, n.value)
    return n.value


def _fasta(path):
    ids, seqs = [], []
    for ln in open(path).read().splitlines():
        if ln.startswith(">"):
            ids.append(ln[1:].split()[0])
            seqs.append(b"")
        else:
            seqs[-1] += ln.strip().encode()
    return ids, seqs


def test_host_layer_on_the_twin_path(hip_lib, engines, oracle):
    """The host library with its engines pinned to AWV_F_ONE_WAVE and to AWV_F_ONE_WAVE | AWV_F_NO_TWIN: the same PAF text
    for the re-run sequences (every line the oracle's) and for the pinned 8 x 10 kbp read set -- config 2's read length,
    LDS staging at its limit -- which must also equal the committed c2_8x10k.expected.paf.  The host layer does not
    report twin counters: the same 56 pairs through the engine form 28 units and give the pinned CIGARs."""
    from allwave_amd import build, ffi, host
    build.build_host()
    host.load()
    scores = "0,5,8,2,24,1"
    seqs, pairs, want = _rerun_oracle(oracle)
    ids = ["r%d" % i for i in range(len(seqs))]
    pin_ids, pin_seqs = _fasta(os.path.join(PIN, "c2_8x10k.fa"))
    assert len(pin_ids) == 8
    text = {}
    try:
        for flags in (ffi.AWV_F_ONE_WAVE, ffi.AWV_F_ONE_WAVE | ffi.AWV_F_NO_TWIN):
            host.set_engine_config(flags=flags, release=True)
            text[flags] = (host.all_pairs_paf(ids, seqs, scores, orientation="forward", sparsification="none"),
                           host.all_pairs_paf(pin_ids, pin_seqs, scores, orientation="mash", sparsification="none"))
    finally:
        host.set_engine_config(flags=0, release=True)
    on, off = text[ffi.AWV_F_ONE_WAVE], text[ffi.AWV_F_ONE_WAVE | ffi.AWV_F_NO_TWIN]
    assert on[0] == off[0] and on[1] == off[1]
    assert len(on[0]) == len(pairs)
    for line, (q, t), (pen, ops) in zip(on[0], pairs, want):
        f = line.split("\t")
        assert (f[0], f[5], f[4], f[-1]) == (ids[q], ids[t], "+", "cg:Z:" + rle(ops)), (q, t)
    expected = open(os.path.join(PIN, "c2_8x10k.expected.paf")).read().splitlines()
    assert sorted(on[1]) == sorted(expected)
    # the same read set through the engine: 28 units, the pinned CIGARs
    cg = {(f[0], f[5]): f[-1] for f in (ln.split("\t") for ln in expected)}
    n = len(pin_ids)
    pin_pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    e, plain_e = engines("ONE_WAVE"), engines("ONE_WAVE", "NO_TWIN")
    for x in (e, plain_e):
        x.set_sequences(pin_seqs)
    got, plain = e.align_pairs(DEFAULT_2P, pin_pairs), plain_e.align_pairs(DEFAULT_2P, pin_pairs)
    print("8 x 10 kbp: units %d shared %d per-orientation %d non-mirror %d" % e.twin_stats())
    assert e.twin_stats()[0] == 28 and plain_e.twin_stats() == NO_UNITS
    TC.same_records(got, plain)
    assert (got[0]["status"] == 0).all()
    for (q, t), ops in zip(pin_pairs, got[1]):
        assert "cg:Z:" + rle(ops) == cg[(pin_ids[q], pin_ids[t])], (q, t)


def test_long_reads_at_the_edge_of_16_bit_rows(engines, oracle):
    """Both orders of: two sequences of exactly 32,759 bases, the last length on 16-bit rows, where the mirrored record's
    off_f - kf and the last-hit entries lie at the edge of the range; 24 kbp against 30 kbp; 9 kbp against 24 kbp, where
    one sequence is staged in LDS and the other is not, and the swapped frame exchanges which.  All 2-3 % apart.
    Three-way equality, 3 units."""
    seqs, pairs = TC.long_read_inputs()
    assert [len(s) for s in seqs] == [TC.LAST_16BIT_LENGTH, TC.LAST_16BIT_LENGTH, 24000, 30000, 9000, 24000]
    want = TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key="long-reads")
    on, off = engines("ONE_WAVE"), engines("ONE_WAVE", "NO_TWIN")
    off.set_sequences(seqs)
    plain = off.align_pairs(DEFAULT_2P, pairs)
    assert off.twin_stats() == NO_UNITS
    on.set_sequences(seqs)
    got = on.align_pairs(DEFAULT_2P, pairs)
    print("long reads: launches %d, units %d shared %d per-orientation %d non-mirror %d" % ((on.stats().launches,) + on.twin_stats()))
    assert on.twin_stats()[0] == 3 and on.twin_stats()[1] > 3, on.twin_stats()
    TC.same_records(got, plain)
    TC.check_records(got, want, seqs, pairs)
    assert on.stats().launches == off.stats().launches
