"""GPU tests (-m gpu) of the shared base case of twin units: a base case under a shared task runs its
wavefronts once, in the first entry's frame, and is backtraced for both orientations -- the swapped one through the mirror
rule of allwave_amd/csrc/twin_base.hpp.

Twin units exist only in the one-wave kernel with 16-bit rows, and a small batch goes four waves per pair, so every case
pins AWV_F_ONE_WAVE and lists each pair in both orders.  Every comparison is three-way -- the default path, the same
configuration with AWV_F_NO_TWIN_BASE (each orientation runs the base case for itself: the path as it was), the CPU oracle,
every record field and every op byte -- and every case that forms a unit with a base case asserts from awv_stats that the
sharing took place: fewer base cases and fewer cell-steps than under the pin, and the expected unit count from
awv_twin_stats.  Oracle results are computed once per input and shared.
"""
import pytest

import penalty_space as PS
import twin_base_cases as BC
import twin_cases as TC
from util import DEFAULT_2P

pytestmark = pytest.mark.gpu

AFFINE = (0, 4, 6, 2)
LARGE_SB = 1100                 # as tests/test_gpu_penalties.py: sets above this get engines with capped scratch
SCRATCH_CAP = 6 << 30
NO_UNITS = (0, 0, 0, 0)
RERUN_COLS = 2048               # first_row_cols of the re-run case: the divergent 6 kbp pairs outgrow such rows


@pytest.fixture(scope="module")
def engines(hip_lib):
    """Engines by (flag names, other awv_engine_config fields), made on first use and closed with the module.  (All of them
    take the first ring-arena allocation as it comes: a test engine has too little work for the probe to pay.)"""
    from allwave_amd import ffi
    made = {}

    def get(*names, **cfg):
        key = (tuple(n for n in names if n), tuple(sorted(cfg.items())))
        if key not in made:
            flags = ffi.AWV_F_NO_ARENA_PROBE
            for n in key[0]:
                flags |= getattr(ffi, "AWV_F_" + n)
            made[key] = ffi.Engine(flags=flags, **cfg)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _cap(scores):
    return {"max_scratch_bytes": SCRATCH_CAP} if PS.derive(scores).sb > LARGE_SB else {}


def _work(e):
    st = e.stats()
    return int(st.n_base), int(st.cell_steps), int(st.launches)


def three_way(engines, oracle, seqs, pairs, scores, key, extra=(), cfg=None, units=None, shares=True, label=""):
    """The default path, AWV_F_NO_TWIN_BASE and the oracle on one both-order list; returns the default path's output."""
    cfg = dict(cfg or {})
    want = TC.oracle_records(oracle, seqs, pairs, scores, key=key)
    on, pin = engines("ONE_WAVE", *extra, **cfg), engines("ONE_WAVE", "NO_TWIN_BASE", *extra, **cfg)
    pin.set_sequences(seqs)
    pinned = pin.align_pairs(scores, pairs)
    ts_pin, w_pin = pin.twin_stats(), _work(pin)
    on.set_sequences(seqs)
    got = on.align_pairs(scores, pairs)
    ts_on, w_on = on.twin_stats(), _work(on)
    print("%s %s %s: units %d shared %d per-orientation %d non-mirror %d; base cases %d (pinned %d), cell-steps %d (pinned %d)" %
          ((label or key, scores, "+".join(extra) or "-") + ts_on + (w_on[0], w_pin[0], w_on[1], w_pin[1])))
    TC.same_records(got, pinned)
    TC.check_records(pinned, want, seqs, pairs)
    TC.check_records(got, want, seqs, pairs)
    if units is None:
        units = len(pairs) // 2
    if units >= 0:      # (-1: the caller asserts the count)
        assert ts_on[0] == units, ts_on
    assert ts_on[0] == ts_pin[0], (ts_on, ts_pin)
    assert ts_on[1:] == ts_pin[1:], (ts_on, ts_pin)     # the searches are the same searches
    if shares:
        assert w_on[0] < w_pin[0] and w_on[1] < w_pin[1], (w_on, w_pin)
    return got, want


# ---- 1. top-level base cases

@pytest.mark.parametrize("scores", [DEFAULT_2P, AFFINE], ids=str)
def test_top_level_base_cases(engines, oracle, scores):
    """Both lengths at most 100: the unit's top task is a base case (equal and unequal lengths, identical sequences, one base
    against many, unrelated sequences, small repeats).  One base case per unit instead of two; and score-only, where a unit
    runs one base case for both scores and counts no more cells than the full alignment of the list."""
    seqs, pairs = BC.top_level_pairs()
    assert all(len(s) <= BC.MIN_LENGTH for s in seqs)
    three_way(engines, oracle, seqs, pairs, scores, "twin-base/top")
    want = TC.oracle_records(oracle, seqs, pairs, scores, key="twin-base/top")
    on, pin = engines("ONE_WAVE"), engines("ONE_WAVE", "NO_TWIN_BASE")
    n = len(pairs) // 2
    assert _work(on)[0] == n and _work(pin)[0] == 2 * n        # (three_way's align_pairs calls)
    full_cells = _work(on)[1]
    sc = on.score_pairs(scores, pairs)
    w_on = _work(on)
    assert on.twin_stats()[0] == n
    pin.set_sequences(seqs)
    sc_pin = pin.score_pairs(scores, pairs)
    w_pin = _work(pin)
    print("score-only: base cases %d (pinned %d), cell-steps %d (pinned %d; the full alignment %d)" % (w_on[0], w_pin[0], w_on[1], w_pin[1], full_cells))
    TC.check_scores(sc, want, pairs)
    assert sc.tobytes() == sc_pin.tobytes()
    assert w_on[0] == n and w_pin[0] == 2 * n and w_on[1] < w_pin[1]
    assert w_on[1] <= full_cells


# ---- 2. base cases that begin or end in a gap component

@pytest.mark.parametrize("scores", [DEFAULT_2P, (0, 7, 12, 2, 36, 1), AFFINE], ids=str)
def test_base_cases_that_begin_or_end_in_a_gap(engines, oracle, scores):
    """Long indels of both gap pieces every 60-200 bases, 300-1500 bp: breakpoints fall inside them, and the base cases on
    either side begin / end in I1, D1, I2 or D2 -- the mirrored backtrace then starts in, and ends in, the twin component."""
    seqs, pairs = BC.gap_component_pairs()
    assert all(300 <= len(s) <= 1500 for s in seqs)
    got, _ = three_way(engines, oracle, seqs, pairs, scores, "twin-base/gaps")
    res = got[0]
    assert (res["num_ins"] + res["num_del"] > 10).all()


# ---- 3. tie-rich pairs

def test_tie_rich_pairs_whose_swap_is_not_the_mirror(engines, oracle):
    """Microsatellites, tandem arrays, homopolymer ends and low-complexity pairs at 300-1500 bp: for at least
    TIE_MIN_NOT_MIRRORED of the 16 the oracle's swapped op string is not the I/D swap of the original -- emitting A's ops with
    I and D exchanged would fail here --, and on some of them every search of the unit ran shared with mirrored breakpoints, so
    the difference lies inside a base case."""
    seqs, pairs = BC.tie_rich_pairs()
    assert all(300 <= len(s) <= 1500 for s in seqs), [len(s) for s in seqs]
    got, want = three_way(engines, oracle, seqs, pairs, DEFAULT_2P, "twin-base/ties")
    differ = TC.not_mirrored(want)
    print("%d of %d unordered pairs: the swapped pair's ops are not the I/D swap" % (differ, len(pairs) // 2))
    assert differ >= BC.TIE_MIN_NOT_MIRRORED
    # one such pair at a time: no search of its own for either orientation and no non-mirror search, so every difference
    # between the two op strings comes out of a shared base case
    inside = 0
    on = engines("ONE_WAVE")
    for k in range(0, len(pairs), 2):
        if want[k + 1][1] == want[k][1].translate(TC.SWAP):
            continue
        on.set_sequences(seqs[k:k + 2])
        one = on.align_pairs(DEFAULT_2P, [(0, 1), (1, 0)])
        units, shared, solo, nonmirror = on.twin_stats()
        assert units == 1 and [one[1][0], one[1][1]] == [want[k][1], want[k + 1][1]]
        inside += solo == 0 and nonmirror == 0
    print("%d of them differ inside a shared base case" % inside)
    assert inside >= 1


# ---- 4. forced gaps: trimmed rows, k_end != 0

def test_forced_gap_trims_rows_inside_a_shared_base_case(engines, oracle):
    """Very unequal lengths that cost less than 250: the wavefronts run off the short side, a pass is discarded and the base
    case goes on step by step with trimmed rows (step-by-step base windows are counted); k_end is -200 .. 200, and each
    pair is listed with the short sequence first and with the long one first."""
    seqs, pairs = BC.forced_gap_pairs()
    three_way(engines, oracle, seqs, pairs, DEFAULT_2P, "twin-base/forced")
    assert int(engines("ONE_WAVE").stats().windows[2]) > 0, "no base case left its passes: the rows were never trimmed"
    assert sorted(set(len(seqs[a]) < len(seqs[b]) for a, b in pairs[::2])) == [False, True]


# ---- 5. the penalty space

@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_penalty_space(engines, oracle, name):
    """Every accepted set of tests/penalty_space.py on the 12 unordered pairs of twin_cases.penalty_inputs, both orders (16
    under the sets that need dearer pairs for a search below the top level, as in tests/test_gpu_twin_space.py)."""
    scores = PS.BY_NAME[name]
    seqs, pairs = TC.penalty_inputs(name)
    assert len(pairs) // 2 == (12 + TC.DEEP_EXTRA if name in TC.DEEP_SETS else 12)
    three_way(engines, oracle, seqs, pairs, scores, ("twin-penalties", name), cfg=_cap(scores), label=name)


# ---- 6. the one-wave pins, and a sequence with an N

@pytest.mark.parametrize("pin", ("SINGLE_STEP", "NO_CHAIN", "NO_DEEP", "NO_PACKED_SEQ", "TWIN_TOP_ONLY"))
def test_one_wave_pins(engines, oracle, pin):
    """Each one-wave pin on the lists of parts 2, 4 and 1.  Under AWV_F_TWIN_TOP_ONLY only the top task is shared, so a base
    case is shared where it is the top task -- part 1's list -- and nowhere on the other two, whose pairs are longer than
    100 bases: there the two runs must count the same work."""
    top_only = pin == "TWIN_TOP_ONLY"
    for key, (seqs, pairs), shares in (("twin-base/gaps", BC.gap_component_pairs(), not top_only),
                                       ("twin-base/forced", BC.forced_gap_pairs(), not top_only),
                                       ("twin-base/top", BC.top_level_pairs(), True)):
        three_way(engines, oracle, seqs, pairs, DEFAULT_2P, key, extra=(pin,), shares=shares)
        if not shares:
            on, off = engines("ONE_WAVE", pin), engines("ONE_WAVE", "NO_TWIN_BASE", pin)
            assert _work(on)[:2] == _work(off)[:2]


def test_sequence_with_an_n(engines, oracle):
    """An N in one sequence of a pair: no 2-bit packed view for it, raw-byte probes in the base case's extension."""
    seqs, pairs = BC.with_an_n()
    assert sum(b"N" in s for s in seqs) == 2
    three_way(engines, oracle, seqs, pairs, DEFAULT_2P, "twin-base/n")


# ---- 7. the failure branch

def test_unit_that_fails_is_rerun(engines, oracle):
    """Rows capped at 2048 columns (twin_cases.rerun_inputs): the divergent 6 kbp pairs end CAPACITY inside their units, one
    orientation keeps its record and the other runs alone, and the host pairs them again for the wider launch; same
    launches and records as under the pin.  A base case's own rows do not depend on first_row_cols -- they are sized by the
    penalties' score bound, which no base case exceeds -- so no size makes a shared base case itself end CAPACITY: only the
    search case exists, and a shared base case's ST_TWIN_REDO branch is reachable by an internal error alone."""
    seqs, pairs = TC.rerun_inputs()
    cfg = {"first_row_cols": RERUN_COLS}
    got, _ = three_way(engines, oracle, seqs, pairs, DEFAULT_2P, "rerun", cfg=cfg, units=-1)
    on, pin = engines("ONE_WAVE", **cfg), engines("ONE_WAVE", "NO_TWIN_BASE", **cfg)
    assert _work(on)[2] == _work(pin)[2] >= 2
    assert on.twin_stats()[0] >= 7, on.twin_stats()     # (six units in the first launch, the counters sum over the call's launches)
    assert (got[0]["status"] == 0).all()


# ---- 8. unit after unit in one workgroup

def test_a_workgroup_takes_unit_after_unit(engines, oracle):
    """workgroups = 2: each workgroup aligns a dozen units in turn, base case after base case in the same history slot,
    metadata log and `events` -- what the second backtrace of one leaves there must not reach the next."""
    ab = []
    for seqs, pairs in (BC.gap_component_pairs(), BC.top_level_pairs(), BC.forced_gap_pairs(), BC.tie_rich_pairs()):
        ab += [(seqs[a], seqs[b]) for a, b in pairs[::2]]
    seqs, pairs = TC.both_orders(ab)
    assert len(pairs) // 2 >= 40
    three_way(engines, oracle, seqs, pairs, DEFAULT_2P, "twin-base/all", cfg={"workgroups": 2})


# ---- 9. the other instantiations

@pytest.mark.parametrize("variant", [("ONE_WAVE", "FORCE_INT32"), ("FOUR_WAVES",)], ids=["force_int32", "four_waves"])
def test_other_instantiations_form_no_unit(engines, oracle, variant):
    """32-bit rows and four waves per pair on the lists of parts 2 and 4: no unit, the oracle's bytes, with and without the pin."""
    for key, (seqs, pairs) in (("twin-base/gaps", BC.gap_component_pairs()), ("twin-base/forced", BC.forced_gap_pairs())):
        want = TC.oracle_records(oracle, seqs, pairs, DEFAULT_2P, key=key)
        outs = []
        for flags in (variant, variant + ("NO_TWIN_BASE",)):
            e = engines(*flags)
            e.set_sequences(seqs)
            outs.append(e.align_pairs(DEFAULT_2P, pairs))
            assert e.twin_stats() == NO_UNITS, (flags, key)
            TC.check_records(outs[-1], want, seqs, pairs)
        TC.same_records(outs[0], outs[1])
