"""GPU tests (-m gpu) of row reuse below level 1: every search below a pair's top-level search that begins at
its origin in M -- the left half, the left half of the left half, and so on -- takes the forward rows of the top-level search's
archive, and every search that ends at its end in M the reverse rows.  Every case runs three ways -- the default path, the
level-1 pin AWV_F_ROW_REUSE_LEVEL1 (only the two halves take: the path as it was) and AWV_F_NO_ROW_REUSE (every search computes
all of its rows) -- and every result field and every CIGAR byte must be equal among the three and equal to the CPU oracle's;
the algorithm's counters (cell-steps, cells of multi-step passes, cells of deep passes, restarted searches, searches, base
cases) must be the same numbers under all three.  Each case then asserts from awv_stats.prof[10] / prof[11] (cell-steps taken
by searches below level 1, and those searches) whether such searches took rows; prof[12] / prof[13] stay the two halves' own
and must not depend on the pin.

The shapes are tests/row_reuse_cases.py's where a search two levels down still runs multi-step passes at them (3.5 kbp at 10
and 20 %), and 7 kbp at 5 %: there a quarter of the pair is 1,750 bases at a score near 300, just above the base case's 250."""
import random

import pytest

import row_reuse_cases as RC
from util import mutate, rand_seq
from twin_cases import check_records, oracle_records, same_records

pytestmark = pytest.mark.gpu

COUNTERS = ("cell_steps", "multi_cell_steps", "deep_cell_steps", "restarts", "n_breakpoints", "n_base", "pairs_completed")


@pytest.fixture(scope="module")
def engines(hip_lib):
    from allwave_amd import ffi
    made = {}

    def get(flags=0, **kw):
        key = (flags, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = ffi.Engine(flags=flags, **kw)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def run_three(engines, oracle, seqs, pairs, scores, key=None, **kw):
    """Aligns the list on the default path, with the level-1 pin and without row reuse; all three against the oracle and
    against each other.  Returns (cell-steps taken below level 1, searches below level 1 that took some, stats of the default
    path, the engine of the default path)."""
    from allwave_amd import ffi
    want = oracle_records(oracle, seqs, pairs, scores, key=key)
    out = []
    for extra in (0, ffi.AWV_F_ROW_REUSE_LEVEL1, ffi.AWV_F_NO_ROW_REUSE):
        e = engines(ffi.AWV_F_ONE_WAVE | extra, **kw)
        e.set_sequences(seqs)
        got = e.align_pairs(scores, pairs)
        out.append((got, e.stats()))
        check_records(got, want, seqs, pairs)
    (on, st_on), (pin, st_pin), (off, st_off) = out
    same_records(on, pin)
    same_records(on, off)
    for name in COUNTERS:
        assert getattr(st_on, name) == getattr(st_pin, name) == getattr(st_off, name), (name, getattr(st_on, name), getattr(st_pin, name), getattr(st_off, name))
    assert all(st_off.prof[i] == 0 for i in (10, 11, 12, 13))
    assert st_pin.prof[10] == 0 and st_pin.prof[11] == 0
    assert (st_pin.prof[12], st_pin.prof[13]) == (st_on.prof[12], st_on.prof[13])  # what the two halves take is the same either way
    assert st_on.launches == st_pin.launches == st_off.launches
    print("below level 1: %d cell-steps in %d searches; level 1: %d in %d; of %d cell-steps in %d searches; restarts %d" %
          (st_on.prof[10], st_on.prof[11], st_on.prof[12], st_on.prof[13], st_on.cell_steps, st_on.n_breakpoints, st_on.restarts))
    return int(st_on.prof[10]), int(st_on.prof[11]), st_on, engines(ffi.AWV_F_ONE_WAVE, **kw)


@pytest.mark.parametrize("d,n", [(0.05, 7000), (0.10, 3500), (0.20, 3500)])
def test_twin_unit_and_the_same_pair_alone(engines, oracle, d, n):
    """The left half's left half and the right half's right half are searched at all three divergences, as a twin unit's
    shared tasks and in the plain tree: both take rows, and what the two halves above them take does not change."""
    cells, searches, st, _ = run_three(engines, oracle, *RC.twin_unit(d, n), RC.DEFAULT_2P, key="rrl-twin-%g-%d" % (d, n))
    assert cells > 0 and searches >= 2
    cells1, searches1, st1, _ = run_three(engines, oracle, *RC.alone(d, n), RC.DEFAULT_2P, key="rrl-alone-%g-%d" % (d, n))
    assert (cells1, searches1) == (cells, searches)  # a shared search takes what A's own search takes
    assert st.pairs_completed == 2 and st1.pairs_completed == 1


def test_breakpoints_in_indel_components(engines, oracle):
    """Top-level breakpoints inside a gap: the two halves meet in I2, D1 or D2, the chains of outer halves still begin and end
    in M at the pair's corners."""
    seqs, pairs = RC.indel_breakpoints()
    cells, searches, _, _ = run_three(engines, oracle, seqs, pairs, RC.DEFAULT_2P, key="rr-indel")
    assert cells > 0 and searches > 0


def two_to_one_blocks():
    """6 kbp against a 4 % copy of it with every second block of 1,000 bases left out: a 2:1 pair whose halves and quarters are
    2:1 as well, with searches on both outer chains below level 1 that run passes."""
    rng = random.Random("row-reuse-levels/2to1/1000/6000/0.04")
    s = rand_seq(rng, 6000)
    m = mutate(s, 0.04, rng)
    return [s, b"".join(bytes(m[i:i + 1000]) for i in range(0, len(m), 2000))], [(0, 1)]


def test_two_to_one_takers_below_level_1_stop_early(engines, oracle):
    """Both halves take the archive to its end (it holds 9,000 / 28 scores, far fewer than their far-apart zones).  The searches
    below them on the two chains take rows too, but stop well before the archive ends: per search they must take strictly
    less than a half does.  (The counters do not say whether the box test or the taker's own margin ended it; on 2:1 inputs
    the CPU row check of DESIGN.md 4.28 finds the box-passing prefix at 80-93 % of a taker's direction below level 1.)"""
    cells, searches, st, _ = run_three(engines, oracle, *two_to_one_blocks(), RC.DEFAULT_2P, key="rrl-2to1-blocks")
    assert st.prof[13] == 2 and st.prof[12] > 0
    assert searches >= 2 and 0 < cells * st.prof[13] < st.prof[12] * searches


def test_two_to_one_unrelated_is_refused_below_level_1(engines, oracle):
    """3 kbp against an unrelated 1.5 kbp (the refusal case): one half takes the few passes inside its box, and the top-level
    rows leave every smaller box on its chain inside the first pass: below level 1 nothing is taken."""
    cells, searches, st, _ = run_three(engines, oracle, *RC.two_to_one(), RC.DEFAULT_2P, key="rr-2to1")
    assert st.prof[13] == 1 and st.prof[12] > 0 and cells == 0 and searches == 0


def test_unrelated_sequences_are_refused(engines, oracle):
    """The top-level rows leave a half's box inside the first pass, and a quarter's box all the more."""
    cells, searches, st, _ = run_three(engines, oracle, *RC.unrelated(), RC.DEFAULT_2P, key="rr-unrelated")
    assert cells == 0 and searches == 0 and st.prof[12] == 0


def restart_pair():
    """7 kbp, 5 % apart (seed 38 of a scan of such pairs): seven searches below the top level run passes, four of them on the
    outer chains below level 1, and one search of the pair is restarted."""
    rng = random.Random("row-reuse-levels/restart/7000/38")
    s = rand_seq(rng, 7000)
    return [mutate(s, 0.025, rng), mutate(s, 0.025, rng)], [(0, 1)]


def test_restarted_search(engines, oracle):
    """A search whose furthest points met inside a far-apart pass runs again with a wider margin and asks the archive again.
    run_three asks for the same number of restarts with and without takers below level 1; here takers below level 1 took rows
    in a pair with a restart.  Which search restarted the counters do not say: a scan of 2,000 such pairs found none whose
    tree is small enough to tell (tests/row_reuse_cases.py's restart case restarts at the top and has no search below level 1
    that runs passes)."""
    cells, searches, st, _ = run_three(engines, oracle, *restart_pair(), RC.DEFAULT_2P, key="rrl-restart-38")
    assert st.restarts > 0 and cells > 0 and searches >= 2
    _, _, st0, _ = run_three(engines, oracle, *RC.restart_case(), RC.DEFAULT_2P, key="rr-restart")
    assert st0.restarts > 0


def test_single_piece_and_edit_penalties(engines, oracle):
    cells, searches, _, _ = run_three(engines, oracle, *RC.twin_unit(), RC.AFFINE, key="rr-affine")
    assert cells > 0 and searches >= 2
    cells, searches, _, _ = run_three(engines, oracle, *RC.twin_unit(), RC.EDIT, key="rr-edit")
    assert cells == 0 and searches == 0  # no multi-step passes under these scores: nothing is archived


def test_two_workgroups_take_many_units_in_turn(engines, oracle):
    """Every unit's searches run with the previous unit's archive behind them until its own top-level search has voided it; some
    of the 45 units split four ways (two breakpoints that are no mirror images), and their B-frame tasks take nothing."""
    seqs, pairs = RC.many_units()
    cells, searches, st, e = run_three(engines, oracle, seqs, pairs, RC.DEFAULT_2P, key="rr-many", workgroups=2)
    ts = e.twin_stats()
    print("units %d shared %d per-orientation %d non-mirror %d" % ts)
    assert cells > 0 and searches > 0 and ts[0] == 45 and ts[3] > 0


def test_capacity_rerun(engines, oracle):
    """Rows capped at 2048 columns: what outgrows them is re-run wider, with reuse on in both launches."""
    cells, searches, st, _ = run_three(engines, oracle, *RC.twin_unit(0.20), RC.DEFAULT_2P, key="rr-twin-0.2", first_row_cols=2048)
    assert st.launches > 1, "no CAPACITY re-run"
    assert cells > 0
