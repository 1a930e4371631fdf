"""GPU tests (-m gpu) of row reuse: in the one-wave kernels with 16-bit rows a pair's top-level breakpoint
search archives the rows of its far-apart passes, and the forward search of its left half and the reverse search of its
right half take them from the archive instead of computing them.  Every case compares every result field and every CIGAR
byte three ways -- the default path, AWV_F_NO_ROW_REUSE (every search computes all of its rows: the path as it was) and
the CPU oracle -- asks that the algorithm's counters (cell-steps, cells of multi-step passes, restarted searches, searches,
base cases) are the same numbers under both settings, and asserts whether rows were taken (awv_stats.prof[12] cell-steps,
prof[13] searches; tests/row_reuse_cases.py says why for each input)."""
import pytest

import row_reuse_cases as RC
from twin_cases import check_records, oracle_records, same_records

pytestmark = pytest.mark.gpu


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


def run_both(engines, oracle, seqs, pairs, scores, base_flags=None, key=None, **kw):
    """Aligns the list with and without row reuse; both against the oracle and against each other.  Returns
    (cell-steps taken from archives, searches that took some, stats with reuse, stats without)."""
    from allwave_amd import ffi
    base = ffi.AWV_F_ONE_WAVE if base_flags is None else base_flags
    want = oracle_records(oracle, seqs, pairs, scores, key=key)
    out = []
    for flags in (base, base | ffi.AWV_F_NO_ROW_REUSE):
        e = engines(flags, **kw)
        e.set_sequences(seqs)
        got = e.align_pairs(scores, pairs)
        st = e.stats()
        out.append((got, st))
        if not any(len(p) > 2 and p[2] for p in pairs):
            check_records(got, want, seqs, pairs)
        else:
            assert [(int(got[0]["penalty"][i]), got[1][i]) for i in range(len(pairs))] == [(p, o) for p, o in want]
    (on, st_on), (off, st_off) = out
    same_records(on, off)
    for name in ("cell_steps", "multi_cell_steps", "deep_cell_steps", "restarts", "n_breakpoints", "n_base", "pairs_completed"):
        assert getattr(st_on, name) == getattr(st_off, name), (name, getattr(st_on, name), getattr(st_off, name))
    assert st_off.prof[12] == 0 and st_off.prof[13] == 0
    print("reused %d of %d cell-steps in %d of %d searches; restarts %d" %
          (st_on.prof[12], st_on.cell_steps, st_on.prof[13], st_on.n_breakpoints, st_on.restarts))
    return int(st_on.prof[12]), int(st_on.prof[13]), st_on, st_off


@pytest.mark.parametrize("d", [0.05, 0.10, 0.20])
def test_twin_unit_and_the_same_pair_alone(engines, oracle, d):
    """A pair in both orders is one unit whose shared top-level search feeds A's and the shared children; listed once it runs
    the plain tree.  Either way both level-1 searches take rows."""
    cells, searches, st, _ = run_both(engines, oracle, *RC.twin_unit(d), RC.DEFAULT_2P, key="rr-twin-%g" % d)
    assert cells > 0 and searches == 2
    cells1, searches1, st1, _ = run_both(engines, oracle, *RC.alone(d), RC.DEFAULT_2P, key="rr-alone-%g" % d)
    assert cells1 > 0 and searches1 == 2
    assert st.pairs_completed == 2 and st1.pairs_completed == 1


def test_divergences_in_one_list(engines, oracle):
    cells, searches, _, _ = run_both(engines, oracle, *RC.divergences(), RC.DEFAULT_2P, key="rr-div")
    assert cells > 0 and searches == 6


def test_two_to_one_takes_only_the_rows_inside_the_box(engines, oracle):
    """Partial: the pair has one level-1 search that runs in the archived frame with passes (the other half is a gap).  It takes
    the passes that lie inside its box and computes the rest: the archive holds 10 passes of 15 scores (4,500 bases / 28), whose
    2 x 150 rows are at most 2 s + 1 cells wide -- taking all of them would be about 22,500 cell-steps per direction, and the box
    test lets through fewer."""
    cells, searches, st, _ = run_both(engines, oracle, *RC.two_to_one(), RC.DEFAULT_2P, key="rr-2to1")
    assert searches == 1 and 0 < cells < sum(2 * s + 1 for s in range(1, 151))


def test_terminal_gap(engines, oracle):
    cells, searches, _, _ = run_both(engines, oracle, *RC.terminal_gap(), RC.DEFAULT_2P, key="rr-gap")
    assert cells > 0 and searches == 2


def test_unrelated_sequences_are_refused(engines, oracle):
    """The parent's rows leave the child's box inside the first pass: nothing is taken."""
    cells, searches, _, _ = run_both(engines, oracle, *RC.unrelated(), RC.DEFAULT_2P, key="rr-unrelated")
    assert cells == 0 and searches == 0


def test_breakpoints_in_indel_components(engines, oracle):
    seqs, pairs = RC.indel_breakpoints()
    comps = RC.top_breakpoint_components(oracle, seqs, pairs, RC.DEFAULT_2P)
    assert comps == [c for _, _, c in RC.INDEL_CASES] and all(c != 0 for c in comps)
    cells, searches, _, _ = run_both(engines, oracle, seqs, pairs, RC.DEFAULT_2P, key="rr-indel")
    assert cells > 0 and searches == 2 * len(pairs)


def test_restarted_search_restarts_alike(engines, oracle):
    """run_both compares awv_stats.restarts of the two settings; the input must restart at all."""
    _, _, st_on, st_off = run_both(engines, oracle, *RC.restart_case(), RC.DEFAULT_2P, key="rr-restart")
    assert st_on.restarts == st_off.restarts and st_off.restarts > 0


def test_single_piece_and_edit_penalties(engines, oracle):
    cells, searches, _, _ = run_both(engines, oracle, *RC.twin_unit(), RC.AFFINE, key="rr-affine")
    assert cells > 0 and searches == 2
    cells, searches, _, _ = run_both(engines, oracle, *RC.twin_unit(), RC.EDIT, key="rr-edit")
    assert cells == 0 and searches == 0  # no multi-step passes under these scores: nothing is archived


def test_two_workgroups_take_many_units_in_turn(engines, oracle):
    """Every unit's top-level search starts with the previous unit's archive behind it."""
    seqs, pairs = RC.many_units()
    cells, searches, st, _ = run_both(engines, oracle, seqs, pairs, RC.DEFAULT_2P, key="rr-many", workgroups=2)
    assert cells > 0 and searches >= len(pairs) // 2


def test_capacity_rerun(engines, oracle):
    """Rows capped at 2048 columns: what outgrows them is re-run wider, with reuse on in both launches."""
    cells, searches, st, st_off = run_both(engines, oracle, *RC.twin_unit(0.20), RC.DEFAULT_2P, key="rr-twin-0.2", first_row_cols=2048)
    assert st.launches == st_off.launches and st.launches > 1, "no CAPACITY re-run"
    assert cells > 0


def test_reverse_complemented_entry(engines, oracle):
    cells, searches, _, _ = run_both(engines, oracle, *RC.revcomp_entry(), RC.DEFAULT_2P)
    assert cells > 0 and searches == 2


@pytest.mark.parametrize("flavour", ["four_waves", "int32"])
def test_other_kernels_keep_no_archive(engines, oracle, flavour):
    from allwave_amd import ffi
    base = ffi.AWV_F_FOUR_WAVES if flavour == "four_waves" else ffi.AWV_F_ONE_WAVE | ffi.AWV_F_FORCE_INT32
    cells, searches, _, _ = run_both(engines, oracle, *RC.twin_unit(), RC.DEFAULT_2P, base_flags=base, key="rr-twin-0.1")
    assert cells == 0 and searches == 0
