"""GPU tests (-m gpu) on the exhaustive lists of tests/exhaustive_cases.py: every ordered pair of the short cores of two
families, bare (a top-level base case) and between flanks that put exactly one top-level breakpoint search into the core.
tests/test_exhaustive_cpu.py shows from the oracle alone that the lists are traps: where the kernels place a breakpoint, or
break a tie at it, differently from the oracle, thousands of pairs come back with other bytes.

No list is sampled: every pair of every list is compared with the CPU oracle -- status, penalty, score, op bytes, the four
counts and both ends -- through align_pairs under every penalty set, under every kernel flavour, as twin units, score-only
and bounded, verified and normalized on the device, and as ranges of one long resident sequence on both strands.  The
oracle's answers are computed once per (family, layout, scores) and shared; comparisons are made on whole arrays."""
import numpy as np
import pytest

import exhaustive_cases as X
import penalty_space as PS
from test_gpu_penalties import FLAVOURS
from util import DEFAULT_2P, EDIT, PENALTY_SETS

pytestmark = pytest.mark.gpu

FAMS = list(X.FAMILIES)
NO_UNITS = (0, 0, 0, 0)


def ids(sets):
    return [",".join(map(str, s)) for s in sets]


def run(e, oracle, fam, name, scores, where=(), twin=False, **kw):
    """The list through align_pairs on `e`, every entry against the oracle; returns the call's output."""
    seqs, pairs = X.twin_lists(fam, name) if twin else X.lists(fam, name)
    want = X.oracle_results(oracle, fam, name, scores, twin=twin)
    e.set_sequences(seqs)
    got = e.align_pairs(scores, pairs, **kw)
    X.check(got[:2], want, fam, name, seqs, pairs, where)
    return got, want, seqs, pairs


# ---- 1. parity

@pytest.mark.parametrize("name", X.LAYOUTS)
@pytest.mark.parametrize("scores", PENALTY_SETS, ids=ids(PENALTY_SETS))
def test_parity(engine, oracle, scores, name):
    """Every (family, layout) list under every penalty set, the engine's own routing and one wave per pair."""
    for fam in FAMS:
        got, want, seqs, pairs = run(engine, oracle, fam, name, scores)
        st = engine.stats()
        assert st.pairs_completed == len(pairs), (fam, name)
        if name == "bare":
            assert st.n_breakpoints == 0, (fam, st.n_breakpoints)
        else:  # one search per pair whose sequences differ, at least (a twin unit counts its shared search once)
            assert st.n_breakpoints > 0, (fam, name)


# ---- 2. the flavour matrix

@pytest.mark.parametrize("flavour", FLAVOURS, ids=[f for f, _ in FLAVOURS])
def test_flavour_matrix(hip_lib, oracle, flavour):
    """AC6 in three layouts under every kernel flavour (one engine per flavour): equal to the oracle; and the long layout, at
    flanks of 600 bases, ran multi-step passes in every flavour and under every set that has them."""
    from allwave_amd import ffi
    flags = 0
    for f in flavour[1]:
        flags |= getattr(ffi, "AWV_F_" + f)
    e = ffi.Engine(flags=flags)
    try:
        for scores in (DEFAULT_2P, (0, 7, 0, 3)):
            for name in ("balanced", "repeat_flanks", "long_k12_12"):
                run(e, oracle, "AC6", name, scores, where=flavour[0])
                if name == "long_k12_12":
                    # (0, 7, 0, 3) has no multi-step pass at any length: its derived depth is 0 (tests/penalty_space.py)
                    d = PS.derive(scores)
                    depth = 0 if "SINGLE_STEP" in flavour[1] else d.multi_T32 if "FORCE_INT32" in flavour[1] else d.multi_T
                    assert (e.stats().multi_cell_steps > 0) == (depth > 0), (flavour[0], scores, e.stats().multi_cell_steps, depth)
    finally:
        e.close()


# ---- 3. twin units

TWIN_FLAGS = ((), ("NO_TWIN",), ("TWIN_TOP_ONLY",), ("NO_TWIN_BASE",))


@pytest.mark.parametrize("scores", [DEFAULT_2P, (0, 4, 6, 2)], ids=ids([DEFAULT_2P, (0, 4, 6, 2)]))
@pytest.mark.parametrize("extra", TWIN_FLAGS, ids=["-".join(f) or "default" for f in TWIN_FLAGS])
def test_twin_units(hip_lib, oracle, extra, scores):
    """The exhaustive form of test_gpu_twin_base.py::test_tie_rich_pairs_whose_swap_is_not_the_mirror: lists that hold every
    entry's swap, on the one-wave engine with and without the twin switches.  Every entry is the oracle's answer for its
    own orientation; units formed unless AWV_F_NO_TWIN forbids them."""
    from allwave_amd import ffi
    flags = ffi.AWV_F_ONE_WAVE
    for f in extra:
        flags |= getattr(ffi, "AWV_F_" + f)
    e = ffi.Engine(flags=flags)
    try:
        for fam, name in (("AC6", "balanced"), ("ACG4", "balanced"), ("AC6", "repeat_flanks"), ("ACG4", "repeat_flanks"),
                          ("AC6", "long_k12_11"), ("ACG4", "long_k12_11")):
            got, want, seqs, pairs = run(e, oracle, fam, name, scores, where=extra, twin=True)
            ts = e.twin_stats()
            n = len(X.family(fam))
            print("%s %s %s %s: twin stats %s" % (extra, scores, fam, name, ts))
            if "NO_TWIN" in extra:
                assert ts == NO_UNITS, (extra, fam, name, ts)
            else:  # at most one unit per unordered pair of different sequences
                assert 0 < ts[0] <= (n * n if name in X.LONG else n * (n - 1) // 2), (extra, fam, name, ts)
    finally:
        e.close()


# ---- 4. score-only and bounds

@pytest.mark.parametrize("name", ["balanced", "long_k12_12"])
@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT], ids=ids([DEFAULT_2P, EDIT]))
def test_score_only_and_bounds(engine, oracle, scores, name):
    from allwave_amd import ffi
    fam = "AC6"
    seqs, pairs = X.lists(fam, name)
    want = X.oracle_results(oracle, fam, name, scores)
    engine.set_sequences(seqs)
    sc = engine.score_pairs(scores, pairs)
    assert (sc["status"] == 0).all() and (sc["penalty"] == want.pen).all(), np.flatnonzero(sc["penalty"] != want.pen)[:5]
    # one below the penalty: proved above the bound; at the penalty: completed
    pos = want.pen > 0
    assert pos.sum() >= len(pairs) - len(X.family(fam))
    below = np.where(pos, want.pen - 1, -1).astype(np.int32)
    sc = engine.score_pairs(scores, pairs, max_penalty=below)
    assert (sc["status"][pos] == ffi.AWV_ST_ABOVE_BOUND).all() and (sc["penalty"][pos] == want.pen[pos]).all()
    assert (sc["status"][~pos] == 0).all() and (sc["penalty"][~pos] == 0).all()
    res, cigs = engine.align_pairs(scores, pairs, max_penalty=below)
    assert (res["status"][pos] == ffi.AWV_ST_ABOVE_BOUND).all() and (res["penalty"][pos] == want.pen[pos]).all()
    assert all(c is None for c, p in zip(cigs, pos) if p) and (res["cigar_len"][pos] == 0).all()
    sc = engine.score_pairs(scores, pairs, max_penalty=want.pen)
    assert (sc["status"] == 0).all() and (sc["penalty"] == want.pen).all()
    X.check(engine.align_pairs(scores, pairs, max_penalty=want.pen), want, fam, name, seqs, pairs, "max_penalty = the penalty")


# ---- 5. verify and normalize on the same outputs

@pytest.mark.parametrize("name", ["balanced", "repeat_flanks"])
@pytest.mark.parametrize("fam", FAMS)
def test_verify_and_normalize(engine, oracle, fam, name):
    """The device's check accepts every alignment, and the device's left- and right-normal forms are the host yardstick's
    applied to the oracle's bytes, with the records unchanged."""
    from allwave_amd import ffi
    scores = DEFAULT_2P
    got, want, seqs, pairs = run(engine, oracle, fam, name, scores, verify=True)
    res0 = got[0]
    assert (got[2]["code"] == ffi.AWV_VF_OK).all(), np.flatnonzero(got[2]["code"] != ffi.AWV_VF_OK)[:5]
    assert engine.verify_stats().pairs == len(pairs) and engine.verify_stats().failed == 0
    plist = pairs.tolist()
    left = None
    for direction in ("left", "right"):
        host = [ffi.normalize_one_host(direction, seqs[q], seqs[t], ops) for (q, t), ops in zip(plist, want.ops)]
        assert all(int(r["code"]) == ffi.AWV_NM_OK for _, r in host)
        norm = [h[0] for h in host]
        moved = sum(1 for a, b in zip(norm, want.ops) if a != b)
        res, cigs = engine.align_pairs(scores, pairs, normalize=direction)
        st = engine.normalize_stats()
        print("%s %s %s: %d of %d op strings moved, %d runs" % (fam, name, direction, moved, len(pairs), st.runs_moved))
        assert res.tobytes() == res0.tobytes(), (fam, name, direction)
        if cigs != norm:
            i = next(i for i in range(len(pairs)) if cigs[i] != norm[i])
            q, t = plist[i]
            assert False, (fam, name, direction, X.core_of(fam, q), X.core_of(fam, t), X.rle(cigs[i]), X.rle(norm[i]), X.rle(want.ops[i]))
        assert st.pairs == len(pairs) and st.runs_moved == sum(int(r["runs_moved"]) for _, r in host)
        if direction == "left":
            assert moved > 0 and st.runs_moved > 0
            left = norm
    # The oracle's backtrace leaves every gap run of these lists right-normal already (the yardstick moves none of them), so
    # the device's right-normal form is also taken of the left-normal strings: it moves runs, and it is the yardstick's.
    recs = res0.copy()
    recs["cigar_off"] = np.concatenate(([0], np.cumsum(recs["cigar_len"], dtype=np.uint64)[:-1]))
    out, nres = engine.normalize_cigars("right", pairs, recs, b"".join(left))
    host = [ffi.normalize_one_host("right", seqs[q], seqs[t], ops) for (q, t), ops in zip(plist, left)]
    assert out.tobytes() == b"".join(h[0] for h in host), (fam, name)
    assert [int(v) for v in nres["runs_moved"]] == [int(r["runs_moved"]) for _, r in host] and engine.normalize_stats().runs_moved > 0


# ---- 6. ranges

@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT], ids=ids([DEFAULT_2P, EDIT]))
def test_ranges_of_one_book(engine, oracle, scores):
    """The balanced AC6 list as intervals of one resident sequence per side, forward and through the reverse complement of
    the query book: the interval starts fall on every word phase, and a neighbour's identical flank lies beyond both ends of
    every interval, so a probe that ran past an end would go on matching."""
    fam, name = "AC6", "balanced"
    seqs, pairs = X.lists(fam, name)
    want = X.oracle_results(oracle, fam, name, scores)
    books, fwd, rev = X.book_ranges(fam, name)
    engine.set_sequences(books)
    for strand, ranges in (("forward", fwd), ("reversed", rev)):
        got = engine.align_ranges(scores, ranges)
        X.check(got, want, fam, name, seqs, pairs, strand)
        sc = engine.score_ranges(scores, ranges)
        assert (sc["status"] == 0).all() and (sc["penalty"] == want.pen).all(), strand
