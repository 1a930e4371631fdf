"""GPU tests (-m gpu) across the penalty space of tests/penalty_space.py.

The kernels are compiled once and every penalty-dependent choice -- the ring depth, the steps per multi-step pass, the
chained sweeps, the base-case history bound -- is made at run time from (x, o1, e1, o2, e2).  These tests run every
accepted set of the list against the oracle, a representative of every derived class under every kernel flavour, check
the engine's own counters and its accept / reject decisions against the Python restatement, check that scaling a set
scales every penalty (a check that does not rely on the oracle), and check the guard that keeps a workgroup's ring arena
below 2 GiB.
"""
import random
import time

import pytest

import penalty_space as PS
import repeats as R
from long_pairs import row_width_pairs
from util import check_against_oracle, mutate, rand_seq, random_pair

pytestmark = pytest.mark.gpu

AWV_ERR_PENALTIES = -4
AWV_ST_CAPACITY = 1
LARGE_SB = 1100                 # sets above this get an engine with capped scratch (base-case history arenas of ~100 MB+ per slot)
SCRATCH_CAP = 6 << 30


def _engine(flags=0, capped=True):
    from allwave_amd import ffi
    return ffi.Engine(flags=flags, max_scratch_bytes=SCRATCH_CAP if capped else 0)


def _pairs(ab):
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    return seqs, pairs


_ORACLE = {}


def _oracle_results(oracle, key, scores, seqs, pairs):
    """(penalty, ops) of every pair, computed once per (set, input) and reused by every engine that runs it."""
    k = (key, tuple(scores))
    if k not in _ORACLE:
        al = oracle.Aligner(scores)
        _ORACLE[k] = [al.align(seqs[a], seqs[b]) for a, b in pairs]
    return _ORACLE[k]


def check_cached(engine, oracle, key, seqs, pairs, scores):
    """check_against_oracle with the oracle's answers cached: bytes, penalty, op counts and ends equal the oracle's."""
    want = _oracle_results(oracle, key, scores, seqs, pairs)
    engine.set_sequences(seqs)
    res, cigs = engine.align_pairs(scores, pairs)
    for i, (a, b) in enumerate(pairs):
        pen, ops = want[i]
        assert res["status"][i] == 0, (key, scores, i, int(res["status"][i]))
        assert res["penalty"][i] == pen and res["score"][i] == -pen, (key, scores, i, len(seqs[a]), len(seqs[b]), int(res["penalty"][i]), pen)
        assert cigs[i] == ops, (key, scores, i, len(seqs[a]), len(seqs[b]))
        c = {k: ops.count(k.encode()) for k in "MXID"}
        assert (res["num_matches"][i], res["num_mismatches"][i], res["num_ins"][i], res["num_del"][i]) == \
               (c["M"], c["X"], c["I"], c["D"]), (key, scores, i)
        assert res["q_end"][i] == len(seqs[a]) and res["t_end"][i] == len(seqs[b]), (key, scores, i)
    return res, cigs


def parity_inputs(name):
    """24 random_pair pairs up to 2.5 kbp and three repeat-family pairs, seeded by the set's name."""
    rng = random.Random("gpu-penalties/" + name)
    ab = [random_pair(rng, 2500) for _ in range(24)]
    ab += [R.microsatellite(rng), R.tandem(rng, total=(1500, 3000)), R.low_complexity(rng, n=(200, 1500))]
    return _pairs(ab)


@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_parity_at_every_accepted_set(engine, oracle, request, name):
    """Every accepted set, the engine's own choice of flavour and one wave per pair: equal to the oracle byte for byte."""
    scores = PS.BY_NAME[name]
    seqs, pairs = parity_inputs(name)
    if PS.derive(scores).sb <= LARGE_SB:
        check_cached(engine, oracle, ("parity", name), seqs, pairs, scores)
        return
    from allwave_amd import ffi
    mode = request.node.callspec.params["engine"]
    e = _engine(ffi.AWV_F_ONE_WAVE if mode == "one_wave" else 0)
    try:
        check_cached(e, oracle, ("parity", name), seqs, pairs, scores)
    finally:
        e.close()


FLAVOUR_SETS = PS.FLAVOUR_SETS


def flavour_inputs(name):
    rng = random.Random("gpu-penalties/flavours/" + name)
    ab = [random_pair(rng, 1500) for _ in range(8)] + [R.microsatellite(rng), R.end_runs(rng, body=(100, 800))]
    return _pairs(ab)


# kernel flavours: name -> the AWV_F_* flags of the engine
FLAVOURS = (("four_waves", ("FOUR_WAVES",)), ("single_step", ("ONE_WAVE", "SINGLE_STEP")),
            ("four_single_step", ("FOUR_WAVES", "SINGLE_STEP")), ("no_chain", ("ONE_WAVE", "NO_CHAIN")),
            ("no_deep", ("ONE_WAVE", "NO_DEEP")), ("four_no_deep", ("FOUR_WAVES", "NO_DEEP")),
            ("force_int32", ("ONE_WAVE", "FORCE_INT32")), ("four_force_int32", ("FOUR_WAVES", "FORCE_INT32")),
            ("no_packed_seq", ("ONE_WAVE", "NO_PACKED_SEQ")), ("four_no_packed_seq", ("FOUR_WAVES", "NO_PACKED_SEQ")))


@pytest.mark.parametrize("flavour", FLAVOURS, ids=[f for f, _ in FLAVOURS])
def test_flavour_matrix(oracle, flavour):
    """Each representative set under one kernel flavour (one engine per flavour, every set through it): equal to the oracle."""
    from allwave_amd import ffi
    flags = 0
    for f in flavour[1]:
        flags |= getattr(ffi, "AWV_F_" + f)
    e = _engine(flags)
    try:
        for name in FLAVOUR_SETS:
            seqs, pairs = flavour_inputs(name)
            check_cached(e, oracle, ("flavours", name), seqs, pairs, PS.BY_NAME[name])
    finally:
        e.close()


@pytest.mark.parametrize("name", FLAVOUR_SETS)
def test_long_pairs_on_every_row_width(oracle, name):
    """32-bit rows, wide16 rows and the sixteen-wave flavour at each representative set (the engine's own routing), and the
    32-bit pair under one wave per pair: equal to the oracle."""
    from allwave_amd import ffi
    scores = PS.BY_NAME[name]
    seqs, pairs = row_width_pairs()
    e = _engine(0)
    try:
        check_cached(e, oracle, "long", seqs, pairs, scores)
    finally:
        e.close()
    e = _engine(ffi.AWV_F_ONE_WAVE)
    try:
        check_cached(e, oracle, "long32", seqs[:2], pairs[:2], scores)
    finally:
        e.close()


def stats_inputs(name):
    """3-4 kbp pairs, 3-8 % apart: long enough for multi-step passes wherever they are instantiated."""
    rng = random.Random("gpu-penalties/stats/" + name)
    ab = []
    for _ in range(4):
        s = rand_seq(rng, rng.randint(3000, 4000))
        ab.append((s, mutate(s, rng.uniform(0.03, 0.08), rng)))
    return _pairs(ab)


def test_stats_match_the_restatement(oracle):
    """On 3-4 kbp pairs under one wave per pair, the kernels ran multi-step passes exactly when the restatement derives
    multi_T > 0 (16-bit rows) and multi_T32 > 0 (AWV_F_FORCE_INT32); AWV_F_NO_DEEP leaves no deep-zone cells,
    AWV_F_SINGLE_STEP no pass at all.  Every result equals the oracle."""
    from allwave_amd import ffi as F
    engines = {k: _engine(f) for k, f in (("w16", F.AWV_F_ONE_WAVE), ("w32", F.AWV_F_ONE_WAVE | F.AWV_F_FORCE_INT32),
                                          ("no_deep", F.AWV_F_ONE_WAVE | F.AWV_F_NO_DEEP),
                                          ("single", F.AWV_F_ONE_WAVE | F.AWV_F_SINGLE_STEP))}
    try:
        for name, scores in PS.ACCEPTED:
            d = PS.derive(scores)
            seqs, pairs = stats_inputs(name)
            for k, e in engines.items():
                check_cached(e, oracle, ("stats", name), seqs, pairs, scores)
                st = e.stats()
                assert st.cell_steps > 0, (name, k)
                if k == "w16" or k == "no_deep":
                    assert (st.multi_cell_steps > 0) == (d.multi_T > 0), (name, k, st.multi_cell_steps, d.multi_T)
                if k == "w32":
                    assert (st.multi_cell_steps > 0) == (d.multi_T32 > 0), (name, k, st.multi_cell_steps, d.multi_T32)
                if k == "no_deep":
                    assert st.deep_cell_steps == 0, (name, st.deep_cell_steps)
                if k == "single":
                    assert st.multi_cell_steps == 0 and st.deep_cell_steps == 0, (name, st.multi_cell_steps)
    finally:
        for e in engines.values():
            e.close()


def test_accept_and_reject_at_each_boundary():
    """Through the ABI: AWV_ERR_PENALTIES on exactly the sets the restatement rejects (scope 126 / 127, sb 4000 / 4001, x = 0,
    e = 0, e2 = 0, o < 0, o2 < 0, match != 0), a completed alignment on every other set.  The engine stays usable after
    a rejection."""
    from allwave_amd import ffi
    rng = random.Random("gpu-penalties/abi")
    s = rand_seq(rng, 300)
    seqs = [s, mutate(s, 0.05, rng)]
    e = _engine(0)
    try:
        e.set_sequences(seqs)
        for name, scores in PS.PENALTY_SPACE:
            if PS.derive(scores).accepted:
                res, cigs = e.align_pairs(scores, [(0, 1)])
                assert res["status"][0] == 0 and cigs[0] is not None, name
            else:
                with pytest.raises(ffi.EngineError) as ex:
                    e.align_pairs(scores, [(0, 1)])
                assert ex.value.code == AWV_ERR_PENALTIES, (name, ex.value.code, str(ex.value))
    finally:
        e.close()


SCALINGS = (((0, 1, 0, 1), (2, 3, 7, 20)), ((0, 3, 4, 1), (2, 3)), ((0, 5, 8, 2, 4, 1), (2, 3)),
            ((0, 5, 4, 1, 12, 2), (2, 4)), ((0, 5, 8, 2, 24, 1), (2,)))


@pytest.mark.parametrize("base,factors", SCALINGS, ids=[str(b) for b, _ in SCALINGS])
def test_scaling_multiplies_every_penalty(oracle, base, factors):
    """Scores times k (still accepted): every GPU penalty is exactly k times the unscaled GPU penalty, and every CIGAR
    re-scores to its penalty under its own scores.  The CIGARs may differ -- the base-case thresholds are absolute scores --
    so only the penalties are compared; this does not rely on the oracle's alignments."""
    from allwave_amd import ffi
    rng = random.Random("gpu-penalties/scale/%s" % (base,))
    ab = [random_pair(rng, 2500) for _ in range(16)] + [R.microsatellite(rng), R.tandem(rng, total=(1500, 3000))]
    seqs, pairs = _pairs(ab)
    for flags in (0, ffi.AWV_F_ONE_WAVE):
        e = _engine(flags)
        try:
            e.set_sequences(seqs)
            ref, _ = e.align_pairs(base, pairs)
            assert (ref["status"] == 0).all()
            for k in factors:
                scores = PS.scaled(base, k)
                assert PS.derive(scores).accepted, scores
                res, cigs = e.align_pairs(scores, pairs)
                assert (res["status"] == 0).all(), scores
                for i, (a, b) in enumerate(pairs):
                    assert res["penalty"][i] == k * ref["penalty"][i], (scores, i, int(res["penalty"][i]), int(ref["penalty"][i]))
                    assert oracle.cigar_check(cigs[i], seqs[a], seqs[b], scores) == (0, res["penalty"][i]), (scores, i)
        finally:
            e.close()


def test_ring_arena_guard_returns_capacity(oracle):
    """(0,3,90,1) has a ring of 128 rows, so 32-bit rows hold at most 419,328 columns below 2 GiB.  A 40 kbp sequence
    against itself with a 450 kbp insertion cannot be searched in such rows: the pair comes back AWV_ST_CAPACITY at once,
    without a launch, and an ordinary pair on the same engine afterwards is still bit-exact."""
    scores = (0, 3, 90, 1)
    assert PS.derive(scores).ring == 128
    rng = random.Random("gpu-penalties/guard")
    a = rand_seq(rng, 40000)
    b = a[:20000] + rand_seq(rng, 450000) + a[20000:]
    e = _engine(0)
    try:
        e.set_sequences([a, b])
        t0 = time.time()
        res, cigs = e.align_pairs(scores, [(0, 1), (1, 0)])
        dt = time.time() - t0
        st = e.stats()
        assert (res["status"] == AWV_ST_CAPACITY).all(), res["status"]
        assert (res["penalty"] == 0).all() and (res["cigar_len"] == 0).all()
        assert cigs == [None, None]
        assert st.cell_steps == 0 and st.launches == 0, (st.cell_steps, st.launches)
        assert dt < 10, dt
        # the same engine, an ordinary pair
        s = rand_seq(rng, 2000)
        check_against_oracle(e, oracle, [s, mutate(s, 0.05, rng)], [(0, 1), (1, 0)], scores)
    finally:
        e.close()
