"""GPU tests of bounded full alignment (awv_align_pairs_bounded / awv_align_ranges_bounded and everything above them): the
contract of include/allwave_hip.h -- status and penalty are the bounded score-only call's, every completed pair's record and
op bytes are the unbounded call's byte for byte, an abandoned pair reports bound + 1 and nothing else -- on the cases of
bounded_cases.py, under every variant pin, through the CAPACITY re-runs, on ranges, with the on-device check, through the
host mirror and from the command line."""
import os
import random
import subprocess

import numpy as np
import pytest

import bounded_cases as BC
from util import DEFAULT_2P, mutate, rand_seq, rle
from verify_cases import revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case_set():
    return BC.cases()


_REFERENCE = {}


def pairs_of(request, case_set):
    """The case list on this engine flavour.  The 200 bp x 17 kbp pair is there for the sixteen-wave flavour, which the engine
    pinned to one wave per pair never takes: there it is left out (one wave would spend a second per call on it)."""
    seqs, pairs = case_set
    assert BC.CASE_NAMES[-1] == "sixteen_waves"
    return pairs[:-1] if request.node.callspec.params["engine"] == "one_wave" else pairs


def reference(engine, request, case_set, scores):
    """The unbounded align_pairs of the case list under `scores` on this engine flavour: computed once, shared, left unchanged."""
    key = (request.node.callspec.params["engine"], scores)
    seqs, pairs = case_set[0], pairs_of(request, case_set)
    engine.set_sequences(seqs)
    if key not in _REFERENCE:
        res, cigs = engine.align_pairs(scores, pairs)
        assert (res["status"] == 0).all(), (scores, res["status"])
        _REFERENCE[key] = (res.copy(), list(cigs))
    return _REFERENCE[key]


# ---- 1. the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", BC.SCORE_SETS)
def test_contract(engine, request, case_set, scores):
    """Every bound kind of {0, P - 1, P, P + 1, 2 P, none} on every case, per kind and mixed within one call, and as a scalar."""
    from allwave_amd import ffi
    seqs, pairs = case_set[0], pairs_of(request, case_set)
    ref_res, ref_cigs = reference(engine, request, case_set, scores)
    pens = ref_res["penalty"]
    # (the cases are what their names say: the 5 % and 12 % pairs cost more than the 250 below which a sub-problem is a base
    # case, so their halves are searched in turn -- the 1 % pair's 120 under the default scores sends both halves straight to
    # the base case --, and the identical pair costs nothing)
    if scores == DEFAULT_2P:
        for name in ("2k_5pct", "2k_12pct"):
            assert pens[BC.CASE_NAMES.index(name)] > 250, (name, pens)
    assert pens[BC.CASE_NAMES.index("identical")] == 0
    for name, bounds in BC.bound_arrays(pens).items():
        res, cigs = engine.align_pairs(scores, pairs, max_penalty=bounds)
        sc = engine.score_pairs(scores, pairs, max_penalty=bounds)
        BC.check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=(scores, name))
    scalar = int(sorted(pens)[len(pens) // 2])
    res, cigs = engine.align_pairs(scores, pairs, max_penalty=scalar)
    sc = engine.score_pairs(scores, pairs, max_penalty=scalar)
    BC.check_contract(ffi, [scalar] * len(pairs), res, cigs, sc, ref_res, ref_cigs, where=(scores, "scalar"))
    assert (res["status"] == ffi.AWV_ST_ABOVE_BOUND).any() and (res["status"] == 0).any()


@pytest.mark.parametrize("scores", BC.SCORE_SETS)
def test_bounded_alignments_are_the_oracles(engine, oracle, request, case_set, scores):
    """A subset against the CPU oracle: at B = P the bounded call's penalty and op bytes are the oracle's."""
    seqs, pairs = case_set
    ref_res, _ = reference(engine, request, case_set, scores)
    sub = BC.case_index("2k_1pct", "base_case_top", "forced_gap", "revcomp", "with_n")
    sp = [pairs[i] for i in sub]
    res, cigs = engine.align_pairs(scores, sp, max_penalty=np.array([ref_res["penalty"][i] for i in sub], dtype=np.int32))
    al = oracle.Aligner(scores)
    for k, (q, t, rc) in enumerate(sp):
        pen, ops = al.align(revcomp(seqs[q]) if rc else seqs[q], seqs[t])
        assert res["status"][k] == 0 and res["penalty"][k] == pen, (scores, k)
        assert cigs[k] == ops, (scores, k, rle(cigs[k])[:60], rle(ops)[:60])


# ---- 2. variant pins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["AWV_F_ONE_WAVE", "AWV_F_FOUR_WAVES", "AWV_F_FORCE_INT32", "AWV_F_SINGLE_STEP", "AWV_F_NO_CHAIN",
                                     "AWV_F_NO_PACKED_SEQ"])
def test_variant_pins(hip_lib, case_set, variant):
    from allwave_amd import ffi
    seqs, pairs = case_set
    sp = [pairs[i] for i in BC.case_index("2k_1pct", "2k_5pct", "2k_12pct", "forced_gap")]
    e = ffi.Engine(flags=getattr(ffi, variant) | ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences(seqs)
        for scores in BC.SCORE_SETS:
            ref_res, ref_cigs = e.align_pairs(scores, sp)
            for name, bounds in BC.bound_arrays(ref_res["penalty"]).items():
                if not name.startswith("mixed") and name not in ("p_minus_1", "p"):
                    continue
                res, cigs = e.align_pairs(scores, sp, max_penalty=bounds)
                sc = e.score_pairs(scores, sp, max_penalty=bounds)
                BC.check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=(variant, scores, name))
    finally:
        e.close()


# ---- 3. re-runs keep their bounds -----------------------------------------------------------------------------------------
def test_capacity_reruns_keep_their_bounds(hip_lib):
    """The pair shape of test_gpu_parity.py's re-run test (6 kbp pairs, first attempt capped at 2048 columns): the pairs that
    come back CAPACITY are re-run wider under the bounds they came with."""
    from allwave_amd import ffi
    rng = random.Random(4242)
    a = rand_seq(rng, 6000)
    seqs = [a, mutate(a, 0.08, rng), mutate(a, 0.01, rng), rand_seq(rng, 1500)]
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    e = ffi.Engine(first_row_cols=2048)
    try:
        e.set_sequences(seqs)
        ref_res, ref_cigs = e.align_pairs(DEFAULT_2P, pairs)
        assert e.stats().launches >= 2 and (ref_res["status"] == 0).all()
        for kind in ("p", "p_minus_1"):
            bounds = np.array([BC.bound_of(kind, int(p)) for p in ref_res["penalty"]], dtype=np.int32)
            res, cigs = e.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds)
            assert e.stats().launches >= 2  # (some pair outgrew the 2048-column rows under its bound too)
            sc = e.score_pairs(DEFAULT_2P, pairs, max_penalty=bounds)
            BC.check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=kind)
            assert (res["status"] == (0 if kind == "p" else ffi.AWV_ST_ABOVE_BOUND)).all()
    finally:
        e.close()


# ---- 4. no recursion for abandoned pairs ----------------------------------------------------------------------------------
def test_abandoned_pairs_do_no_more_work_than_score_only(engine, request, case_set):
    """A list of above-bound pairs longer than 100 bp only: the bounded alignment does exactly the work of the bounded
    score-only call -- the top-level search, stopped at the bound: the same cells, base cases and searches, no sub-problem."""
    from allwave_amd import ffi
    seqs, pairs = case_set
    ref_res, _ = reference(engine, request, case_set, DEFAULT_2P)
    sub = BC.case_index("2k_1pct", "2k_5pct", "2k_12pct", "forced_gap", "unrelated_1k", "revcomp", "with_n")
    sp = [pairs[i] for i in sub]
    for frac in (0.0, 0.5, 1.0):
        bounds = np.array([max(int(ref_res["penalty"][i] * frac) - 1, 0) for i in sub], dtype=np.int32)
        res, cigs = engine.align_pairs(DEFAULT_2P, sp, max_penalty=bounds)
        st_a = engine.stats()
        a = (st_a.cell_steps, st_a.n_base, st_a.n_breakpoints, st_a.pairs_completed)
        sc = engine.score_pairs(DEFAULT_2P, sp, max_penalty=bounds)
        st_s = engine.stats()
        assert (res["status"] == ffi.AWV_ST_ABOVE_BOUND).all() and (sc["status"] == ffi.AWV_ST_ABOVE_BOUND).all()
        assert a == (st_s.cell_steps, st_s.n_base, st_s.n_breakpoints, st_s.pairs_completed), (frac, a)
        assert a[3] == 0, (frac, a)


# ---- 5. ranges ------------------------------------------------------------------------------------------------------------
def test_ranges(engine, case_set):
    """Interior rectangles of the 2 kbp pairs on both strands, a base-case rectangle and empty-side ranges: the same contract
    against score_ranges and the unbounded align_ranges."""
    from allwave_amd import ffi
    seqs, pairs = case_set
    engine.set_sequences(seqs)
    rng = random.Random("bounded/ranges")
    ranges = []
    for i in BC.case_index("2k_1pct", "2k_5pct", "2k_12pct"):
        q, t, _ = pairs[i]
        for rc in (0, 1):
            qb, tb = rng.randrange(1, 400), rng.randrange(1, 400)
            ranges.append((q, t, rc, qb, qb + rng.randrange(700, 1500), tb, tb + rng.randrange(700, 1500)))
    q, t, _ = pairs[BC.CASE_NAMES.index("2k_5pct")]
    ranges += [(q, t, 0, 300, 390, 300, 395), (q, t, 0, 500, 500, 100, 160), (q, t, 1, 40, 90, 700, 700), (q, t, 0, 7, 7, 9, 9)]
    for scores in BC.SCORE_SETS:
        ref_res, ref_cigs = engine.align_ranges(scores, ranges)
        assert (ref_res["status"] == 0).all()
        assert engine.align_ranges(scores, ranges, max_penalty=None)[0].tobytes() == ref_res.tobytes()
        for name, bounds in BC.bound_arrays(ref_res["penalty"]).items():
            res, cigs = engine.align_ranges(scores, ranges, max_penalty=bounds)
            sc = engine.score_ranges(scores, ranges, max_penalty=bounds)
            BC.check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=("ranges", scores, name))


# ---- 6. verify ------------------------------------------------------------------------------------------------------------
def test_verify_with_bounds(engine, request, case_set):
    from allwave_amd import ffi
    seqs, pairs = case_set[0], pairs_of(request, case_set)
    ref_res, ref_cigs = reference(engine, request, case_set, DEFAULT_2P)
    for name in ("mixed0", "mixed3", "p_minus_1"):
        bounds = BC.bound_arrays(ref_res["penalty"])[name]
        res, cigs, vres = engine.align_pairs(DEFAULT_2P, pairs, verify=True, max_penalty=bounds)
        sc = engine.score_pairs(DEFAULT_2P, pairs, max_penalty=bounds)
        BC.check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=("verify", name))
        done = res["status"] == 0
        assert (vres["code"][done] == ffi.AWV_VF_OK).all() and (vres["code"][~done] == ffi.AWV_VF_SKIPPED).all(), (name, vres["code"])
        vs = engine.verify_stats()
        assert vs.failed == 0 and vs.pairs == len(pairs)
    ranges = [(q, t, rc, 0, len(seqs[q]), 0, len(seqs[t])) for q, t, rc in pairs[:4]]
    bounds = np.array([BC.bound_of(k, int(p)) for k, p in zip(("p", "p_minus_1", "none", "zero"), ref_res["penalty"][:4])], dtype=np.int32)
    res, cigs, vres = engine.align_ranges(DEFAULT_2P, ranges, verify=True, max_penalty=bounds)
    assert list(res["status"]) == [0, ffi.AWV_ST_ABOVE_BOUND, 0, 0]  # (the fourth pair is the identical one: P = 0)
    assert list(vres["code"]) == [ffi.AWV_VF_OK, ffi.AWV_VF_SKIPPED, ffi.AWV_VF_OK, ffi.AWV_VF_OK]
    assert engine.verify_stats().failed == 0


# ---- 7. host mirror -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clusters():
    """12 sequences of about 1 kbp: three clusters, about 3 % inside a cluster and 15 % between clusters."""
    rng = random.Random("bounded/clusters")
    root = rand_seq(rng, 1000)
    seqs = []
    for c in range(3):
        centre = mutate(root, 0.075, rng)
        seqs += [mutate(centre, 0.015, rng) for _ in range(4)]
    return ["c%d_%d" % (i // 4, i % 4) for i in range(12)], seqs


SCORES_2P = "0,5,8,2,24,1"


@pytest.fixture(scope="module")
def host_lib(hip_lib):
    from allwave_amd import build, host
    build.build_host()
    host.load()
    return host


@pytest.mark.parametrize("orientation,devices", [("forward", None), ("wfa", None), ("mash", None), ("forward", [0, 0])])
def test_host_mirror(host_lib, clusters, orientation, devices):
    host = host_lib
    ids, seqs = clusters
    kw = dict(orientation=orientation, devices=devices, min_batch_pairs=16)
    full = host.all_pairs_paf(ids, seqs, SCORES_2P, **kw)
    assert len(full) == 132 and host.last_bounds() == dict(pairs=0, above_penalty=0, above_divergence=0)
    pens = [BC.paf_penalty(DEFAULT_2P, ln) for ln in full]
    B = sorted(pens)[len(pens) // 3]
    kept = [ln for ln, p in zip(full, pens) if p <= B]
    assert 0 < len(kept) < len(full)
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, max_penalty=B, **kw)
    assert sorted(got) == sorted(kept)
    if devices is None:
        assert got == kept  # (one slot: pair-list order)
    assert host.last_bounds() == dict(pairs=132, above_penalty=len(full) - len(kept), above_divergence=0)
    for d in (0.08, 0.0, 0.5):
        kept_d = [ln for ln in full if BC.within_divergence(BC.paf_ops(ln), d)]
        got = host.all_pairs_paf(ids, seqs, SCORES_2P, max_divergence=d, verify=True, **kw)
        assert set(got) == set(kept_d) and len(got) == len(kept_d), (d, len(got), len(kept_d))
        assert host.last_bounds() == dict(pairs=132, above_penalty=0, above_divergence=len(full) - len(kept_d))
        assert host.last_verify()["failures"] == [] and host.last_verify()["pairs"] == 132
    assert 0 < len([ln for ln in full if BC.within_divergence(BC.paf_ops(ln), 0.08)]) < len(full)
    # both bounds: the smaller penalty bound applies, and a pair has to pass both
    both = [ln for ln, p in zip(full, pens) if p <= B and BC.within_divergence(BC.paf_ops(ln), 0.08)]
    got = host.all_pairs_paf(ids, seqs, SCORES_2P, max_penalty=B, max_divergence=0.08, **kw)
    assert sorted(got) == sorted(both)
    lb = host.last_bounds()
    assert lb["pairs"] == 132 and lb["above_penalty"] + lb["above_divergence"] == len(full) - len(both)
    # every consumer is handed exactly the kept pairs
    for mode in ("for_each", "next", "par_for_each", "par_collect"):
        got = host.iterate(ids, seqs, SCORES_2P, mode=mode, orientation=orientation, devices=devices, min_batch_pairs=16, chunk=50,
                           max_penalty=B)
        assert sorted(got) == sorted(kept), mode
        assert host.last_bounds()["above_penalty"] == len(full) - len(kept), mode
    # the bounds hold for the one call they were given to
    assert host.all_pairs_paf(ids, seqs, SCORES_2P, **kw) == full or devices is not None
    nb, nl = host.all_pairs_paf_count(ids, seqs, SCORES_2P, orientation=orientation, max_divergence=0.08)[:2]
    assert nl == len([ln for ln in full if BC.within_divergence(BC.paf_ops(ln), 0.08)])


def test_host_ranges(host_lib, clusters):
    host = host_lib
    ids, seqs = clusters
    rng = random.Random("bounded/host-ranges")
    ranges = []
    for k in range(30):
        q, t = rng.randrange(12), rng.randrange(12)
        qb, tb = rng.randrange(0, 300), rng.randrange(0, 300)
        ranges.append((q, t, 0, qb, qb + rng.randrange(200, 600), tb, tb + rng.randrange(200, 600)))
    full = host.align_ranges(ids, seqs, ranges, SCORES_2P)
    pens = [BC.paf_penalty(DEFAULT_2P, ln) for ln in full]
    B = sorted(pens)[len(pens) // 2]
    for devices in (None, [0, 0]):
        assert host.align_ranges(ids, seqs, ranges, SCORES_2P, devices=devices, max_penalty=B) == [ln for ln, p in zip(full, pens) if p <= B]
        assert host.last_bounds()["above_penalty"] == sum(p > B for p in pens)
        kept = [ln for ln in full if BC.within_divergence(BC.paf_ops(ln), 0.1)]
        assert host.align_ranges(ids, seqs, ranges, SCORES_2P, devices=devices, max_divergence=0.1) == kept
        assert host.last_bounds() == dict(pairs=30, above_penalty=0, above_divergence=len(full) - len(kept))


# ---- 8. CLI ---------------------------------------------------------------------------------------------------------------
def test_cli(host_lib, clusters, tmp_path):
    from allwave_amd import build
    host = host_lib
    ids, seqs = clusters
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))

    def run(*args):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-s", SCORES_2P] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines(), r.stderr.splitlines()[-1]

    full, summary = run("-p", "none", "--wfa-orientation")
    assert len(full) == 132 and "above the bound" not in summary
    pens = [BC.paf_penalty(DEFAULT_2P, ln) for ln in full]
    B = sorted(pens)[len(pens) // 3]
    kept = [ln for ln, p in zip(full, pens) if p <= B]
    got, summary = run("-p", "none", "--wfa-orientation", "--max-align-penalty", str(B), "--verify")
    assert got == kept and "%d/132" % len(kept) in summary and ", %d pairs above the bound" % (132 - len(kept)) in summary
    assert "verified 132 pairs, 0 failed" in summary
    kept_d = [ln for ln in full if BC.within_divergence(BC.paf_ops(ln), 0.08)]
    got, summary = run("-p", "none", "--wfa-orientation", "--max-divergence", "0.08")
    assert got == kept_d and 0 < len(kept_d) < 132 and ", %d pairs above the bound" % (132 - len(kept_d)) in summary
    got, summary = run("-p", "none", "--wfa-orientation", "--max-divergence", "0.08", "--devices", "0,0")
    assert sorted(got) == sorted(kept_d)
    # --align-paf: the surviving lines, in input order
    rng = random.Random("bounded/cli-ranges")
    lines = []
    for k in range(30):
        q, t = rng.randrange(12), rng.randrange(12)
        qb, tb = rng.randrange(0, 300), rng.randrange(0, 300)
        lines.append("\t".join(str(v) for v in (ids[q], len(seqs[q]), qb, qb + rng.randrange(200, 600), "+", ids[t], len(seqs[t]), tb,
                                                 tb + rng.randrange(200, 600), 0, 0, 255)))
    lines.insert(7, "nobody\t10\t0\t5\t+\t%s\t%d\t0\t5\t0\t0\t255" % (ids[0], len(seqs[0])))
    paf_in = tmp_path / "map.paf"
    paf_in.write_text("\n".join(lines) + "\n")
    full_r, _ = run("--align-paf", str(paf_in))
    assert len(full_r) == 30
    pens_r = [BC.paf_penalty(DEFAULT_2P, ln) for ln in full_r]
    Br = sorted(pens_r)[15]
    got, summary = run("--align-paf", str(paf_in), "--max-align-penalty", str(Br))
    assert got == [ln for ln, p in zip(full_r, pens_r) if p <= Br]
    assert "1 bad lines" in summary and ", %d pairs above the bound" % sum(p > Br for p in pens_r) in summary
