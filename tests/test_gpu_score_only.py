"""GPU tests (-m gpu) of score-only alignment: awv_score_pairs (Engine.score_pairs), its penalty bound, the host library's
AllPairIterator::scores (host.all_pairs_scores) and the CLI's --score-only.

The penalty of a score-only call is the top-level breakpoint search's score, without the recursion, the base cases of the
sub-problems or a CIGAR: it must equal the oracle's optimal penalty and what align_pairs reports, under every kernel flavour,
row width and variant pin.  A bound B reports every pair above it as AWV_ST_ABOVE_BOUND (penalty B + 1) and leaves every
other pair exact; it must also cut the work of unrelated pairs (deterministic cell counters, not timing)."""
import random
import subprocess

import numpy as np
import pytest

import penalty_space as PS
import repeats as R
from util import DEFAULT_2P, EDIT, PENALTY_SETS, mutate, rand_seq, random_pair

pytestmark = pytest.mark.gpu

COMP = {65: 84, 84: 65, 67: 71, 71: 67}
LARGE_SB = 1100                 # (as tests/test_gpu_penalties.py: such sets get an engine with capped scratch)
SCRATCH_CAP = 6 << 30


def rc(s):
    return bytes(COMP.get(b, 78) for b in reversed(s))


def _pairs(ab):
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    return seqs, pairs


def _oracle_penalties(oracle, seqs, pairs, scores):
    al = oracle.Aligner(scores)
    out = []
    for p in pairs:
        q = seqs[p[0]]
        if len(p) > 2 and p[2]:
            q = rc(q)
        out.append(al.align(q, seqs[p[1]])[0])
    return out


def check_scores(engine, oracle, seqs, pairs, scores, want=None):
    """score_pairs: status 0 and the oracle's penalty for every pair, equal to align_pairs's penalty too."""
    from allwave_amd import ffi
    engine.set_sequences(seqs)
    if want is None:
        want = _oracle_penalties(oracle, seqs, pairs, scores)
    sc = engine.score_pairs(scores, pairs)
    res, _ = engine.align_pairs(scores, pairs, want_cigars=False)
    for i, p in enumerate(pairs):
        assert sc["status"][i] == ffi.AWV_ST_COMPLETED, (scores, i, int(sc["status"][i]))
        assert sc["penalty"][i] == want[i], (scores, i, len(seqs[p[0]]), len(seqs[p[1]]), int(sc["penalty"][i]), want[i])
        assert res["status"][i] == 0 and res["penalty"][i] == sc["penalty"][i], (scores, i)
    return sc, want


def random_inputs(seed, n=40, maxlen=1500):
    rng = random.Random(seed)
    return _pairs([random_pair(rng, maxlen) for _ in range(n)])


@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_random_pairs_exact(engine, oracle, scores):
    seqs, pairs = random_inputs("score-only/random/%s" % (scores,))
    check_scores(engine, oracle, seqs, pairs, scores)


def test_edge_pairs_exact(engine, oracle):
    """Empty and identical sequences, lengths on both sides of FALLBACK_MIN_LENGTH (the top level as a base case), and
    reverse-complement pairs."""
    rng = random.Random("score-only/edges")
    s = rand_seq(rng, 700)
    ab = [(b"", b""), (b"", b"ACGT"), (b"ACGTTGCA", b""), (s, s), (s[:50], s[:50])]
    for n in (1, 7, 99, 100, 101, 130):
        a = rand_seq(rng, n)
        ab += [(a, mutate(a, 0.1, rng)), (a, rand_seq(rng, max(1, n // 2))), (a, a + rand_seq(rng, 3))]
    seqs, pairs = _pairs(ab)
    pairs = [(a, b, 0) for a, b in pairs]
    # reverse-complement pairs: q_revcomp = 1 scores reverse_complement(query) against the target
    for _ in range(6):
        a = rand_seq(rng, rng.choice([80, 150, 900]))
        seqs += [rc(mutate(a, 0.03, rng)), a]
        pairs.append((len(seqs) - 2, len(seqs) - 1, 1))
    pairs.append((len(seqs) - 2, len(seqs) - 1, 0))
    for scores in (DEFAULT_2P, EDIT, (0, 4, 6, 2)):
        check_scores(engine, oracle, seqs, pairs, scores)


@pytest.mark.parametrize("name", [n for n, _ in PS.ACCEPTED])
def test_every_accepted_penalty_set(engine, oracle, request, name):
    scores = PS.BY_NAME[name]
    rng = random.Random("score-only/penalties/" + name)
    seqs, pairs = _pairs([random_pair(rng, 1200) for _ in range(10)] + [R.microsatellite(rng)])
    if PS.derive(scores).sb <= LARGE_SB:
        check_scores(engine, oracle, seqs, pairs, scores)
        return
    from allwave_amd import ffi
    mode = request.node.callspec.params["engine"]
    e = ffi.Engine(flags=ffi.AWV_F_ONE_WAVE if mode == "one_wave" else 0, max_scratch_bytes=SCRATCH_CAP)
    try:
        check_scores(e, oracle, seqs, pairs, scores)
    finally:
        e.close()


@pytest.mark.parametrize("cls", sorted(R.SMALL))
def test_repeat_classes_exact(engine, oracle, cls):
    rng = random.Random("score-only/repeats/" + cls)
    seqs, pairs = _pairs([R.SMALL[cls](rng) for _ in range(3)])
    pairs += [(b, a) for a, b in pairs]
    check_scores(engine, oracle, seqs, pairs, DEFAULT_2P)


def long_inputs():
    """Pairs of 32,760 bases or more (32-bit rows, and the 16-bit searches of sub-problems inside them) and a pair whose
    length difference sends it to the sixteen-wave flavour."""
    rng = random.Random("score-only/long")
    a = rand_seq(rng, 34000)
    b = rand_seq(rng, 18000)
    ab = [(a, mutate(a, 0.01, rng)), (mutate(a, 0.02, rng)[:33500], a), (b, mutate(b, 0.01, rng)[2000:3500])]
    return _pairs(ab)


def test_long_and_unequal_pairs_exact(engine, oracle):
    seqs, pairs = long_inputs()
    check_scores(engine, oracle, seqs, pairs, DEFAULT_2P)


VARIANT_FLAGS = ("AWV_F_FORCE_INT32", "AWV_F_NO_PACKED_SEQ", "AWV_F_FOUR_WAVES", "AWV_F_ONE_WAVE", "AWV_F_SINGLE_STEP",
                 "AWV_F_NO_DEEP", "AWV_F_NO_CHAIN", "AWV_F_NO_WIDE16", "first_row_cols")


@pytest.fixture(scope="module")
def variant_inputs(oracle):
    seqs, pairs = random_inputs("score-only/variants", n=24, maxlen=2500)
    lseqs, lpairs = long_inputs()
    k = len(seqs)
    seqs += lseqs
    pairs += [(a + k, b + k) for a, b in lpairs]
    return seqs, pairs, _oracle_penalties(oracle, seqs, pairs, DEFAULT_2P)


@pytest.mark.parametrize("variant", VARIANT_FLAGS)
def test_variant_pins_agree(hip_lib, oracle, variant_inputs, variant):
    """Every variant pin gives the same penalties; a narrow first attempt (first_row_cols) takes the CAPACITY re-run path."""
    from allwave_amd import ffi
    seqs, pairs, want = variant_inputs
    if variant == "first_row_cols":
        e = ffi.Engine(flags=ffi.AWV_F_NO_ARENA_PROBE, first_row_cols=2048)
    else:
        e = ffi.Engine(flags=getattr(ffi, variant) | ffi.AWV_F_NO_ARENA_PROBE)
    try:
        check_scores(e, oracle, seqs, pairs, DEFAULT_2P, want)
        if variant == "first_row_cols":
            assert e.stats().launches > 1  # some pair outgrew the 2048-column rows and was re-run wider
    finally:
        e.close()


@pytest.fixture(scope="module")
def bound_inputs(oracle):
    """Pairs with a spread of penalties: clean mutations at several divergences, unrelated pairs, forced gaps."""
    rng = random.Random("score-only/bound")
    ab = []
    for d in (0.0, 0.002, 0.01, 0.03, 0.08, 0.15):
        for n in (300, 1200, 2500):
            s = rand_seq(rng, n)
            ab.append((s, mutate(s, d, rng)))
    ab += [(rand_seq(rng, 800), rand_seq(rng, 900)), (rand_seq(rng, 60), rand_seq(rng, 70))]
    s = rand_seq(rng, 1500)
    ab.append((s, s[:400] + s[900:]))
    seqs, pairs = _pairs(ab)
    return seqs, pairs, _oracle_penalties(oracle, seqs, pairs, DEFAULT_2P)


def test_bound_semantics(engine, bound_inputs):
    from allwave_amd import ffi
    seqs, pairs, want = bound_inputs
    engine.set_sequences(seqs)
    pens = sorted(set(want))
    bounds = {0, pens[len(pens) // 4], pens[len(pens) // 2], pens[-1] - 1, pens[-1]}
    p = pens[len(pens) // 2]
    bounds |= {p, p - 1}  # B = p passes that pair, B = p - 1 flags it
    for B in sorted(b for b in bounds if b >= 0):
        sc = engine.score_pairs(DEFAULT_2P, pairs, max_penalty=B)
        for i in range(len(pairs)):
            if want[i] > B:
                assert sc["status"][i] == ffi.AWV_ST_ABOVE_BOUND and sc["penalty"][i] == B + 1, (B, i, want[i], int(sc["status"][i]))
            else:
                assert sc["status"][i] == ffi.AWV_ST_COMPLETED and sc["penalty"][i] == want[i], (B, i, want[i], int(sc["penalty"][i]))
    i = want.index(p)
    assert engine.score_pairs(DEFAULT_2P, [pairs[i]], max_penalty=p)["status"][0] == ffi.AWV_ST_COMPLETED
    assert engine.score_pairs(DEFAULT_2P, [pairs[i]], max_penalty=p - 1)["status"][0] == ffi.AWV_ST_ABOVE_BOUND
    with pytest.raises(ValueError):
        engine.score_pairs(DEFAULT_2P, pairs, max_penalty=-1)


@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT])
def test_bound_saves_work(engine, scores):
    """Unrelated pairs of a few kbp: a bound of 200 stops their searches early -- under a tenth of the unbounded cells."""
    from allwave_amd import ffi
    rng = random.Random("score-only/unrelated")
    seqs = [rand_seq(rng, rng.randint(2500, 4000)) for _ in range(24)]
    pairs = [(i, i + 1) for i in range(0, 24, 2)] + [(i + 1, i) for i in range(0, 24, 2)]
    engine.set_sequences(seqs)
    full = engine.score_pairs(scores, pairs)
    c_full = engine.stats().cell_steps
    bounded = engine.score_pairs(scores, pairs, max_penalty=200)
    c_bound = engine.stats().cell_steps
    assert (full["status"] == 0).all() and (full["penalty"] > 200).all()
    assert (bounded["status"] == ffi.AWV_ST_ABOVE_BOUND).all() and (bounded["penalty"] == 201).all()
    assert c_bound < 0.1 * c_full, (c_bound, c_full)


def test_score_only_does_less_work(engine):
    """Config-2-shaped pairs (10 kbp, 5 % divergence): the score-only call computes at most 3/4 of align_pairs's cells and
    the same penalties."""
    from allwave_amd import synth
    data, offs, _ = synth.generate(12, 10000, 0.05, 2)
    pairs = synth.all_pairs(12)
    engine.set_sequences((data, offs))
    sc = engine.score_pairs(DEFAULT_2P, pairs)
    c_score = engine.stats().cell_steps
    res, _ = engine.align_pairs(DEFAULT_2P, pairs, want_cigars=False)
    c_align = engine.stats().cell_steps
    assert (sc["status"] == 0).all() and (res["status"] == 0).all()
    assert (sc["penalty"] == res["penalty"]).all()
    assert c_score <= 0.75 * c_align, (c_score, c_align)


def test_no_arena_limit(hip_lib, request):
    """max_arena_bytes caps the CIGAR arena of a launch: align_pairs needs many launches for it, score-only needs none of
    it -- one launch for the call's one flavour group."""
    from allwave_amd import ffi, synth
    data, offs, _ = synth.generate(48, 10000, 0.05, 3)
    pairs = synth.all_pairs(48)
    e = ffi.Engine(max_arena_bytes=1 << 20, flags=ffi.AWV_F_NO_ARENA_PROBE)
    try:
        e.set_sequences((data, offs))
        sc = e.score_pairs(DEFAULT_2P, pairs)
        n_score = e.stats().launches
        res, _ = e.align_pairs(DEFAULT_2P, pairs, want_cigars=False)
        n_align = e.stats().launches
    finally:
        e.close()
    assert (sc["status"] == 0).all() and (sc["penalty"] == res["penalty"]).all()
    assert n_score == 1, n_score
    assert n_align >= 20, n_align


def test_score_pairs_errors(engine):
    from allwave_amd import ffi
    engine.set_sequences([b"ACGT", b"ACGA"])
    with pytest.raises(ffi.EngineError) as ei:
        engine.score_pairs(DEFAULT_2P, [(0, 5)])
    assert ei.value.code == ffi.AWV_ERR_ARG
    import ctypes as C
    pen = ffi.Penalties.from_scores(DEFAULT_2P)
    pairs = np.zeros(1, dtype=ffi.PAIR_DTYPE)
    L = ffi.load()
    assert L.awv_score_pairs(engine._h, C.byref(pen), pairs.ctypes.data, 1, -1, None) == ffi.AWV_ERR_ARG
    out = np.zeros(1, dtype=ffi.SCORE_DTYPE)
    assert L.awv_score_pairs(engine._h, C.byref(pen), pairs.ctypes.data, -1, -1, out.ctypes.data) == ffi.AWV_ERR_ARG
    assert len(engine.score_pairs(DEFAULT_2P, np.zeros((0, 2), dtype=np.int32))) == 0


# ---- host library and CLI ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(hip_lib):
    from allwave_amd import build, host as H
    build.build_host()
    H.load()
    return H


def paf_penalty(line, scores):
    """The penalty of a PAF record's alignment, from its cg:Z: CIGAR (= match, X mismatch, I / D gaps: the cheaper piece)."""
    import re
    cg = [f for f in line.split("\t") if f.startswith("cg:Z:")][0][5:]
    x, o1, e1 = scores[1], scores[2], scores[3]
    o2, e2 = (scores[4], scores[5]) if len(scores) == 6 else (o1, e1)
    pen = 0
    for n, op in re.findall(r"(\d+)([=XID])", cg):
        n = int(n)
        pen += 0 if op == "=" else n * x if op == "X" else min(o1 + n * e1, o2 + n * e2)
    return pen


def host_inputs():
    rng = random.Random("score-only/host")
    base = rand_seq(rng, 1500)
    seqs = []
    for i in range(10):
        s = mutate(base, 0.04, rng)
        seqs.append(rc(s) if i % 3 == 1 else s)
    return ["s%d" % i for i in range(len(seqs))], seqs


@pytest.mark.parametrize("sparsification", ["none", "giant:0.9", "tree:2:1:0.2"])
def test_host_scores_match_iterate(host, sparsification):
    """host.all_pairs_scores over the same plan as host.iterate (mash orientation, the sparsification, two engines on
    device 0): the same pairs, strands and penalties -- those of the PAF records' CIGARs."""
    ids, seqs = host_inputs()
    scores = "0,5,8,2,24,1"
    lines = host.iterate(ids, seqs, scores, mode="for_each", sparsification=sparsification, orientation="mash", devices=[0, 0])
    got = host.all_pairs_scores(ids, seqs, scores, orientation="mash", sparsification=sparsification, devices=[0, 0])
    assert len(got) == len(lines) > 0
    paf = {}
    for l in lines:
        f = l.split("\t")
        paf[(f[0], f[5])] = (f[4], paf_penalty(l, DEFAULT_2P))
    assert len(paf) == len(lines)
    for r in got:
        key = (ids[r["query_idx"]], ids[r["target_idx"]])
        assert r["status"] == 0
        assert paf[key] == ("-" if r["is_reverse"] else "+", int(r["penalty"])), key
    bounded = host.all_pairs_scores(ids, seqs, scores, orientation="mash", sparsification=sparsification, devices=[0, 0],
                                    max_penalty=int(np.median(got["penalty"])))
    for f in ("query_idx", "target_idx", "is_reverse"):
        assert (bounded[f] == got[f]).all(), f
    B = int(np.median(got["penalty"]))
    assert ((bounded["status"] == 4) == (got["penalty"] > B)).all()
    assert (bounded["penalty"] == np.where(got["penalty"] > B, B + 1, got["penalty"])).all()


def test_host_scores_wfa_orientation_and_shard(host):
    """WFA orientation (two full alignments choose the strand, the final one is scored) and with_shard: the shards together
    give the whole list's records."""
    ids, seqs = host_inputs()
    scores = "0,5,8,2,24,1"
    whole = host.all_pairs_scores(ids, seqs, scores, orientation="wfa")
    lines = host.iterate(ids, seqs, scores, mode="for_each", orientation="wfa")
    assert len(whole) == len(lines)
    for r, l in zip(whole, lines):
        f = l.split("\t")
        assert (f[0], f[5], f[4]) == (ids[r["query_idx"]], ids[r["target_idx"]], "-" if r["is_reverse"] else "+")
        assert r["penalty"] == paf_penalty(l, DEFAULT_2P)
    parts = [host.all_pairs_scores(ids, seqs, scores, orientation="wfa", shard=(k, 3)) for k in range(3)]
    key = lambda a: sorted(tuple(int(v) for v in r) for r in a)
    assert key(np.concatenate(parts)) == key(whole)


def test_cli_score_only(host, oracle, tmp_path):
    """--score-only --forward-only lists the pairs of --forward-only's PAF in the same order, with the oracle's penalties;
    --max-penalty leaves out exactly the pairs above it."""
    from allwave_amd import build
    rng = random.Random("score-only/cli")
    base = rand_seq(rng, 900)
    seqs = [mutate(base, d, rng) for d in (0.0, 0.01, 0.03, 0.06, 0.1)] + [rand_seq(rng, 500)]
    ids = ["r%d" % i for i in range(len(seqs))]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s desc\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    common = [build.CLI_BIN, "-i", str(fa), "-p", "none", "--forward-only", "--no-progress"]
    r = subprocess.run(common + ["-o", str(tmp_path / "o.paf")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    paf = (tmp_path / "o.paf").read_text().splitlines()
    r = subprocess.run(common + ["--score-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(paf) == len(seqs) * (len(seqs) - 1)
    al = oracle.Aligner(DEFAULT_2P)
    by_id = dict(zip(ids, seqs))
    pens = []
    for o, p in zip(out, paf):
        f, g = o.split("\t"), p.split("\t")
        assert len(f) == 6
        assert (f[0], f[1], f[2], f[3], f[4]) == (g[0], g[1], g[5], g[6], g[4]) and f[4] == "+"
        want = al.align(by_id[f[0]], by_id[f[2]])[0]
        assert int(f[5]) == want, (f, want)
        pens.append(want)
    B = sorted(pens)[len(pens) // 2]
    r = subprocess.run(common + ["--score-only", "--max-penalty", str(B)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [o for o, p in zip(out, pens) if p <= B]
