"""GPU tests (-m gpu): the penalties of every kernel path at 10-150 kbp against the banded Gotoh DP (oracle/gotoh.c), which
has none of BiWFA's logic -- not against the oracle, a BiWFA written with the same view of breakpoints, gap-component splits
and termination as the kernels.

For every pair: status 0; penalty == gotoh_penalty_banded(..., bound=penalty) (a penalty above the optimum makes the DP
find a lower one, a penalty below it makes the DP return more); the CIGAR is valid and re-scores to the penalty; the
M/X/I/D counts and q_end / t_end are the CIGAR's.  The paths are those of the routing in assign_groups (batch_plan.hpp, the
NG = 9 group table): one wave with 16-bit rows and multi-step passes, four and sixteen waves, 32-bit rows, wide16 rows,
chains through LDS, 16-bit sub-searches inside 32-bit launches, in-place packed, staged and raw-byte probes, reverse
complements and restarted searches; where the engine's counters can show that a path ran, the test asserts it.  The DP
calls run on a thread pool while the next engine call runs.  Score-only calls (awv_score_pairs) are held to the same DP,
with no bound and with bounds around each pair's optimum.
"""
import collections
import random

import pytest

import long_pairs as LP
import penalty_space as PS
import repeats as R
from util import DEFAULT_2P, EDIT, mutate, rand_seq

pytestmark = pytest.mark.gpu

COMP = {65: 84, 84: 65, 67: 71, 71: 67, 97: 84, 116: 65, 99: 71, 103: 67}
LARGE_SB = 1100                 # (as tests/test_gpu_penalties.py: such sets get an engine with capped scratch)
SCRATCH_CAP = 6 << 30
CHECKED = collections.Counter()  # pairs checked per path, printed at the end of the module


def rc(s):
    """The query an (q, t, 1) pair aligns: reverse complement, upper case, anything else N (alignment.rs:178-190)."""
    return bytes(COMP.get(b, 78) for b in reversed(s))


def _engine(flags=0, scores=DEFAULT_2P):
    from allwave_amd import ffi
    return ffi.Engine(flags=flags, max_scratch_bytes=SCRATCH_CAP if PS.derive(scores).sb > LARGE_SB else 0)


def _flags(*names):
    from allwave_amd import ffi
    f = 0
    for n in names:
        f |= getattr(ffi, "AWV_F_" + n)
    return f


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\npairs checked against the banded DP per path:")
    for path, n in sorted(CHECKED.items()):
        print("  %-40s %d" % (path, n))


class DPCheck:
    """Engine calls checked against the banded DP.  The DP answers are futures on the oracle's thread pool (cached per
    unordered pair, set and bound: the DP is symmetric); finish() waits for them and asserts."""

    def __init__(self, oracle):
        self.o = oracle
        self.pending = []
        self.cache = {}

    def dp(self, q, t, scores, bound):
        key = (min(q, t), max(q, t), tuple(scores), bound)
        if key not in self.cache:
            self.cache[key] = self.o.dp_pool().submit(self.o.gotoh_penalty_banded, q, t, scores, bound)
        return self.cache[key]

    @staticmethod
    def pair_seqs(seqs, p):
        q = rc(seqs[p[0]]) if len(p) > 2 and p[2] else seqs[p[0]]
        return q, seqs[p[1]]

    def align(self, e, seqs, pairs, scores, path):
        """align_pairs on e; returns (penalties, stats of the call)."""
        e.set_sequences(seqs)
        res, cigs = e.align_pairs(scores, pairs)
        st = e.stats()
        pens = []
        for i, p in enumerate(pairs):
            q, t = self.pair_seqs(seqs, p)
            what = (path, tuple(scores), tuple(p), len(q), len(t))
            assert res["status"][i] == 0, what + (int(res["status"][i]),)
            pen = int(res["penalty"][i])
            assert res["score"][i] == -pen, what
            assert self.o.cigar_check(cigs[i], q, t, scores) == (0, pen), what + (pen,)
            c = {k: cigs[i].count(k.encode()) for k in "MXID"}
            assert (res["num_matches"][i], res["num_mismatches"][i], res["num_ins"][i], res["num_del"][i]) == \
                   (c["M"], c["X"], c["I"], c["D"]), what
            assert res["q_end"][i] == c["M"] + c["X"] + c["D"] == len(q), what
            assert res["t_end"][i] == c["M"] + c["X"] + c["I"] == len(t), what
            self.pending.append((what + (pen,), self.dp(q, t, scores, pen), (pen,)))
            pens.append(pen)
        CHECKED[path] += len(pairs)
        return pens, st

    def score_only(self, e, seqs, pairs, scores, pens, path):
        """score_pairs on e with no bound (the DP-checked penalties of align), with the median penalty as the bound, and
        with opt - 1, opt and opt + 1 for each pair: AWV_ST_ABOVE_BOUND with penalty B + 1 exactly where the DP bounded
        by B returns more than B, else status 0 and the DP's penalty."""
        from allwave_amd import ffi
        e.set_sequences(seqs)
        sc = e.score_pairs(scores, pairs)
        for i, p in enumerate(pairs):
            assert sc["status"][i] == ffi.AWV_ST_COMPLETED and sc["penalty"][i] == pens[i], \
                (path, tuple(scores), tuple(p), int(sc["status"][i]), int(sc["penalty"][i]), pens[i])
        med = sorted(pens)[len(pens) // 2]
        checks = [(med, pairs, e.score_pairs(scores, pairs, max_penalty=med))]
        for p, opt in zip(pairs, pens):
            for B in (opt - 1, opt, opt + 1):
                if B >= 0:
                    checks.append((B, [p], e.score_pairs(scores, [p], max_penalty=B)))
        for B, ps, out in checks:
            for i, p in enumerate(ps):
                q, t = self.pair_seqs(seqs, p)
                self.pending.append(((path + "/score-only", tuple(scores), tuple(p), B), self.dp(q, t, scores, B),
                                     (B, int(out["status"][i]), int(out["penalty"][i]))))
        CHECKED[path + "/score-only"] += len(pairs)

    def finish(self):
        """Waits for the DP and asserts: (pen,) -- align's penalty is the DP's; (B, status, penalty) -- a score-only
        answer under bound B."""
        from allwave_amd import ffi
        for what, fut, want in self.pending:
            dp = fut.result()
            if len(want) == 1:
                assert dp == want[0], what + ("DP", dp)
                continue
            B, status, penalty = want
            if dp > B:
                assert status == ffi.AWV_ST_ABOVE_BOUND and penalty == B + 1, what + ("DP", dp, status, penalty)
            else:
                assert status == ffi.AWV_ST_COMPLETED and penalty == dp, what + ("DP", dp, status, penalty)
        self.pending = []


@pytest.fixture
def dpc(oracle):
    c = DPCheck(oracle)
    yield c
    for _, fut, _ in c.pending:  # (a test that failed before its finish(): drop the DP calls it left)
        fut.cancel()


def config2_pairs():
    """Config-2-shaped pairs: eight pairs of 10 kbp reads, each 5 % from a common root."""
    from allwave_amd import synth
    data, offs, _ = synth.generate(16, 10000, 0.05, 2)
    seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(16)]
    return seqs, [tuple(int(v) for v in p) for p in synth.all_pairs(16)[::29][:8]]


def test_one_wave_sixteen_bit_passes(dpc):
    """One wave per pair, 16-bit rows: multi-step passes with the deep margin zone, without it (AWV_F_NO_DEEP), without
    chained sweeps (AWV_F_NO_CHAIN) and step by step (AWV_F_SINGLE_STEP)."""
    seqs, pairs = config2_pairs()
    for name, flags in (("one_wave", ("ONE_WAVE",)), ("no_deep", ("ONE_WAVE", "NO_DEEP")),
                        ("no_chain", ("ONE_WAVE", "NO_CHAIN")), ("single_step", ("ONE_WAVE", "SINGLE_STEP"))):
        e = _engine(_flags(*flags))
        try:
            _, st = dpc.align(e, seqs, pairs, DEFAULT_2P, "one_wave16/" + name)
        finally:
            e.close()
        # (thresholds as test_multi_step_passes_all_presets measured them)
        if name == "one_wave":
            assert st.multi_cell_steps > 0.3 * st.cell_steps and st.deep_cell_steps > 0, (name, st.multi_cell_steps,
                                                                                         st.cell_steps, st.deep_cell_steps)
        elif name == "no_deep":
            assert st.multi_cell_steps > 0.2 * st.cell_steps and st.deep_cell_steps == 0, (name, st.multi_cell_steps,
                                                                                          st.cell_steps, st.deep_cell_steps)
        elif name == "no_chain":
            assert st.multi_cell_steps > 0, name
        else:
            assert st.multi_cell_steps == 0, name
    dpc.finish()


def test_four_waves(dpc):
    """Four waves per pair: pinned (AWV_F_FOUR_WAVES) on the config-2 pairs, and chosen by the engine for a length
    difference of 4,096 or more."""
    seqs, pairs = config2_pairs()
    e = _engine(_flags("FOUR_WAVES"))
    try:
        _, st = dpc.align(e, seqs, pairs, DEFAULT_2P, "four_waves/pinned")
        assert st.multi_cell_steps > 0
    finally:
        e.close()
    rng = random.Random("dp/four")
    a = rand_seq(rng, 14000)
    seqs = [a, mutate(a, 0.02, rng)[2000:9000], mutate(a, 0.03, rng)[:9500]]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0)]
    assert all(4096 <= abs(len(seqs[p]) - len(seqs[q])) < 16384 for p, q in pairs)
    e = _engine()
    try:
        dpc.align(e, seqs, pairs, DEFAULT_2P, "four_waves/dl>=4096")
    finally:
        e.close()
    dpc.finish()


def test_sixteen_waves(dpc):
    """Sixteen waves per pair (length difference >= 16,384) at default flags: the sixteen-wave pair of the row-width inputs
    and the 17.5 k difference of test_very_unequal_lengths, both orders."""
    seqs, pairs = LP.row_width_pairs()
    useqs, upairs = LP.very_unequal()
    seqs = seqs[4:] + useqs
    pairs = [(0, 1), (1, 0)] + [(a + 2, b + 2) for a, b in upairs[:2]]
    assert all(abs(len(seqs[p]) - len(seqs[q])) >= 16384 for p, q in pairs)
    e = _engine()
    try:
        _, st = dpc.align(e, seqs, pairs, DEFAULT_2P, "sixteen_waves")
        assert st.pairs_completed == len(pairs)
    finally:
        e.close()
    dpc.finish()


def _exact_length(rng, s, n):
    return s[:n] + rand_seq(rng, max(0, n - len(s)))


def test_32bit_rows(dpc):
    """32-bit rows: both lengths >= 32,760 (the engine's choice of flavour, and one wave per pair), AWV_F_FORCE_INT32 on the
    config-2 pairs under one and four waves, and the 32,759 / 32,760 edge of the row width."""
    rseqs, rpairs = LP.row_width_pairs()
    lseqs, lpairs = LP.random_long()
    seqs = rseqs[:2] + lseqs[2:6]
    pairs = [(0, 1), (1, 0), (2, 3), (4, 5)]
    assert all(min(len(seqs[p]), len(seqs[q])) >= 32760 for p, q in pairs)
    for name, flags in (("auto", ()), ("one_wave", ("ONE_WAVE",))):
        e = _engine(_flags(*flags))
        try:
            _, st = dpc.align(e, seqs, pairs, DEFAULT_2P, "rows32/" + name)
            assert st.pairs_completed == len(pairs)
        finally:
            e.close()
    cseqs, cpairs = config2_pairs()
    for name, flags in (("force_int32", ("ONE_WAVE", "FORCE_INT32")), ("four_force_int32", ("FOUR_WAVES", "FORCE_INT32"))):
        e = _engine(_flags(*flags))
        try:
            _, st = dpc.align(e, cseqs, cpairs, DEFAULT_2P, "rows32/" + name)
            assert st.multi_cell_steps > 0
        finally:
            e.close()
    rng = random.Random("dp/edge")
    a = rand_seq(rng, 32760)
    b = mutate(a, 0.01, rng)
    seqs = [a[:32759], _exact_length(rng, b, 32759), a, _exact_length(rng, b, 32760)]
    e = _engine()
    try:
        dpc.align(e, seqs, [(0, 1), (1, 0), (2, 3), (3, 2), (0, 3), (2, 1)], DEFAULT_2P, "rows32/edge_32759_32760")
    finally:
        e.close()
    dpc.finish()


def test_wide16_rows(dpc):
    """16-bit min(h, v) rows: the shorter sequence below 32,760, the longer at or above it -- a 3 kbp infix of 36 kbp, a
    30 kbp prefix of 40 kbp at 1 %, a 32,759-base sequence against a 33 kbp one and a reverse-complemented infix; and the
    same pairs on 32-bit rows (AWV_F_NO_WIDE16)."""
    rseqs, _ = LP.row_width_pairs()
    rng = random.Random("dp/wide16")
    root = rand_seq(rng, 40000)
    seqs = rseqs[2:4] + [root, mutate(root, 0.01, rng)[:30000], mutate(root, 0.005, rng)[:32759], root[:33000],
                         rc(rseqs[3])]
    pairs = [(0, 1, 0), (1, 0, 0), (2, 3, 0), (3, 2, 0), (4, 5, 0), (5, 4, 0), (6, 0, 1)]
    assert all(min(len(seqs[p[0]]), len(seqs[p[1]])) < 32760 <= max(len(seqs[p[0]]), len(seqs[p[1]])) for p in pairs)
    for name, flags in (("wide16", ()), ("no_wide16", ("NO_WIDE16",))):
        e = _engine(_flags(*flags))
        try:
            dpc.align(e, seqs, pairs, DEFAULT_2P, "wide16/" + name)
        finally:
            e.close()
    dpc.finish()


def test_lds_chain_and_sub16(dpc):
    """70 kbp at 2-3 % (the inputs of test_unstaged_long_pairs_chain_through_lds): 32-bit rows, four waves, top levels too
    long to stage, the middle sweep of chained passes kept in LDS (compute_rows_multi's LCH), and the same with chaining off; and the
    150 kbp pair at 1.5 % of test_packed_probes_of_unstaged_sub_problems, whose sub-problems below 32,760 bases are searched
    with 16-bit rows inside the 32-bit launch (kp.sub16)."""
    rng = random.Random(1234)
    a = rand_seq(rng, 70000)
    seqs = [a, mutate(a, 0.02, rng), mutate(a, 0.03, rng)]
    pairs = [(0, 1), (1, 2), (2, 0)]
    for name, flags in (("lds_chain", ()), ("no_chain", ("NO_CHAIN",))):
        e = _engine(_flags(*flags))
        try:
            _, st = dpc.align(e, seqs, pairs, DEFAULT_2P, "70kbp/" + name)
            assert st.multi_cell_steps > 0.8 * st.cell_steps, (name, st.multi_cell_steps, st.cell_steps)
        finally:
            e.close()
    rng = random.Random(777)
    a = rand_seq(rng, 150000)
    e = _engine()
    try:
        dpc.align(e, [a, mutate(a, 0.015, rng)], [(0, 1), (1, 0)], DEFAULT_2P, "150kbp/sub16")
    finally:
        e.close()
    dpc.finish()


def test_probe_paths(dpc):
    """20 kbp pairs under one wave per pair (sub-problems too long for its staging region: in-place packed words,
    seq_mode 2) and under the engine's own choice (staged), the raw-byte probes (AWV_F_NO_PACKED_SEQ), a pair with an N and
    a lowercase stretch (raw bytes kept), and reverse-complemented queries (q_revcomp = 1)."""
    rng = random.Random("dp/probes")
    c = rand_seq(rng, 20000)
    f = mutate(c, 0.04, rng)
    n = bytearray(mutate(c, 0.03, rng))
    n[7000] = ord("N")
    n[12000:12400] = bytes(n[12000:12400]).lower()
    seqs = [c, mutate(c, 0.06, rng), rc(f), bytes(n), rc(f).lower()]
    pairs = [(0, 1, 0), (1, 0, 0), (2, 0, 1), (2, 1, 1), (3, 0, 0), (0, 3, 0), (4, 0, 1)]
    for name, flags in (("one_wave_in_place", ("ONE_WAVE",)), ("auto", ()), ("no_packed_seq", ("NO_PACKED_SEQ",)),
                        ("one_wave_no_packed_seq", ("ONE_WAVE", "NO_PACKED_SEQ"))):
        e = _engine(_flags(*flags))
        try:
            dpc.align(e, seqs, pairs, DEFAULT_2P, "probes/" + name)
        finally:
            e.close()
    dpc.finish()


@pytest.mark.parametrize("case", R.RESTART_CASES, ids=[c[0] for c in R.RESTART_CASES])
def test_restarts(dpc, case):
    """Searches that met inside a pass and were run again step by step: the restart path ran, and the penalty is the DP's."""
    name, gen, seed = case
    a, b = gen(random.Random(seed))
    for flags in ((), ("ONE_WAVE",)):
        e = _engine(_flags(*flags))
        try:
            _, st = dpc.align(e, [a, b], [(0, 1), (1, 0)], DEFAULT_2P, "restarts/" + name)
            assert st.restarts > 0, (seed, flags)
        finally:
            e.close()
    dpc.finish()


@pytest.mark.parametrize("scores,full", LP.ORACLE_SETS, ids=["%s%s" % (",".join(map(str, s)), "" if f else "/gaps")
                                                             for s, f in LP.ORACLE_SETS])
def test_long_repeats_and_forced_gaps(dpc, scores, full):
    """The inputs the oracle is held to in tests/test_gotoh_banded.py: 20-70 kbp pairs, the very unequal shapes, 12-40 kbp
    tandem arrays, 4.2 and 16.5 kbp copy deletions, forced gaps around the piece crossover and of 4 and 17 kbp."""
    e = _engine(0, scores)
    try:
        for name, seqs, pairs in LP.oracle_inputs(scores, full):
            dpc.align(e, seqs, pairs, scores, "long/" + name)
    finally:
        e.close()
    dpc.finish()


@pytest.mark.parametrize("name", PS.FLAVOUR_SETS)
def test_flavour_sets_on_every_row_width(dpc, name):
    """Every representative set on a 32-bit-row pair, a wide16 pair and a sixteen-wave pair (the inputs of
    test_long_pairs_on_every_row_width), and the 32-bit pair on one wave."""
    scores = PS.BY_NAME[name]
    seqs, pairs = LP.row_width_pairs()
    e = _engine(0, scores)
    try:
        dpc.align(e, seqs, pairs, scores, "flavour_sets/row_widths")
    finally:
        e.close()
    e = _engine(_flags("ONE_WAVE"), scores)
    try:
        dpc.align(e, seqs, pairs[:2], scores, "flavour_sets/one_wave32")
    finally:
        e.close()
    dpc.finish()


@pytest.mark.parametrize("scores", [DEFAULT_2P, EDIT])
def test_score_only(dpc, scores):
    """awv_score_pairs on the row-width pairs, the very unequal shapes, the forced gaps, the tandem arrays, the copy
    deletions and the restart cases (and the random long pairs at the default set): with no bound it returns the DP's
    penalty; with a bound B it reports AWV_ST_ABOVE_BOUND exactly where the DP bounded by B exceeds B."""
    groups = [("row_widths",) + LP.row_width_pairs(), ("very_unequal",) + LP.very_unequal(),
              ("forced_gaps",) + LP.forced_gaps(scores), ("long_tandem",) + LP.long_tandem(),
              ("cnv_deletions",) + LP.cnv_deletions()]
    groups.append(("restarts",) + LP.pair_list([gen(random.Random(seed)) for _, gen, seed in R.RESTART_CASES], True))
    if scores == DEFAULT_2P:
        groups.append(("random_long",) + LP.random_long())
    e = _engine(0, scores)
    try:
        for name, seqs, pairs in groups:
            pens, _ = dpc.align(e, seqs, pairs, scores, "score/" + name)
            dpc.score_only(e, seqs, pairs, scores, pens, "score/" + name)
    finally:
        e.close()
    dpc.finish()
