"""Cases for the bounded-alignment tests (test_bounded_cpu.py, test_gpu_bounded.py): the seeded pair list, the bounds tried
around each pair's penalty, the contract of awv_align_pairs_bounded as one check, and plain Python versions of the divergence
bound and the divergence filter to compare against."""
import math
import random

import numpy as np

from util import DEFAULT_2P, EDIT, mutate, rand_seq
from verify_cases import expand_cg, rescore, revcomp

AFFINE_1P = (0, 4, 6, 2)
SCORE_SETS = (DEFAULT_2P, EDIT, AFFINE_1P)
DIVERGENCES = (0, 0.01, 0.05, 0.1, 0.3, 0.6, 0.99)
#: the bounds tried on a pair of penalty P
BOUND_KINDS = ("zero", "p_minus_1", "p", "p_plus_1", "two_p", "none")
RECORD_ZERO_FIELDS = ("cigar_len", "num_matches", "num_mismatches", "num_ins", "num_del", "q_end", "t_end")


def bound_of(kind, p):
    """The bound of `kind` for a pair of penalty p (-1: unbounded).  P = 0 has no bound below it: P - 1 is then 0 too."""
    return {"zero": 0, "p_minus_1": max(p - 1, 0), "p": p, "p_plus_1": p + 1, "two_p": 2 * p, "none": -1}[kind]


def cmax(scores):
    gap = scores[2] + scores[3]
    if len(scores) == 6:
        gap = min(gap, scores[4] + scores[5])
    return max(scores[1], gap)


def divergence_bound(scores, plen, tlen, d):
    """The closed form of include/allwave_hip.h: cmax * (floor(d (plen + tlen) / (2 - d)) + 1); -1: no bound."""
    if d >= 1:
        return -1
    b = cmax(scores) * (math.floor(d * (plen + tlen) / (2.0 - d)) + 1)
    return -1 if b > 2 ** 31 - 1 else b


def edits_columns(ops):
    """(#X + #I + #D, columns) of op bytes."""
    return len(ops) - ops.count(b"M"), len(ops)


def within_divergence(ops, d):
    """The filter of AllPairIterator::with_max_divergence: (double)E <= d * (double)columns."""
    e, c = edits_columns(ops)
    return float(e) <= d * float(c)


def paf_ops(line):
    """The op bytes of a PAF line's cg:Z: tag."""
    return expand_cg(line.split("\t")[-1][len("cg:Z:"):])


def paf_penalty(scores, line):
    """The penalty of a PAF line (its op string re-scored: the alignment is optimal, so this is the pair's penalty)."""
    return rescore(scores, paf_ops(line))


# ---- the pair list --------------------------------------------------------------------------------------------------------
#: name -> index into pairs() / what the case is there for
CASE_NAMES = ("2k_1pct", "2k_5pct", "2k_12pct", "identical", "base_case_top", "forced_gap", "unrelated_1k", "revcomp", "with_n",
              "sixteen_waves")


def cases():
    """(seqs, pairs): pairs[i] = (q, t, q_revcomp) is the case CASE_NAMES[i]."""
    rng = random.Random("bounded/cases")
    a = rand_seq(rng, 2000)
    seqs, pairs = [a], []

    def add(q, t=0, rc=0):
        seqs.append(q)
        pairs.append((len(seqs) - 1, t, rc))

    for d in (0.01, 0.05, 0.12):          # P above 250: the top level searches and recurses
        add(mutate(a, d, rng))
    add(bytes(a))                          # P = 0
    s80 = rand_seq(rng, 80)                # both lengths <= 100: the top level is a base case
    seqs.append(s80)
    add(mutate(s80, 0.1, rng)[:100], len(seqs) - 1)
    add(mutate(a[700:1000], 0.03, rng))    # 300 bp against 2 kbp: a forced gap, BP_END_REACHED candidates
    u = rand_seq(rng, 1000)                # two unrelated sequences
    seqs.append(u)
    add(rand_seq(rng, 1000), len(seqs) - 1)
    add(revcomp(mutate(a, 0.05, rng)), 0, 1)
    n = bytearray(mutate(a, 0.05, rng))    # an 'N': the raw-byte path
    n[1000] = ord("N")
    add(bytes(n))
    long_t = rand_seq(rng, 17000)          # 200 bp against 17 kbp: the sixteen-wave flavour
    seqs.append(long_t)
    add(mutate(long_t[8000:8200], 0.02, rng), len(seqs) - 1)
    assert len(pairs) == len(CASE_NAMES)
    return seqs, pairs


def case_index(*names):
    return [CASE_NAMES.index(n) for n in names]


def bound_arrays(pens):
    """{name: int32 array, one bound per pair}: every bound kind for all pairs at once, and a mixed array in which
    neighbouring pairs get different kinds (rotated once, so that every pair meets two kinds in mixed company)."""
    pens = [int(p) for p in pens]
    out = {k: np.array([bound_of(k, p) for p in pens], dtype=np.int32) for k in BOUND_KINDS}
    for shift in (0, 3):
        out["mixed%d" % shift] = np.array([bound_of(BOUND_KINDS[(i + shift) % len(BOUND_KINDS)], p) for i, p in enumerate(pens)], dtype=np.int32)
    return out


def check_contract(ffi, bounds, res, cigs, sc, ref_res, ref_cigs, where=""):
    """The contract of awv_align_pairs_bounded (include/allwave_hip.h) for one call: `res`, `cigs` its records and op bytes
    under `bounds`, `sc` the score-only records under the same bounds, `ref_res` / `ref_cigs` the unbounded call's."""
    for i, b in enumerate(bounds):
        b, p = int(b), int(ref_res["penalty"][i])
        ctx = (where, i, b, p)
        assert ref_res["status"][i] == ffi.AWV_ST_COMPLETED, ctx
        assert (res["status"][i], res["penalty"][i]) == (sc["status"][i], sc["penalty"][i]), ctx + (int(res["status"][i]), int(res["penalty"][i]))
        if b < 0 or p <= b:
            assert res["status"][i] == ffi.AWV_ST_COMPLETED, ctx
            assert res[i].tobytes() == ref_res[i].tobytes(), ctx + (res[i], ref_res[i])
            assert cigs[i] == ref_cigs[i], ctx
        else:
            assert res["status"][i] == ffi.AWV_ST_ABOVE_BOUND, ctx + (int(res["status"][i]),)
            assert res["penalty"][i] == b + 1 and res["score"][i] == -(b + 1), ctx
            for f in RECORD_ZERO_FIELDS:
                assert res[f][i] == 0, ctx + (f, int(res[f][i]))
            assert cigs[i] is None, ctx
