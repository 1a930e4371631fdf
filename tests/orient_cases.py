"""Inputs and the reference answer for the WFA-orientation tests (test_orient_rule_cpu.py, test_gpu_orient.py).

The reference's determine_orientation_wfa (alignment.rs:157-175): align the query and its reverse complement against the
target under the orientation penalties, E = #X + #I + #D of each CIGAR, forward iff E_f <= E_r.  `strand_facts` gets both
from the CPU oracle.  cmin / cmax are computed here from their definition, not read from the product."""
import random

from util import mutate, rand_seq

COMP = {65: 84, 84: 65, 67: 71, 71: 67, 97: 84, 116: 65, 99: 71, 103: 67}
RULE_SCORES = [(0, 1, 1, 1), (0, 2, 2, 2), (0, 3, 4, 1), (0, 4, 6, 2), (0, 5, 8, 2, 24, 1)]
HI_NONE = 2 ** 31 - 1


def rc(s):
    return bytes(COMP.get(b, 78) for b in reversed(s))


def cmin_cmax(scores):
    """every edit column of an optimal CIGAR adds at least cmin and at most cmax to the penalty"""
    s = list(scores)
    x, o1, e1 = s[1], s[2], s[3]
    if len(s) == 6:
        o2, e2 = s[4], s[5]
        return min(x, e1, e2), max(x, min(o1 + e1, o2 + e2))
    return min(x, e1), max(x, o1 + e1)


def edits(ops):
    return sum(1 for c in ops if c in b"XID")


def strand_facts(aligner, q, t):
    """((P_f, E_f), (P_r, E_r)) of the oracle's alignments of q and of rc(q) against t"""
    pf, of = aligner.align(q, t)
    pr, orr = aligner.align(rc(q), t)
    return (pf, edits(of)), (pr, edits(orr))


def rule_pairs(n, seed):
    """n random (query, target) pairs: lengths 50 - 2,000, divergence 0 - 40 %, half the queries reverse-complemented, some
    unrelated, some with an empty or one-base side, and the ties: identical and palindromic inputs."""
    rng = random.Random(seed)
    out = [(b"ACGT" * 25, b"ACGT" * 25), (b"ACGT" * 100, b"ACGT" * 100), (b"AATT" * 40, b"AATT" * 40), (b"GAATTC", b"GAATTC")]
    while len(out) < n:
        u = rng.random()
        m = int(round(50 * 40 ** rng.random()))  # 50 .. 2,000, log-uniform
        a = rand_seq(rng, m)
        if u < 0.08:
            b = rand_seq(rng, rng.choice([0, 1, 1, 0, 2]))
            q, t = (a, b) if rng.random() < 0.5 else (b, a)
        elif u < 0.2:
            q, t = a, rand_seq(rng, max(50, min(2000, int(m * rng.uniform(0.5, 1.5)))))
        else:
            q, t = mutate(a, rng.uniform(0.0, 0.4), rng), a
        if rng.random() < 0.5:
            q = rc(q)
        out.append((q, t))
    return out


def reads(rng, n, length, d):
    """n reads of ~`length` bases, pairwise divergence ~d (each one the root mutated at d / 2), every second one
    reverse-complemented"""
    root = rand_seq(rng, length)
    out = []
    for i in range(n):
        r = mutate(root, d / 2, rng)
        out.append(rc(r) if i % 2 else r)
    return out


def all_pairs(lo, hi):
    return [(i, j) for i in range(lo, hi) for j in range(lo, hi) if i != j]


def oracle_strands(oracle, seqs, pairs, scores):
    """per pair ((P_f, E_f), (P_r, E_r)) and the reference's answer: reverse iff not E_f <= E_r"""
    al = oracle.Aligner(scores)
    facts = [strand_facts(al, seqs[p[0]], seqs[p[1]]) for p in pairs]
    return facts, [0 if f[1] <= r[1] else 1 for f, r in facts]
