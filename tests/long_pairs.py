"""Seeded long pairs (20-150 kbp, forced gaps of up to 17 kbp, long repeat arrays) for the checks against the banded Gotoh DP
(oracle/gotoh.c, awo_gotoh_penalty_banded), shared by the CPU tests of the oracle and the GPU tests of every kernel path.

The banded DP costs about min(plen, tlen) * (|dl| + 2m) cells, where m is the largest margin with g(|dl| + 2m) <= the
penalty: low-divergence long pairs and long forced gaps stay cheap, divergent long pairs do not.  Every builder returns
(seqs, pairs) with pairs as (q_idx, t_idx) index tuples.
"""
import random

import penalty_space as PS
import repeats as R
from util import DEFAULT_2P, EDIT, mutate, rand_seq


def pair_list(ab, both_orders=False):
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        k = len(seqs) - 2
        pairs.append((k, k + 1))
        if both_orders:
            pairs.append((k + 1, k))
    return seqs, pairs


def crossover(scores):
    """The gap length at which a 2-piece set's second piece becomes the cheaper one (None: the pieces never cross at a
    positive length, or the set is gap-affine)."""
    s = [int(v) for v in scores]
    if len(s) != 6 or s[3] == s[5]:
        return None
    L = (s[4] - s[2]) / (s[3] - s[5])
    return int(L) if L > 0 else None


def random_long(seed="long/random"):
    """20-70 kbp pairs at 1-3 % (util.mutate: substitutions and 1-base indels)."""
    rng = random.Random(seed)
    ab = []
    for n, d in ((20000, 0.03), (35000, 0.01), (50000, 0.02), (70000, 0.01)):
        a = rand_seq(rng, n)
        ab.append((a, mutate(a, d, rng)))
    return pair_list(ab)


def very_unequal():
    """The shapes of test_very_unequal_lengths: a 1.5 kbp infix of a 19 kbp sequence (dl = 17.5 k) and a 13 kbp prefix
    (dl = 6 k), both 4 % diverged, both orders."""
    rng = random.Random(31337)
    a = rand_seq(rng, 19000)
    b = mutate(a, 0.04, rng)[7000:8500]
    c = mutate(a, 0.04, rng)[:13000]
    return [a, b, c], [(1, 0), (0, 1), (2, 0), (0, 2)]


def long_tandem(seed="long/tandem"):
    """Tandem arrays of 12-40 kbp: a 171 b unit and a random one."""
    rng = random.Random(seed)
    return pair_list([R.tandem(rng, total=(12000, 20000), unit_len=171), R.tandem(rng, total=(30000, 40000))])


def cnv_deletions(seed="long/cnv"):
    """One copy of a 4.2 kbp and of a 16.5 kbp unit deleted from a tandem array of it: a forced gap of that length inside
    sequence that matches on both sides of it at every copy."""
    rng = random.Random(seed)
    return pair_list([R.cnv_deletion(rng, 4200, 4), R.cnv_deletion(rng, 16500, 3)])


def forced_gaps(scores, seed="long/gaps"):
    """A 12 kbp sequence at 0.5 % against itself with one gap: one base short of, at and one base past the set's piece
    crossover length (where there is one), and 4,096 and 17,000 bases -- the breakpoint of a BiWFA level falls inside a
    long gap.  Deletions and insertions alternate."""
    rng = random.Random("%s/%s" % (seed, tuple(scores)))
    lengths = [4096, 17000]
    L = crossover(scores)
    if L is not None:
        lengths = [max(1, L - 1), L, L + 1] + lengths
    ab = []
    for i, g in enumerate(lengths):
        a = rand_seq(rng, 12000 + g)
        cut = rng.randint(2000, 9000)
        b = mutate(a[:cut] + a[cut + g:], 0.005, rng)
        ab.append((a, b) if i % 2 == 0 else (b, a))
    return pair_list(ab)


def oracle_inputs(scores, full):
    """What the oracle is checked on at a set: the forced gaps always; with full, also the random long pairs, the very
    unequal shapes, the tandem arrays and the copy deletions.  Returns [(name, seqs, pairs)]."""
    out = [("forced_gaps", *forced_gaps(scores))]
    if full:
        out += [("random_long", *random_long()), ("very_unequal", *very_unequal()), ("long_tandem", *long_tandem()),
                ("cnv_deletions", *cnv_deletions())]
    return out


# (penalty set, full): every input at the default and the edit sets, the forced gaps and one tandem set at a handful of
# the representatives of penalty_space.FLAVOUR_SETS (a chain of two sweeps, an inverted and a crossing 2-piece set, the
# deepest ring, a gap-affine set with e = 2 and the widest base-case history)
ORACLE_SETS = [(DEFAULT_2P, True), (EDIT, True)] + [(PS.BY_NAME[n], False) for n in
                                                    ("2p_chain2", "2p_inverted", "2p_crossing_at_5", "ring256_2p_chain3",
                                                     "affine_T2_e2", "sb4000")]


def row_width_pairs():
    """A 32-bit-row pair (both >= 32760), a wide16 pair (shorter < 32760, longer >= 32760) and a sixteen-wave pair
    (length difference >= 16384), both orders of each."""
    rng = random.Random("gpu-penalties/long")
    a = rand_seq(rng, 33500)
    b = mutate(a, 0.003, rng)
    c = rand_seq(rng, 36000)
    d = mutate(c[9000:12000], 0.01, rng)
    g = rand_seq(rng, 3000)
    h = mutate(g[:1500] + rand_seq(rng, 16500) + g[1500:], 0.003, rng)
    assert min(len(a), len(b)) >= 32760 and min(len(c), len(d)) < 32760 <= max(len(c), len(d))
    assert abs(len(g) - len(h)) >= 16384
    seqs = [a, b, c, d, g, h]
    return seqs, [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4)]
