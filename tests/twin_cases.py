"""Inputs shared by tests/test_twin_plan_cpu.py and tests/test_gpu_twin.py: a pair list that exercises the pairing of an
entry (q, t) with its swapped entry (t, q) (allwave_amd/csrc/twin_plan.hpp)."""
import random

from util import mutate, rand_seq


def pairing_sequences():
    """0-5: related 1.2-2 kbp sequences; 6: empty; 7, 8: identical; 9, 10: 60 and 100 bases; 11: 90 bases."""
    rng = random.Random("twin-pairing")
    base = rand_seq(rng, 1600)
    seqs = [mutate(base, d, rng) for d in (0.0, 0.03, 0.06, 0.1, 0.04, 0.08)]
    seqs.append(b"")
    same = mutate(base, 0.05, rng)[:1300]
    seqs += [same, same]
    short = rand_seq(rng, 100)
    seqs += [mutate(short, 0.1, rng)[:60], short, mutate(short, 0.05, rng)[:90]]
    return seqs


#: (q, t, q_revcomp); the comments say what the pairing must do with the entry
PAIRING_LIST = [
    (0, 1, 0), (1, 0, 0),      # a pair and its twin
    (0, 2, 0),                 # the twin is missing
    (3, 3, 0),                 # (i, i): never a twin unit
    (2, 3, 0), (2, 3, 0), (3, 2, 0),  # listed twice, one twin: one copy stays single
    (4, 5, 0), (4, 5, 0),      # listed twice without a twin
    (1, 2, 1), (2, 1, 1), (1, 2, 0), (2, 1, 0),  # q_revcomp entries next to their plain versions: only the plain ones pair
    (0, 6, 0), (6, 0, 0),      # an empty sequence
    (6, 6, 0),
    (7, 8, 0), (8, 7, 0),      # identical sequences: BP_END_REACHED at the top
    (9, 10, 0), (10, 9, 0), (11, 9, 0), (9, 11, 0),  # both lengths <= 100: the min-length base case
    (5, 0, 0), (3, 4, 0), (0, 5, 0),   # twins far apart in the list
    (1, 4, 1), (4, 1, 0),      # a q_revcomp entry and a plain swapped one: single both
]


def check_plan(entries, units):
    """units: [(first, twin)] as the pairing returns them.  Every entry in exactly one unit, twins are true swaps of plain
    entries with q != t, and no twin was left unused: among the single units no two are swaps of each other."""
    seen = []
    for f, w in units:
        seen.append(f)
        if w >= 0:
            seen.append(w)
            (q, t, rc), (q2, t2, rc2) = entries[f], entries[w]
            assert rc == 0 and rc2 == 0 and q != t and (q2, t2) == (t, q), (entries[f], entries[w])
            assert f < w
    assert sorted(seen) == list(range(len(entries)))
    firsts = [f for f, _ in units]
    assert firsts == sorted(firsts)  # units keep the order of their first entries
    single = [entries[f] for f, w in units if w < 0 and entries[f][2] == 0 and entries[f][0] != entries[f][1]]
    keys = set((q, t) for q, t, _ in single)
    assert not any((t, q) in keys for q, t in keys), "two single units are swaps of each other"
