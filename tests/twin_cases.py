"""Inputs and comparisons shared by the twin-unit tests: tests/test_twin_plan_cpu.py, tests/test_gpu_twin.py,
tests/test_twin_space_cpu.py and tests/test_gpu_twin_space.py.  A pair list that exercises the pairing of an entry (q, t)
with its swapped entry (t, q) (allwave_amd/csrc/twin_plan.hpp), both-order lists over the penalty space, the sequences of
the re-run, routing and long-read cases, and the record-by-record comparisons against the CPU oracle."""
import random

import penalty_space as PS
import repeats as R
from util import mutate, rand_seq

SWAP = bytes.maketrans(b"ID", b"DI")
_RC = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


def rc(s):
    return bytes(s).translate(_RC)[::-1]


def same_records(a, b):
    ra, ca = a
    rb, cb = b
    for name in ra.dtype.names:
        assert (ra[name] == rb[name]).all(), name
    assert ca == cb


_ORACLE = {}


def oracle_records(oracle, seqs, pairs, scores, key=None):
    """(penalty, ops) of every entry, a q_revcomp entry's query reverse-complemented.  key: computed once per (key, scores)
    and shared by every test that runs the input; the cached list is never changed."""
    k = (key, tuple(scores))
    if key is not None and k in _ORACLE:
        return _ORACLE[k]
    al = oracle.Aligner(scores)
    out = []
    for p in pairs:
        q = rc(seqs[p[0]]) if len(p) > 2 and p[2] else seqs[p[0]]
        out.append(al.align(q, seqs[p[1]]))
    if key is not None:
        _ORACLE[k] = out
    return out


def check_records(got, want, seqs, pairs):
    """Every field of every record and every op byte against the oracle's (penalty, ops)."""
    res, cigs = got
    for i, (pen, ops) in enumerate(want):
        assert res["status"][i] == 0 and res["penalty"][i] == pen and res["score"][i] == -pen, (i, pairs[i])
        assert cigs[i] == ops and res["cigar_len"][i] == len(ops), (i, pairs[i])
        c = [ops.count(k) for k in b"MXID"]
        assert [res["num_matches"][i], res["num_mismatches"][i], res["num_ins"][i], res["num_del"][i]] == c, (i, pairs[i])
        assert res["q_end"][i] == c[0] + c[1] + c[3] == len(seqs[pairs[i][0]]), (i, pairs[i])
        assert res["t_end"][i] == c[0] + c[1] + c[2] == len(seqs[pairs[i][1]]), (i, pairs[i])


def check_scores(got, want, pairs):
    """A score-only call's records against the oracle's penalties."""
    for i, (pen, _) in enumerate(want):
        assert got["status"][i] == 0 and got["penalty"][i] == pen, (i, pairs[i], int(got["penalty"][i]), pen)


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


def both_orders(ab):
    """[(a, b)] -> sequences a0, b0, a1, b1, ... and the list (0, 1), (1, 0), (2, 3), (3, 2), ...: every pair and its twin."""
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs += [(len(seqs) - 2, len(seqs) - 1), (len(seqs) - 1, len(seqs) - 2)]
    return seqs, pairs


def twelve():
    """12 sequences of 1.2-3 kbp, 3-15 % apart, the first of 1.5 kbp: their 132 directed pairs = 66 twin units; and one
    more pair, the 1.5 kbp sequence against one of 5 kbp, listed in one direction only."""
    rng = random.Random("twin-twelve")
    base = rand_seq(rng, 5000)
    lens = [1500] + [rng.randint(1200, 3000) for _ in range(11)] + [5000]
    seqs = [mutate(base[:n], rng.uniform(0.015, 0.075), rng) for n in lens]  # two mutated copies: 3-15 % between them
    pairs = [(i, j) for i in range(12) for j in range(12) if i != j] + [(0, 12)]
    return seqs, pairs


#: the sets of penalty_space.ACCEPTED under which the oracle breaks ties differently in the two orders of most pairs of
#: penalty_inputs, with the count of such pairs (of 12) the inputs must keep (tests/test_twin_space_cpu.py)
TIE_RICH = ("affine_e3_o0", "2p_T2", "2p_o2_zero", "2p_piece1_never", "scope101_T5", "scope125", "ring256_scope126_T4")
TIE_RICH_MIN = 7
TIE_TOTAL_MIN = 80


#: sets under which no pair of the 12 above costs enough for a search below the top level (tests/test_twin_space_cpu.py,
#: from the oracle alone: second_level): each gets DEEP_EXTRA more divergent pairs, so that "a search below the top level ran
#: shared" can be asked of every set
DEEP_SETS = ("edit_unit", "edit_allwave", "affine_T2_x2", "2p_o2_zero", "scope125")
DEEP_EXTRA = 4


def second_level(scores, penalty):
    """Whether a pair of this penalty has a breakpoint search below the top level whatever its breakpoint: the halves'
    scores add up to the penalty (an indel breakpoint pays its open twice at most), and a half above FALLBACK_MIN_SCORE is
    searched again."""
    d = PS.derive(scores)
    return penalty > 2 * PS.FALLBACK_MIN_SCORE + 2 * max(d.o1, d.o2)


def penalty_inputs(name, unordered=None):
    """The both-order list of one accepted penalty set: six random pairs of 0.8-2.5 kbp, 3-12 % apart, then two
    microsatellite pairs, a tandem array, two pairs with homopolymer ends and a low-complexity pair -- 12 unordered pairs,
    24 entries, seeded by the set's name; under the DEEP_SETS four more pairs of 4 kbp, 20 % apart, follow them.
    unordered: only the first so many pairs."""
    rng = random.Random("twin-penalties/" + name)
    ab = []
    for _ in range(6):
        s = rand_seq(rng, rng.randint(800, 2500))
        ab.append((s, mutate(s, rng.uniform(0.03, 0.12), rng)))
    ab += [R.microsatellite(rng), R.microsatellite(rng), R.tandem(rng, total=(1500, 3000)), R.end_runs(rng), R.end_runs(rng),
           R.low_complexity(rng, n=(200, 1500))]
    if name in DEEP_SETS:
        rng = random.Random("twin-penalties/deep/" + name)
        for _ in range(DEEP_EXTRA):
            s = rand_seq(rng, 4000)
            ab.append((s, mutate(s, 0.2, rng)))
    return both_orders(ab[:unordered])


def not_mirrored(want):
    """Of a both-order list's oracle records: the unordered pairs whose (j, i) CIGAR is not the I/D swap of the (i, j) one."""
    return sum(1 for k in range(0, len(want), 2) if want[k + 1][1] != want[k][1].translate(SWAP))


def rerun_inputs():
    """The four sequences of test_gpu_parity.py::test_narrow_first_attempt_is_rerun_with_wider_rows -- 6 kbp, copies 8 % and
    1 % away, an unrelated 1.5 kbp -- and their 12 directed pairs: with rows capped at 2048 columns the divergent pairs end
    CAPACITY in the first launch and are re-run wider."""
    rng = random.Random(4242)
    a = rand_seq(rng, 6000)
    seqs = [a, mutate(a, 0.08, rng), mutate(a, 0.01, rng), rand_seq(rng, 1500)]
    return seqs, [(i, j) for i in range(4) for j in range(4) if i != j]


def interleaved(n):
    """The unordered pairs of n sequences, each followed by its twin: (0, 1), (1, 0), (0, 2), (2, 0), ..."""
    out = []
    for i in range(n):
        for j in range(i + 1, n):
            out += [(i, j), (j, i)]
    return out


ROUTING_NSEQ = 66


def routing_inputs():
    """66 sequences of 300-450 bases, each 2-6 % from one base: 4,290 directed pairs of even cost, one batch."""
    rng = random.Random("twin-routing")
    base = rand_seq(rng, 450)
    seqs = [mutate(base[:rng.randint(300, 450)], rng.uniform(0.02, 0.06), rng) for _ in range(ROUTING_NSEQ)]
    n = ROUTING_NSEQ
    return seqs, [(i, j) for i in range(n) for j in range(n) if i != j]


LAST_16BIT_LENGTH = 32759   # engine.hip: 16-bit rows while both lengths are below 32,760


def long_read_inputs():
    """Three long pairs 2-3 % apart, both orders: both sequences of exactly 32,759 bases (the last length on 16-bit rows);
    24 kbp against 30 kbp; 9 kbp against 24 kbp (one sequence is staged in LDS, the other is not).  The shorter sequence
    of the unequal pairs is a copy of a slice from the middle of the longer one."""
    rng = random.Random("twin-long-reads")

    def exact(s, n):  # a mutated copy brought to exactly n bases at its end
        return s[:n] if len(s) >= n else s + rand_seq(rng, n - len(s))

    a = rand_seq(rng, LAST_16BIT_LENGTH)
    b = exact(mutate(a, 0.025, rng), LAST_16BIT_LENGTH)
    c = rand_seq(rng, 30000)
    d = exact(mutate(c[3000:27100], 0.02, rng), 24000)
    e = rand_seq(rng, 24000)
    f = exact(mutate(e[7000:16050], 0.03, rng), 9000)
    return both_orders([(a, b), (d, c), (f, e)])
