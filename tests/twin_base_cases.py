"""Inputs of the shared-base-case tests: tests/test_twin_base_cpu.py (the mirror rule of
allwave_amd/csrc/twin_base.hpp, proved with a scalar WFA on the CPU) and tests/test_gpu_twin_base.py (the kernel that runs a
twin unit's base case once and backtraces it for both orientations)."""
import random

import repeats as R
import twin_cases as TC
from util import mutate, rand_seq

SCORE_CAP = 250          # FALLBACK_MIN_SCORE: a sub-problem that costs at most this much is a base case
MIN_LENGTH = 100         # FALLBACK_MIN_LENGTH: a pair of at most this length is a base case whatever it costs
C_M, C_I1, C_I2, C_D1, C_D2 = range(5)      # components as the kernels number them

#: the penalty sets of the CPU proof
CPU_SETS = ((0, 5, 8, 2, 24, 1), (0, 4, 6, 2, 26, 1), (0, 1, 1, 1), (0, 3, 4, 1), (0, 6, 5, 3))

_SMALL_RUNS = (3, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def _clip(ab, n=400):
    a, b = ab
    return a[:n], b[:n]


def tie_rich_small(rng):
    """One pair of each tie-rich family of tests/repeats.py at base-case size: both lengths 1-400."""
    return [_clip(R.microsatellite(rng, flank=(5, 120))),
            _clip(R.tandem(rng, total=(120, 380), unit_len=rng.randint(8, 60), flank=(0, 20))),
            _clip(R.end_runs(rng, body=(20, 250), lengths=_SMALL_RUNS)),
            _clip(R.low_complexity(rng, n=(20, 380)))]


def rotated(rng):
    """A periodic sequence against the same period rotated by half of it, some between shared random flanks: the shift costs one
    insertion and one deletion of half a period each, and which of the two comes first is a tie -- the backtrace decides it by
    its candidate order, which prefers a deletion in either orientation.  So the swapped pair's ops are not the I/D swap,
    under every penalty set.  (Flanks, more copies on one side or a little noise, which some draws get, may undo the tie.)"""
    period = rand_seq(rng, rng.choice((2, 2, 4, 6)))
    while len(set(period)) < 2:
        period = rand_seq(rng, len(period))
    off = len(period) // 2
    reps = max(4, rng.randint(20, 300) // len(period))
    flank = rng.random() < 0.3
    left, right = rand_seq(rng, rng.randint(0, 25) if flank else 0), rand_seq(rng, rng.randint(0, 25) if flank else 0)
    a = left + period * reps + right
    b = left + (period[off:] + period[:off]) * (reps + rng.choice((0, 0, 0, 0, 0, 0, 1, 2))) + right
    if rng.random() < 0.15:
        b = mutate(b, 0.01, rng)
    return _clip((a, b) if rng.random() < 0.5 else (b, a))


def replaced_block(rng):
    """A block of 30-70 bases replaced by an unrelated one of another length: an insertion next to a deletion wherever two
    gaps cost less than the mismatches."""
    s = rand_seq(rng, rng.randint(40, 300))
    cut = rng.randrange(len(s) + 1)
    a = s[:cut] + rand_seq(rng, rng.randint(30, 70)) + s[cut:]
    b = s[:cut] + rand_seq(rng, rng.randint(30, 70)) + s[cut:]
    return _clip((a, mutate(b, 0.01, rng)))


def plain_small(rng):
    """Mutated copies and unequal lengths, 1-400 bases: a few per call, among them one base against many and a forced gap."""
    out = []
    for n in (1, 2, rng.randint(3, 30), rng.randint(31, 100), rng.randint(101, 400)):
        s = rand_seq(rng, n)
        out.append((s, mutate(s, rng.choice((0.0, 0.02, 0.05, 0.1)), rng)[:400] or b"A"))
    s = rand_seq(rng, rng.randint(20, 200))
    cut = rng.randrange(len(s) + 1)
    out.append((s, s[:cut] + rand_seq(rng, rng.randint(1, 150)) + s[cut:]))
    out.append((rand_seq(rng, 1), rand_seq(rng, rng.randint(1, 60))))
    return out


def cpu_pairs(seed):
    """The unordered pairs of the CPU proof before the penalty filter: every tie-rich family, rotated periods, replaced
    blocks and the plain shapes, 30 draws."""
    rng = random.Random("twin-base-cpu/%s" % (seed,))
    ab = []
    for _ in range(30):
        ab += tie_rich_small(rng)
        ab += [rotated(rng), rotated(rng), rotated(rng), replaced_block(rng)]
        ab += plain_small(rng)
    return ab


def gap_components(scores):
    return (C_M, C_I1, C_D1, C_I2, C_D2) if len(scores) == 6 else (C_M, C_I1, C_D1)


# ---- GPU inputs

def indel_rich(rng, n, gaps):
    """A low-divergence pair with long insertions and deletions every 60-200 bases: breakpoints fall inside them, so the
    base cases on either side begin / end in a gap component (the idea of tests/test_gpu_base_case.py at 300-1500 bp)."""
    a = rand_seq(rng, n)
    b = bytearray()
    i = 0
    while i < n:
        step = rng.randrange(60, 200)
        b += a[i:i + step]
        i += step
        g = rng.choice(gaps)
        if rng.random() < 0.5:
            i += g
        else:
            b += rand_seq(rng, g)
    return a, mutate(bytes(b), 0.01, rng)


def top_level_pairs():
    """Pairs of at most 100 bases -- the FALLBACK_MIN_LENGTH route: the top task is a base case whatever it costs --, equal and
    unequal lengths, identical sequences, one base against many, unrelated sequences."""
    rng = random.Random("twin-base/top")
    ab = []
    for n in (1, 2, 3, 17, 63, 64, 65, 99, 100):
        s = rand_seq(rng, n)
        ab.append((s, mutate(s, 0.1, rng)[:100] or b"C"))
    s = rand_seq(rng, 100)
    ab += [(s, s), (s[:1], s), (s[:40], s), (b"A", b"C"), (b"G", b"G"), (rand_seq(rng, 90), rand_seq(rng, 100)),
           (s[:30] + s[70:], s)]
    ab += [_clip(p, 100) for p in tie_rich_small(rng)]
    return TC.both_orders(ab)


def gap_component_pairs():
    """300-1500 bp with indels of both gap pieces close together."""
    rng = random.Random("twin-base/gaps")
    ab = [indel_rich(rng, n, gaps) for n, gaps in ((360, (12, 30)), (700, (12, 30, 60)), (1000, (40, 90, 220)), (1500, (15, 25, 120)),
                                                   (900, (100, 180)), (1200, (5, 9, 14)))]
    return TC.both_orders([(a[:1500], b[:1500]) for a, b in ab])


TIE_SEED = 5            # chosen on the CPU for the condition tests/test_gpu_twin_base.py asserts from the oracle
TIE_MIN_NOT_MIRRORED = 8


def rotated_long(rng):
    """rotated() at 300-1400 bases, without flanks, the second sequence 5-20 % from the rotated array in its own alphabet."""
    period = rand_seq(rng, rng.choice((2, 4, 6)))
    while len(set(period)) < 2:
        period = rand_seq(rng, len(period))
    off = len(period) // 2
    reps = rng.randint(300, 1400) // len(period)
    return period * reps, mutate((period[off:] + period[:off]) * reps, rng.uniform(0.05, 0.2), rng, bytes(set(period)))[:1500]


def tie_rich_pairs():
    """16 tie-rich pairs at 300-1500 bp, 5-20 % apart: microsatellites or low complexity, tandem arrays, homopolymer ends
    and rotated periods, four of each."""
    rng = random.Random("twin-base/ties/%d" % TIE_SEED)
    ab = []
    for i in range(4):
        if i % 2:
            a = rand_seq(rng, rng.randint(300, 1000), b"AT")
            ab.append((a, mutate(a, rng.uniform(0.05, 0.2), rng, b"AT")[:1500]))
        else:
            a, b = R.microsatellite(rng, flank=(150, 500))
            ab.append((a, mutate(b, rng.uniform(0.05, 0.2), rng)[:1500]))
        a, b = R.tandem(rng, total=(400, 1300), unit_len=rng.randint(8, 80), flank=(0, 100))
        ab.append((a[:1500], mutate(b, rng.uniform(0.05, 0.1), rng)[:1500]))
        a, b = R.end_runs(rng, body=(300, 1200), lengths=_SMALL_RUNS)
        ab.append((a, mutate(b, rng.uniform(0.05, 0.12), rng)))
        ab.append(rotated_long(rng))
    return TC.both_orders(ab)


def forced_gap_pairs():
    """Very unequal lengths whose whole alignment costs less than 250: one forced gap of 120-200 bases next to 40-120 bases
    that match -- the wavefronts run off the short side, a pass is discarded and the base case goes on step by step with
    trimmed rows, k_end != 0 (tests/test_gpu_base_case.py::test_forced_gap_trims_rows_inside_a_base_case, both orders)."""
    rng = random.Random("twin-base/forced")
    ab = []
    for short, gap in ((40, 200), (60, 200), (90, 160), (120, 120), (101, 140)):
        s = rand_seq(rng, short)
        cut = rng.randrange(0, short + 1)
        t = s[:cut] + rand_seq(rng, gap) + s[cut:]
        ab += [(s, t), (mutate(t, 0.01, rng), s)]
    return TC.both_orders(ab)


def with_an_n():
    """The first pairs of gap_component_pairs with an N in one sequence: no 2-bit packed view, raw-byte probes."""
    seqs, pairs = gap_component_pairs()
    seqs = [bytes(s) for s in seqs[:6]]
    seqs[0] = seqs[0][:100] + b"N" + seqs[0][101:]
    seqs[3] = seqs[3][:57] + b"N" + seqs[3][58:]
    return seqs, pairs[:6]
