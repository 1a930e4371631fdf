"""Inputs of the row-reuse tests (tests/test_gpu_row_reuse.py): pairs whose level-1 searches are long enough
to run multi-step passes -- 3-4 kbp, 5-20 % apart, so that a half exceeds AWV_MIN_PASS_LEN and 250 in score -- and pairs on
which the archived rows leave a child's box early.  Every builder is seeded and returns (sequences, pair list)."""
import random

import repeats as R
from util import mutate, rand_seq

DEFAULT_2P = (0, 5, 8, 2, 24, 1)
AFFINE = (0, 4, 6, 2)        # one piece, passes of 4 scores
EDIT = (0, 1, 1, 1)          # no multi-step passes at all: nothing to archive


def _pair(seed, n, d):
    rng = random.Random("row-reuse/%s" % seed)
    s = rand_seq(rng, n)
    return mutate(s, d / 2, rng), mutate(s, d / 2, rng)


def twin_unit(d=0.10, n=3500, seed="twin"):
    """One pair in both orders: a twin unit (shared top-level search, children in A's frame)."""
    a, b = _pair("%s/%g" % (seed, d), n, d)
    return [a, b], [(0, 1), (1, 0)]


def alone(d=0.10, n=3500, seed="twin"):
    """The same pair listed once: no unit, the plain tree."""
    a, b = _pair("%s/%g" % (seed, d), n, d)
    return [a, b], [(0, 1)]


def divergences():
    """3-4 kbp pairs at 5, 10 and 20 %, each in one order."""
    seqs, pairs = [], []
    for i, d in enumerate((0.05, 0.10, 0.20)):
        a, b = _pair("div/%d" % i, 3000 + 400 * i, d)
        seqs += [a, b]
        pairs.append((2 * i, 2 * i + 1))
    return seqs, pairs


def two_to_one():
    """3 kbp against an unrelated 1.5 kbp: a 2:1 pair whose alignment is gaps and mismatches throughout.  The top-level forward
    rows spread over far more of the matrix than the left child's box holds: the oracle's rows say about two thirds of that
    child's far-apart rows lie inside its box (762 of 1136), the rest must be computed."""
    rng = random.Random("row-reuse/unrelated")
    s = rand_seq(rng, 3000)
    return [s, rand_seq(rng, 1500)], [(0, 1)]


def unrelated():
    """Two unrelated 2 kbp sequences: the parent's rows leave the child's box within the first pass, so nothing can be taken."""
    rng = random.Random("row-reuse/unrelated-2k")
    return [rand_seq(rng, 2000), rand_seq(rng, 2000)], [(0, 1)]


def terminal_gap():
    """4 kbp with 600 more bases in front against a 10 % copy: a 600-base terminal gap.  The oracle's rows stay inside both
    children's boxes throughout their far-apart zones."""
    rng = random.Random("row-reuse/terminal-gap")
    s = rand_seq(rng, 4000)
    return [rand_seq(rng, 600) + s, mutate(s, 0.10, rng)], [(0, 1)]


#: (generator, seed number, component of the top-level breakpoint): found by a scan of 24 seeds each with the oracle's trace
INDEL_CASES = (("micro", 0, 2), ("micro", 16, 3), ("micro", 19, 2), ("tandem", 0, 4), ("tandem", 4, 2), ("tandem", 11, 4))


def indel_breakpoints():
    """Microsatellites and 171-base tandem arrays with a copy-number change between flanks of equal length (tests/repeats.py),
    3 % noise on both sides: the change lies at the middle of the score, so the top-level breakpoint falls inside the gap --
    in I2, D1 or D2 (INDEL_CASES; tests/test_gpu_row_reuse.py checks it with top_breakpoint_components)."""
    seqs, pairs = [], []
    for kind, i, _ in INDEL_CASES:
        rng = random.Random("row-reuse/indel/%s/%d" % (kind, i))
        a, b = R.microsatellite(rng, flank=(1700, 1800)) if kind == "micro" else R.tandem(rng, total=(1200, 2000), unit_len=171, flank=(1400, 1500))
        a, b = mutate(a, 0.03, rng), mutate(b, 0.03, rng)
        seqs += [a, b]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    return seqs, pairs


def restart_case():
    """One of tests/repeats.py's RESTART_CASES: a search whose furthest points met inside a far-apart pass is run again."""
    name, gen, seed = R.RESTART_CASES[0]
    a, b = gen(random.Random(seed))
    return [a, b], [(0, 1), (1, 0)]


def many_units(n=10):
    """n sequences of 3 kbp, all directed pairs: with two workgroups each takes many units in turn."""
    rng = random.Random("row-reuse/many")
    base = rand_seq(rng, 3000)
    seqs = [mutate(base, rng.uniform(0.03, 0.08), rng) for _ in range(n)]
    return seqs, [(i, j) for i in range(n) for j in range(n) if i != j]


def revcomp_entry():
    """A q_revcomp entry: the query is aligned reverse-complemented (never part of a twin unit)."""
    a, b = _pair("revcomp", 3500, 0.08)
    rc = bytes(a).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    return [rc, b], [(0, 1, 1)]


def top_breakpoint_components(oracle_module, seqs, pairs, scores):
    """The component (0 = M, 1 = I1, 2 = I2, 3 = D1, 4 = D2) of every pair's top-level breakpoint, from the oracle's own trace
    (AWO_DEBUG, read in a child process: the trace goes to stderr)."""
    import json
    import os
    import subprocess
    import sys
    code = ("import sys, json; sys.path.insert(0, %r); import oracle as O; d = json.load(sys.stdin); al = O.Aligner(d['scores'])\n"
            "for p, t in d['pairs']:\n    sys.stderr.write('[pair]\\n'); sys.stderr.flush(); al.align(bytes.fromhex(p), bytes.fromhex(t))\n"
            % os.path.dirname(os.path.abspath(oracle_module.__file__)))
    data = json.dumps({"scores": list(scores), "pairs": [(bytes(seqs[p[0]]).hex(), bytes(seqs[p[1]]).hex()) for p in pairs]})
    r = subprocess.run([sys.executable, "-c", code], input=data, capture_output=True, text=True, timeout=120, env=dict(os.environ, AWO_DEBUG="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    comps, fresh = [], False
    for line in r.stderr.splitlines():
        if line.startswith("[pair]"):
            fresh = True
        elif fresh and "bp score" in line:
            comps.append(int(line.split(" comp ")[1].split()[0]))
            fresh = False
    return comps
