"""Seeded repeat-rich pair generators for the parity tests.

Uniform-random ACGT leaves a WFA almost no room for ties: few diagonals reach a score at once and the
optimal alignment is nearly unique.  On repeats (microsatellites, tandem arrays, copy-number changes,
low-complexity sequence) co-optimal alignments multiply and the CIGAR is decided by tie-breaking --
the breakpoint search's first hit in ascending k, the backtrace's choice among equal candidates, the
known-optimum stop.  Runs of A or T at a sequence's ends also meet the zero (= "AAAA...") pad words
around the 2-bit packed sequences, which only the length clamp of every probe keeps out of a match.

Every generator takes a random.Random and returns (pattern, text).  Size keywords default to the
ranges the families are defined with; the CPU tests pass smaller ones (the Gotoh check is quadratic).
"""
from util import mutate, rand_seq

END_RUN_LENGTHS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)  # around the 16/32-base probes, 8-byte raw probe, 64 lanes


def _noise(s, rng, dmax):
    return mutate(s, rng.uniform(0.0, dmax), rng) if dmax > 0 else s


def microsatellite(rng, flank=(30, 400)):
    """Random flanks around an array of a 1-6 base unit, 20-400 bases long; the other sequence has the
    array expanded or contracted by 1-20 units, then 0-2 % noise."""
    unit = rand_seq(rng, rng.randint(1, 6))
    n = max(1, rng.randint(20, 400) // len(unit))
    dn = rng.randint(1, 20) * rng.choice((-1, 1))
    m = max(0, n + dn)
    left, right = rand_seq(rng, rng.randint(*flank)), rand_seq(rng, rng.randint(*flank))
    a = left + unit * n + right
    b = _noise(left + unit * m + right, rng, 0.02)
    return (a, b) if rng.random() < 0.5 else (b, a)


def end_runs(rng, body=(100, 1500), lengths=END_RUN_LENGTHS, where=None):
    """Poly-A or poly-T runs at the start and/or end of a sequence (run lengths straddling the probe
    widths); the other sequence carries the same kind of run at the same end, of an independently drawn
    length, around a 0-3 % copy of the body."""
    core = rand_seq(rng, rng.randint(*body))
    where = where or rng.choice(("head", "tail", "both"))
    base = rng.choice(b"AT")

    def wrap(s):
        h = bytes([base]) * rng.choice(lengths) if where in ("head", "both") else b""
        t = bytes([rng.choice(b"AT")]) * rng.choice(lengths) if where in ("tail", "both") else b""
        return h + s + t

    a = wrap(core)
    b = wrap(_noise(core, rng, 0.03))
    return a, b


def tandem(rng, total=(3000, 40000), unit_len=None, flank=(0, 300)):
    """An array of copies of a 171 b unit or a random 20-500 b unit, each copy 1-5 % diverged from it,
    3-40 kbp long; the other sequence has 1-3 copies fewer or more (an extra copy is a diverged copy of
    one beside it), 0-1 % noise, same flanks."""
    if unit_len is None:
        unit_len = 171 if rng.random() < 0.4 else rng.randint(20, 500)
    unit = rand_seq(rng, unit_len)
    ncopy = max(3, rng.randint(*total) // unit_len)
    copies = [mutate(unit, rng.uniform(0.01, 0.05), rng) for _ in range(ncopy)]
    other = list(copies)
    for _ in range(rng.randint(1, 3)):
        i = rng.randrange(len(other))
        if rng.random() < 0.5 and len(other) > 2:
            del other[i]
        else:
            other.insert(i, mutate(other[i], rng.uniform(0.01, 0.05), rng))
    left, right = rand_seq(rng, rng.randint(*flank)), rand_seq(rng, rng.randint(*flank))
    a = left + b"".join(copies) + right
    b = _noise(left + b"".join(other) + right, rng, 0.01)
    return (a, b) if rng.random() < 0.5 else (b, a)


def cnv_duplication(rng, seg=(50, 3000), flank=(200, 2000)):
    """A 50 b - 3 kbp segment repeated 2-5 times in place in one sequence, once in the other; 0-1 % noise."""
    s = rand_seq(rng, rng.randint(*seg))
    left, right = rand_seq(rng, rng.randint(*flank)), rand_seq(rng, rng.randint(*flank))
    a = left + s * rng.randint(2, 5) + right
    b = _noise(left + s + right, rng, 0.01)
    return (a, b) if rng.random() < 0.5 else (b, a)


def cnv_deletion(rng, unit_len, ncopy, flank=(200, 1000), noise=0.005):
    """One copy deleted from a tandem array of ncopy copies (1-3 % diverged) of a unit_len unit: the
    deletion is unit_len bases long, inside sequence that matches on both sides of it at every copy.
    The shorter sequence also carries up to `noise` divergence."""
    unit = rand_seq(rng, unit_len)
    copies = [mutate(unit, rng.uniform(0.01, 0.03), rng) for _ in range(ncopy)]
    i = rng.randrange(ncopy)
    left, right = rand_seq(rng, rng.randint(*flank)), rand_seq(rng, rng.randint(*flank))
    a = left + b"".join(copies) + right
    b = _noise(left + b"".join(copies[:i] + copies[i + 1:]) + right, rng, noise)
    return (a, b) if rng.random() < 0.5 else (b, a)


def cnv(rng, seg=(50, 3000), flank=(200, 2000)):
    """Either a segment duplicated in place or one copy of a short tandem array deleted."""
    if rng.random() < 0.5:
        return cnv_duplication(rng, seg, flank)
    u = rng.randint(max(20, seg[0]), max(20, min(seg[1], 600)))
    return cnv_deletion(rng, u, rng.randint(3, 6), (flank[0] // 2, flank[1] // 2))


def low_complexity(rng, n=(200, 2000)):
    """Random sequence over a two-letter alphabet (AT only or GC only) against a 2-10 % copy in the same
    alphabet, or a periodic sequence against itself offset by part of a period (b"AC" * n against
    b"CA" * (n + k), and the like for periods of 2-4)."""
    length = rng.randint(*n)
    if rng.random() < 0.5:
        alpha = rng.choice((b"AT", b"GC"))
        a = rand_seq(rng, length, alpha)
        b = mutate(a, rng.uniform(0.02, 0.10), rng, alpha)
    else:
        period = rand_seq(rng, rng.randint(2, 4))
        while len(set(period)) < 2:
            period = rand_seq(rng, len(period))
        off = rng.randint(1, len(period) - 1)
        k = rng.randint(0, 12)
        reps = max(2, length // len(period))
        a = period * reps
        b = (period[off:] + period[:off]) * (reps + k)
        if rng.random() < 0.5:
            b = mutate(b, 0.005, rng)
    return (a, b) if rng.random() < 0.5 else (b, a)


def exact_blocks(rng, block=(2000, 10000), nblocks=(2, 4)):
    """2-10 kbp identical blocks separated by rare differences (a substitution or a 1-3 base indel):
    extension runs across many 2-bit words and past a multi-step pass's window."""
    a, b = bytearray(), bytearray()
    for i in range(rng.randint(*nblocks)):
        s = rand_seq(rng, rng.randint(*block))
        a += s
        b += s
        kind = rng.randrange(3)
        if kind == 0:
            c = rng.choice(b"ACGT")
            a.append(c)
            b.append(rng.choice([x for x in b"ACGT" if x != c]))
        elif kind == 1:
            a += rand_seq(rng, rng.randint(1, 3))
        else:
            b += rand_seq(rng, rng.randint(1, 3))
    return bytes(a), bytes(b)


# name -> generator at sizes whose Gotoh check stays cheap on the CPU (every sequence <= ~4.5 kbp)
SMALL = {
    "microsatellite": lambda rng: microsatellite(rng),
    "end_runs": lambda rng: end_runs(rng),
    "tandem": lambda rng: tandem(rng, total=(600, 3500), flank=(0, 200)),
    "cnv": lambda rng: cnv(rng, seg=(50, 900), flank=(100, 600)),
    "low_complexity": lambda rng: low_complexity(rng),
    "exact_blocks": lambda rng: exact_blocks(rng, block=(800, 1800), nblocks=(2, 2)),
}


# (generator, seed): pairs on which breakpoint searches met inside a multi-step pass and were run again step by step
# (awv_stats.restarts), found by a per-pair scan of 300 seeded repeat pairs on an MI355X -- restarts came up on about half
# of the tandem, copy-number and microsatellite pairs and on nearly every long-exact-block pair
RESTART_CASES = (("tandem", lambda rng: tandem(rng, total=(3000, 12000)), "restart/tandem/1"),
                 ("exact_blocks", lambda rng: exact_blocks(rng), "restart/exact_blocks/0"),
                 ("microsatellite", lambda rng: microsatellite(rng), "restart/microsatellite/48"))


def path_cells(ops):
    """The DP cells (i, j) an alignment's path visits; ops are the oracle's op bytes (M/X consume both
    sequences, D the pattern, I the text)."""
    i = j = 0
    cells = {(0, 0)}
    for c in ops:
        if c in b"MX":
            i += 1
            j += 1
        elif c == ord("D"):
            i += 1
        else:
            j += 1
        cells.add((i, j))
    return cells


def tie_cells(aligner, p, t):
    """How far apart two optimal alignments of (p, t) lie: the oracle's path, and the path of the
    reversed pair reversed back.  Both are optimal; on a pair with a unique optimum they coincide.
    Returns the number of DP cells on exactly one of the two paths."""
    _, ops = aligner.align(p, t)
    _, rops = aligner.align(p[::-1], t[::-1])
    return len(path_cells(ops) ^ path_cells(rops[::-1]))

