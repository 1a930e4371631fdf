"""Cases for gap-run normalization (csrc/normalize_device.hpp): an independent step-by-step shifter (the definition, one left
step at a time), random edit scripts with sequences that make them true, hand-made traps with their expected strings, and
the case lists the GPU tests run -- shared here so that the CPU tests can check them against the oracle."""
import random

import numpy as np

import repeats
import verify_cases as V
from util import DEFAULT_2P, rand_seq

OK, SKIPPED, BAD_OP, LENGTHS = 0, 1, 2, 3
P1 = (0, 4, 6, 2)
ALIGN_SCORES = (DEFAULT_2P, P1)  # the two penalty sets of the aligning calls
GENERATORS = ("microsatellite", "tandem", "cnv", "low_complexity", "end_runs")


def runs(ops):
    """[(op, length)] of the maximal runs."""
    out = []
    for c in ops:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [tuple(r) for r in out]


def gap_runs(ops):
    return [r for r in runs(ops) if r[0] in b"ID"]


def step_left(pattern, text, ops):
    """The left-normal form by the definition: single left steps of maximal gap runs until none can take one.  Returns
    (op bytes, total steps taken)."""
    ops = bytearray(ops)
    steps, changed = 0, True
    while changed:
        changed = False
        c, q, t = 0, 0, 0
        while c < len(ops):
            g = ops[c]
            if g not in b"ID":
                c, q, t = c + 1, q + 1, t + 1
                continue
            e = c
            while e < len(ops) and ops[e] == g:
                e += 1
            L = e - c
            seq, p = (pattern, q) if g == ord("D") else (text, t)
            # one step at a time, as often as this run can go now
            while c >= 1 and ops[c - 1] == ord("M") and seq[p - 1] == seq[p + L - 1] and not (c >= 2 and ops[c - 2] == g):
                ops[c - 1], ops[c + L - 1] = g, ord("M")
                c, p, q, t = c - 1, p - 1, q - 1, t - 1
                steps += 1
                changed = True
            if g == ord("D"):
                q += L
            else:
                t += L
            c += L
    return bytes(ops), steps


def step_normal(direction, pattern, text, ops):
    """The left- / right-normal form by single steps; right is the mirror image of left."""
    if direction == "left":
        return step_left(pattern, text, ops)
    out, steps = step_left(pattern[::-1], text[::-1], ops[::-1])
    return out[::-1], steps


def build_pair(rng, ops, alphabet):
    """(pattern, text) over `alphabet` that make the op string true: 'M' over equal bytes, 'X' over different ones."""
    p, t = bytearray(), bytearray()
    for op in ops:
        a = rng.choice(alphabet)
        if op == ord("M"):
            p.append(a)
            t.append(a)
        elif op == ord("X"):
            p.append(a)
            t.append(rng.choice([b for b in alphabet if b != a]))
        elif op == ord("I"):
            t.append(a)
        else:
            p.append(a)
    return bytes(p), bytes(t)


def random_script(rng, max_cols=200):
    """A random edit script of 0 .. max_cols columns over a 1- to 4-letter alphabet, with its sequences.  Short alphabets and
    short 'M' runs between gaps: runs meet, link and block each other."""
    alphabet = b"ACGT"[:rng.randint(1, 4)]
    n = rng.randint(0, max_cols)
    kinds = b"MID" if len(alphabet) == 1 else rng.choice([b"MXID", b"MMMID", b"MMXIDID"])
    ops = bytearray()
    while len(ops) < n:
        op = rng.choice(kinds)
        ops += bytes([op]) * rng.randint(1, 12 if op == ord("M") else 4)
    ops = bytes(ops[:n])
    p, t = build_pair(rng, ops, alphabet)
    return p, t, ops


def traps():
    """[(name, direction, pattern, text, ops, expected ops)]: every expectation is stated, not computed."""
    out = []

    def add(name, p, t, ops, want, direction="left"):
        out.append((name, direction, p, t, ops, want))

    add("gap at a homopolymer's end goes to column 0", b"A" * 7, b"A" * 8, b"M" * 7 + b"I", b"I" + b"M" * 7)
    add("deletion at a homopolymer's end goes to column 0", b"A" * 9, b"A" * 6, b"M" * 6 + b"DDD", b"DDD" + b"M" * 6)
    add("unit insertion moves by whole units", b"T" + b"ACG" * 3 + b"T", b"T" + b"ACG" * 4 + b"T", b"M" * 10 + b"III" + b"M",
        b"M" + b"III" + b"M" * 10)
    add("unit insertion moves a partial unit further", b"TG" + b"ACG" * 3 + b"T", b"TG" + b"ACG" * 4 + b"T", b"M" * 11 + b"III" + b"M",
        b"M" + b"III" + b"M" * 11)
    add("an X blocks a run", b"AACAA", b"AAGAAA", b"MMXMMI", b"MMXIMM")
    add("a differing base stops a run", b"CAAAA", b"CAAAAA", b"MMMMMI", b"MIMMMM")
    add("linked I..M..D each follow the one before", b"A" * 6, b"A" * 6, b"MMIMMDM", b"IDMMMMM")
    add("same-type runs stop one M short", b"A" * 5, b"A" * 7, b"MMIMMIM", b"IMIMMMM")
    add("I directly followed by D", b"A" * 4, b"A" * 4, b"MMIDM", b"IDMMM")
    add("all gaps", b"AA", b"AA", b"IIDD", b"IIDD")
    add("empty", b"", b"", b"", b"")
    add("nothing to move", b"ACGT", b"ACGT", b"MMMM", b"MMMM")
    add("right: gap at a homopolymer's start goes to the last column", b"A" * 7, b"A" * 8, b"I" + b"M" * 7, b"M" * 7 + b"I", "right")
    add("right: unit deletion moves to the array's end", b"T" + b"AC" * 4 + b"G", b"T" + b"AC" * 3 + b"G", b"M" + b"DD" + b"M" * 7,
        b"M" * 7 + b"DD" + b"M", "right")
    add("right: linked runs", b"A" * 6, b"A" * 6, b"MDMMIMM", b"MMMMMDI", "right")
    # shifts of exactly k columns: the lane, chunk and multi-chunk edges; stopped by a differing base, by an X, by column 0
    for k in (15, 16, 17, 63, 64, 65, 1023, 1024, 1025):
        add("shift of %d stopped by a base" % k, b"C" + b"A" * k, b"C" + b"A" * (k + 1), b"M" * (k + 1) + b"I", b"M" + b"I" + b"M" * k)
        add("shift of %d stopped by an X" % k, b"C" + b"A" * k, b"A" * (k + 2), b"X" + b"M" * k + b"I", b"X" + b"I" + b"M" * k)
        add("shift of %d to column 0" % k, b"A" * (k + 2), b"A" * k, b"M" * k + b"DD", b"DD" + b"M" * k)
        add("right: shift of %d" % k, b"A" * k + b"C", b"A" * (k + 1) + b"C", b"I" + b"M" * (k + 1), b"M" * k + b"I" + b"M", "right")
    # runs that straddle a chunk edge (1,024 bytes from the 16-byte boundary below the string), moved and not
    add("run over a chunk edge, moved", b"G" + b"A" * 1010, b"G" + b"A" * 1060, b"M" * 1001 + b"I" * 50 + b"M" * 10,
        b"M" + b"I" * 50 + b"M" * 1010)
    add("run over a chunk edge, blocked", b"A" * 1000 + b"C" + b"A" * 10, b"A" * 1000 + b"G" + b"T" * 50 + b"A" * 10,
        b"M" * 1000 + b"X" + b"I" * 50 + b"M" * 10, b"M" * 1000 + b"X" + b"I" * 50 + b"M" * 10)
    add("linked runs over two chunks", b"A" * 2100, b"A" * 2100, b"M" * 1020 + b"I" * 10 + b"M" * 1060 + b"D" * 10 + b"M" * 10,
        b"I" * 10 + b"D" * 10 + b"M" * 2090)
    return out


def refusals():
    """[(name, pattern, text, ops, code, column)]: strings that are refused untouched."""
    return [("bad byte", b"AAAA", b"AAAA", b"MMNM", BAD_OP, 2),
            ("bad byte first", b"AAAA", b"AAAA", b"=MMM", BAD_OP, 0),
            ("bad byte in the second chunk", b"A" * 1500, b"A" * 1500, b"M" * 1200 + b"S" + b"M" * 299, BAD_OP, 1200),
            ("bad byte wins over lengths", b"AAA", b"AAAA", b"MMMN", BAD_OP, 3),
            ("pattern too long", b"AAAAA", b"AAAA", b"MMMM", LENGTHS, 0),
            ("text too short", b"AAAA", b"AAA", b"MMMM", LENGTHS, 0),
            ("I and D exchanged", b"AAAA", b"AAAAA", b"MMMMD", LENGTHS, 0),
            ("empty string, bases left", b"A", b"", b"", LENGTHS, 0)]


def as_tuple(rec):
    return tuple(int(rec[f]) for f in ("code", "runs_moved", "columns_moved", "max_shift", "reserved"))


# ---- the case lists of the GPU tests ---------------------------------------------------------------------------------------

def device_cases(seed=91):
    """The caller-supplied strings of the GPU tests as one resident set:
    (seqs, pairs [n, 3], ranges [n, 7], [(pattern, text, ops)] as the pairs see them, the same as the ranges see them).
    The traps and the refusals' sequences, random scripts (N and lower-case alphabets among them), long scripts of several
    chunks, and q_revcomp pairs whose query is the stored reverse complement.  Range k cuts its intervals out of sequences
    with flanks around them."""
    rng = random.Random(seed)
    items = [(p, t, ops, False) for _, _, p, t, ops, _ in traps()]
    for k in range(60):
        p, t, ops = random_script(rng, 200)
        items.append((p, t, ops, k % 3 == 0))
    for alphabet in (b"ACGTN", b"acgt", b"AaNn"):
        for _ in range(6):
            ops = random_ops_long(rng, rng.randint(50, 400))
            p, t = build_pair(rng, ops, alphabet)
            items.append((p, t, ops, False))
    for k in range(8):  # several chunks, repeat-rich: two letters, short matches between the gaps
        ops = random_ops_long(rng, rng.randint(2000, 5000))
        p, t = build_pair(rng, ops, b"AC" if k % 4 else b"ACGT")
        items.append((p, t, ops, k % 2 == 1))
    seqs, pairs, ranges, seen_p, seen_r = [], [], [], [], []
    for p, t, ops, rev in items:
        if rev and not set(p) <= set(b"ACGT"):
            rev = False
        q = V.revcomp(p) if rev else p
        seqs += [q, t]
        pairs.append((len(seqs) - 2, len(seqs) - 1, int(rev)))
        seen_p.append((p, t, ops))
        # the range: the same strings inside flanked sequences, the query interval on the query's forward strand
        fl = [rand_seq(rng, rng.randint(0, 9)) for _ in range(4)]
        seqs += [fl[0] + q + fl[1], fl[2] + t + fl[3]]
        ranges.append((len(seqs) - 2, len(seqs) - 1, int(rev), len(fl[0]), len(fl[0]) + len(q), len(fl[2]), len(fl[2]) + len(t)))
        seen_r.append((p, t, ops))
    return seqs, np.array(pairs, dtype=np.int32), np.array(ranges, dtype=np.int32), seen_p, seen_r


def random_ops_long(rng, n):
    ops = bytearray()
    while len(ops) < n:
        op = rng.choice(b"MMMXIDID")
        ops += bytes([op]) * (rng.randint(1, 40) if op == ord("M") else rng.randint(1, 6))
    return bytes(ops[:n])


def repeat_set(seed=92, per_class=3):
    """The pair list of the aligning-call GPU tests: per_class pairs from every tests/repeats.py SMALL generator named in
    GENERATORS.  Returns (seqs, pairs [n, 3], class name per pair); sequence 2 k is pair k's pattern, 2 k + 1 its text."""
    rng = random.Random(seed)
    seqs, pairs, names = [], [], []
    for name in GENERATORS:
        for _ in range(per_class):
            p, t = repeats.SMALL[name](rng)
            seqs += [p, t]
            pairs.append((len(seqs) - 2, len(seqs) - 1, 0))
            names.append(name)
    return seqs, np.array(pairs, dtype=np.int32), names


def homopolymer_case(seed=93, runs_wanted=320, total=30000):
    """A 30 kbp homopolymer-rich pair whose op string holds at least 300 gap runs, most of them free to move a long way:
    stretches of one base with single-base indels, separated by rare other bases.  Returns (pattern, text, ops)."""
    rng = random.Random(seed)
    ops = bytearray()
    per = total // runs_wanted
    for k in range(runs_wanted):
        ops += b"M" * rng.randint(per - 6, per + 8)
        ops += bytes([rng.choice(b"ID")]) * rng.randint(1, 3)
    ops += b"M" * 50
    p, t = bytearray(), bytearray()
    for c, op in enumerate(ops):
        base = ord("C") if c % 6000 == 5999 else ord("A")  # a blocker every 6,000 columns
        if op != ord("I"):
            p.append(base)
        if op != ord("D"):
            t.append(base)
    # make every M column true: a column's two bases are equal by construction (both `base`)
    return bytes(p), bytes(t), bytes(ops)
