"""What the tests of the cs difference string share (csrc/cs_device.hpp, csrc/cs.hip): a Python restatement of the contract in
include/allwave_hip.h (cs_of), its inverse (apply_cs: the pattern and the run-length CIGAR from a cs string and the target
alone), the case list -- the smallest shapes at which the walk can go wrong -- and the random alignments and slices, each built
once."""
import random
import re

import numpy as np

import clip_cases as K
import normalize_cases as N
import verify_cases as V
from util import rand_seq

OK, SKIPPED, BAD_OP, LENGTHS = range(4)
MODES = ("short", "long")
M_RUNS = (9, 10, 99, 100, 999, 1000, 1023, 1024, 1025, 100000)  # the digit thresholds; runs over 1, 2 and about 100 chunks
GAP_STARTS = tuple(range(0, 18)) + tuple(range(1008, 1041))     # across lane words (16 bytes) and across the chunk edge (1,024 bytes)
X_COLUMNS = (15, 16, 1023, 1024)
NOT_COMPLETED = 1  # awv_result.status of the case that has a string and no text (AWV_ST_CAPACITY)

_RUN = re.compile(rb"(.)\1*", re.S)


def cs_of(ops, pattern, text, mode, slice=None):
    """The contract, restated: (cs text, code) of the op string -- of its slice (col_beg, col_end, q_skip, t_skip) -- over
    pattern and text.  mode: "short" or "long"."""
    b, e, p, t = (0, len(ops), 0, 0) if slice is None else slice
    ops = bytes(ops[b:e])
    if set(ops) - set(b"MXID"):
        return b"", BAD_OP
    if p + len(ops) - ops.count(b"I") > len(pattern) or t + len(ops) - ops.count(b"D") > len(text):
        return b"", LENGTHS
    out = bytearray()
    for m in _RUN.finditer(ops):
        op, n = m.group(1), m.end() - m.start()
        if op == b"M":
            out += b":%d" % n if mode == "short" else b"=" + text[t:t + n].upper()
        elif op == b"X":
            for k in range(n):
                out += b"*" + text[t + k:t + k + 1].lower() + pattern[p + k:p + k + 1].lower()
        elif op == b"I":
            out += b"-" + text[t:t + n].lower()
        else:
            out += b"+" + pattern[p:p + n].lower()
        p += n if op != b"I" else 0
        t += n if op != b"D" else 0
    return bytes(out), OK


_ITEM = re.compile(rb":([0-9]+)|=([A-Za-z]+)|\*([a-z])([a-z])|\+([a-z]+)|-([a-z]+)")


def apply_cs(text_seq, cs):
    """The inverse, for upper-case sequences: (pattern, run-length CIGAR in the letters of util.rle) rebuilt from a cs string
    (either mode) and the target alone."""
    pattern, runs, t, at = bytearray(), [], 0, 0

    def add(n, letter):
        if runs and runs[-1][1] == letter:
            runs[-1][0] += n
        else:
            runs.append([n, letter])

    for m in _ITEM.finditer(cs):
        assert m.start() == at, (at, cs[at:at + 20])
        at = m.end()
        count, same, x_t, x_q, ins, dele = m.groups()
        if count is not None or same is not None:
            n = int(count) if count is not None else len(same)
            assert same is None or same == text_seq[t:t + n]
            pattern += text_seq[t:t + n]
            t += n
            add(n, "=")
        elif x_t is not None:
            assert x_t.upper() == text_seq[t:t + 1]
            pattern += x_q.upper()
            t += 1
            add(1, "X")
        elif ins is not None:
            pattern += ins.upper()
            add(len(ins), "I")
        else:
            assert dele.upper() == text_seq[t:t + len(dele)]
            t += len(dele)
            add(len(dele), "D")
    assert at == len(cs)
    return bytes(pattern), "".join("%d%s" % (n, c) for n, c in runs)


KNOWN = dict(text=b"CGATCGATAAATAGAGTAGGAATAGCA", pattern=b"CGATCGAATAGAGTAGGTCGAATTGCA",
             ops=b"M" * 6 + b"I" * 3 + b"M" * 10 + b"D" * 3 + b"M" * 4 + b"X" + b"M" * 3,
             short=b":6-ata:10+gtc:4*at:3", long=b"=CGATCG-ata=AATAGAGTAG+gtc=GAAT*at=GCA")  # minimap2's manual


def random_ops(rng, n, alphabet=b"MMMMXID"):
    """n op bytes in runs of 1 .. 12 (now and then a long one)."""
    ops = bytearray()
    while len(ops) < n:
        ops += bytes([rng.choice(alphabet)]) * (rng.randint(1, 12) if rng.random() < 0.9 else rng.randint(13, 1500))
    return bytes(ops[:n])


def case_list():
    """[(name, pattern, text, ops, status, q_revcomp)], in a fixed order.  Most cases share one pair of unrelated random
    sequences, long enough for every string: the walk judges no column, so 'M' over differing bases is the rule there."""
    rng = random.Random(411)
    big_p, big_t = rand_seq(rng, 100200), rand_seq(rng, 100200)
    out = []

    def add(name, ops, p=big_p, t=big_t, status=0, rev=False):
        out.append((name, p, t, ops, status, rev))

    add("empty", b"")
    for op in b"MXID":
        add("one column " + chr(op), bytes([op]))
    add("known answer", KNOWN["ops"], KNOWN["pattern"], KNOWN["text"])
    for n in M_RUNS:
        add("M run of %d" % n, b"M" * n)
        add("M run of %d, then an X" % n, b"M" * n + b"X")
    for op in (b"I", b"D"):
        for start in GAP_STARTS:
            for n in range(1, 41):  # one run of n between two others, beginning at column `start`
                add("%s run of %d at %d" % (op.decode(), n, start), b"M" * start + op * n + b"M" * 3)
    for c in X_COLUMNS:
        add("X at column %d" % c, b"M" * c + b"X" + b"M" * 5)
        add("X at column %d, last" % c, b"M" * c + b"X")
    add("2048 alternating columns", b"XM" * 1024)
    add("2048 alternating columns, M first", b"MX" * 1024)
    for lead in (5, 12, 1017):
        add("I run then D run at %d" % lead, b"M" * lead + b"I" * 7 + b"D" * 9 + b"M" * 4)
        add("D run then I run at %d" % lead, b"M" * lead + b"D" * 7 + b"I" * 9 + b"M" * 4)
    add("gaps only", b"IIIDDDDIID")
    add("a long M run after a break at a lane's first byte", b"X" * 16 + b"M" * 2000 + b"XMXMXMXMXMXMXMX")
    mixed = random_ops(rng, 3000)
    for sh in range(16):
        add("mixed string at residue %d" % sh, mixed)
    odd = b"ACGTNnacgtRYry-*.\x00\x7fAZaz@[`{" * 4
    add("N, lower case and non-letters", random_ops(rng, 60, b"MXID")[:60], odd, odd[::-1])
    add("N, lower case and non-letters, long runs", b"M" * 30 + b"X" * 30 + b"I" * 20 + b"D" * 20, odd, odd[::-1])
    add("an M over differing bases, an X over equal ones", b"MMXM", b"AAAA", b"ACAA")
    add("not completed", b"MMXMMIIMM", status=NOT_COMPLETED)
    add("a stray byte", b"MMMNMM")
    add("a stray byte in the second chunk", b"M" * 1200 + b"=" + b"M" * 30)
    add("a stray byte wins over the lengths", b"MMMMN", b"ACG", b"ACG")
    add("exactly as long as both", b"MMMXD" + b"I", b"ACGTA", b"ACGAC")
    add("one base too long for the pattern", b"MMMXD" + b"I", b"ACGT", b"ACGAC")
    add("one base too long for the text", b"MMMXD" + b"I", b"ACGTA", b"ACGA")
    add("one base too long for the pattern, in the second chunk", b"M" * 1100 + b"D", big_p[:1100], big_t[:1100])
    add("empty string over empty sequences", b"", b"", b"")
    for k in range(12):  # true alignments; the stored query is the reverse complement of the pattern
        ops = N.random_ops_long(rng, rng.choice([1, 17, 300, 1024, 2500]))
        p, t = N.build_pair(rng, ops, b"ACGT")
        add("q_revcomp alignment %d" % k, ops, p, t, rev=True)
    return out


def residues(cases):
    """The residue modulo 16 of every case's first byte in the packed arena: all sixteen for the mixed string, a cycle else."""
    return [int(c[0].rsplit(" ", 1)[1]) if c[0].startswith("mixed string at residue") else (7 * k + 3) % 16 for k, c in enumerate(cases)]


def resident(cases):
    """The cases as a resident sequence set: (seqs, pairs [n, 3]); equal sequences are stored once, a q_revcomp case stores the
    reverse complement of its pattern."""
    seqs, where, pairs = [], {}, []

    def index(s):
        if s not in where:
            where[s] = len(seqs)
            seqs.append(s)
        return where[s]

    for _, p, t, _, _, rev in cases:
        pairs.append((index(V.revcomp(p) if rev else p), index(t), int(rev)))
    return seqs, np.array(pairs, dtype=np.int32)


def pack(cases):
    """The cases as records and an arena (clip_cases.pack_arena: a junk byte between strings, the residues of residues())."""
    return K.pack_arena([c[3] for c in cases], residues(cases), [c[4] for c in cases])


def random_alignments(seed=412, count=300):
    """[(pattern, text, ops)]: 300 true alignments over ACGT, 0 .. 2,600 columns, lane and chunk sizes among them."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.choice([0, 1, 2, 15, 16, 17, 31, 1023, 1024, 1025]) if k % 3 == 0 else rng.randint(0, 2600)
        ops = N.random_ops_long(rng, n) if k % 2 else random_ops(rng, n)
        p, t = N.build_pair(rng, ops, b"ACGT")
        out.append((p, t, ops))
    return out


def random_slices(strings, seed=413, count=200):
    """[(string index, (col_beg, col_end, q_skip, t_skip))] with the true skips: empty slices, whole strings, and slices that begin
    and end inside runs."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        i = rng.randrange(len(strings))
        ops = strings[i]
        n = len(ops)
        b = rng.randint(0, n)
        e = b if k % 10 == 0 else n if k % 10 == 1 else rng.randint(b, n)
        out.append((i, (b, e, b - ops[:b].count(b"I"), b - ops[:b].count(b"D"))))
    return out


def range_cases(seed=414):
    """Ranges on both strands: (seqs, ranges [n, 7], [(pattern, text, ops)] as the ranges see them).  The alignments sit inside
    sequences with flanks around them; the query interval is on the query's forward strand.  The last two ranges have an empty
    query interval (an 'I' run alone) and two empty intervals (an empty string)."""
    rng = random.Random(seed)
    items = [(p, t, ops, k % 2 == 1) for k, (p, t, ops) in enumerate(random_alignments(seed, 40))]
    items += [(b"", b"ACGTTGCA", b"I" * 8, False), (b"", b"", b"", True)]
    seqs, ranges, seen = [], [], []
    for p, t, ops, rev in items:
        fl = [rand_seq(rng, rng.randint(0, 9)) for _ in range(4)]
        q = V.revcomp(p) if rev else p
        seqs += [fl[0] + q + fl[1], fl[2] + t + fl[3]]
        ranges.append((len(seqs) - 2, len(seqs) - 1, int(rev), len(fl[0]), len(fl[0]) + len(q), len(fl[2]), len(fl[2]) + len(t)))
        seen.append((p, t, ops))
    return seqs, np.array(ranges, dtype=np.int32), seen
