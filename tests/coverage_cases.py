"""What the tests of the per-base depth share (csrc/coverage_device.hpp, csrc/coverage.hip): a Python restatement of the contract
in include/allwave_hip.h (coverage_of: a plain loop over columns that knows nothing of runs), an independent reading of a PAF
(coverage_from_paf: columns 1-9 and cg:Z: only, whole runs at a time), the case list -- the smallest shapes at which the
kernel's walk can go wrong, over a small resident set -- and the random alignments, each built once."""
import random
import re

import numpy as np

import cs_cases as X
import normalize_cases as N
from util import rand_seq

OK, SKIPPED, BAD_OP, LENGTHS = range(4)
TARGET, QUERY, BOTH = 1, 2, 3
ROLES = (TARGET, QUERY, BOTH)
ROLE_NAMES = {TARGET: "target", QUERY: "query", BOTH: "both"}
NOT_COMPLETED = 1  # awv_result.status of a case that has a string and adds nothing (AWV_ST_CAPACITY)


def code_of(ops, span, skips, lens=None):
    """The item's code: a byte outside MXID first, then the consumed bases against what the skips leave of the rectangle."""
    pb, pe, tb, te = span
    if set(ops) - set(b"MXID"):
        return BAD_OP
    if skips[0] + len(ops) - ops.count(b"I") > pe - pb or skips[1] + len(ops) - ops.count(b"D") > te - tb:
        return LENGTHS
    return OK


def coverage_of(ops, span, strand, skips, roles, lens):
    """The contract, restated: what the op string `ops` over the rectangle span = (pb, pe, tb, te), from the skips = (q_skip,
    t_skip) on, adds to a query of lens[0] and a target of lens[1] bases.  strand: "+" or "-" (the pattern is the query's reverse
    complement; the rectangle's pattern coordinates are that copy's).  Returns (code, (q_aligned, q_matched), (t_aligned,
    t_matched)): uint32 arrays per forward-strand base, all zero unless the code is OK."""
    qa, qm = np.zeros(lens[0], dtype=np.uint32), np.zeros(lens[0], dtype=np.uint32)
    ta, tm = np.zeros(lens[1], dtype=np.uint32), np.zeros(lens[1], dtype=np.uint32)
    code = code_of(ops, span, skips)
    if code != OK:
        return code, (qa, qm), (ta, tm)
    x, y = span[0] + skips[0], span[2] + skips[1]
    for op in ops:
        if op in b"MX":
            f = lens[0] - 1 - x if strand == "-" else x
            if roles & TARGET:
                ta[y] += 1
                tm[y] += op == ord("M")
            if roles & QUERY:
                qa[f] += 1
                qm[f] += op == ord("M")
        x += op != ord("I")
        y += op != ord("D")
    return code, (qa, qm), (ta, tm)


def counts_of(ops):
    """(aligned_cols, matched_cols, boundaries) of an awv_cov_item with code OK: boundaries = 2 x (maximal runs of aligned columns
    + maximal runs of 'M')."""
    aligned = sum(op in b"MX" for op in ops)
    runs_a = len(re.findall(rb"[MX]+", ops))
    runs_m = len(re.findall(rb"M+", ops))
    return aligned, ops.count(b"M"), 2 * (runs_a + runs_m)


class Tracks:
    """The two depth tracks of a sequence set, concatenated in set order, and the sum of items into them."""

    def __init__(self, lens):
        self.lens = [int(n) for n in lens]
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.aligned = np.zeros(int(self.offsets[-1]), dtype=np.uint32)
        self.matched = np.zeros(int(self.offsets[-1]), dtype=np.uint32)

    def add(self, q, t, ops, strand, roles, span=None, skips=(0, 0), times=1):
        """One item of the pair (q, t), `times` times over; span None: the whole of both sequences.  Returns its code."""
        lens = (self.lens[q], self.lens[t])
        span = (0, lens[0], 0, lens[1]) if span is None else span
        code, (qa, qm), (ta, tm) = coverage_of(ops, span, strand, skips, roles, lens)
        for s, a, m in ((q, qa, qm), (t, ta, tm)):
            lo, hi = self.offsets[s], self.offsets[s + 1]
            self.aligned[lo:hi] += a * np.uint32(times)
            self.matched[lo:hi] += m * np.uint32(times)
        return code

    def equals(self, aligned, matched):
        return np.array_equal(self.aligned, aligned) and np.array_equal(self.matched, matched)


def span_of_range(r, lens):
    """(q, t, strand, span) of a range (q_idx, t_idx, q_revcomp, q_beg, q_end, t_beg, t_end): the query interval, on the forward
    strand, in the coordinates of the copy that is aligned."""
    q, t, rev, qb, qe, tb, te = (int(v) for v in r)
    return q, t, "-" if rev else "+", ((lens[q] - qe, lens[q] - qb, tb, te) if rev else (qb, qe, tb, te))


_CG = re.compile(r"(\d+)([=XIDM])")


def coverage_from_paf(lines, ids, lens, roles):
    """The tracks (a Tracks) that a PAF's lines describe, from columns 1-9 and cg:Z: alone, a run at a time: the query's interval
    [col 3, col 4) is on its forward strand and is walked from its end backwards on a '-' line; in a PAF 'I' consumes the
    query and 'D' the target."""
    where = {name: k for k, name in enumerate(ids)}
    tr = Tracks(lens)
    for line in lines:
        f = line.rstrip("\n").split("\t")
        q, t = where[f[0]], where[f[5]]
        qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
        assert int(f[1]) == lens[q] and int(f[6]) == lens[t]
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0][5:]
        qpos, tpos = 0, ts
        for n, op in _CG.findall(cg):
            n = int(n)
            if op in "=XM":
                lo = qe - qpos - n if f[4] == "-" else qs + qpos
                for s, at, on in ((t, tpos, roles & TARGET), (q, lo, roles & QUERY)):
                    if on:
                        tr.aligned[tr.offsets[s] + at:tr.offsets[s] + at + n] += 1
                        if op != "X":
                            tr.matched[tr.offsets[s] + at:tr.offsets[s] + at + n] += 1
            qpos += n if op != "D" else 0
            tpos += n if op != "I" else 0
        assert qpos == qe - qs and tpos == te, line
    return tr


def format_tracks(ids, tracks):
    """The lines of the command-line tool's --coverage file: name, beg, end, aligned, matched per maximal interval on which both
    tracks are constant, every sequence end to end in input order."""
    out = []
    for s, name in enumerate(ids):
        lo, hi = int(tracks.offsets[s]), int(tracks.offsets[s + 1])
        a, m = tracks.aligned[lo:hi], tracks.matched[lo:hi]
        beg = 0
        for p in range(1, hi - lo + 1):
            if p == hi - lo or a[p] != a[beg] or m[p] != m[beg]:
                out.append("%s\t%d\t%d\t%d\t%d" % (name, beg, p, a[beg], m[beg]))
                beg = p
    return out


# ---- the case list ---------------------------------------------------------------------------------------------------------

SET_LENS = (17, 1024, 1025, 2049, 2100, 2100)  # the resident set: a string lands on the shortest sequences that hold it
LENGTHS_NAMED = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)
RESIDUES = (0, 1, 15)


def resident_set(seed=510):
    rng = random.Random(seed)
    return [rand_seq(rng, n) for n in SET_LENS]


def _fit(need, k):
    """The shortest sequence of the set with `need` bases or more (the two longest take turns)."""
    s = min(i for i, n in enumerate(SET_LENS) if n >= need)
    return s + (k & 1) if SET_LENS[s] == 2100 else s


def case_list():
    """[(name, q, t, rev, ops, slice or None, status, residue)] over resident_set(), in a fixed order.  Whole-string cases fill
    the rectangle of the whole pair; a slice comes with its true skips unless the name says otherwise."""
    rng = random.Random(511)
    out = []

    def add(name, ops, rev=None, slice=None, status=0, pair=None, residue=None):
        k = len(out)
        need_q, need_t = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        q, t = pair if pair is not None else (_fit(need_q, k), _fit(need_t, k + (k >> 1)))
        out.append((name, q, t, int(k % 2 if rev is None else rev), ops, slice, status, RESIDUES[k % 3] if residue is None else residue))

    for n in LENGTHS_NAMED:
        for res in RESIDUES:
            add("runs n=%d at residue %d" % (n, res), X.random_ops(rng, n), residue=res)
            add("alignment-like n=%d at residue %d" % (n, res), N.random_ops_long(rng, n), residue=res)
        add("all M n=%d" % n, b"M" * n)
        add("alternating n=%d" % n, (b"MX" * n)[:n])
        add("alternating gaps n=%d" % n, (b"MIXD" * n)[:n])
    for res in RESIDUES:  # an aligned run, and an 'M' run inside it, across a lane's 16 bytes and a chunk's 1,024
        for edge in (16, 1024):
            e = edge - res
            add("aligned run across byte %d" % edge, b"I" * (e - 5) + b"XXM" * 4 + b"D" * 3, residue=res)
            add("M run across byte %d" % edge, b"X" * (e - 5) + b"M" * 11 + b"X" * 2, residue=res)
            add("class change on byte %d" % edge, b"M" * e + b"I" * 2 + b"M" * 3, residue=res)
            add("class change on byte %d, X to M" % edge, b"X" * e + b"M" * 3, residue=res)
            add("gap ends on byte %d" % edge, b"M" * 2 + b"D" * (e - 2) + b"X" * 2 + b"M", residue=res)
            add("string ends on byte %d" % edge, b"D" * 3 + b"M" * (e - 3), residue=res)
            add("string ends one behind byte %d" % edge, b"M" * e + b"X", residue=res)
    add("begins with a gap", b"III" + b"M" * 30 + b"X")
    add("begins with both gaps", b"DDII" + b"M" * 30)
    add("ends in a gap", b"M" * 20 + b"X" + b"DDD")
    add("ends in X", b"M" * 40 + b"XX")
    add("ends in X behind a gap", b"M" * 40 + b"I" + b"X")
    add("all gaps", b"IIIDDDDIID")
    add("all gaps over a chunk", b"I" * 700 + b"D" * 700)
    add("all X", b"X" * 1100)
    add("fills both sequences exactly", b"M" * 17, pair=(0, 0))
    add("fills both sequences exactly, reverse", b"MX" * 8 + b"M", rev=1, pair=(0, 0))
    add("a sequence against itself over two chunks", b"M" * 1000 + b"X" * 25, pair=(2, 2))
    add("not completed", b"MMXMMIIMM", status=NOT_COMPLETED)
    add("a stray byte at column 0", b"N" + b"M" * 40)
    add("a stray byte at the last column", b"M" * 40 + b"=")
    add("a stray byte at the last column of the second chunk", b"M" * 1500 + b"?")
    add("a stray zero byte", b"MM\x00MM")
    add("one base too long for the query", b"M" * 17 + b"D", pair=(0, 1))
    add("one base too long for the target", b"M" * 17 + b"I", pair=(1, 0))
    add("one base too long for the query, reverse", b"M" * 17 + b"D", rev=1, pair=(0, 1))
    mixed = X.random_ops(rng, 2200)
    while 2200 - min(mixed.count(b"I"), mixed.count(b"D")) > 2100:  # (it has to fit the two longest sequences)
        mixed = X.random_ops(rng, 2200)
    for k, (b, e) in enumerate(((0, 2200), (1, 2199), (15, 17), (16, 1040), (1023, 1025), (1024, 2049), (700, 700), (2200, 2200), (333, 1777))):
        sl = (b, e, b - mixed[:b].count(b"I"), b - mixed[:b].count(b"D"))
        add("slice [%d, %d)" % (b, e), mixed, slice=sl, pair=(4, 5) if k % 2 else (5, 4))
    add("slice with skips of its own", b"M" * 30, slice=(10, 20, 1000, 7), pair=(3, 4))
    add("slice whose skip leaves too little", b"M" * 30, slice=(10, 20, 2040, 0), pair=(3, 4))
    add("slice whose skip is beyond the sequence", b"M" * 30, slice=(10, 10, 5000, 0), pair=(3, 4))
    add("slice that cuts off a stray byte", b"MMMM?MMMM", slice=(5, 9, 5, 5))
    add("slice that keeps a stray byte", b"MMMM?MMMM", slice=(4, 9, 4, 4))
    return out


def case_item(case):
    """(ops of the item, skips) of a case: the slice's columns and skips, or the whole string."""
    _, _, _, _, ops, sl, _, _ = case
    return (ops, (0, 0)) if sl is None else (ops[sl[0]:sl[1]], (sl[2], sl[3]))


def expected_items(cases):
    """[(code, aligned_cols, matched_cols, boundaries)] of the cases."""
    out = []
    for case in cases:
        _, q, t, _, _, _, status, _ = case
        ops, skips = case_item(case)
        code = SKIPPED if status != 0 else code_of(ops, (0, SET_LENS[q], 0, SET_LENS[t]), skips)
        out.append((code,) + (counts_of(ops) if code == OK else (0, 0, 0)))
    return out


def expected_tracks(cases, roles, times=1):
    tr = Tracks(SET_LENS)
    for case in cases:
        _, q, t, rev, _, _, status, _ = case
        ops, skips = case_item(case)
        if status == 0:
            tr.add(q, t, ops, "-" if rev else "+", roles, skips=skips, times=times)
    return tr


def random_alignments(seed=512, count=300):
    """[(qlen, tlen, span, strand, ops, slice or None)]: 300 alignments of 0 .. 2,600 columns; every third one is a range's
    rectangle inside longer sequences, every fourth one a slice with its true skips."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.choice([0, 1, 2, 15, 16, 17, 31, 1023, 1024, 1025]) if k % 5 == 0 else rng.randint(0, 2600)
        ops = N.random_ops_long(rng, n) if k % 2 else X.random_ops(rng, n)
        need_q, need_t = n - ops.count(b"I"), n - ops.count(b"D")
        fl = [rng.randint(0, 9) if k % 3 == 0 else 0 for _ in range(4)]
        span = (fl[0], fl[0] + need_q, fl[2], fl[2] + need_t)
        sl = None
        if k % 4 == 0:
            b = rng.randint(0, n)
            e = rng.randint(b, n)
            sl = (b, e, b - ops[:b].count(b"I"), b - ops[:b].count(b"D"))
        out.append((span[1] + fl[1], span[3] + fl[3], span, "-" if k % 2 else "+", ops, sl))
    return out
