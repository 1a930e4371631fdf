"""What the tests of the allele table share (csrc/variants_device.hpp, csrc/variants.hip): a Python restatement of the contract in
include/allwave_hip.h -- a plain loop over columns into a dict keyed by the row key, with its own modular arithmetic in Python
integers; it knows nothing of lanes, chunks or runs owned by breaks -- an independent reading of a PAF's cg:Z:, and the case list:
the smallest shapes at which the kernel's walk, its hash scan and its carries can go wrong, over a small resident set."""
import random
import re

import numpy as np

import coverage_cases as V
import cs_cases as X
import normalize_cases as N
from util import rand_seq
from verify_cases import revcomp

OK, SKIPPED, BAD_OP, LENGTHS = range(4)
SNV, DEL, INS = 0, 1, 2
TYPE_NAMES = {SNV: "snv", DEL: "del", INS: "ins"}
NOT_COMPLETED = V.NOT_COMPLETED
MOD = (1 << 61) - 1
BASE = 0x1b873593a5c1f2e7
ROW_DTYPE = np.dtype([("t_idx", "<i4"), ("pos", "<i4"), ("type", "<i4"), ("len", "<i4"), ("hash", "<u8"), ("rep", "<u8"), ("count", "<u4"),
                      ("reserved", "<u4")])

code_of = V.code_of
case_item = V.case_item


def upper(c):
    return c - 32 if 97 <= c <= 122 else c


def hash_of(allele):
    h = 0
    for c in allele:
        h = (h * BASE + upper(c)) % MOD
    return h


def rep_of(q, rev, p_beg):
    return (q << 32) | (int(bool(rev)) << 31) | p_beg


def events_of(q, t, rev, pattern, ops, span, skips):
    """The contract, restated: (code, [(t, pos, type, len, hash, rep)] in column order) of the op string `ops` over the rectangle
    span = (pb, pe, tb, te) of the aligned copy `pattern` of query q (its reverse complement when rev) and target t, from the
    skips on.  No events unless the code is OK."""
    code = code_of(ops, span, skips)
    if code != OK:
        return code, []
    x, y = span[0] + skips[0], span[2] + skips[1]
    out = []
    gap = None  # the gap run in progress: [op, x, y, columns]
    for k, op in enumerate(ops):
        if op == ord("X"):
            out.append((t, y, SNV, 1, hash_of(pattern[x:x + 1]), rep_of(q, rev, x)))
        if op in b"ID":
            if gap is None:
                gap = [op, x, y, 0]
            gap[3] += 1
        x += op != ord("I")
        y += op != ord("D")
        if gap is not None and (k + 1 == len(ops) or ops[k + 1] != gap[0]):
            gop, gx, gy, n = gap
            if gop == ord("I"):
                out.append((t, gy, DEL, n, 0, rep_of(q, rev, gx)))
            else:
                out.append((t, gy, INS, n, hash_of(pattern[gx:gx + n]), rep_of(q, rev, gx)))
            gap = None
    return code, out


def counts_of(events):
    """(snv, ins, del) of an awv_var_item."""
    return tuple(sum(1 for e in events if e[2] == ty) for ty in (SNV, INS, DEL))


def as_rows(events):
    """Events in order as count-1 rows."""
    rows = np.zeros(len(events), dtype=ROW_DTYPE)
    for k, (t, pos, ty, n, h, rep) in enumerate(events):
        rows[k] = (t, pos, ty, n, h, rep, 1, 0)
    return rows


class Table:
    """The table: a dict from the row key to [count, rep]."""

    def __init__(self):
        self.rows = {}
        self.items = self.events = 0

    def add_events(self, events, times=1):
        for t, pos, ty, n, h, rep in events:
            row = self.rows.setdefault((t, pos, ty, n, h), [0, rep])
            row[0] += times
            row[1] = min(row[1], rep)
        self.events += len(events) * times

    def add(self, seqs, q, t, rev, ops, span=None, skips=(0, 0), times=1):
        """One item of the pair (q, t) of the set `seqs`, `times` times over; span None: the whole of both.  Returns its code."""
        pattern = revcomp(seqs[q]) if rev else seqs[q]
        span = (0, len(seqs[q]), 0, len(seqs[t])) if span is None else span
        code, events = events_of(q, t, rev, pattern, ops, span, skips)
        self.add_events(events, times)
        self.items += times
        return code

    def array(self):
        rows = np.zeros(len(self.rows), dtype=ROW_DTYPE)
        for k, key in enumerate(sorted(self.rows)):
            rows[k] = key + (self.rows[key][1], self.rows[key][0], 0)
        return rows


def same(a, b):
    """Exact equality of two structured arrays of rows."""
    return a.dtype == b.dtype == ROW_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


_CG = re.compile(r"(\d+)([=XIDM])")


def table_from_paf(lines, ids, seqs):
    """The table that a PAF's lines describe, from columns 1-9 and cg:Z: alone: the lines' run-length text expanded to op bytes
    (in a PAF 'I' consumes the query and 'D' the target: the engine's 'D' and 'I') over the rectangle the columns name."""
    where = {name: k for k, name in enumerate(ids)}
    tb = Table()
    for line in lines:
        f = line.rstrip("\n").split("\t")
        q, t, rev = where[f[0]], where[f[5]], f[4] == "-"
        qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0][5:]
        ops = b"".join({"=": b"M", "M": b"M", "X": b"X", "I": b"D", "D": b"I"}[op] * int(n) for n, op in _CG.findall(cg))
        span = (len(seqs[q]) - qe, len(seqs[q]) - qs, ts, te) if rev else (qs, qe, ts, te)
        assert tb.add(seqs, q, t, rev, ops, span=span) == OK, line
    return tb


def format_table(ids, seqs, rows, min_count=1):
    """The lines of the command-line tool's --variants file."""
    out = []
    for r in rows:
        if int(r["count"]) < min_count:
            continue
        t, pos, ty, n, rep = int(r["t_idx"]), int(r["pos"]), int(r["type"]), int(r["len"]), int(r["rep"])
        ref = seqs[t][pos:pos + n].decode().upper() if ty != INS else "."
        copy = revcomp(seqs[rep >> 32]) if (rep >> 31) & 1 else seqs[rep >> 32]
        alt = copy[rep & 0x7fffffff:(rep & 0x7fffffff) + n].decode().upper() if ty != DEL else "."
        out.append("%s\t%d\t%s\t%d\t%s\t%s\t%d" % (ids[t], pos, TYPE_NAMES[ty], n, ref, alt, int(r["count"])))
    return out


# ---- the case list ---------------------------------------------------------------------------------------------------------

SET_LENS = V.SET_LENS  # (17, 1024, 1025, 2049, 2100, 2100): a string lands on the shortest sequences that hold it
LENGTHS_NAMED = V.LENGTHS_NAMED
RESIDUES = V.RESIDUES


def resident_set(seed=530):
    """Sequence 4 holds lower-case letters and N; sequence 5 is its reverse complement, so that the q_revcomp copy of 5 is the
    upper-cased copy of 4: the same alleles through a forward and a reverse query."""
    rng = random.Random(seed)
    seqs = [rand_seq(rng, n) for n in SET_LENS[:4]] + [rand_seq(rng, SET_LENS[4], b"ACGTACGTacgtNn")]
    return seqs + [revcomp(seqs[4])]


def case_list():
    """[(name, q, t, rev, ops, slice or None, status, residue)] over resident_set(), in a fixed order.  Whole-string cases fill
    the rectangle of the whole pair; a slice comes with its true skips unless the name says otherwise."""
    rng = random.Random(531)
    out = []

    def add(name, ops, rev=None, slice=None, status=0, pair=None, residue=None):
        k = len(out)
        need_q, need_t = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        q, t = pair if pair is not None else (V._fit(need_q, k), V._fit(need_t, k + (k >> 1)))
        out.append((name, q, t, int(k % 2 if rev is None else rev), ops, slice, status, RESIDUES[k % 3] if residue is None else residue))

    for n in LENGTHS_NAMED:
        for res in RESIDUES:
            add("runs n=%d at residue %d" % (n, res), X.random_ops(rng, n), residue=res)
            add("alignment-like n=%d at residue %d" % (n, res), N.random_ops_long(rng, n), residue=res)
        add("all X n=%d" % n, b"X" * n)
        add("all D n=%d" % n, b"D" * n)
        add("all I n=%d" % n, b"I" * n)
        add("alternating gaps n=%d" % n, (b"MIXD" * n)[:n])
    for res in RESIDUES:
        add("X at column 0 and at the last column", b"X" + b"M" * 1500 + b"X", residue=res)
        add("a D run inside one lane", b"M" * (20 - res) + b"D" * 5 + b"M" * 9, residue=res)
        add("two D runs inside one lane", b"M" * (17 - res) + b"DDD" + b"M" + b"DDDD" + b"X" + b"DD" + b"M" * 9, residue=res)
        for edge in (16, 1024):
            e = edge - res
            add("a D run across byte %d" % edge, b"M" * (e - 5) + b"D" * 11 + b"M" * 2, residue=res)
            add("a D run ending on byte %d" % edge, b"M" * (e - 7) + b"D" * 7 + b"X" + b"M" * 3, residue=res)
            add("a D run beginning on byte %d" % edge, b"M" * e + b"D" * 6 + b"M" * 3, residue=res)
            add("an I run across byte %d" % edge, b"X" * (e - 5) + b"I" * 11 + b"X" * 2, residue=res)
            add("I then D across byte %d" % edge, b"M" * (e - 3) + b"III" + b"DDDD" + b"M", residue=res)
            add("D then I across byte %d" % edge, b"M" * (e - 3) + b"DDD" + b"IIII" + b"M", residue=res)
            add("the string ends in a D run on byte %d" % edge, b"M" * (e - 4) + b"D" * 4, residue=res)
        add("a D run across several lanes", b"M" * 7 + b"D" * 75 + b"M" * 5, residue=res)
        add("a D run over three chunks", b"M" * (1000 - res) + b"D" * 1090 + b"XM", residue=res, pair=(4, 3))
        add("a D run over three chunks that ends the string", b"X" * (900 - res) + b"D" * 1190, residue=res, pair=(5, 3))
        add("a D run from column 0 over a chunk", b"D" * 1030 + b"M" * 4, residue=res)
        add("an I run over three chunks", b"M" * (1000 - res) + b"I" * 1060 + b"XM", residue=res, pair=(1, 4))
    add("begins with both gaps", b"DDII" + b"M" * 30)
    add("ends in an I run", b"M" * 20 + b"X" + b"III")
    add("I directly followed by D, and the reverse", b"MM" + b"II" + b"DDD" + b"M" + b"DD" + b"I" + b"MM")
    # two different insertions of equal length at one site of target 3: two rows
    add("an insertion of 3 before base 10, from query 1", b"M" * 10 + b"DDD" + b"M" * 20, rev=0, pair=(1, 3))
    add("an insertion of 3 before base 10, from query 2", b"M" * 10 + b"DDD" + b"M" * 20, rev=0, pair=(2, 3))
    # the same alleles through a forward query and the q_revcomp copy of its reverse complement: one row each, count 2
    shared = b"M" * 30 + b"X" + b"M" * 8 + b"D" * 21 + b"M" * 1000 + b"XX" + b"I" * 3 + b"M" * 5 + b"D" * 2
    add("an alignment of query 4, forward", shared, rev=0, pair=(4, 3))
    add("the same alignment of query 5's reverse complement", shared, rev=1, pair=(5, 3))
    add("lower case and N in the alleles", b"X" * 40 + b"D" * 40 + b"M" * 3 + b"D" * 17 + b"X", rev=0, pair=(4, 2))
    add("fills both sequences exactly", b"X" * 17, pair=(0, 0))
    add("an insertion before tlen", b"M" * 17 + b"D" * 9, pair=(1, 0))
    add("a deletion of the whole target", b"I" * 17, pair=(1, 0))
    add("not completed", b"MMXMMIIMM", status=NOT_COMPLETED)
    add("a stray byte at column 0", b"N" + b"X" * 40)
    add("a stray byte at the last column", b"XD" * 20 + b"=")
    add("a stray byte at the last column of the second chunk", b"X" * 1500 + b"?")
    add("one base too long for the query", b"X" * 17 + b"D", pair=(0, 1))
    add("one base too long for the target", b"X" * 17 + b"I", pair=(1, 0))
    add("one base too long for the query, reverse", b"X" * 17 + b"D", rev=1, pair=(0, 1))
    mixed = X.random_ops(rng, 2200)
    while 2200 - min(mixed.count(b"I"), mixed.count(b"D")) > 2100:  # (it has to fit the two longest sequences)
        mixed = X.random_ops(rng, 2200)
    for k, (b, e) in enumerate(((0, 2200), (1, 2199), (15, 17), (16, 1040), (1023, 1025), (1024, 2049), (700, 700), (2200, 2200), (333, 1777))):
        sl = (b, e, b - mixed[:b].count(b"I"), b - mixed[:b].count(b"D"))
        add("slice [%d, %d)" % (b, e), mixed, slice=sl, pair=(4, 5) if k % 2 else (5, 4))
    cut = b"M" * 10 + b"I" * 12 + b"M" * 10 + b"D" * 12 + b"M" * 10
    add("a slice that cuts an I run on both sides", cut, slice=(14, 19, 10, 14), pair=(1, 2))
    add("a slice that cuts a D run on both sides", cut, slice=(36, 41, 24, 32), pair=(1, 2))
    add("a slice from inside the I run to inside the D run", cut, slice=(15, 40, 10, 15), pair=(1, 2))
    add("slice with skips of its own", b"X" * 30, slice=(10, 20, 1000, 7), pair=(3, 4))
    add("slice whose skip leaves too little", b"X" * 30, slice=(10, 20, 2040, 0), pair=(3, 4))
    add("slice that cuts off a stray byte", b"XXXX?XXXX", slice=(5, 9, 5, 5))
    add("slice that keeps a stray byte", b"XXXX?XXXX", slice=(4, 9, 4, 4))
    return out


def case_events(seqs, case):
    """(code, events) of a case."""
    _, q, t, rev, _, _, status, _ = case
    if status != 0:
        return SKIPPED, []
    ops, skips = case_item(case)
    return events_of(q, t, rev, revcomp(seqs[q]) if rev else seqs[q], ops, (0, len(seqs[q]), 0, len(seqs[t])), skips)


def expected_items(seqs, cases):
    """[(code, snv, ins, del)] of the cases."""
    out = []
    for case in cases:
        code, events = case_events(seqs, case)
        out.append((code,) + counts_of(events))
    return out


def expected_table(seqs, cases, times=1):
    tb = Table()
    for case in cases:
        tb.add_events(case_events(seqs, case)[1], times)
        tb.items += times
    return tb


def random_items(seed=532, count=300):
    """[(q_idx, t_idx, rev, pattern, tlen, span, ops, slice or None)]: coverage_cases' 300 random alignments with a pattern each --
    both strands, every third one a range's rectangle inside longer sequences, every fourth one a slice with its true skips."""
    rng = random.Random(seed)
    out = []
    for k, (qlen, tlen, span, strand, ops, sl) in enumerate(V.random_alignments(seed, count)):
        out.append((k % 7, k % 5, strand == "-", rand_seq(rng, qlen, b"ACGTacgtN" if k % 6 == 0 else b"ACGT"), tlen, span, ops, sl))
    return out
