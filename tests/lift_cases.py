"""What the tests of the liftover share (csrc/lift_device.hpp, csrc/lift.hip): a Python restatement of the contract in
include/allwave_hip.h (lift_of: the two columns by their definitions, over per-column position lists), a brute-force reading of
the same sentence (brute_of: enumerate the columns, filter, take min and max), the formats of the command-line tool, and the case
list -- the smallest shapes at which the kernel's walk and its probes can go wrong, over a small resident set."""
import random
import re

import cs_cases as X
import normalize_cases as N
from util import rand_seq

OK, SKIPPED, BAD_OP, LENGTHS, UNALIGNED, OUTSIDE = range(6)
FROM_TARGET, FROM_QUERY = 1, 2
SIDES = (FROM_TARGET, FROM_QUERY)
SIDE_NAMES = {FROM_TARGET: "target", FROM_QUERY: "query", 3: "both"}
NOT_COMPLETED = 1  # awv_result.status of a case that has a string and no lift (AWV_ST_CAPACITY)
FIELDS = ("code", "col_beg", "col_end", "q_skip", "t_skip", "src_beg", "src_end", "dst_beg", "dst_end", "num_matches", "num_mismatches", "num_ins", "num_del")
ROW_FIELDS = ("region", "q_idx", "t_idx", "flags", "src_beg", "src_end", "dst_beg", "dst_end", "num_matches", "num_mismatches", "num_ins", "num_del")
ROW_REVCOMP, ROW_FROM_QUERY = 1, 2


def only(code):
    return (code,) + (0,) * 12


def _walk(ops, span, strand, sl, status, frm, beg, end, qlen):
    """What lift_of and brute_of share: the item's code, else the item's columns with their positions and the interval in the
    item's own coordinates."""
    if status != 0:
        return SKIPPED, None
    cb, ce, q_skip, t_skip = (0, len(ops), 0, 0) if sl is None else sl
    item = ops[cb:ce]
    pb, pe, tb, te = span
    if set(item) - set(b"MXID"):
        return BAD_OP, None
    if q_skip + len(item) - item.count(b"I") > pe - pb or t_skip + len(item) - item.count(b"D") > te - tb:
        return LENGTHS, None
    a, b = (qlen - end, qlen - beg) if frm == FROM_QUERY and strand == "-" else (beg, end)
    xs, ys = [], []
    x, y = pb + q_skip, tb + t_skip
    for op in item:
        xs.append(x)
        ys.append(y)
        x += op != ord("I")
        y += op != ord("D")
    src, s0, s1 = (ys, tb + t_skip, y) if frm == FROM_TARGET else (xs, pb + q_skip, x)
    return OK, (item, cb, q_skip, t_skip, xs, ys, src, s0, s1, a, b)


def _result(w, strand, frm, qlen, kb, ke):
    item, cb, q_skip, t_skip, xs, ys, _, _, _, _, _ = w
    core = item[kb:ke]
    x0, x1, y0, y1 = xs[kb], xs[ke - 1] + 1, ys[kb], ys[ke - 1] + 1
    qi = (qlen - x1, qlen - x0) if strand == "-" else (x0, x1)
    s, d = ((y0, y1), qi) if frm == FROM_TARGET else (qi, (y0, y1))
    return (OK, cb + kb, cb + ke, q_skip + kb - item[:kb].count(b"I"), t_skip + kb - item[:kb].count(b"D"), s[0], s[1], d[0], d[1],
            core.count(b"M"), core.count(b"X"), core.count(b"I"), core.count(b"D"))


def lift_of(ops, span, strand, frm, beg, end, qlen, sl=None, status=0):
    """The contract, restated: [beg, end) of the source's forward strand through the op string `ops` (its slice sl = (col_beg,
    col_end, q_skip, t_skip)) over the rectangle span = (pb, pe, tb, te) of a query of qlen bases.  strand "-": the pattern is the
    query's reverse complement.  Returns the 13 FIELDS of an awv_lift_result."""
    code, w = _walk(ops, span, strand, sl, status, frm, beg, end, qlen)
    if code != OK:
        return only(code)
    item, src, s0, s1, a, b = w[0], w[6], w[7], w[8], w[9], w[10]
    if max(a, s0) >= min(b, s1):
        return only(OUTSIDE)
    n = len(item)
    col_beg = min([k for k in range(n) if item[k] in b"MX" and src[k] >= a], default=n)
    col_end = 1 + max([k for k in range(n) if item[k] in b"MX" and src[k] < b], default=-1)
    if col_beg >= col_end:
        return only(UNALIGNED)
    return _result(w, strand, frm, qlen, col_beg, col_end)


def brute_of(ops, span, strand, frm, beg, end, qlen, sl=None, status=0):
    """The same sentence read the other way: the aligned columns whose source position lies in the interval; the first and the last."""
    code, w = _walk(ops, span, strand, sl, status, frm, beg, end, qlen)
    if code != OK:
        return only(code)
    item, src, s0, s1, a, b = w[0], w[6], w[7], w[8], w[9], w[10]
    consuming = [k for k in range(len(item)) if item[k] != (ord("D") if frm == FROM_TARGET else ord("I")) and a <= src[k] < b]
    if not consuming:
        assert not (max(a, s0) < min(b, s1))
        return only(OUTSIDE)
    inside = [k for k in consuming if item[k] in b"MX"]
    if not inside:
        return only(UNALIGNED)
    return _result(w, strand, frm, qlen, min(inside), max(inside) + 1)


def span_of_range(r, lens):
    """(q, t, strand, span) of a range (q_idx, t_idx, q_revcomp, q_beg, q_end, t_beg, t_end), the query interval on its forward strand."""
    q, t, rev, qb, qe, tb, te = (int(v) for v in r)
    return q, t, "-" if rev else "+", ((lens[q] - qe, lens[q] - qb, tb, te) if rev else (qb, qe, tb, te))


# ---- the table and the command-line tool's files --------------------------------------------------------------------------

def parse_bed(text, ids, lens):
    """(regions [(seq, beg, end)], labels, [(line, class)] of the bad lines) of a BED text, as the command-line tool reads it: three
    or more tab-separated columns, names resolved against the FASTA's, 0 <= beg < end <= length, a non-empty fourth column the
    label (else '.'); empty lines and lines that begin with '#', 'track' or 'browser' are no regions and no errors."""
    where = {}
    for k, name in enumerate(ids):
        where.setdefault(name, k)
    regions, labels, bad = [], [], []
    for no, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line.strip(" \t") or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t")
        if len(f) < 3:
            bad.append((no, "bad_line"))
        elif f[0] not in where:
            bad.append((no, "unknown_name"))
        elif not (f[1].isascii() and f[1].isdigit() and f[2].isascii() and f[2].isdigit() and int(f[1]) < int(f[2]) <= lens[where[f[0]]]):
            bad.append((no, "bad_line"))
        else:
            regions.append((where[f[0]], int(f[1]), int(f[2])))
            labels.append(f[3] if len(f) > 3 and f[3] else ".")
    return regions, labels, bad


def format_rows(rows, regions, labels, ids):
    """The lines of the command-line tool's --liftover-out file, one per row in the table's order."""
    out = []
    for r in rows:
        r = dict(zip(ROW_FIELDS, (int(v) for v in r)))
        src, dst = (r["q_idx"], r["t_idx"]) if r["flags"] & ROW_FROM_QUERY else (r["t_idx"], r["q_idx"])
        assert regions[r["region"]][0] == src
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d" % (ids[src], r["src_beg"], r["src_end"], labels[r["region"]], ids[dst], r["dst_beg"], r["dst_end"],
                                                                      "-" if r["flags"] & ROW_REVCOMP else "+", r["num_matches"], r["num_mismatches"], r["num_ins"],
                                                                      r["num_del"]))
    return out


def rows_of(regions, from_mask, items, lens):
    """The table an engine holds after lifting `regions` through items = [(q, t, rev, ops, span or None, slice or None)]: the OK
    lifts of every region on an item's target (from_mask & 1) or query (& 2), as sorted ROW_FIELDS tuples."""
    rows = []
    for q, t, rev, ops, span, sl in items:
        span = (0, lens[q], 0, lens[t]) if span is None else span
        for g, (seq, beg, end) in enumerate(regions):
            for frm in SIDES:
                if from_mask & frm and seq == (t if frm == FROM_TARGET else q):
                    r = lift_of(ops, span, "-" if rev else "+", frm, beg, end, lens[q], sl=sl)
                    if r[0] == OK:
                        rows.append((g, q, t, (ROW_REVCOMP if rev else 0) | (ROW_FROM_QUERY if frm == FROM_QUERY else 0)) + r[5:])
    return sorted(rows)


_CG = re.compile(r"(\d+)([=XID])")


def items_from_paf(lines, ids, lens):
    """[(q, t, rev, ops, span, None)] of a PAF's lines, from columns 1-9 and cg:Z: alone: the op bytes ('=' is M; the PAF's I
    consumes the query, which is 'D' in op bytes, its D the target, 'I'), the rectangle in the coordinates of the aligned copy."""
    where = {name: k for k, name in enumerate(ids)}
    items = []
    for line in lines:
        f = line.rstrip("\n").split("\t")
        q, t, rev = where[f[0]], where[f[5]], f[4] == "-"
        qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0][5:]
        ops = b"".join({"=": b"M", "X": b"X", "I": b"D", "D": b"I"}[op] * int(n) for n, op in _CG.findall(cg))
        items.append((q, t, int(rev), ops, ((lens[q] - qe, lens[q] - qs) if rev else (qs, qe)) + (ts, te), None))
    return items


# ---- the case list ---------------------------------------------------------------------------------------------------------

SET_LENS = (17, 1024, 1025, 2049, 2100, 2100, 9000, 9000)  # the resident set: a string lands on the shortest sequences that hold it
LENGTHS_NAMED = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)
RESIDUES = (0, 1, 15)


def resident_set(seed=530):
    rng = random.Random(seed)
    return [rand_seq(rng, n) for n in SET_LENS]


def _fit(need, k):
    s = min(i for i, n in enumerate(SET_LENS) if n >= need)
    return s + (k & 1) if SET_LENS[s] in (2100, 9000) else s


def _around(rng, frm, lo, hi, length, count):
    """`count` random intervals of the source, of which most meet [lo, hi) (clamped to the sequence)."""
    out = []
    for _ in range(count):
        b = rng.randint(max(lo - 3, 0), max(min(hi + 2, length - 1), 0))
        e = rng.randint(b + 1, min(b + rng.choice([1, 2, 5, 40, 3000]), length))
        out.append((frm, b, e))
    return out


def case_list():
    """[(name, q, t, rev, ops, slice or None, status, residue, queries)] over resident_set(), in a fixed order; queries =
    [(from, beg, end)], valid on the source sequence.  Whole-string cases have the rectangle of the whole pair."""
    rng = random.Random(531)
    out = []

    def add(name, ops, queries, rev=None, slice=None, status=0, pair=None, residue=None, both_sides=False):
        k = len(out)
        need_q, need_t = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        q, t = pair if pair is not None else (_fit(need_q, k), _fit(need_t, k + (k >> 1)))
        rev = int(k % 2 if rev is None else rev)
        qs = []
        for frm, b, e in (queries(q, t, rev) if callable(queries) else queries):
            qs.append((frm, b, e))
            if both_sides:
                qs.append((3 - frm, b, e))
        for frm, b, e in qs:
            assert 0 <= b < e <= SET_LENS[t if frm == FROM_TARGET else q], (name, frm, b, e)
        out.append((name, q, t, rev, ops, slice, status, RESIDUES[k % 3] if residue is None else residue, qs))

    def standard(ops, n_random=6):
        """the whole sequences, random intervals around the consumed spans, 1-base intervals: from both sides"""
        def make(q, t, rev):
            qs = []
            for frm, length, used in ((FROM_TARGET, SET_LENS[t], len(ops) - ops.count(b"D")), (FROM_QUERY, SET_LENS[q], len(ops) - ops.count(b"I"))):
                lo, hi = (length - used, length) if frm == FROM_QUERY and rev else (0, used)
                qs.append((frm, 0, length))
                qs += _around(rng, frm, lo, hi, length, n_random)
                qs += [(frm, p, p + 1) for p in sorted({lo, max(hi - 1, 0), rng.randint(lo, max(hi - 1, lo))}) if p < length]
            return qs
        return make

    for n in LENGTHS_NAMED:
        for res in RESIDUES:
            ops = X.random_ops(rng, n)
            add("runs n=%d at residue %d" % (n, res), ops, standard(ops), residue=res)
            ops = N.random_ops_long(rng, n)
            add("alignment-like n=%d at residue %d" % (n, res), ops, standard(ops), residue=res)
        add("all M n=%d" % n, b"M" * n, standard(b"M" * n))
        ops = (b"MIXD" * n)[:n]
        add("alternating gaps n=%d" % n, ops, standard(ops))
    # a probe's answer in the last column of a lane's 16 bytes, the first of the next lane, the last column of a chunk, the
    # first of the next chunk: forward pairs of all-aligned columns, so source position = column = byte - residue
    for res in RESIDUES:
        ops = (b"MX" * 1100)[:2049]
        qs = []
        for byte in (15, 16, 1023, 1024, 2047, 2048):
            col = byte - res
            qs += [(FROM_TARGET, col, col + 3), (FROM_TARGET, max(col - 3, 0), col + 1), (FROM_QUERY, col, col + 1), (FROM_QUERY, max(col - 1, 0), col + 2)]
        add("answers on lane and chunk edges at residue %d" % res, ops, qs, rev=0, residue=res, pair=(4, 5))
    # a source-only gap run across a chunk boundary that holds the interval's begin (it resolves a chunk later) or its end (a chunk earlier)
    for res in RESIDUES:
        ops = b"M" * 1000 + b"I" * 60 + b"M" * 500  # 'I' consumes the text only: source-only from the target
        add("text-only run across byte 1024 at residue %d" % res, ops,
            [(FROM_TARGET, 1010, 1200), (FROM_TARGET, 900, 1030), (FROM_TARGET, 1005, 1050), (FROM_TARGET, 1000, 1060), (FROM_TARGET, 999, 1061), (FROM_TARGET, 1059, 1061)],
            rev=0, residue=res)
        ops = b"X" * 1000 + b"D" * 60 + b"M" * 500
        add("pattern-only run across byte 1024 at residue %d, reverse" % res, ops,
            [(FROM_QUERY, SET_LENS[3] - e, SET_LENS[3] - b) for b, e in ((1010, 1200), (900, 1030), (1005, 1050), (1000, 1060), (999, 1061))], rev=1, residue=res, pair=(3, 3))
    # a destination-only run at each edge of an interval: excluded; inside: included
    edges = b"M" * 10 + b"D" * 5 + b"M" * 10 + b"D" * 4 + b"X" * 10
    add("pattern-only runs at the edges, from the target", edges, [(FROM_TARGET, 10, 20), (FROM_TARGET, 9, 21), (FROM_TARGET, 0, 30), (FROM_TARGET, 10, 11)], rev=0)
    edges = b"M" * 10 + b"I" * 5 + b"M" * 10 + b"I" * 4 + b"X" * 10
    add("text-only runs at the edges, from the query", edges, [(FROM_QUERY, 10, 20), (FROM_QUERY, 9, 21), (FROM_QUERY, 0, 30), (FROM_QUERY, 19, 20)], rev=0)
    # more than 64 queries answered inside one chunk; many of them equal
    ops = N.random_ops_long(rng, 900)
    add("300 queries inside one chunk", ops, lambda q, t, rev: _around(rng, FROM_TARGET, 0, 800, SET_LENS[t], 200) + _around(rng, FROM_QUERY, 0, 800, SET_LENS[q], 100), residue=15)
    add("130 queries with one answer", b"D" * 3 + b"M" * 500, [(FROM_TARGET, 7, 9)] * 70 + [(FROM_QUERY, 0, 600)] * 60, rev=0)
    # many chunks with no query, queries only in the first and in the last chunk; and a long string with queries all over
    ops = N.random_ops_long(rng, 8800)
    add("eight chunks, queries at both ends only", ops, [(FROM_TARGET, 3, 20), (FROM_TARGET, 8650, 8700), (FROM_QUERY, 8640, 8660), (FROM_QUERY, 0, 2), (FROM_TARGET, 1, 8999)])
    add("eight chunks, queries all over", ops, standard(ops, n_random=40))
    # nested, duplicate and 1-base intervals on every column type
    ops = b"MMXIIMDDXMIDMXDIMM"
    used_t, used_q = len(ops) - ops.count(b"D"), len(ops) - ops.count(b"I")
    add("every 1-base interval, nested and duplicate ones", ops,
        [(FROM_TARGET, p, p + 1) for p in range(used_t)] + [(FROM_QUERY, p, p + 1) for p in range(used_q)] +
        [(FROM_TARGET, 1, 13), (FROM_TARGET, 3, 9), (FROM_TARGET, 4, 5), (FROM_TARGET, 3, 9), (FROM_QUERY, 1, 13), (FROM_QUERY, 5, 8), (FROM_QUERY, 5, 8)], rev=0, pair=(0, 0))
    add("every 1-base interval, reverse", ops, [(FROM_QUERY, p, p + 1) for p in range(17)] + [(FROM_TARGET, p, p + 1) for p in range(17)], rev=1, pair=(0, 0))
    # intervals that cover, overhang, touch and miss the item's source span
    add("a string shorter than its rectangle", b"XMMMMIMMMM", [(1, 0, 17), (1, 0, 10), (1, 9, 12), (1, 10, 12), (1, 12, 17), (1, 8, 9)], pair=(0, 0), rev=0, both_sides=True)
    add("a string shorter than its rectangle, reverse", b"XMMMMDMMMM", [(FROM_QUERY, 0, 17), (FROM_QUERY, 7, 17), (FROM_QUERY, 5, 8), (FROM_QUERY, 5, 7), (FROM_QUERY, 0, 5), (FROM_QUERY, 16, 17),
                                                                         (FROM_TARGET, 0, 17), (FROM_TARGET, 9, 11), (FROM_TARGET, 8, 9)], pair=(0, 0), rev=1)
    add("a slice whose span begins behind its skips", b"M" * 30, [(1, 0, 2049), (1, 0, 12), (1, 0, 10), (1, 19, 25), (1, 20, 25), (1, 12, 13), (2, 1000, 1015), (2, 1009, 1011), (2, 1020, 1021)],
        slice=(10, 20, 1010, 10), pair=(3, 3), rev=0)
    add("all gaps", b"IIIDDDDIID", standard(b"IIIDDDDIID"))
    add("all gaps over a chunk", b"I" * 700 + b"D" * 700, standard(b"I" * 700 + b"D" * 700))
    # slices with skips
    mixed = X.random_ops(rng, 2200)
    while 2200 - min(mixed.count(b"I"), mixed.count(b"D")) > 2100:
        mixed = X.random_ops(rng, 2200)
    for k, (b, e) in enumerate(((0, 2200), (1, 2199), (15, 17), (16, 1040), (1023, 1025), (1024, 2049), (700, 700), (2200, 2200), (333, 1777))):
        sl = (b, e, b - mixed[:b].count(b"I"), b - mixed[:b].count(b"D"))
        item = mixed[b:e]

        def make(q, t, rev, sl=sl, item=item):
            qs = []
            for frm, length, skip, used in ((FROM_TARGET, SET_LENS[t], sl[3], len(item) - item.count(b"D")), (FROM_QUERY, SET_LENS[q], sl[2], len(item) - item.count(b"I"))):
                lo, hi = (length - skip - used, length - skip) if frm == FROM_QUERY and rev else (skip, skip + used)
                qs += [(frm, 0, length)] + _around(rng, frm, lo, hi, length, 5)
            return qs
        add("slice [%d, %d)" % (b, e), mixed, make, slice=sl, pair=(4, 5) if k % 2 else (5, 4))
    add("slice whose skip leaves too little", b"M" * 30, [(1, 0, 100), (2, 2040, 2049)], slice=(10, 20, 2040, 0), pair=(3, 4))
    add("slice that cuts off a stray byte", b"MMMM?MMMM", [(1, 0, 17), (2, 6, 8)], slice=(5, 9, 5, 5), pair=(0, 0))
    add("slice that keeps a stray byte", b"MMMM?MMMM", [(1, 0, 17), (2, 6, 8)], slice=(4, 9, 4, 4), pair=(0, 0))
    # whole items without a lift
    add("not completed", b"MMXMMIIMM", [(1, 0, 5), (2, 2, 3)], status=NOT_COMPLETED)
    add("a stray byte behind the last query", b"M" * 1500 + b"?", [(1, 0, 10), (2, 5, 40), (1, 100, 101)])
    add("a stray byte at column 0", b"N" + b"M" * 40, [(1, 10, 20)])
    add("one base too long for the query", b"M" * 17 + b"D", [(1, 0, 17), (2, 3, 4)], pair=(0, 1))
    add("one base too long for the target", b"M" * 17 + b"I", [(1, 0, 17), (2, 3, 4)], pair=(1, 0))
    return out


def expected(cases):
    """Per case the FIELDS tuples of its queries."""
    out = []
    for name, q, t, rev, ops, sl, status, _, queries in cases:
        span = (0, SET_LENS[q], 0, SET_LENS[t])
        out.append([lift_of(ops, span, "-" if rev else "+", frm, b, e, SET_LENS[q], sl=sl, status=status) for frm, b, e in queries])
    return out


def range_case_list():
    """[(name, range, ops, queries)]: records of awv_lift_ranges, rectangles with non-zero pb and tb inside sequences 4 .. 7 of the
    resident set, on both strands; range = (q_idx, t_idx, q_revcomp, q_beg, q_end, t_beg, t_end)."""
    rng = random.Random(532)
    out = []
    for k, n in enumerate((0, 1, 16, 17, 300, 1023, 1025, 1900, 1900)):
        ops = N.random_ops_long(rng, n) if k % 2 else X.random_ops(rng, n)
        need_q, need_t = n - ops.count(b"I"), n - ops.count(b"D")
        q, t, rev = 4 + k % 4, 4 + (k + 1 + k // 4) % 4, k % 2
        qb, tb = 5 + 3 * k, 40 - 2 * k
        slack = k % 3  # the rectangle may be longer than what the string consumes
        r = (q, t, rev, qb, qb + need_q + slack, tb, tb + need_t + slack)
        lens = (SET_LENS[q], SET_LENS[t])
        qs = [(FROM_TARGET, 0, lens[1]), (FROM_QUERY, 0, lens[0])]
        qs += _around(rng, FROM_TARGET, tb, tb + need_t, lens[1], 6) + _around(rng, FROM_QUERY, qb, qb + need_q, lens[0], 6)
        qs += [(FROM_TARGET, max(tb - 1, 0), tb + 1), (FROM_QUERY, qb, qb + 1), (FROM_TARGET, tb + need_t, tb + need_t + 1)]
        out.append(("range %d of %d columns" % (k, n), r, ops, qs))
    return out


def flat_queries(case_queries, seed=533):
    """The cases' queries as one list [(record, from, beg, end)] in a shuffled order, and per case and query its place in it."""
    flat = [(i, frm, b, e) for i, qs in enumerate(case_queries) for frm, b, e in qs]
    order = list(range(len(flat)))
    random.Random(seed).shuffle(order)
    place = {}
    for pos, k in enumerate(order):
        place[k] = pos
    shuffled = [flat[k] for k in order]
    where, k = [], 0
    for qs in case_queries:
        where.append([place[k + j] for j in range(len(qs))])
        k += len(qs)
    return shuffled, where
