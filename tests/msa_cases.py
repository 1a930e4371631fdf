"""The target-anchored multiple alignment (include/allwave_hip.h, csrc/msa_device.hpp) restated in Python, and the case list the
CPU and GPU tests share: msa_of is a per-column reading of the contract that shares no code with the product."""
import random
import re

import numpy as np

from util import rand_seq
from verify_cases import revcomp

OK, SKIPPED, BAD_OP, LENGTHS, NOT_CHOSEN = 0, 1, 2, 3, 4
NOT_COMPLETED = 1  # awv_result.status of a case that has a string and no row (AWV_ST_CAPACITY)
ITEM_FIELDS = ("code", "target", "row", "bases", "col_beg", "col_end")
TARGET_FIELDS = ("t_idx", "rows", "width", "off")

KNOWN = dict(text=b"CGATCGATAAATAGAGTAGGAATAGCA", pattern=b"CGATCGAATAGAGTAGGTCGAATTGCA", ops=b"MMMMMMIIIMMMMMMMMMMDDDMMMMXMMM",
             row0=b"CGATCGATAAATAGAGTAG---GAATAGCA", row1=b"CGATCG---AATAGAGTAGGTCGAATTGCA", row2=b"CGATCGATAAATAGAGTAGT--GAATAGCA")
KNOWN["pattern2"] = KNOWN["text"][:19] + b"T" + KNOWN["text"][19:]
KNOWN["ops2"] = b"M" * 19 + b"D" + b"M" * 8


def upper(b):
    return b - 32 if 97 <= b <= 122 else b


def item_code(ops, span, skips):
    """The code of one op string over what its rectangle leaves behind the skips."""
    if any(o not in b"MXID" for o in ops):
        return BAD_OP
    pb, pe, tb, te = span
    if len(ops) - ops.count(b"I") > pe - pb - skips[0] or len(ops) - ops.count(b"D") > te - tb - skips[1]:
        return LENGTHS
    return OK


def msa_of(seqs, targets, items):
    """The whole call.  seqs: the resident sequences; targets: distinct indices; items: [(q, t, rev, ops, span or None, slice or
    None, status)] with ops the whole op string, span (pb, pe, tb, te) in pattern / text coordinates and slice (col_beg, col_end,
    q_skip, t_skip).  Returns dict(items=[(code, target, row, bases, col_beg, col_end)], targets=[(t_idx, rows, width, off)],
    blocks=[2-D uint8 array per target], ins=[widths per target], runs, bases, columns, failed, bytes)."""
    where = {s: j for j, s in enumerate(targets)}
    ins = [[0] * (len(seqs[s]) + 1) for s in targets]
    walked = []  # per item: None, or (j, pattern, ops, x0, y0)
    codes = []
    columns = failed = runs = 0
    for q, t, rev, ops, span, sl, status in items:
        if t not in where:
            codes.append(NOT_CHOSEN)
            walked.append(None)
            continue
        if status != 0:
            codes.append(SKIPPED)
            walked.append(None)
            continue
        pattern = revcomp(seqs[q]) if rev else bytes(seqs[q])
        span = (0, len(pattern), 0, len(seqs[t])) if span is None else span
        skips = (0, 0)
        if sl is not None:
            ops, skips = ops[sl[0]:sl[1]], (sl[2], sl[3])
        code = item_code(ops, span, skips)
        codes.append(code)
        columns += len(ops)
        failed += code != OK
        walked.append((where[t], pattern, ops, span[0] + skips[0], span[2] + skips[1]) if code == OK else None)
    for w in walked:  # the widths: the widest 'D' run at every slot
        if w is None:
            continue
        j, _, ops, _, y = w
        run = 0
        for op in ops + b"\0":
            if op == ord("D"):
                run += 1
                continue
            if run:
                ins[j][y] = max(ins[j][y], run)
                runs += 1
                run = 0
            y += 1
    cols = []
    for j in range(len(targets)):
        acc, c = 0, []
        for p, w in enumerate(ins[j]):
            acc += w
            c.append(p + acc)
        cols.append(c)
    rows = [1] * len(targets)
    out_items, placed = [], []
    for code, w in zip(codes, walked):
        if w is None:
            out_items.append((code, -1 if code == NOT_CHOSEN else None, 0, 0, 0, 0))
            continue
        j, pattern, ops, x, y = w
        at, k = {}, 0
        for op in ops:
            k = k + 1 if op == ord("D") else 0
            if op == ord("D"):
                at[cols[j][y] - ins[j][y] + k - 1] = upper(pattern[x])
            elif op != ord("I"):
                at[cols[j][y]] = upper(pattern[x])
            x += op != ord("I")
            y += op != ord("D")
        out_items.append((OK, j, rows[j], len(at), min(at) if at else 0, max(at) + 1 if at else 0))
        placed.append((j, rows[j], at))
        rows[j] += 1
    # (the target index of a skipped or failed item of a chosen target)
    out_items = [(c, where[items[i][1]] if tg is None else tg, r, b, cb, ce) for i, (c, tg, r, b, cb, ce) in enumerate(out_items)]
    blocks, tg_out, off = [], [], 0
    for j, s in enumerate(targets):
        W = cols[j][-1]
        blk = np.full((rows[j], W), ord("-"), dtype=np.uint8)
        for p, b in enumerate(seqs[s]):
            blk[0, cols[j][p]] = upper(b)
        blocks.append(blk)
        tg_out.append((s, rows[j], W, off))
        off += rows[j] * W
    for j, r, at in placed:
        for c, b in at.items():
            blocks[j][r, c] = b
    return dict(items=out_items, targets=tg_out, blocks=blocks, ins=ins, runs=runs, bases=sum(i[3] for i in out_items), columns=columns,
                failed=failed, bytes=off)


def arena_of(blocks):
    """The blocks as the one arena a call returns."""
    return np.concatenate([b.reshape(-1) for b in blocks]) if blocks else np.zeros(0, dtype=np.uint8)


def ops_from_rows(row0, row):
    """Reads an item's row against the target's column by column: the op string up to M / X ('M' for both), over the item's
    span of non-gap columns of either row.  A column where both rows hold '-' is dropped."""
    nz = [c for c in range(len(row)) if row[c] != ord("-")]
    if not nz:
        return b""
    out = bytearray()
    for c in range(len(row)):
        a, b = row0[c] != ord("-"), row[c] != ord("-")
        if a and b:
            out += b"M"
        elif b:
            out += b"D"
        elif a and nz[0] < c < nz[-1]:
            out += b"I"
    return bytes(out)


def expand(spec):
    """"6M3I" -> b"MMMMMMIII"."""
    return b"".join(m.group(2).encode() * int(m.group(1)) for m in re.finditer(r"(\d+)(.)", spec))


# ---- the case list ---------------------------------------------------------------------------------------------------------

SET_LENS = (10, 27, 27, 64, 300, 1100, 1300, 2200, 2200, 40, 500, 28, 33)
TARGETS = (8, 1, 10, 0, 9, 6, 12)  # 12 has no items; 3 has one and is not chosen
RESIDUES = (0, 1, 15)


def resident_set(seed=710):
    """Thirteen sequences of 10 .. 2,200 bases: 1, 2 and 11 are the known answer's, 4 is lower case, 5 and 10 hold 'N' and 'n'."""
    rng = random.Random(seed)
    seqs = [rand_seq(rng, n) for n in SET_LENS]
    seqs[1], seqs[2], seqs[11] = KNOWN["text"], KNOWN["pattern"], KNOWN["pattern2"]
    seqs[4] = seqs[4].lower()
    for s in (5, 10):
        b = bytearray(seqs[s])
        for k in range(3, len(b), 37):
            b[k] = ord("N") if k % 2 else ord("n")
        for k in range(5, len(b), 11):
            b[k] = ord(chr(b[k]).lower())
        seqs[s] = bytes(b)
    return seqs


def case_list():
    """[(name, q, t, rev, ops, slice or None, status, residue)] over resident_set(), in a fixed order: ONE call on TARGETS."""
    out = []

    def add(name, q, t, ops, rev=0, slice=None, status=0, residue=None):
        ops = expand(ops) if isinstance(ops, str) else ops
        out.append((name, q, t, rev, ops, slice, status, RESIDUES[len(out) % 3] if residue is None else residue))

    def at_bytes(res, n, runs):
        """n columns of 'M' with 'D' runs at the given arena bytes (byte = residue + column): [(first byte, length)]."""
        ops = bytearray(b"M" * n)
        for b, length in runs:
            ops[b - res:b - res + length] = b"D" * length
        return bytes(ops)

    add("known answer", 2, 1, KNOWN["ops"])
    add("known answer, the second item", 11, 1, KNOWN["ops2"])
    for res in RESIDUES:
        add("D on a lane's last byte, on the next lane's first, a run across the two, and on a chunk's last byte, residue %d" % res, 7, 8,
            at_bytes(res, 1100, [(15, 1), (32, 1), (47, 2), (1023, 1)]), residue=res)
        add("D on a chunk's first byte and a run across two chunks, residue %d" % res, 7, 8, at_bytes(res, 2100, [(1024, 1), (2047, 2)]), residue=res)
    add("a D run of 60 across byte 1024", 7, 6, "1000M60D100M", residue=0)
    add("a D run longer than a chunk", 7, 6, "10M1100D10M")
    add("D runs at slot 0 and at slot L", 3, 0, "3D10M2D")
    add("DI at one place", 3, 9, "5M2D3I5M")
    add("ID at the same place", 3, 9, "5M3I2D5M")
    add("one of three at a slot: 1 D", 4, 10, "30M1D20M")
    add("one of three at a slot: 3 D", 5, 10, "30M3D20M")
    add("one of three at a slot: 2 D", 6, 10, "30M2D20M")
    add("a slice that cuts a D run at either end", 5, 10, "10M6D10M6D10M", slice=(12, 30, 12, 10))
    add("a slice with skips of its own", 5, 10, "30M", slice=(5, 25, 7, 9))
    add("a q_revcomp item", 4, 10, "50M2D40M1X9M", rev=1)
    add("a q_revcomp item that begins and ends with D", 5, 9, "2D4I30M3D", rev=1)
    add("an item whose target is not chosen", 4, 3, "10M")
    add("a record that is not completed, target not chosen", 4, 3, "10M", status=NOT_COMPLETED)
    add("an empty op string", 4, 10, "")
    add("only I", 4, 10, "7I")
    add("a record that is not completed", 5, 10, "20M9D5M", status=NOT_COMPLETED)
    add("a string one base too long", 3, 0, "11M")
    add("a string one base too long for the query", 0, 9, "10M1D")
    add("a stray byte behind a D run longer than every other item's", 5, 10, expand("20M9D5M") + b"=" + expand("3M"))
    add("a stray byte behind a long D run, second chunk", 7, 6, expand("10M1200D20M") + b"?")
    for k in range(8):  # more items than two workgroups take in one trip each
        add("filler %d" % k, 4 + k % 3, 9 if k % 2 else 0, "%dM%dD%dM" % (k + 1, k % 4, 3))
    return out


def case_items(cases):
    """The cases as msa_of's items."""
    return [(q, t, rev, ops, None, sl, status) for _, q, t, rev, ops, sl, status, _ in cases]


def fields(rec, names):
    return tuple(int(rec[n]) for n in names)


# ---- items rebuilt from a run's own PAF lines ------------------------------------------------------------------------------

_CG = re.compile(r"(\d+)([=XIDM])")
_OPS = {"=": b"M", "M": b"M", "X": b"X", "I": b"D", "D": b"I"}  # (in a PAF 'I' consumes the query and 'D' the target)


def items_from_paf(lines, ids, lens, targets):
    """(items, names) of the PAF lines whose target is chosen, in the rows' order (q_idx, q_revcomp, pattern begin, then target
    begin): msa_of's items from columns 1-9 and cg:Z: alone -- cg:Z: expanded, I/D swapped back, the rectangle from columns 3, 4, 8
    and 9, the query interval turned onto the aligned copy on a '-' line -- and per item its row's name."""
    where = {name: k for k, name in enumerate(ids)}
    out = []
    for line in lines:
        f = line.rstrip("\n").split("\t")
        q, t, rev = where[f[0]], where[f[5]], int(f[4] == "-")
        if t not in targets:
            continue
        qs, qe, ts, te = int(f[2]), int(f[3]), int(f[7]), int(f[8])
        cg = [x for x in f[12:] if x.startswith("cg:Z:")][0][5:]
        ops = b"".join(_OPS[op] * int(n) for n, op in _CG.findall(cg))
        span = (lens[q] - qe, lens[q] - qs, ts, te) if rev else (qs, qe, ts, te)
        assert len(ops) - ops.count(b"I") == qe - qs and len(ops) - ops.count(b"D") == te - ts, line
        out.append(((q, rev, span[0], ts), (q, t, rev, ops, span, None, 0), "%s/%d-%d%s" % (f[0], qs, qe, f[4])))
    out.sort(key=lambda o: o[0])
    return [o[1] for o in out], [o[2] for o in out]


def blocks_from_paf(lines, ids, seqs, targets):
    """{target: (names, block)} as host.last_msa() returns it, from the PAF lines alone."""
    lens = [len(s) for s in seqs]
    items, names = items_from_paf(lines, ids, lens, targets)
    w = msa_of(seqs, list(targets), items)
    out = {}
    for j, t in enumerate(targets):
        out[t] = ([ids[t]] + [nm for nm, it in zip(names, items) if it[1] == t], w["blocks"][j])
    return out


def diverged_family(seed=740, n=12):
    """Twelve sequences of about 300 .. 1,500 bp: diverged copies, with indels, of three roots; one member is reverse-complemented,
    some are lower case in part."""
    rng = random.Random(seed)
    from util import mutate
    roots = [rand_seq(rng, m) for m in (320, 800, 1450)]
    seqs = []
    for k in range(n):
        s = mutate(roots[k % 3], 0.02 + 0.01 * (k % 5), rng)
        if k == 4:
            s = revcomp(s)
        if k % 4 == 1:
            s = s[:50] + s[50:120].lower() + s[120:]
        seqs.append(s)
    return ["s%d" % k for k in range(n)], seqs
