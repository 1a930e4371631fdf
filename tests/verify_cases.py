"""Cases for the verification tests (test_verify_cpu.py, test_gpu_verify.py): the golden vectors, a seeded set of single
edits of each, hand-built op strings, and a plain Python walk of the contract in include/allwave_hip.h to compare against."""
import os
import random
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

OK, SKIPPED, BAD_OP, OVERRUN, M_DIFFERS, X_EQUAL, SHORT, COUNTS, PENALTY = range(9)
#: rc of the oracle's cigar check -> code (0: COUNTS, PENALTY or OK, by the record)
ORACLE_CLASS = {-5: BAD_OP, -2: OVERRUN, -3: M_DIFFERS, -4: X_EQUAL, -6: SHORT, -7: SHORT}
EDIT_KINDS = ("m_to_x", "x_to_m", "drop", "dup", "swap_id", "set_n", "penalty_plus_1", "matches_minus_1", "text_subst")


def expand_cg(cg):
    """A PAF cg string back to op bytes: the reference's mapping undone ('=' -> M, X -> X, D -> I, I -> D)."""
    tr = {"=": b"M", "X": b"X", "D": b"I", "I": b"D"}
    out = []
    pos = 0
    for m in re.finditer(r"(\d+)([=XID])", cg):
        assert m.start() == pos, cg
        pos = m.end()
        out.append(tr[m.group(2)] * int(m.group(1)))
    assert pos == len(cg), cg
    return b"".join(out)


def load_kats():
    """[(name, scores, pattern, text, penalty, op bytes)] of tests/golden/oracle_kats.tsv."""
    rows = []
    for line in open(os.path.join(HERE, "golden", "oracle_kats.tsv")):
        if line.startswith("#"):
            continue
        name, scores, pattern, text, penalty, cg = line.rstrip("\n").split("\t")
        rows.append((name, tuple(int(v) for v in scores.split(",")), pattern.encode(), text.encode(), int(penalty), expand_cg(cg)))
    return rows


def gap_cost(scores, length):
    g = scores[2] + length * scores[3]
    if len(scores) == 6:
        g = min(g, scores[4] + length * scores[5])
    return g


def rescore(scores, ops):
    pen, i = 0, 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        if ops[i] == ord("X"):
            pen += (j - i) * scores[1]
        elif ops[i] in b"ID":
            pen += gap_cost(scores, j - i)
        i = j
    return pen


def record_for(scores, ops, status=0):
    """The record an engine would hand out with these op bytes (a tuple in RESULT_DTYPE order, cigar_off 0)."""
    c = {k: ops.count(k.encode()) for k in "MXID"}
    pen = rescore(scores, ops)
    return [status, pen, -pen, len(ops), 0, c["M"], c["X"], c["I"], c["D"], c["M"] + c["X"] + c["D"], c["M"] + c["X"] + c["I"]]


def walk(scores, pattern, text, ops, rec):
    """The contract, column by column: (code, column, penalty)."""
    if rec[0] != 0:
        return SKIPPED, -1, -1
    q = t = 0
    for c, op in enumerate(ops):
        if op not in b"MXID":
            return BAD_OP, c, -1
        if (op != ord("I") and q >= len(pattern)) or (op != ord("D") and t >= len(text)):
            return OVERRUN, c, -1
        if op == ord("M") and pattern[q] != text[t]:
            return M_DIFFERS, c, -1
        if op == ord("X") and pattern[q] == text[t]:
            return X_EQUAL, c, -1
        q += op != ord("I")
        t += op != ord("D")
    pen = rescore(scores, ops)
    if q != len(pattern) or t != len(text):
        return SHORT, -1, pen
    want = record_for(scores, ops)
    if rec[3] != want[3] or rec[5:] != want[5:]:
        return COUNTS, -1, pen
    if rec[1] != pen or rec[2] != -rec[1]:
        return PENALTY, -1, pen
    return OK, -1, pen


def edited_cases():
    """[(kind, vector index, scores, pattern, text, ops, record)]: every edit kind applied once, at a seeded place, to every
    golden vector it can be applied to.  The record is the unedited vector's, with cigar_len following the op string."""
    out = []
    for vi, (name, scores, pattern, text, penalty, ops) in enumerate(load_kats()):
        base = record_for(scores, ops)
        assert base[1] == penalty, name
        for kind in EDIT_KINDS:
            rng = random.Random("verify/%d/%s" % (vi, kind))
            o, rec, txt = bytearray(ops), list(base), bytearray(text)
            cols = {k: [i for i, b in enumerate(ops) if b == ord(k)] for k in "MXID"}
            if kind == "m_to_x":
                if not cols["M"]:
                    continue
                o[rng.choice(cols["M"])] = ord("X")
            elif kind == "x_to_m":
                if not cols["X"]:
                    continue
                o[rng.choice(cols["X"])] = ord("M")
            elif kind == "drop":
                if not ops:
                    continue
                del o[rng.randrange(len(ops))]
            elif kind == "dup":
                if not ops:
                    continue
                i = rng.randrange(len(ops))
                o.insert(i, ops[i])
            elif kind == "swap_id":
                if not (cols["I"] or cols["D"]):
                    continue
                i = rng.choice(cols["I"] + cols["D"])
                o[i] = ord("D") if ops[i] == ord("I") else ord("I")
            elif kind == "set_n":
                if not ops:
                    continue
                o[rng.randrange(len(ops))] = ord("N")
            elif kind == "penalty_plus_1":
                rec[1] += 1
            elif kind == "matches_minus_1":
                rec[5] -= 1
            elif kind == "text_subst":
                if not cols["M"]:
                    continue
                c = rng.choice(cols["M"])
                t = sum(1 for b in ops[:c] if b != ord("D"))
                txt[t] = rng.choice([b for b in b"ACGT" if b != txt[t]])
            rec[3] = len(o)
            out.append((kind, vi, scores, pattern, bytes(txt), bytes(o), rec))
    return out


def build_from_ops(rng, ops, alphabet=b"ACGT"):
    """(pattern, text) that the op bytes align, column by column."""
    p, t = bytearray(), bytearray()
    for op in ops:
        b = rng.choice(alphabet)
        if op == ord("M"):
            p.append(b)
            t.append(b)
        elif op == ord("X"):
            p.append(b)
            t.append(rng.choice([x for x in alphabet if x != b]))
        elif op == ord("I"):
            t.append(b)
        else:
            p.append(b)
    return bytes(p), bytes(t)


def random_ops(rng, n, gap_every=400, gap_len=(1, 40)):
    """About n op bytes: matches with a mismatch every ~30 columns and a gap run every ~gap_every."""
    out = bytearray()
    while len(out) < n:
        out += b"M" * rng.randint(1, 60)
        u = rng.random()
        if u < 30.0 / gap_every:
            out += bytes([rng.choice(b"ID")]) * rng.randint(*gap_len)
        else:
            out += b"X"
    return bytes(out) + b"M"


def revcomp(s):
    """The engine's reverse complement: ACGT in either case -> the upper-case complement, anything else -> 'N'."""
    tr = {ord("A"): "T", ord("a"): "T", ord("T"): "A", ord("t"): "A", ord("C"): "G", ord("c"): "G", ord("G"): "C", ord("g"): "C"}
    return "".join(tr.get(b, "N") for b in reversed(s)).encode()


def as_records(recs):
    from allwave_amd import ffi
    a = np.zeros(len(recs), dtype=ffi.RESULT_DTYPE)
    for i, r in enumerate(recs):
        a[i] = tuple(r)
    return a
