"""Cases for the clipping tests (test_clip_cpu.py, test_gpu_clip.py): a brute force of the segment definition in
include/allwave_hip.h to compare the host yardstick against, hand-built op strings, seeded generators, and the PAF line a
clip turns an alignment's line into."""
import random

import numpy as np

import util
import verify_cases as V

OK, SKIPPED, EMPTY, BAD_OP = range(4)
BONUSES = (1, 2, 3, 5)
PENALTY_SETS = list(dict.fromkeys(util.PENALTY_SETS + [util.EDIT, util.DEFAULT_2P]))
FIELDS = ("code", "reserved", "score", "col_beg", "col_end", "q_skip", "t_skip", "num_matches", "num_mismatches", "num_ins", "num_del",
          "penalty", "reserved2")


def as_tuple(rec):
    return tuple(int(rec[f]) for f in FIELDS)


def segment_record(scores, a, ops, b, e):
    """The record of the segment [b, e) of `ops`, from the definition: the segment re-scored as an op string of its own."""
    seg, head = ops[b:e], ops[:b]
    c = {k: seg.count(k.encode()) for k in "MXID"}
    pen = V.rescore(scores, seg)
    return (OK, 0, a * c["M"] - pen, b, e, len(head) - head.count(b"I"), len(head) - head.count(b"D"), c["M"], c["X"], c["I"], c["D"], pen, 0)


def brute_force(scores, a, ops):
    """The segment definition, O(n^2) segments: maximal score, then the smallest end, then the largest begin; empty when no
    segment scores above 0.  (No walk, no deltas: every segment is re-scored on its own.)"""
    for c, op in enumerate(ops):
        if op not in b"MXID":
            return (BAD_OP, 0, 0, c, c, 0, 0, 0, 0, 0, 0, 0, 0)
    best, where = 0, None
    for e in range(1, len(ops) + 1):
        for b in range(e - 1, -1, -1):  # (the largest begin first; only a strictly larger score replaces)
            s = a * ops[b:e].count(b"M") - V.rescore(scores, ops[b:e])
            if s > best:
                best, where = s, (b, e)
    if where is None:
        return (EMPTY,) + (0,) * 12
    return segment_record(scores, a, ops, *where)


def random_ops(rng, n, runs=(1, 9), alphabet=b"MXID"):
    """About n op bytes (at most n) in runs of runs[0] .. runs[1] equal ops."""
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.choice(alphabet)]) * rng.randint(*runs)
    return bytes(out[:n])


def fixed_cases():
    """[(name, scores, a, ops, expected record or None)]: None where the brute force is the expectation."""
    p2, p1 = util.DEFAULT_2P, (0, 4, 6, 2)
    cases = [
        ("empty string", p2, 1, b"", (EMPTY,) + (0,) * 12),
        ("all M", p2, 2, b"M" * 37, (OK, 0, 74, 0, 37, 0, 0, 37, 0, 0, 0, 0, 0)),
        ("all X", p2, 1, b"X" * 9, (EMPTY,) + (0,) * 12),
        ("all gaps", p2, 1, b"I" * 5 + b"D" * 7 + b"I", (EMPTY,) + (0,) * 12),
        ("single M", p1, 3, b"M", (OK, 0, 3, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0)),
        # two segments of score 10 with a gap of cost 6 + 2 * 2 = 10 between them: S returns to the minimum's value at the
        # gap's last column, so the minimum moves there (a tie replaces it), and the right segment only ties the best (a tie
        # never replaces it): the left one is the clip -- whole, 10 + 10 - 10, ties too, with a later end
        ("tie: equal segments, a gap that costs the left one", p1, 1, b"M" * 10 + b"II" + b"M" * 10, (OK, 0, 10, 0, 10, 0, 0, 10, 0, 0, 0, 0, 0)),
        # the same with flanks: the clip begins after the leading X
        ("tie with flanks", p1, 1, b"X" + b"M" * 10 + b"DD" + b"M" * 10 + b"X", (OK, 0, 10, 1, 11, 1, 1, 10, 0, 0, 0, 0, 0)),
        # 2-piece 8 + 2 L against 24 + L: the second piece is the cheaper one from L = 17 on; a run of 30 costs 54, and the
        # two flanks of 60 are worth bridging it
        ("2-piece run on its second piece", p2, 1, b"M" * 60 + b"D" * 30 + b"M" * 60, (OK, 0, 66, 0, 150, 0, 0, 120, 0, 0, 30, 54, 0)),
        ("I run then D run are two runs", p2, 1, b"M" * 40 + b"III" + b"DD" + b"M" * 40, (OK, 0, 54, 0, 85, 0, 0, 80, 0, 3, 2, 26, 0)),
    ]
    return cases


def bad_op_cases():
    return [(b"MMMNMM", 3), (b"N", 0), (b"MMMM\x00", 4), (b"MmM", 1), (b"M" * 40 + b"=" + b"Q", 40)]


# ---- device cases: op strings whose events fall on lane (16 bytes) and chunk (1,024 bytes) boundaries -------------------

def boundary_strings(sh):
    """Op strings built for a string that starts `sh` bytes behind a 16-byte boundary: the kernel's lanes hold bytes
    16 k .. 16 k + 15 and its chunks bytes 1024 k .. 1024 k + 1023 of the string counted from that boundary, so column
    c sits at byte sh + c.  [(name, ops)]"""
    C = 1024

    def col(byte):  # the column at byte position `byte`
        return byte - sh

    out = []
    # gap runs that straddle a lane boundary and a chunk boundary, on both sides
    for name, start_byte, length in (("gap ends at lane boundary", 48 - 5, 5), ("gap begins at lane boundary", 48, 5),
                                     ("gap straddles lane boundary", 48 - 3, 7), ("gap ends at chunk boundary", C - 20, 20),
                                     ("gap begins at chunk boundary", C, 20), ("gap straddles chunk boundary", C - 9, 30),
                                     ("gap straddles two chunks", C - 3, C + 9)):
        s = col(start_byte)
        out.append((name, b"M" * s + b"I" * length + b"M" * 300))
        out.append((name + " (D, X flanks)", b"X" + b"M" * (s - 1) + b"D" * length + b"M" * 90 + b"X"))
    # a best segment that begins in one chunk and ends two chunks later
    out.append(("segment over three chunks", b"X" * col(C - 100) + (b"M" * 99 + b"X") * 21 + b"X" * 50))
    # the running minimum tied between two chunks (a = x = 1: S is at its minimum before the first M, in chunk 0, and again
    # behind the 50 X, in chunk 1); the later one must win: the clip is the last 200 M, not the 300 columns that score the same
    out.append(("minimum tied between two chunks", b"X" * col(C - 40) + b"M" * 50 + b"X" * 50 + b"M" * 200))
    # the best tied between two chunks: the earlier one must win
    out.append(("best tied between two chunks", b"M" * col(C - 30) + b"X" * (C + 100) + b"M" * col(C - 30)))
    # an all-gap chunk between two M chunks
    out.append(("all-gap chunk", b"M" * col(C) + b"I" * C + b"M" * C))
    out.append(("all-gap chunk, two runs", b"M" * col(C) + b"I" * 500 + b"D" * 524 + b"M" * C))
    # a 2-piece run that switches piece across a chunk boundary (8 + 2 L against 24 + L: at L = 17)
    out.append(("2-piece switch across a chunk boundary", b"M" * col(C - 10) + b"D" * 40 + b"M" * 500))
    out.append(("2-piece switch at the chunk's first column", b"M" * col(C - 16) + b"I" * 40 + b"M" * 500))
    return out


def length_strings(rng, lengths=(0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 5003)):
    """One alignment-like and one run-rich random string per length."""
    out = []
    for n in lengths:
        out.append(("alignment-like n=%d" % n, V.random_ops(rng, n, gap_every=200)[:n]))
        out.append(("runs n=%d" % n, random_ops(rng, n)))
    return out


def pack_arena(strings, offsets_mod16=None, status=None):
    """Op strings into one arena, string k starting at residue offsets_mod16[k] modulo 16 (default: k mod 16), with a junk
    byte between strings (so a read past a string's end is seen).  Returns (RESULT_DTYPE records, arena bytes)."""
    from allwave_amd import ffi
    recs = np.zeros(len(strings), dtype=ffi.RESULT_DTYPE)
    arena = bytearray()
    for k, ops in enumerate(strings):
        want = (k if offsets_mod16 is None else offsets_mod16[k]) % 16
        arena += b"?" * ((want - len(arena)) % 16 or 16)
        recs[k]["status"] = 0 if status is None else status[k]
        recs[k]["cigar_off"] = len(arena)
        recs[k]["cigar_len"] = len(ops)
        arena += ops
    arena += b"?" * 7
    return recs, bytes(arena)


# ---- sequence sets with partial homology ---------------------------------------------------------------------------------

def flanked_set(seed=5, n_pairs=40, unrelated_every=7):
    """2 * n_pairs sequences of about 300 .. 3,000 bp: pair k is (2 k, 2 k + 1), a shared core mutated at 5 % with unrelated
    random flanks of 0 .. 800 bp on either side of either sequence; every `unrelated_every`-th pair shares no core; odd
    pairs hold the reverse complement of the query.  Returns (seqs, int pairs [n, 3])."""
    rng = random.Random(seed)
    seqs, pairs = [], []
    for k in range(n_pairs):
        core = util.rand_seq(rng, rng.randint(300, 1400))
        other = util.rand_seq(rng, len(core)) if k % unrelated_every == unrelated_every - 1 else util.mutate(core, 0.05, rng)

        def flank():
            return util.rand_seq(rng, rng.choice([0, 0, rng.randint(1, 800)]))

        q = flank() + core + flank()
        t = flank() + other + flank()
        rev = k % 2
        seqs += [V.revcomp(q) if rev else q, t]
        pairs.append((2 * k, 2 * k + 1, rev))
    return seqs, np.asarray(pairs, dtype=np.int32)


def clipped_paf_fields(cl, q_len, t_len, qb, qe, tb, is_rev):
    """Columns 3, 4, 8, 9 of the clipped line by the coordinate rule of csrc/host/allwave.hpp: [qb, qe) the query's range on
    its forward strand (the whole sequence on a pair list), tb the target range's start."""
    qspan = int(cl["num_matches"]) + int(cl["num_mismatches"]) + int(cl["num_del"])
    tspan = int(cl["num_matches"]) + int(cl["num_mismatches"]) + int(cl["num_ins"])
    if is_rev:
        qend = qe - int(cl["q_skip"])
        qstart = qend - qspan
    else:
        qstart = qb + int(cl["q_skip"])
        qend = qstart + qspan
    tstart = tb + int(cl["t_skip"])
    return qstart, qend, tstart, tstart + tspan
