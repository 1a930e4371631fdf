"""Cases for the splitting tests (test_split_cpu.py, test_gpu_split.py): the recursion of include/allwave_hip.h over a Python
clip walk to compare the host yardstick against, the properties a split has by definition (checked with clip_cases' brute
force), hand-built op strings for the kernel, and sequence sets whose alignments break into several segments."""
import random

import numpy as np

import clip_cases as K
import util

OK, SKIPPED, EMPTY, BAD_OP = K.OK, K.SKIPPED, K.EMPTY, K.BAD_OP
PENALTY_SETS = [util.DEFAULT_2P, util.EDIT, (0, 4, 6, 2)]
BONUSES = (1, 2, 5)
MIN_SCORES = (1, 3, 10, 40)
OP_MIXES = (b"MMMMXID", b"MXID")


def py_clip(scores, a, ops):
    """The clip's walk (include/allwave_hip.h) in Python: (score, b, e), None when nothing scores above 0, or ("bad", column)."""
    s = min_s = best = 0
    min_i = b = e = run_start = 0
    prev = None
    for c, op in enumerate(ops):
        if op not in b"MXID":
            return ("bad", c)
        if op != prev:
            run_start, prev = c, op
        if op == ord("M"):
            s += a
        elif op == ord("X"):
            s -= scores[1]
        else:
            run = c - run_start + 1
            s -= K.V.gap_cost(scores, run) - (K.V.gap_cost(scores, run - 1) if run > 1 else 0)
        if s <= min_s:
            min_s, min_i = s, c + 1
        if s - min_s > best:
            best, b, e = s - min_s, min_i, c + 1
    return (best, b, e) if best > 0 else None


def py_split(scores, a, min_score, ops):
    """split(c) by the recursion, each slice clipped as an op string of its own: (code, column, [(b, e)] ascending)."""
    whole = py_clip(scores, a, ops)
    if whole is not None and whole[0] == "bad":
        return BAD_OP, whole[1], []

    def segments(lo, hi):
        if hi <= lo:
            return []
        r = py_clip(scores, a, ops[lo:hi])
        if r is None or r[0] < min_score:
            return []
        b, e = lo + r[1], lo + r[2]
        return segments(lo, b) + [(b, e)] + segments(e, hi)

    segs = segments(0, len(ops))
    return (OK if segs else EMPTY), -1, segs


def expected(scores, a, min_score, ops):
    """((code, count, column), [segment records as tuples]) from py_split; a segment's record is the definition's
    (clip_cases.segment_record: the slice re-scored, the prefixes counted from column 0)."""
    code, column, segs = py_split(scores, a, min_score, ops)
    return (code, len(segs), column), [K.segment_record(scores, a, ops, b, e) for b, e in segs]


def got(index, segs):
    return (int(index["code"]), int(index["count"]), int(index["column"])), [K.as_tuple(s) for s in segs]


def check_properties(scores, a, min_score, ops, segs):
    """What a split is by definition, with the brute force as the judge.  segs: [(b, e)]."""
    score = lambda b, e: a * ops[b:e].count(b"M") - K.V.rescore(scores, ops[b:e])
    at = 0
    for b, e in segs:
        assert at <= b < e <= len(ops), (segs, "disjoint and ascending")
        assert ops[b] == ord("M") and ops[e - 1] == ord("M"), (segs, "begins and ends with M")
        assert score(b, e) >= min_score
        at = e
    bounds = [0] + [x for be in segs for x in be] + [len(ops)]
    for lo, hi in zip(bounds[0::2], bounds[1::2]):  # the remainders
        r = K.brute_force(scores, a, ops[lo:hi])
        assert r[0] == EMPTY or r[2] < min_score, (segs, lo, hi, "a remainder holds a segment")
    whole = K.brute_force(scores, a, ops)
    if whole[0] == OK and whole[2] >= min_score:
        assert (whole[3], whole[4]) in segs
        assert whole[2] == max(score(b, e) for b, e in segs)
    assert len(segs) <= a * ops.count(b"M") // min_score


# ---- device cases ---------------------------------------------------------------------------------------------------------

NOISE = b"XXI" * 60  # 180 columns that no segment bridges under any penalty set above with a <= 5 flanks of 40


def island_string(blocks, noise=NOISE):
    """M blocks of the given lengths with noise between them."""
    return noise.join(b"M" * n for n in blocks)


def kernel_strings(rng):
    """[(name, ops)] for the kernel under DEFAULT_2P, a = 1, min_score = 20 (see test_gpu_split.py): every shape the issue
    names that one op string can show."""
    C = 1024
    out = []
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049):
        out.append(("alignment-like n=%d" % n, K.V.random_ops(rng, n, gap_every=200)[:n]))
        out.append(("runs n=%d" % n, K.random_ops(rng, n, alphabet=b"MMMMMMXID")))
        out.append(("islands n=%d" % n, (island_string([30, 45, 25, 60, 35, 50, 40, 70, 33, 44, 55, 66]) * 2)[:n]))
    # a second segment whose col_beg lands on every offset modulo 16 and on both sides of the chunk boundary
    for k in range(16):
        out.append(("col_beg = %d mod 16" % k, b"M" * 50 + b"X" * (30 + k) + b"M" * 40 + b"X" * 3))
    for d in (-17, -16, -1, 0, 1, 15, 16):
        out.append(("col_beg at chunk boundary %+d" % d, b"M" * 100 + b"X" * (C - 100 + d) + b"M" * 60))
    out.append(("remainder of length 1 (left)", b"M" + b"X" + b"M" * 30))      # M X | 30 M: [0, 1) scores 1 < 20, remainder "MX" ...
    out.append(("remainder of length 1 (right)", b"M" * 30 + b"X"))
    out.append(("remainder of length 1 (between)", b"M" * 30 + b"X" * 40 + b"M" * 30 + b"X" + b"M" * 2))
    out.append(("all X", b"X" * 700))
    out.append(("all X over chunks", b"X" * 2100))
    out.append(("two equal-score segments", b"M" * 40 + b"X" * 50 + b"M" * 40))
    out.append(("two equal-score segments over a chunk boundary", b"M" * 40 + b"X" * (C - 30) + b"M" * 40))
    # a gap run that straddles a chunk boundary inside a right remainder: the remainder [e, n) is scanned from its own first
    # byte, so its chunks are not the whole string's -- place the run across both boundaries
    out.append(("gap over the string's chunk boundary in a right remainder", b"M" * 500 + b"X" * 200 + b"M" * 300 + b"D" * 48 + b"M" * 100))
    out.append(("gap over the remainder's chunk boundary", b"M" * 500 + b"X" * 200 + b"M" * (C - 224) + b"I" * 48 + b"M" * 100))
    out.append(("long gap inside a right remainder", b"M" * 900 + b"X" * 300 + b"M" * 60 + b"D" * 1100 + b"M" * 25))
    # three-level recursion: the best block in the middle, the next best in the middle of either half, and so on: 15 segments
    out.append(("three-level recursion", island_string([30, 50, 32, 70, 34, 52, 36, 90, 31, 51, 33, 71, 35, 53, 37])))
    out.append(("three-level recursion, short noise", island_string([30, 50, 32, 70, 34, 52, 36, 90, 31, 51, 33, 71, 35, 53, 37], b"X" * 20)))
    return out


def island_set(seed=11, n_pairs=12):
    """2 * n_pairs sequences of about 2 kbp: pair k is (2 k, 2 k + 1), a shared sequence mutated at 3 % in which one or two
    islands of 200 .. 600 bases are replaced by unrelated sequence in the target; every third pair also loses 700 target
    bases next to a 60-base flank at the end (a long deletion next to a short flank); odd pairs hold the reverse complement
    of the query.  Returns (seqs, int pairs [n, 3])."""
    rng = random.Random(seed)
    seqs, pairs = [], []
    for k in range(n_pairs):
        q = util.rand_seq(rng, rng.randint(1800, 2300))
        t = bytearray(util.mutate(q, 0.03, rng))
        for i in range(1 + k % 2):
            n = rng.randint(200, 600)
            at = rng.randint(200, 700) + i * 900
            t[at:at + n] = util.rand_seq(rng, n)
        t = bytes(t)
        if k % 3 == 2:
            t = t[:len(t) - 760] + t[len(t) - 60:]
        rev = k % 2
        seqs += [K.V.revcomp(q) if rev else q, t]
        pairs.append((2 * k, 2 * k + 1, rev))
    return seqs, np.asarray(pairs, dtype=np.int32)


def segment_lines(ffi, scores, a, min_score, line):
    """The lines the line `line` of an unsplit run becomes under --split a --split-min-score min_score: one per segment of
    the yardstick's split of the line's own op string, in column order, by the coordinate rule of csrc/host/allwave.hpp
    (clip_cases.clipped_paf_fields); columns 3-4 and 8-9 of `line` are the range that was aligned."""
    f = line.split("\t")
    ops = K.V.expand_cg(f[-1][5:])
    _, segs = ffi.split_one_host(scores, a, min_score, ops)
    out = []
    for cl in segs:
        qs, qe, ts, te = K.clipped_paf_fields(cl, int(f[1]), int(f[6]), int(f[2]), int(f[3]), int(f[7]), f[4] == "-")
        nm, nx = int(cl["num_matches"]), int(cl["num_mismatches"])
        seg = ops[int(cl["col_beg"]):int(cl["col_end"])]
        out.append("\t".join(f[:2] + [str(qs), str(qe), f[4]] + f[5:7] + [str(ts), str(te), str(nm), str(max(qe - qs, te - ts)), "60",
                                                                        "gi:f:%.6f" % (nm / (nm + nx)), "cg:Z:" + util.rle(seg)]))
    return out
