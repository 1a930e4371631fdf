"""Inputs of the reuse tests (tests/test_reuse_cpu.py, tests/test_gpu_reuse.py): lists in which item k + 1 is a trap for the
state item k leaves behind in a persistent workgroup -- the registers, LDS region, DFS stack, event arena and history slot
that one workgroup takes item after item through.

Both dispatch orders are stable host sorts: the scan kernels (verify.hip, clip.hip, split.hip) take records by descending
cigar_len, a record that is not completed counting as 0; the align engine (engine.hip) takes pairs by descending
ql + tl + 4 |ql - tl|.  Every list here has a sort key that strictly decreases in list order (the one exception, the list of
key-0 records, is ordered by the sort's stability alone), so at workgroups = 1 the processing order is the list order."""
import random
from collections import namedtuple

import numpy as np

import repeats as R
import split_cases as S
import twin_base_cases as TB
import twin_cases as TC
import verify_cases as V
from util import mutate, rand_seq

CHUNK = 1024

# ---- scan-kernel records ----------------------------------------------------------------------------------------------------

#: one record of a scan list.  kind: what the record is meant to be (decided again by the host yardsticks in
#: test_reuse_cpu.py); ops: its op bytes; status: the record's status (0: completed); pattern, text: the sequences the verify
#: kernel walks (the pattern is what the kernel reads: a q_revcomp record stores its reverse complement); rc: q_revcomp
ScanRec = namedtuple("ScanRec", "kind ops status pattern text rc")

SEG15 = [30, 50, 32, 70, 34, 52, 36, 90, 31, 51, 33, 71, 35, 53, 37]  # split_cases "three-level recursion"


def _plain(rng, n):
    return V.random_ops(rng, n, gap_every=200)[:n]


def _ops_of(kind, rng, n, g):
    """The op string of `kind` with exactly n columns; g: the gap op of the gap traps (b"I" or b"D")."""
    if kind in ("plain", "m_differs0", "x_equal0", "overrun", "short", "revcomp", "forward", "exact"):
        return _plain(rng, n)
    if kind == "gap_tail":  # the run is open at the last chunk boundary wherever the string starts, and at the last column
        run = 1100 if n >= 1300 else n - 930 if n >= 1000 else max(1, min(n - 1, rng.randint(1, 40)))
        return _plain(rng, n - run) + g * run
    if kind == "gap_head":
        run = min(n, rng.randint(1, 30))
        return g * run + (b"M" + _plain(rng, n))[:n - run]
    if kind == "pos_tail":
        k = min(n, 300)
        return _plain(rng, n - k) + b"M" * k
    if kind == "x_then_m":
        m = min(n, rng.randint(5, 40))
        return b"X" * (n - m) + b"M" * m
    if kind == "neg_tail":  # far below zero, and a few columns above the minimum at the end
        return (_plain(rng, n // 6) + b"X" * n)[:max(n - 3, 0)] + b"M" * min(n, 3)
    if kind == "all_m":
        return b"M" * n
    if kind in ("bad3", "bad1030", "badlast"):
        col = {"bad3": 3, "bad1030": 1030, "badlast": n - 1}[kind]
        o = bytearray(_plain(rng, n))
        o[col] = ord("N")
        return bytes(o)
    if kind == "all_x":
        return b"X" * n
    if kind == "all_gaps":
        return (b"I" * (n // 2) + b"D" * n)[:n]
    if kind == "seg15":
        s = S.island_string(SEG15)
        return s + b"X" * (n - len(s))
    if kind == "seg15_short":
        s = S.island_string(SEG15, b"X" * 20)
        return s + b"X" * (n - len(s))
    if kind == "seg1":
        return (b"X" * 40 + b"M" * 60 + b"X" * n)[:n]
    if kind == "seg0":
        return (b"XXI" * n)[:n]
    raise ValueError(kind)


def _record(kind, rng, n, g, status=0):
    ops = _ops_of(kind, rng, n, g)
    built = bytes(b if b in b"MXID" else ord("M") for b in ops)  # (a bad byte: the sequences are those of an 'M' there)
    p, t = V.build_from_ops(rng, built)
    if kind == "m_differs0":  # a text base under an M of chunk 0 changed
        col = ops.index(b"M", 400)
        at = col - ops[:col].count(b"D")
        t = t[:at] + bytes([next(b for b in b"ACGT" if b != t[at])]) + t[at + 1:]
    elif kind == "x_equal0":  # an M of chunk 0 claimed as X
        col = ops.index(b"M", 700)
        ops = ops[:col] + b"X" + ops[col + 1:]
    elif kind == "overrun":   # the op string goes on behind both sequences' ends
        p, t = V.build_from_ops(rng, ops[:n - 7])
    elif kind == "short":     # the op string ends before the sequences do
        p, t = p + b"ACG", t + b"TT"
    return ScanRec(kind, ops, status, p, t, 1 if kind == "revcomp" else 0)


#: (kind of A, kind of B): B runs on the state A leaves.  Groups with a length condition are placed by _main_list.
_GROUPS = [("gap_tail", "gap_head"), ("pos_tail", "x_then_m"), ("neg_tail", "all_m"), ("bad3", "plain"), ("badlast", "plain"),
           ("all_x", "plain"), ("all_gaps", "plain"), ("overrun", "exact"), ("short", "exact"), ("revcomp", "forward"), ("bad1030", "plain")]


def _main_list(seed, g):
    """About 230 records from 5,000 columns down to 1, the groups above in rotation; the fifteen-segment strings, whose
    lengths are given, and the 3-chunk verify failures where the lengths pass theirs."""
    rng = random.Random("reuse/scan/%s" % seed)
    out = []
    n = 5000
    placed = set()
    k = 0

    def step():
        nonlocal n
        n -= rng.randint(1, 55) if n > 100 else rng.randint(1, 3)

    def emit(kinds):
        for kind in kinds:
            if n < 1:
                return
            out.append(_record(kind, rng, n, g))
            step()

    full15, short15 = len(S.island_string(SEG15)), len(S.island_string(SEG15, b"X" * 20))
    while n >= 1:
        if "seg15" not in placed and n <= full15 + 120:
            placed.add("seg15")
            assert n >= full15
            emit(("seg15", "seg1", "seg0", "plain"))
        elif "fail0" not in placed and n <= 3000:
            placed.add("fail0")
            emit(("m_differs0", "plain", "x_equal0", "plain"))
            assert n > 2 * CHUNK
        elif "seg15_short" not in placed and n <= short15 + 120:
            placed.add("seg15_short")
            assert n >= short15
            emit(("seg0", "seg15_short", "seg1", "seg0", "plain"))
        else:
            grp = _GROUPS[k % len(_GROUPS)]
            k += 1
            if grp[0] == "bad1030" and n < 1100:
                continue
            if grp[0] in ("bad3", "overrun") and n < 12:
                continue
            emit(grp)
    return out


def _zero_list(seed):
    """Records whose sort key is 0 -- not completed, or without a column -- behind two plain ones: only the sort's
    stability orders them.  What follows a key-0 record in one wave can only be another."""
    rng = random.Random("reuse/scan/zero/%s" % seed)
    out = [_record("plain", rng, 700, b"I"), _record("gap_tail", rng, 300, b"D")]
    for k in range(24):  # skipped, no column, no column, skipped, ...
        if k % 3 == 0:
            out.append(_record("gap_tail" if k % 2 else "pos_tail", rng, rng.randint(200, 1500), b"D", status=1 + (k // 3) % 4)._replace(kind="skipped"))
        else:
            out.append(ScanRec("len0", b"", 0, b"", b"", 0))
    return out


_SCAN = {}


def scan_lists():
    """{name: [ScanRec]}, built once and never changed."""
    if not _SCAN:
        _SCAN["main-I"] = _main_list("I", b"I")
        _SCAN["main-D"] = _main_list("D", b"D")
        _SCAN["zero"] = _zero_list(0)
    return _SCAN


def scan_key(rec):
    return len(rec.ops) if rec.status == 0 else 0


def dispatch_order(keys):
    """The host's stable sort by descending key."""
    return sorted(range(len(keys)), key=lambda i: -keys[i])


def pack_back_to_back(recs):
    """The op strings one behind the other, without a byte between them: (RESULT_DTYPE records with status, cigar_off and
    cigar_len set, arena bytes)."""
    from allwave_amd import ffi
    out = np.zeros(len(recs), dtype=ffi.RESULT_DTYPE)
    arena = bytearray()
    for k, r in enumerate(recs):
        out[k]["status"] = r.status
        out[k]["cigar_off"] = len(arena)
        out[k]["cigar_len"] = len(r.ops)
        arena += r.ops
    return out, bytes(arena)


def verify_inputs(recs, scores):
    """(sequences, pairs [n, 3], RESULT_DTYPE records, arena) of a scan list for the verify kernel: record k is the pair
    (2 k, 2 k + 1), its claimed counts and penalty those of its own op string under `scores`."""
    out, arena = pack_back_to_back(recs)
    seqs, pairs = [], []
    for k, r in enumerate(recs):
        seqs += [V.revcomp(r.pattern) if r.rc else r.pattern, r.text]
        pairs.append((2 * k, 2 * k + 1, r.rc))
        built = bytes(b if b in b"MXID" else ord("M") for b in r.ops)
        claimed = V.record_for(scores, built, r.status)
        claimed[3], claimed[4] = len(r.ops), int(out[k]["cigar_off"])
        out[k] = tuple(claimed)
    return seqs, np.asarray(pairs, dtype=np.int32), out, arena


def verify_ranges_list(seed=0):
    """[ScanRec] for awv_verify_ranges, and per record (q_beg, t_beg): records on intervals that begin at pb, tb that are no
    multiples of 4 (every other one on the reverse strand) alternate with forward records on whole sequences."""
    rng = random.Random("reuse/scan/ranges/%s" % seed)
    recs, begs = [], []
    n = 2600
    k = 0
    while n >= 1:
        if k % 2 == 0:
            recs.append(_record("revcomp" if k % 4 == 0 else "plain", rng, n, b"I")._replace(kind="range"))
            begs.append((4 * rng.randint(0, 9) + 1 + k // 2 % 3, 4 * rng.randint(0, 9) + 1 + (k // 2 + 1) % 3))
        else:
            recs.append(_record("forward", rng, n, b"I"))
            begs.append((0, 0))
        n -= rng.randint(20, 110)
        k += 1
    return recs, begs


def verify_range_inputs(recs, begs, scores, rng):
    """As verify_inputs, with RANGE_DTYPE rows: record k's sequences lie at begs[k] inside longer ones."""
    out, arena = pack_back_to_back(recs)
    seqs, ranges = [], []
    for k, (r, (qb, tb)) in enumerate(zip(recs, begs)):
        stored = V.revcomp(r.pattern) if r.rc else r.pattern
        tail = 0 if (qb, tb) == (0, 0) else rng.randint(1, 30)
        seqs += [rand_seq(rng, qb) + stored + rand_seq(rng, tail), rand_seq(rng, tb) + r.text + rand_seq(rng, tail)]
        ranges.append((2 * k, 2 * k + 1, r.rc, qb, qb + len(stored), tb, tb + len(r.text)))
        claimed = V.record_for(scores, r.ops, r.status)
        claimed[3], claimed[4] = len(r.ops), int(out[k]["cigar_off"])
        out[k] = tuple(claimed)
    return seqs, np.asarray(ranges, dtype=np.int32), out, arena


def open_at_last_chunk_boundary(ops, sh):
    """Whether the string's last run, of a gap op, began before the last chunk boundary of a string that starts sh bytes
    behind a 16-byte boundary (bytes are counted from that boundary), or fills a string that has no boundary."""
    run = len(ops) - len(ops.rstrip(ops[-1:]))
    last_boundary = (sh + len(ops) - 1) // CHUNK * CHUNK - sh  # the column at the last chunk's first byte
    return ops[-1:] in (b"I", b"D") and (last_boundary <= 0 or run > len(ops) - last_boundary)


def clip_from(scores, a, ops, s0=0, min0=0):
    """split_cases.py_clip with a start state: the running score and its minimum as another string's walk left them.
    (score, b, e), or None when nothing scores above 0."""
    s, min_s, best = s0, min0, 0
    min_i = b = e = run_start = 0
    prev = None
    for c, op in enumerate(ops):
        if op != prev:
            run_start, prev = c, op
        if op == ord("M"):
            s += a
        elif op == ord("X"):
            s -= scores[1]
        else:
            run = c - run_start + 1
            s -= V.gap_cost(scores, run) - (V.gap_cost(scores, run - 1) if run > 1 else 0)
        if s <= min_s:
            min_s, min_i = s, c + 1
        if s - min_s > best:
            best, b, e = s - min_s, min_i, c + 1
    return (best, b, e) if best > 0 else None


def end_state(scores, a, ops):
    """(running score, its minimum) behind the last column of `ops`, from 0."""
    s = min_s = 0
    run_start, prev = 0, None
    for c, op in enumerate(ops):
        if op != prev:
            run_start, prev = c, op
        if op == ord("M"):
            s += a
        elif op == ord("X"):
            s -= scores[1]
        else:
            run = c - run_start + 1
            s -= V.gap_cost(scores, run) - (V.gap_cost(scores, run - 1) if run > 1 else 0)
        min_s = min(min_s, s)
    return s, min_s


def default_path_records(n=12288, seed=0):
    """n records of 1 .. 64 columns, the kinds of the lists above in rotation (SKIPPED and column-free records among them):
    what the default launch, 16 waves per CU, takes several records per wave of."""
    rng = random.Random("reuse/scan/default/%s" % seed)
    kinds = ["gap_tail", "gap_head", "pos_tail", "x_then_m", "neg_tail", "all_m", "bad3", "plain", "badlast", "plain", "all_x", "plain",
             "all_gaps", "exact", "short", "exact", "overrun", "forward", "revcomp", "forward", "seg1", "seg0", "skipped", "plain", "len0", "plain"]
    out = []
    for k in range(n):
        kind = kinds[k % len(kinds)]
        m = rng.randint(1, 64)
        if kind in ("bad3", "overrun") and m < 12:
            m += 12
        if kind == "len0":
            out.append(ScanRec("len0", b"", 0, b"", b"", 0))
        elif kind == "skipped":
            out.append(_record("gap_tail", rng, m, b"I", status=1 + k % 4)._replace(kind="skipped"))
        else:
            out.append(_record(kind, rng, m, b"ID"[k // len(kinds) % 2:][:1]))
    return out


# ---- align pairs ------------------------------------------------------------------------------------------------------------

def pair_key(ql, tl):
    """The align engine's dispatch cost (engine.hip)."""
    return ql + tl + 4 * abs(ql - tl)


def _exact(rng, s, n):
    """`s` brought to exactly n bases at its end."""
    return s[:n] if len(s) >= n else s + rand_seq(rng, n - len(s))


def _mismatches(rng, s, d):
    """A copy of `s` with mismatches only, a fraction d of its bases: the same length."""
    out = bytearray(s)
    for i in rng.sample(range(len(s)), max(1, int(d * len(s)))):
        out[i] = rng.choice([b for b in b"ACGT" if b != s[i]])
    return bytes(out)


def _related(rng, n, d, m=None):
    """(s, t): n random bases and a copy d apart, of exactly m (default n) bases."""
    s = rand_seq(rng, n)
    return s, _exact(rng, mutate(s, d, rng), n if m is None else m)


def _small_tail(rng, k):
    """(i) two pairs with both lengths <= 100, the last entries of every list: the second runs on the first's state."""
    a, b = rand_seq(rng, 70 + k), rand_seq(rng, 80 - k)
    return [("small", a, _exact(rng, mutate(a, 0.1, rng), 95), 0), ("small", b, _mismatches(rng, b, 0.08), 0)]


def _align_entries():
    """{list name: [(kind, pattern source, text, q_revcomp)]}: the stored query is the pattern source (reverse-complemented by
    the engine when q_revcomp is set)."""
    L = {}
    rng = random.Random("reuse/align/deep")
    out = []
    s, t = _related(rng, 3000, 0.17)
    out.append(("a-divergent", s, t, 0))                       # (a) several search levels, a deep DFS stack ...
    s = rand_seq(rng, 2900)
    t = bytearray(s)
    for i in (17, 1450, 2888):
        t[i] = ord("A") if s[i] != ord("A") else ord("C")
    out.append(("a-three-mismatches", s, bytes(t), 0))         # ... then one search, a tiny score
    for n, gaps in ((1500, (15, 25, 120)), (1000, (40, 90, 220))):
        a, b = TB.indel_rich(rng, n, gaps)                     # (h) base cases that begin or end in I1 / D1 / I2 / D2 ...
        out.append(("h-indel-rich", a, _exact(rng, b, n - 40), 0))
        s = rand_seq(rng, n - 150)
        out.append(("h-mismatch-only", s, _mismatches(rng, s, 0.04), 0))   # ... then mismatches only
    L["deep"] = out + _small_tail(rng, 0)

    rng = random.Random("reuse/align/bytes")
    out = []
    s, t = _related(rng, 2800, 0.05)
    out.append(("b-with-N", s[:1200] + b"N" + s[1201:], t, 0))  # (b) no packed view, raw-byte probes ...
    out.append(("b-acgt",) + _related(rng, 2700, 0.05) + (0,))  # ... then a packed pair ...
    s, t = _related(rng, 2600, 0.06)
    out.append(("b-with-N", s, t[:77] + b"N" + t[78:], 0))      # ... and the reverse order
    s = rand_seq(rng, 2400)
    out.append(("d-identical", s, s, 0))                        # (d) BP_END_REACHED ...
    out.append(("d-divergent",) + _related(rng, 2300, 0.12) + (0,))
    s, t = _related(rng, 1000, 0.06)
    out.append(("c-revcomp", TC.rc(s), t, 1))                   # (c) q_revcomp = 1 on (q, t) ...
    out.append(("c-forward", TC.rc(s), t, 0))                   # ... and 0 on the same indices: the same key, kept in order by the sort's stability
    out.append(("plain",) + _related(rng, 900, 0.05) + (0,))
    L["bytes"] = out + _small_tail(rng, 3)

    rng = random.Random("reuse/align/gaps")
    out = [("e-empty", b"", rand_seq(rng, 500), 0),             # (e) an empty sequence against 500 bases ...
           ("plain",) + _related(rng, 1200, 0.05) + (0,)]       # ... then a normal pair
    for short, gap, eq in ((60, 200, 550), (40, 200, 530), (90, 160, 480), (101, 140, 440), (120, 120, 400)):
        s = rand_seq(rng, short)                                # (f) a forced gap, trimmed rows ...
        cut = rng.randrange(0, short + 1)
        t = s[:cut] + rand_seq(rng, gap) + s[cut:]
        out.append(("f-forced-gap", s, t, 0) if short != 90 else ("f-forced-gap", t, s, 0))
        out.append(("f-equal-length",) + _related(rng, eq, 0.04) + (0,))   # ... then an equal-length pair
    L["gaps"] = out + _small_tail(rng, 6)

    name, gen, seed = R.RESTART_CASES[2]
    a, b = gen(random.Random(seed))                             # (g) a pair whose searches restart on the device (repeats.py)
    for order, (p, t) in (("ab", (a, b)), ("ba", (b, a))):
        rng = random.Random("reuse/align/restart/" + order)
        L["restart-" + order] = [("g-restart", p, t, 0), ("plain",) + _related(rng, 800, 0.05) + (0,)] + _small_tail(rng, 9)
    return L


_ALIGN = {}


def align_lists():
    """{name: (seqs, pairs [(q, t, q_revcomp)], kinds)}, built once and never changed.  No sequence is shared between entries
    but by the two (c) entries."""
    if not _ALIGN:
        for name, entries in _align_entries().items():
            seqs, pairs, kinds = [], [], []
            for kind, q, t, rc in entries:
                if kind == "c-forward":
                    pairs.append((pairs[-1][0], pairs[-1][1], rc))
                else:
                    seqs += [q, t]
                    pairs.append((len(seqs) - 2, len(seqs) - 1, rc))
                kinds.append(kind)
            _ALIGN[name] = (seqs, pairs, kinds)
    return _ALIGN


def capacity_list():
    """twin_cases.rerun_inputs in dispatch order (a pair and its swap share a key: the sort's stability orders them), and the
    entries that are divergent 6 kbp pairs."""
    seqs, pairs = TC.rerun_inputs()
    keys = [pair_key(len(seqs[q]), len(seqs[t])) for q, t in pairs]
    pairs = [pairs[i] for i in dispatch_order(keys)]
    divergent = [(q, t) in ((0, 1), (1, 0), (1, 2), (2, 1)) for q, t in pairs]  # 8 % and about 9 % apart; (0, 2) is 1 % apart, 3 is 1.5 kbp
    return seqs, [(q, t, 0) for q, t in pairs], divergent


def align_keys(seqs, pairs):
    return [pair_key(len(seqs[p[0]]), len(seqs[p[1]])) for p in pairs]


def as_ranges(seqs, pairs, first=0, seed=0):
    """The list as awv_range_pairs over longer resident sequences: (resident seqs, ranges [n, 7]).  Entry k's query interval
    begins at a position that is first + k modulo 16, its target interval at 5 (first + k) + 3 modulo 16; every odd entry
    is stored on the other strand (the query's reverse complement resident, q_revcomp flipped), so pattern and text -- and
    the oracle's answer -- are the pair list's."""
    rng = random.Random("reuse/align/ranges/%s" % seed)
    res, ranges = [], []
    for k, (q, t, rc) in enumerate(pairs):
        stored, text = seqs[q], seqs[t]
        if k % 2:
            stored, rc = TC.rc(stored), 1 - rc
        qb = 16 * rng.randint(0, 3) + (first + k) % 16
        tb = 16 * rng.randint(0, 3) + (5 * (first + k) + 3) % 16
        res += [rand_seq(rng, qb) + stored + rand_seq(rng, rng.randint(0, 40)), rand_seq(rng, tb) + text + rand_seq(rng, rng.randint(0, 40))]
        ranges.append((2 * k, 2 * k + 1, rc, qb, qb + len(stored), tb, tb + len(text)))
    return res, np.asarray(ranges, dtype=np.int32)


def bounds_for(want, every):
    """Per-pair bounds from the oracle's penalties: P // 2 for every `every`-th entry (abandoned mid-search whenever P > 0),
    -1 -- no bound -- for the others."""
    return np.asarray([pen // 2 if k % every == every - 1 else -1 for k, (pen, _) in enumerate(want)], dtype=np.int32)
