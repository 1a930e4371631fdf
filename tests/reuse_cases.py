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


# ---- the five newer record passes: normalize.hip, encode.hip, cs.hip, coverage.hip, variants.hip ---------------------------------
# They take records in the scan kernels' order and carry more from chunk to chunk: the run carry (the column the run in progress
# began at, the op before the chunk), the characters, runs and events so far, the bases consumed, the hash of the 'D' run in
# progress, lane-local counts and a lane-local "bad byte seen", the class of the column before the chunk, and normalize's link
# state.  The lists above serve them as they are; the lists below add what they lack: adjacencies chosen for that state.

DIGITS = (9, 10, 99, 100, 999, 1000)  # run lengths at which the text of a run gains a digit

#: (kind of A, kind of B, B begins on a 16-byte boundary): the trap groups of pass-I / pass-D.  coverage.hip's carried class reaches
#: a record's first column only in lane 0's byte 0 -- at any other offset the byte before column 0 is masked out.
_PASS_GROUPS = [("gap_tail", "gap_head", False), ("many_runs", "one_run", False), ("pos_tail", "digits", True), ("plain", "x_first", False),
                ("many_runs", "one_event", False), ("revcomp", "forward", False), ("badlast", "plain", False), ("overrun", "plain", False),
                ("bad3", "plain", False), ("all_gaps", "plain", False)]


def _pass_record(kind, rng, n, g, k):
    """A record of the lists above, or one of the kinds only these lists have (k: which of the digit thresholds)."""
    if kind == "many_runs":    # runs of 1 .. 3 columns of every op: a long text, many runs, many events
        ops = bytearray()
        while len(ops) < n:
            ops += bytes([rng.choice(b"MXMIMD")]) * rng.randint(1, 3)
        ops = bytes(ops[:n])
    elif kind == "one_run":
        ops = b"M" * n
    elif kind == "one_event":  # its only event is its last column
        ops = b"M" * (n - 1) + b"X"
    elif kind == "x_first":    # its first column reads both sequences' first bases
        ops = (b"X" + _plain(rng, n))[:n]
    elif kind == "digits":     # its first run is an 'M' run of a digit threshold (the largest that fits, else all of it)
        fit = [d for d in DIGITS if d < n]
        d = DIGITS[k % len(DIGITS)] if DIGITS[k % len(DIGITS)] < n else fit[-1] if fit else n
        ops = (b"M" * d + b"X" + _plain(rng, n))[:n]
    else:
        return _record(kind, rng, n, g)
    p, t = V.build_from_ops(rng, ops)
    return ScanRec(kind, ops, 0, p, t, 0)


def _decreasing_list(rng, groups, make):
    """Records from 5,000 columns down to 1, the groups in rotation, stored back to back: make(kind, n, instance) is a record of n
    columns.  A group whose B begins on a 16-byte boundary shortens its A by up to 15 columns to get there."""
    out = []
    n, k, off = 5000, 0, 0
    while n >= 1:
        a, b, aligned = groups[k % len(groups)]
        k += 1
        if a in ("bad3", "overrun") and n < 12:
            continue
        if aligned:
            if n <= 16:
                continue
            n -= (off + n) % 16
        for kind in (a, b):
            if n < 1:
                break
            out.append(make(kind, n, k // len(groups)))
            assert len(out[-1].ops) == n, (kind, n)
            off += n
            n -= rng.randint(1, 55) if n > 100 else rng.randint(1, 3)
    return out


def _pass_list(seed, g):
    rng = random.Random("reuse/pass/%s" % seed)
    return _decreasing_list(rng, _PASS_GROUPS, lambda kind, n, k: _pass_record(kind, rng, n, g, k))


# normalize.hip moves a gap run only through bases that repeat, which verify_cases.build_from_ops' random sequences almost never
# offer: these records lie in a homopolymer.  Every 'M' is A over A and every run is free to go as far as its bound allows, unless
# an 'X' (A over C) or a column of G stands in its way.

def _hp_content(rng, n):
    """n columns: 'M' runs of 5 .. 40 with gap runs of 1 .. 3 between them."""
    ops = bytearray()
    while len(ops) < n:
        ops += b"M" * rng.randint(5, 40) + bytes([rng.choice(b"ID")]) * rng.randint(1, 3)
    return bytes(ops[:n])


def _hp_pair(ops, other=()):
    """(pattern, text) of the homopolymer under `ops`; the columns in `other`, all 'M', hold G."""
    p, t = bytearray(), bytearray()
    for c, op in enumerate(ops):
        b = ord("G") if c in other else ord("A")
        if op != ord("I"):
            p.append(b)
        if op != ord("D"):
            t.append(ord("C") if op == ord("X") else b)
    return bytes(p), bytes(t)


#: the trap groups of norm-left (and, mirrored, of norm-right)
_NORM_GROUPS = [("n_tail_unmoved", "n_head_moves", False), ("n_tail_moved", "n_head_blocked", False), ("n_gap_tail", "n_gap_head_other", False),
                ("n_moves_many", "n_blocked", False)]
HEAD_M = (1, 2, 17, 70, 300, 1030)  # the 'M' columns before the first run of n_head_moves: inside a lane, over lanes, over a chunk


def _norm_record(kind, rng, n, g, k):
    """A homopolymer record of n columns; g: the gap op of its trap."""
    o = b"D" if g == b"I" else b"I"
    other = ()
    if kind == "n_tail_unmoved":    # the last gap run stands behind an 'X' and does not move; 1 .. 3 'M' columns end the string
        ops = (_hp_content(rng, n) + b"X" + g * rng.randint(1, 5) + b"M" * rng.randint(1, 3))[-n:]
    elif kind == "n_head_moves":    # M^m g^L: the run goes to column 0
        L = rng.randint(1, 4)
        m = max(min(HEAD_M[k % len(HEAD_M)], n - L), 0)
        ops = (b"M" * m + g * L + b"X" + _hp_content(rng, n))[:n]
    elif kind == "n_tail_moved":    # the last gap run moves 40 columns or more; two 'M' columns end the string
        ops = (_hp_content(rng, n) + b"M" * 40 + g * rng.randint(1, 5) + b"MM")[-n:]
    elif kind == "n_head_blocked":  # M^m g^L with a G d columns before the run: it moves by d
        m, L = rng.randint(4, 40), rng.randint(1, 4)
        ops = (b"M" * m + g * L + b"X" + _hp_content(rng, n))[:n]
        other = (m - 1 - rng.randint(0, 3),)
        if other[0] >= n or ops[other[0]] != ord("M"):
            other = ()
    elif kind == "n_gap_tail":      # ends inside a gap run
        ops = (_hp_content(rng, n) + g * (1100 if n >= 1300 else rng.randint(1, 30)))[-n:]
    elif kind == "n_gap_head_other":  # begins with a run of the other gap op
        ops = (o * rng.randint(1, 30) + b"M" + _hp_content(rng, n))[:n]
    elif kind == "n_moves_many":
        ops = _hp_content(rng, n)
    elif kind == "n_blocked":       # every gap run stands behind an 'X': nothing moves
        ops = bytearray()
        while len(ops) < n:
            ops += b"M" * rng.randint(5, 40) + b"X" + bytes([rng.choice(b"ID")]) * rng.randint(1, 3)
        ops = bytes(ops[:n])
    else:
        raise ValueError(kind)
    p, t = _hp_pair(ops, other)
    return ScanRec(kind, ops, 0, p, t, 0)


def _norm_list(seed):
    rng = random.Random("reuse/norm/%s" % seed)
    return _decreasing_list(rng, _NORM_GROUPS, lambda kind, n, k: _norm_record(kind, rng, n, b"ID"[k % 2:][:1], k))


def mirrored(rec):
    """The record as a right-normalizing wave walks it: the reversed op string over the reversed sequences."""
    return rec._replace(ops=rec.ops[::-1], pattern=rec.pattern[::-1], text=rec.text[::-1])


_PASS = {}


def pass_lists():
    """{name: [ScanRec]}, built once and never changed: the lists of the five newer passes.  norm-right is a list of its own,
    mirrored: a right-normalizing wave walks a string from its end, so there A's "end" is its column 0."""
    if not _PASS:
        _PASS["pass-I"] = _pass_list("I", b"I")
        _PASS["pass-D"] = _pass_list("D", b"D")
        _PASS["norm-left"] = _norm_list("left")
        _PASS["norm-right"] = [mirrored(r) for r in _norm_list("right")]
    return _PASS


def all_lists():
    """The scan lists and the pass lists."""
    out = dict(scan_lists())
    out.update(pass_lists())
    return out


def offsets_of(recs):
    """Where each record's op string begins in the back-to-back arena."""
    return [int(v) for v in np.concatenate(([0], np.cumsum([len(r.ops) for r in recs])))[:-1]]


# ---- what the five passes must give: the host yardsticks, record by record ---------------------------------------------------------

def range_geometry(seqs, ranges):
    """Per range (aligned copy of the whole query, (pb, pe, tb, te) in its coordinates): a q_revcomp range's interval, given on the
    forward strand, seen from the reverse complement."""
    out = []
    for q, t, rc, qb, qe, tb, te in (tuple(int(v) for v in r) for r in ranges):
        ql = len(seqs[q])
        out.append((V.revcomp(seqs[q]), (ql - qe, ql - qb, tb, te)) if rc else (seqs[q], (qb, qe, tb, te)))
    return out


def encode_want(ffi, recs):
    """(awv_cigar_text array, text bytes) of a list: offsets in record order."""
    out = np.zeros(len(recs), dtype=ffi.CIGAR_TEXT_DTYPE)
    text = bytearray()
    for k, r in enumerate(recs):
        out[k]["off"] = len(text)
        if r.status == 0 and r.ops:
            t, rec = ffi.encode_one_host(r.ops)
            out[k]["len"], out[k]["runs"] = rec["len"], rec["runs"]
            assert len(t) == int(rec["len"])
            text += t
    return out, bytes(text)


def cs_want(ffi, mode, recs):
    """(awv_cs_text array, text bytes) of a list."""
    out = np.zeros(len(recs), dtype=ffi.CS_TEXT_DTYPE)
    text = bytearray()
    for k, r in enumerate(recs):
        out[k]["off"] = len(text)
        if r.status != 0:
            out[k]["code"] = ffi.AWV_CST_SKIPPED
            continue
        t, rec = ffi.cs_one_host(mode, r.pattern, r.text, r.ops)
        out[k]["len"], out[k]["code"] = rec["len"], rec["code"]
        assert len(t) == int(rec["len"])
        text += t
    return out, bytes(text)


def coverage_want(ffi, roles, recs, seqs, geometry=None):
    """(awv_cov_item array, aligned, matched) of a list whose record k is the pair (2 k, 2 k + 1) of `seqs`: the tracks of all
    sequences in set order.  geometry: range_geometry's, for a list of ranges."""
    items = np.zeros(len(recs), dtype=ffi.COV_ITEM_DTYPE)
    aligned, matched = [], []
    for k, r in enumerate(recs):
        ql, tl = len(seqs[2 * k]), len(seqs[2 * k + 1])
        qt = (np.zeros(ql, dtype=np.uint32), np.zeros(ql, dtype=np.uint32))
        tt = (np.zeros(tl, dtype=np.uint32), np.zeros(tl, dtype=np.uint32))
        if r.status != 0:
            items[k]["code"] = ffi.AWV_CV_SKIPPED
        else:
            items[k], _, _ = ffi.coverage_one_host(roles, r.rc, ql, tl, r.ops, span=None if geometry is None else geometry[k][1], q_tracks=qt, t_tracks=tt)
        aligned += [qt[0], tt[0]]
        matched += [qt[1], tt[1]]
    return items, np.concatenate(aligned), np.concatenate(matched)


def variants_want(ffi, recs, seqs, geometry=None):
    """(awv_var_item array, [events of record k]) of a list whose record k is the pair (2 k, 2 k + 1) of `seqs`."""
    items = np.zeros(len(recs), dtype=ffi.VAR_ITEM_DTYPE)
    events = []
    for k, r in enumerate(recs):
        if r.status != 0:
            items[k]["code"] = ffi.AWV_VR_SKIPPED
            events.append(np.zeros(0, dtype=ffi.VARIANT_DTYPE))
            continue
        pattern, span = (r.pattern, None) if geometry is None else geometry[k]
        items[k], ev = ffi.variants_one_host(2 * k, 2 * k + 1, r.rc, pattern, len(seqs[2 * k + 1]), r.ops, span=span)
        events.append(ev)
    return items, events


def normalize_want(ffi, direction, recs, tail=b""):
    """(the arena afterwards, awv_norm_result array) of a list stored back to back with `tail` behind the last string."""
    out = np.zeros(len(recs), dtype=ffi.NORM_DTYPE)
    arena = bytearray()
    for k, r in enumerate(recs):
        if r.status != 0:
            out[k]["code"] = ffi.AWV_NM_SKIPPED
            arena += r.ops
        else:
            ops, out[k] = ffi.normalize_one_host(direction, r.pattern, r.text, r.ops)
            arena += ops
    return bytes(arena + tail), out


# ---- the ninth and tenth record passes: lift.hip, msa.hip ---------------------------------------------------------------------------
# They take records in the scan kernels' order too.  msa.hip's width and emit kernels carry the bases consumed (cq, ct), one past the
# last column so far that is no 'D' (run0) and whether the column before the chunk is a 'D' (prev_d); lift.hip carries the four op
# counts of the chunks before (tm, tx, ti, td), the answer behind the last aligned column so far (last_a) and the probe cursors
# (pp), and leaves five arrays in LDS.  The lists above serve both as they are.  What they trap here:
#   gap_tail -> gap_head (main-D, pass-D: 'D')   run0: B's leading 'D' run would begin at A's last column that is no 'D' -- it comes
#                                                out too narrow, or not at all; (main-I, pass-I: 'I') last_a: a query that ends inside
#                                                B's leading run of text-only columns would end at A's last aligned column
#   all_gaps -> plain                            prev_d: A ends in 'D', B begins with another op -- where B begins on a 16-byte
#                                                boundary (lift_msa_inputs puts it there) a carried bit counts a run that is none
#   any record with columns -> any with a base   cq / ct, the four counts: B would be walked from where A ended
#   the record with 200 queries -> the next      pp: B's probes would be behind the cursor and never answered
# lift.hip dispatches only records that have a query: its processing order at one workgroup is the list order restricted to them.

FROM_TARGET, FROM_QUERY = 1, 2   # AWV_LIFT_FROM_*
LIFT_SIDES = (FROM_TARGET, FROM_QUERY)
HEAVY = (130, 70)                # the queries of a record that has many: from the target, from the query


def lift_msa_inputs(recs):
    """(sequences, pairs [n, 3], RESULT_DTYPE records, arena) of a scan list for lift.hip and msa.hip: record k is the pair (2 k,
    2 k + 1), the strings back to back -- but a record that begins with an op other than 'D' behind one that ends in 'D' begins on
    the next 16-byte boundary, where alone msa.hip's carried prev_d can reach its first column (the bytes between hold 'D')."""
    from allwave_amd import ffi
    out = np.zeros(len(recs), dtype=ffi.RESULT_DTYPE)
    arena = bytearray()
    seqs, pairs = [], []
    for k, r in enumerate(recs):
        if k and recs[k - 1].ops[-1:] == b"D" and r.ops and r.ops[:1] != b"D":
            arena += b"D" * (-len(arena) % 16)
        out[k]["status"], out[k]["cigar_off"], out[k]["cigar_len"] = r.status, len(arena), len(r.ops)
        arena += r.ops
        seqs += [V.revcomp(r.pattern) if r.rc else r.pattern, r.text]
        pairs.append((2 * k, 2 * k + 1, r.rc))
    return seqs, np.asarray(pairs, dtype=np.int32).reshape(-1, 3), out, bytes(arena)


def has_query(k):
    """Every third record gets no query, and lift.hip does not dispatch it (the second of three: the key-0 list's SKIPPED records
    are every third from index 2 on and keep theirs)."""
    return k % 3 != 1


def sound(r):
    """Whether both passes walk the record as a sound one (awvcs::whole_code's rule) where it is the pair of its own sequences."""
    return (r.status == 0 and all(b in b"MXID" for b in r.ops) and len(r.ops) - r.ops.count(b"I") <= len(r.pattern)
            and len(r.ops) - r.ops.count(b"D") <= len(r.text))


def heavy_records(recs):
    """The records that get HEAVY queries: the first one, and the last one with a query that has two chunks wherever it begins
    (1,040 columns or more) and a sound record as the next one with a query -- which has fewer columns.  A list without such a
    record has the first one only."""
    ks = [k for k in range(len(recs)) if has_query(k)]
    two = [a for a, b in zip(ks, ks[1:]) if recs[a].status == 0 and len(recs[a].ops) >= CHUNK + 16 and sound(recs[b])]
    return sorted({0, two[-1]} if two else {0})


def lift_side(r, frm, qlen, tlen, span):
    """(s0, used, length, gap) of a record seen from one side, in the item's own coordinates: where its source bases begin, how
    many its string consumes, the source sequence's length, and the gap op that consumes the source alone."""
    pb, pe, tb, te = span
    if frm == FROM_TARGET:
        return tb, len(r.ops) - r.ops.count(b"D"), tlen, b"I"
    return pb, len(r.ops) - r.ops.count(b"I"), qlen, b"D"


def lift_queries(recs, seqs, seed, geometry=None):
    """[(record, from, beg, end)], deterministic, for a list whose record k is the pair (2 k, 2 k + 1) of `seqs` (geometry:
    range_geometry's, for a list of ranges), intervals on the source's forward strand.  From both sides of every record that gets
    any: the first base, the first few, the last base, the whole source interval, an interval that ends inside the leading run of
    source-only columns and one that begins inside the trailing one (where the record has them), and two random ones.  Every third
    record gets NO query: lift.hip does not dispatch it, so the processing order at one workgroup is the list order restricted to
    the records with a query.  heavy_records get HEAVY more: 100 from the target with both ends at source offsets 100 .. 900
    (one chunk answers 200 probes, 64 a step) or, in a record of more than two chunks, 1,100 .. 1,800 (the second chunk does),
    the others anywhere -- some stay pending into the chunks behind.  A record without a base on a side gets no query there."""
    rng = random.Random("reuse/lift/%s" % seed)
    heavy = heavy_records(recs)
    out = []
    for k, r in enumerate(recs):
        if not has_query(k):
            continue
        qlen, tlen = len(seqs[2 * k]), len(seqs[2 * k + 1])
        span = (0, qlen, 0, tlen) if geometry is None else geometry[k][1]
        for frm in LIFT_SIDES:
            s0, u, length, gap = lift_side(r, frm, qlen, tlen, span)
            head, tail = len(r.ops) - len(r.ops.lstrip(gap)), len(r.ops) - len(r.ops.rstrip(gap))
            item = [(s0, s0 + 1), (s0, s0 + min(4, max(u, 1))), (s0 + u - 1, s0 + u), (s0, s0 + u)]
            if head:
                item.append((s0, s0 + (head + 1) // 2))
            if tail:
                item.append((s0 + u - (tail + 1) // 2, s0 + u + 2))
            for _ in range(2):
                b = rng.randint(max(s0 - 3, 0), s0 + u + 2)
                item.append((b, b + rng.choice([1, 2, 5, 40, 3000])))
            if k in heavy:
                lo, hi = (1100, 1800) if len(r.ops) > 2 * CHUNK + 16 else (min(100, u // 3), min(900, u))
                for j in range(HEAVY[frm - 1]):
                    if frm == FROM_TARGET and j < 100:
                        b = s0 + rng.randint(lo, hi)
                        item.append((b, min(b + rng.randint(1, 60), s0 + max(hi, 1))))
                    else:
                        b = rng.randint(max(s0 - 3, 0), s0 + u + 2)
                        item.append((b, b + rng.choice([1, 7, 300, 3000])))
            for a, b in item:
                a, b = max(a, 0), min(b, length)
                if a < b:
                    out.append((k, frm) + ((qlen - b, qlen - a) if frm == FROM_QUERY and r.rc else (a, b)))
    return out


def lift_want(ffi, recs, queries, seqs, geometry=None):
    """The LIFT_DTYPE array of a list's queries: ffi.lift_one_host, the yardstick, one call per query (a record that is not
    completed: SKIPPED)."""
    out = np.zeros(len(queries), dtype=ffi.LIFT_DTYPE)
    for j, (k, frm, beg, end) in enumerate(queries):
        r = recs[k]
        if r.status != 0:
            out[j]["code"] = ffi.AWV_LF_SKIPPED
            continue
        out[j] = ffi.lift_one_host(frm, r.rc, len(seqs[2 * k]), len(seqs[2 * k + 1]), r.ops, beg, end, span=None if geometry is None else geometry[k][1])
    return out


def lift_walked(recs, queries):
    """(records, columns) a launch walks: the completed records that have a query, each once."""
    done = sorted({q[0] for q in queries if recs[q[0]].status == 0})
    return len(done), sum(len(recs[k].ops) for k in done)


def msa_layout(recs, seqs, shared, seed=0):
    """(sequences, pairs [n, 3], targets) of a list in one of two layouts.  own targets: record k is the pair (2 k, 2 k + 1) and the
    targets are all odd sequences -- every block has one item.  shared targets: three sequences S are appended to the set, each as
    long as the list's longest op string or longer, and record k is the pair (2 k, S[k mod 3]): a string may be shorter than its
    rectangle, so every well-formed string whose own query holds it stays sound, about a third of the list's items lie on each
    target from slot 0 on, the atomic maximum has contention and an item's row depends on widths other waves decided."""
    n = len(recs)
    if not shared:
        return list(seqs), np.asarray([(2 * k, 2 * k + 1, r.rc) for k, r in enumerate(recs)], dtype=np.int32).reshape(-1, 3), list(range(1, 2 * n, 2))
    rng = random.Random("reuse/msa/shared/%s" % seed)
    longest = max([len(r.ops) for r in recs] + [1])
    extra = [rand_seq(rng, longest + d) for d in (0, 7, 31)]
    pairs = np.asarray([(2 * k, 2 * n + k % 3, r.rc) for k, r in enumerate(recs)], dtype=np.int32).reshape(-1, 3)
    return list(seqs) + extra, pairs, [2 * n, 2 * n + 1, 2 * n + 2]


def msa_items(recs, pairs, geometry=None):
    """The records as msa_cases.msa_of's items."""
    return [(int(p[0]), int(p[1]), int(p[2]), r.ops, None if geometry is None else geometry[k][1], None, r.status) for k, (r, p) in enumerate(zip(recs, pairs))]


def msa_want(seqs, targets, items):
    """msa_cases.msa_of's answer to one call, with what the GPU tests compare byte for byte: `item_array` (MSA_ITEM_DTYPE),
    `target_array` (MSA_TARGET_DTYPE) and `arena`, the blocks one behind the other."""
    import msa_cases as M
    from allwave_amd import ffi
    w = M.msa_of(seqs, list(targets), items)
    w["item_array"] = np.array(w["items"], dtype=ffi.MSA_ITEM_DTYPE) if items else np.zeros(0, dtype=ffi.MSA_ITEM_DTYPE)
    w["target_array"] = np.array(w["targets"], dtype=ffi.MSA_TARGET_DTYPE) if targets else np.zeros(0, dtype=ffi.MSA_TARGET_DTYPE)
    w["arena"] = M.arena_of(w["blocks"])
    return w


def msa_host_of(ffi, seqs, s, items):
    """ffi.msa_host, the C yardstick, on the items of target s: (ins, width, codes, block)."""
    mine = [(V.revcomp(seqs[q]) if rev else bytes(seqs[q]), None if status != 0 else ops, span, sl) for q, t, rev, ops, span, sl, status in items if t == s]
    return ffi.msa_host(seqs[s], mine)


# the launch geometry of msa.hip's scan and target kernels: tiles of 1,024 slots, trips of 64 x 256 = 16,384 bases

GEOMETRY_LENS = (1023, 1024, 2047, 2048, 16500)  # len + 1 = 1,024, 1,025, 2,048, 2,049; one target longer than a trip
GEOMETRY_SLOTS = (0, 1023, 1024, 2047, 2048, 16383, 16384)


def geometry_slots(length):
    """The slots of a target of that length that get 'D' runs: those of GEOMETRY_SLOTS that exist, len - 1 and len."""
    return sorted({s for s in GEOMETRY_SLOTS if s <= length} | {length - 1, length})


def geometry_set(seed=0):
    """(sequences, ranges [n, 7], op strings, msa_of's items, targets) for awv_msa_ranges: five targets of GEOMETRY_LENS bases
    (sequences 0 .. 4) and four queries of 96 bases; at every slot of geometry_slots two items (a third at slot 0) with 'D' runs of
    different widths, M^a D^w M^b of a few dozen columns placed by tb = slot - a, every other one on the reverse strand."""
    rng = random.Random("reuse/msa/geometry/%s" % seed)
    seqs = [rand_seq(rng, n) for n in GEOMETRY_LENS] + [rand_seq(rng, 96) for _ in range(4)]
    ranges, strings, items = [], [], []
    for t, length in enumerate(GEOMETRY_LENS):
        for i, slot in enumerate(geometry_slots(length)):
            for w in ((1 + i % 3, 4 + i % 4) + ((9,) if slot == 0 else ())):
                a, b = min(slot, rng.randint(3, 20)), min(length - slot, rng.randint(1, 20))
                ops = b"M" * a + b"D" * w + b"M" * b
                q, rev = len(GEOMETRY_LENS) + len(items) % 4, len(items) % 2
                qb = rng.randint(0, 96 - (a + w + b))
                ranges.append((q, t, rev, qb, qb + a + w + b, slot - a, slot + b))
                pb = 96 - (qb + a + w + b) if rev else qb
                items.append((q, t, rev, ops, (pb, pb + a + w + b, slot - a, slot + b), None, 0))
                strings.append(ops)
    return seqs, np.asarray(ranges, dtype=np.int32), strings, items, list(range(len(GEOMETRY_LENS)))
