"""Inputs of the exhaustive tests (tests/test_exhaustive_cpu.py, tests/test_gpu_exhaustive.py): every ordered pair of the
short cores of two families, bare and between flanks that put one top-level BiWFA breakpoint search into the core.

Nothing here is sampled.  A family is every string over its alphabet up to a length (AC6: 127 cores, ACG4: 121); a layout
turns a core into the query-side and into the target-side sequence; a list is (sequences, pairs) with every ordered pair of
cores in it.  The flanks of a layout are drawn once from a random.Random seeded by the layout's name, so two builds of a
list are byte-identical.  tests/test_exhaustive_cpu.py proves from the oracle alone that the lists are traps: every pair
whose two sequences differ has exactly one breakpoint search, and the BiWFA op string differs from the unidirectional one
on well above 5 % of the pairs of every flanked layout -- a kernel that places the breakpoint, or breaks a tie at it,
differently from the oracle returns other bytes on thousands of pairs.

The long layouts have flanks of FLANK_LONG = 600 bases (two sequences of about 1,206 bases: more than the 1,024 summed bases
from which the kernels run multi-step passes)."""
import itertools
import random
from collections import namedtuple

import numpy as np

from util import rand_seq, rle

FAMILIES = {"AC6": (b"AC", 6), "ACG4": (b"ACG", 4)}
FLANK_SHORT = 140   # flank bases of the short layouts, on one side or 70 / 70
FLANK_LONG = 600    # flank bases on either side in the long layouts
IDENTICAL = ("bare", "core_at_end", "core_at_start", "balanced", "repeat_flanks")
LONG = ("long_k12_12", "long_k12_11", "long_k11_12", "long_k12_9")
LAYOUTS = IDENTICAL + LONG
#: flank seeds that are not the layout's name: with its own name as seed long_k11_12 missed the trap condition of
#: tests/test_exhaustive_cpu.py (ACG4 under the default penalties: 3.7 % of the pairs, 5 % are asked for)
FLANK_SEEDS = {"long_k11_12": "long_k11_12/2"}


def cores(alphabet, maxlen):
    """Every string over `alphabet` of length 0 .. maxlen, by length, then in the alphabet's order."""
    return [bytes(c) for n in range(maxlen + 1) for c in itertools.product(bytes(alphabet), repeat=n)]


def family(name):
    return cores(*FAMILIES[name])


def _substituted(s, k):
    """`s` with k evenly spaced substitutions: base (2 i + 1) len / 2 k becomes the next base of ACGT."""
    out = bytearray(s)
    for i in range(k):
        at = (2 * i + 1) * len(s) // (2 * k)
        out[at] = b"ACGT"[(b"ACGT".index(out[at]) + 1) % 4]
    return bytes(out)


class Layout(namedtuple("Layout", "name ql qr tl tr")):
    """The flanks of the query side (ql, qr) and of the target side (tl, tr)."""

    def query(self, core):
        return self.ql + core + self.qr

    def target(self, core):
        return self.tl + core + self.tr

    @property
    def identical(self):
        return (self.ql, self.qr) == (self.tl, self.tr)


def layout(name):
    """The layout of that name, its flanks drawn from random.Random(name)."""
    rng = random.Random("exhaustive/" + FLANK_SEEDS.get(name, name))
    if name == "bare":
        L = R = b""
    elif name == "core_at_end":
        L, R = rand_seq(rng, FLANK_SHORT), b""
    elif name == "core_at_start":
        L, R = b"", rand_seq(rng, FLANK_SHORT)
    elif name == "balanced":
        L, R = rand_seq(rng, FLANK_SHORT // 2), rand_seq(rng, FLANK_SHORT // 2)
    elif name == "repeat_flanks":  # a core's gap can slide into either flank
        L, R = rand_seq(rng, 60) + b"A" * 10, b"AC" * 5 + rand_seq(rng, 60)
    elif name.startswith("long_k"):
        kl, kr = (int(v) for v in name[len("long_k"):].split("_"))
        L, R = rand_seq(rng, FLANK_LONG), rand_seq(rng, FLANK_LONG)
        return Layout(name, L, R, _substituted(L, kl), _substituted(R, kr))
    else:
        raise ValueError(name)
    return Layout(name, L, R, L, R)


def build(fam, name):
    """(sequences, pairs [n, 2] int32) of one list, built anew.  Identical flanks: one sequence per core, the cores in order,
    and every ordered (i, j), self pairs included -- both orders of every pair, so twin units form.  Long layouts: the n
    queries, then the n targets, and every (q_i, t_j)."""
    lay, cs = layout(name), family(fam)
    n = len(cs)
    if lay.identical:
        seqs = [lay.query(c) for c in cs]
        pairs = [(i, j) for i in range(n) for j in range(n)]
    else:
        seqs = [lay.query(c) for c in cs] + [lay.target(c) for c in cs]
        pairs = [(i, n + j) for i in range(n) for j in range(n)]
    return seqs, np.asarray(pairs, dtype=np.int32)


_LISTS = {}


def lists(fam, name):
    """build(fam, name), built once and never changed."""
    if (fam, name) not in _LISTS:
        _LISTS[fam, name] = build(fam, name)
    return _LISTS[fam, name]


def twin_lists(fam, name):
    """The list with every entry's swap in it: the list itself under identical flanks; under a long layout (q_i, t_j) with
    (t_j, q_i) interleaved after each."""
    seqs, pairs = lists(fam, name)
    if layout(name).identical:
        return seqs, pairs
    both = np.empty((2 * len(pairs), 2), dtype=np.int32)
    both[0::2] = pairs
    both[1::2] = pairs[:, ::-1]
    return seqs, both


def core_of(fam, index):
    """The core of sequence `index` of any list of the family."""
    cs = family(fam)
    return cs[index % len(cs)]


#: the oracle's answers for one list: penalties (int32 [n]), op strings (list of bytes), op counts (int32 [n, 4]: M X I D)
Want = namedtuple("Want", "pen ops counts")


def _want(results):
    pen = np.asarray([p for p, _ in results], dtype=np.int32)
    ops = [o for _, o in results]
    counts = np.asarray([[o.count(k) for k in b"MXID"] for o in ops], dtype=np.int32).reshape(len(ops), 4)
    return Want(pen, ops, counts)


def in_chunks(oracle, n, work):
    """work(first, last) over [0, n) in slices on the oracle's thread pool (the oracle's calls release the interpreter lock);
    the slices' lists joined in order."""
    step = max(256, -(-n // 64))
    jobs = [oracle.dp_pool().submit(work, a, min(a + step, n)) for a in range(0, n, step)]
    return [x for j in jobs for x in j.result()]


def oracle_pairs(oracle, seqs, pairs, scores):
    """[(penalty, ops)] of awo_align for every entry, each slice on an aligner of its own."""
    pairs = np.asarray(pairs).tolist()

    def work(a, b):
        al = oracle.Aligner(scores)
        return [al.align(seqs[q], seqs[t]) for q, t in pairs[a:b]]

    return in_chunks(oracle, len(pairs), work)


_ORACLE = {}


def oracle_results(oracle, fam, name, scores, twin=False):
    """The oracle's Want for lists(fam, name) -- twin: for twin_lists(fam, name) --, computed once per (family, layout,
    scores) and shared by every test of the module's lifetime; never changed."""
    key = (fam, name, tuple(scores), bool(twin) and not layout(name).identical)
    if key not in _ORACLE:
        if key[3]:
            seqs, pairs = lists(fam, name)
            plain = oracle_results(oracle, fam, name, scores)
            swapped = oracle_pairs(oracle, seqs, pairs[:, ::-1], scores)
            both = [r for k, s in enumerate(swapped) for r in ((int(plain.pen[k]), plain.ops[k]), s)]
            _ORACLE[key] = _want(both)
        else:
            seqs, pairs = lists(fam, name)
            _ORACLE[key] = _want(oracle_pairs(oracle, seqs, pairs, scores))
    return _ORACLE[key]


def records(want):
    """[(penalty, ops)] of a Want."""
    return [(int(p), o) for p, o in zip(want.pen, want.ops)]


def check(got, want, fam, name, seqs, pairs, where=()):
    """Every record field and every op byte of an aligning call against the oracle's: status 0; penalty, score, cigar_len,
    the four counts, q_end and t_end.  A difference is reported with the family, the layout, the two cores and the RLE of
    both strings."""
    res, cigs = got
    pairs = np.asarray(pairs)
    ql = np.asarray([len(s) for s in seqs], dtype=np.int64)
    ok = (res["status"] == 0) & (res["penalty"] == want.pen) & (res["score"] == -want.pen.astype(np.int64))
    ok &= res["cigar_len"] == np.asarray([len(o) for o in want.ops], dtype=np.int64)
    for k, f in enumerate(("num_matches", "num_mismatches", "num_ins", "num_del")):
        ok &= res[f] == want.counts[:, k]
    ok &= (res["q_end"] == ql[pairs[:, 0]]) & (res["t_end"] == ql[pairs[:, 1]])
    if ok.all() and cigs == want.ops:
        return
    bad = [i for i in range(len(pairs)) if not ok[i] or cigs[i] != want.ops[i]]
    i = bad[0]
    q, t = int(pairs[i][0]), int(pairs[i][1])
    assert False, (where, fam, name, "entry %d of %d differs (%d in all)" % (i, len(pairs), len(bad)), "cores", core_of(fam, q), core_of(fam, t),
                   "status %d penalty %d, the oracle's %d" % (res["status"][i], res["penalty"][i], want.pen[i]),
                   "got", rle(cigs[i]) if cigs[i] is not None else None, "want", rle(want.ops[i]))


_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(_RC)[::-1]


def book_ranges(fam="AC6", name="balanced"):
    """The list as ranges of three resident sequences: 0 the query book -- the list's sequences one behind the other --,
    1 the target book (the same bytes: the flanks are identical), 2 the reverse complement of the query book.  Returns
    (books, forward ranges [n, 7], reversed ranges [n, 7]): entry k of either is pair k of the list, the reversed one
    through book 2 with q_revcomp set.  The neighbouring record's identical flank lies directly beyond both ends of every
    interval, so a probe that runs past an interval's end goes on matching."""
    seqs, pairs = lists(fam, name)
    assert layout(name).identical
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int64)
    book = b"".join(seqs)
    total = len(book)
    q, t = pairs[:, 0], pairs[:, 1]
    zero = np.zeros(len(pairs), dtype=np.int64)
    fwd = np.stack([zero, zero + 1, zero, off[q], off[q + 1], off[t], off[t + 1]], axis=1).astype(np.int32)
    rev = np.stack([zero + 2, zero + 1, zero + 1, total - off[q + 1], total - off[q], off[t], off[t + 1]], axis=1).astype(np.int32)
    return [book, book, revcomp(book)], fwd, rev
