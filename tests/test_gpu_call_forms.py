"""GPU tests of the aligning call forms (the table): what each of the entry points refuses before anything is
launched, that every form returns the plain form's records, op bytes and texts, and that an accepted call resets the counters of
the steps it asks for and of no other.  Five pairs in batches of two: every `+ first` offset into the outputs is exercised."""
import ctypes as C
import random

import numpy as np
import pytest

from util import DEFAULT_2P

pytestmark = pytest.mark.gpu

BONUS, MIN_SCORE = 3, 5
NO_BOUND = 1 << 20  # a bound no pair of these sequences reaches: it binds nothing, but the call takes the bounded form
PAIRS = [(0, 1), (1, 0), (0, 2), (2, 3), (3, 1)]  # (0, 1) and (1, 0): a twin unit in the forms that allow one
STEPS = ("verify", "clip", "split", "normalize", "encode", "cs")
# what _align_plain is asked for, and the steps whose counters the call resets
FORMS = [("plain", {}, ()),
         ("verified", {"verify": True}, ("verify",)),
         ("bounded", {"max_penalty": NO_BOUND}, ()),
         ("bounded_verified", {"max_penalty": NO_BOUND, "verify": True}, ("verify",)),
         ("clipped", {"clip": BONUS}, ("clip",)),
         ("split", {"split": (BONUS, MIN_SCORE), "verify": True}, ("verify", "split")),
         ("encoded", {"encode": True}, ("encode",)),
         ("cs", {"cs": "short"}, ("cs",)),
         ("cs_encoded_verified", {"cs": "long", "encode": True, "verify": True, "max_penalty": NO_BOUND}, ("verify", "encode", "cs"))]
# the arguments of each entry point between the engine and penalties and the sink and user
SIGNATURES = {"": ("list", "n", "res"),
              "_verified": ("list", "n", "res", "vout"),
              "_bounded": ("list", "n", "bounds", "res", "vout"),
              "_clipped": ("list", "n", "bounds", "bonus", "res", "vout", "cout"),
              "_encoded": ("list", "n", "bounds", "bonus", "res", "vout", "cout", "tout"),
              "_cs": ("list", "n", "bounds", "bonus", "res", "vout", "cout", "tout", "mode", "csout"),
              "_split": ("list", "n", "bounds", "bonus", "min_score", "res", "vout", "seg_first", "iout", "sout")}


def sequences():
    rng = random.Random(7)
    base = bytes(rng.choice(b"ACGT") for _ in range(56))

    def sub(s, at):
        return s[:at] + bytes([b"ACGT"[(b"ACGT".index(s[at]) + 1) % 4]]) + s[at + 1:]
    s1 = sub(sub(base, 10), 30)
    s2 = sub(base[:20] + base[23:], 40)          # a 3-base deletion
    s3 = sub(base[4:25] + b"GTA" + base[25:50], 8)  # a 3-base insertion
    return [base, s1, s2, s3]


@pytest.fixture(scope="module")
def world(hip_lib):
    """The engine with its four sequences, the two lists, and the plain form's answer for each (computed once)."""
    from allwave_amd import ffi
    e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=2)
    seqs = sequences()
    assert all(30 <= len(s) <= 60 for s in seqs)
    e.set_sequences(seqs)
    ranges = [(q, t, 0, 0, len(seqs[q]), 0, len(seqs[t])) for q, t in PAIRS]
    ranges[2] = (0, 2, 0, 5, 40, 3, 40)  # a proper sub-interval of both
    lists = {"pairs": (e.align_pairs, e._pair_array(PAIRS), [(seqs[q], seqs[t]) for q, t in PAIRS]),
             "ranges": (e.align_ranges, e._range_array(ranges), [(seqs[r[0]][r[3]:r[4]], seqs[r[1]][r[5]:r[6]]) for r in ranges])}
    plain = {}
    for kind, (align, arr, _) in lists.items():
        res, cigs = align(DEFAULT_2P, arr)
        assert (res["status"] == 0).all() and all(cigs) and e.stats().launches > 0
        assert any(b"I" in c or b"D" in c for c in cigs) and any(b"X" in c for c in cigs)
        plain[kind] = (res, cigs)
    yield e, seqs, lists, plain
    e.close()


def snapshot(e):
    """All six steps' stats, every field of each."""
    return {step: tuple(getattr(st, f) for f, _ in st._fields_) for step in STEPS for st in [getattr(e, step + "_stats")()]}


# ---- the equality ladder

@pytest.mark.parametrize("kind", ["pairs", "ranges"])
@pytest.mark.parametrize("n", [5, 1, 0])
def test_every_form_returns_the_plain_forms_answer(world, kind, n):
    from allwave_amd import ffi
    e, _, lists, plain = world
    align, arr, subs = lists[kind]
    res0, cig0 = plain[kind][0][:n], plain[kind][1][:n]
    if n < 5:  # (cigar_off is relative to the batch: the shorter list's own plain call is the yardstick of its records)
        res0, cig1 = align(DEFAULT_2P, arr[:n])
        assert cig1 == cig0 and len(res0) == n
    for name, kw, _ in FORMS:
        out = align(DEFAULT_2P, arr[:n], **kw)
        assert out[0].dtype == ffi.RESULT_DTYPE and out[0].tobytes() == res0.tobytes(), (name, n)
        if "encode" in kw:
            assert out[1] == [ffi.encode_one_host(ops)[0] for ops in cig0], (name, n)
        else:
            assert out[1] == cig0, (name, n)
        if "verify" in kw:
            assert len(out[2]) == n and (out[2]["code"] == ffi.AWV_VF_OK).all(), (name, n)
        if "cs" in kw:
            texts, csout = out[-1]
            assert texts == [ffi.cs_one_host(kw["cs"], p, t, ops)[0] for (p, t), ops in zip(subs[:n], cig0)], (name, n)
            assert len(csout) == n and all(texts)
        if "clip" in kw:
            assert len(out[-1]) == n and (out[-1]["col_end"] > out[-1]["col_beg"]).all(), (name, n)
        if "split" in kw:
            index, segments = out[-1]
            assert len(index) == n == len(segments) and all(len(s) >= 1 for s in segments), (name, n)


# ---- the counter rule

@pytest.mark.parametrize("kind", ["pairs", "ranges"])
def test_an_accepted_call_resets_its_own_steps_counters_and_no_others(world, kind):
    e, _, lists, _ = world
    align, arr, _ = lists[kind]
    # every step has counted something before the first snapshot
    align(DEFAULT_2P, arr, verify=True, clip=BONUS, encode=True, cs="short", normalize="left")
    align(DEFAULT_2P, arr, split=(BONUS, MIN_SCORE))
    assert all(s[1] > 0 for s in snapshot(e).values())
    for name, kw, asked in FORMS:
        for n in (5, 0):
            before = snapshot(e)
            align(DEFAULT_2P, arr[:n], **kw)
            first = snapshot(e)
            align(DEFAULT_2P, arr[:n], **kw)
            second = snapshot(e)
            for step in STEPS:
                if step in asked:  # reset, not accumulated (a call without pairs launches nothing: its stats are empty)
                    assert first[step][1:] == second[step][1:] and (first[step][1] == n), (name, n, step)
                    assert n > 0 or first[step] == (0,) * len(first[step]), (name, n, step)
                else:
                    assert before[step] == first[step] == second[step], (name, n, step)
    # normalize: the engine's mode asks for it, in whichever form
    e.set_normalize("left")
    try:
        for name, kw, asked in FORMS[:2]:
            before = snapshot(e)
            align(DEFAULT_2P, arr, **kw)
            first = snapshot(e)
            align(DEFAULT_2P, arr, **kw)
            second = snapshot(e)
            for step in STEPS:
                if step == "normalize" or step in asked:
                    assert first[step][1:] == second[step][1:] and first[step][1] == 5, (name, step)
                else:
                    assert before[step] == first[step] == second[step], (name, step)
        before = snapshot(e)
        e.score_pairs(DEFAULT_2P, PAIRS)  # score-only: no step runs, the mode notwithstanding
        assert snapshot(e) == before
    finally:
        e.set_normalize(None)
    before = snapshot(e)
    align(DEFAULT_2P, arr)
    assert snapshot(e) == before and before["normalize"][1] == 5


# ---- the refusals: one fault each

class Caller:
    """Calls the entry points themselves, with arguments that are valid but for the ones a case replaces."""

    def __init__(self, e, lists):
        from allwave_amd import ffi
        self.ffi, self.e, self.L = ffi, e, ffi.load()
        self.lists = {k: v[1] for k, v in lists.items()}
        self.pen = ffi.Penalties.from_scores(DEFAULT_2P)
        n = 5
        self.keep = {"res": np.zeros(n, dtype=ffi.RESULT_DTYPE), "vout": np.zeros(n, dtype=ffi.VERIFY_DTYPE), "cout": np.zeros(n, dtype=ffi.CLIP_DTYPE),
                     "tout": np.zeros(n, dtype=ffi.CIGAR_TEXT_DTYPE), "csout": np.zeros(n, dtype=ffi.CS_TEXT_DTYPE),
                     "iout": np.zeros(n, dtype=ffi.SPLIT_INDEX_DTYPE), "bounds": np.full(n, NO_BOUND, dtype=np.int32),
                     "seg_first": {k: e.split_layout(v, BONUS, MIN_SCORE) for k, v in self.lists.items()}}
        self.keep["sout"] = np.zeros(int(max(s[-1] for s in self.keep["seg_first"].values())), dtype=ffi.CLIP_DTYPE)
        self.score_out = np.zeros(n, dtype=ffi.SCORE_DTYPE)

    def args(self, kind, suffix, over):
        k = self.keep
        a = {"list": self.lists[kind].ctypes.data, "n": 5, "bounds": k["bounds"].ctypes.data, "bonus": BONUS, "min_score": MIN_SCORE,
             "mode": self.ffi.AWV_CS_SHORT, "seg_first": k["seg_first"][kind].ctypes.data}
        a.update({name: k[name].ctypes.data for name in ("res", "vout", "cout", "tout", "csout", "iout", "sout")})
        assert set(over) <= set(a), over
        a.update({name: (v.ctypes.data if isinstance(v, np.ndarray) else v) for name, v in over.items()})
        return [a[name] for name in SIGNATURES[suffix]]

    def align(self, kind, suffix, engine=None, **over):
        h = self.e._h if engine is None else engine._h
        sink = self.ffi.CS_SINK_FN() if suffix == "_cs" else self.ffi.SINK_FN()
        return getattr(self.L, "awv_align_%s%s" % (kind, suffix))(h, C.byref(self.pen), *self.args(kind, suffix, over), sink, None)

    def score(self, fn, engine=None, **over):
        h = self.e._h if engine is None else engine._h
        a = {"list": self.lists["ranges" if fn == "awv_score_ranges" else "pairs"].ctypes.data, "n": 5, "bounds": self.keep["bounds"].ctypes.data}
        assert set(over) <= set(a), over
        a.update({name: (v.ctypes.data if isinstance(v, np.ndarray) else v) for name, v in over.items()})
        bound = -1 if fn == "awv_score_pairs" else a["bounds"]
        return getattr(self.L, fn)(h, C.byref(self.pen), a["list"], a["n"], bound, self.score_out.ctypes.data)

    def refused(self, call, code, message, engine=None):
        """`call` answers `code` with `message` in awv_last_error(), and launches nothing.  The call's own stats start from an
        accepted empty call's zeros: whether a refused call has cleared them already is not part of the contract."""
        e = self.e if engine is None else engine
        if engine is None:
            assert self.align("pairs", "", n=0) == self.ffi.AWV_OK
        before = e.stats().launches
        assert before == 0
        rc = call()
        assert rc == code and message.encode() in self.L.awv_last_error(), (rc, self.L.awv_last_error(), message)
        assert e.stats().launches == before


@pytest.fixture(scope="module")
def caller(world):
    e, _, lists, _ = world
    return Caller(e, lists)


def test_refusals_of_a_forms_own_arguments(world, caller):
    from allwave_amd import ffi
    c, ARG = caller, ffi.AWV_ERR_ARG
    for kind in ("pairs", "ranges"):
        c.refused(lambda: c.align(kind, "_verified", vout=None), ARG, "align_%s_verified: null vout" % kind)
        for bonus in (0, 32768):
            c.refused(lambda: c.align(kind, "_clipped", bonus=bonus), ARG, "align_clipped: match_bonus must be in [1, 32767]")
            c.refused(lambda: c.align(kind, "_split", bonus=bonus), ARG, "align_split: match_bonus must be in [1, 32767]")
        c.refused(lambda: c.align(kind, "_clipped", cout=None), ARG, "align_clipped: null cout")
        c.refused(lambda: c.align(kind, "_split", min_score=0), ARG, "align_split: min_score must be >= 1")
        c.refused(lambda: c.align(kind, "_split", seg_first=None), ARG, "align_split: null seg_first or iout")
        down = c.keep["seg_first"][kind][::-1].copy()
        c.refused(lambda: c.align(kind, "_split", seg_first=down), ARG, "align_split: seg_first must ascend")
        short = np.zeros(6, dtype=np.uint64)  # ascending, and no entry owns a slot
        c.refused(lambda: c.align(kind, "_split", seg_first=short), ARG, "owns fewer slots than awv_split_slots(a, min_score, min(plen, tlen))")
        c.refused(lambda: c.align(kind, "_encoded", tout=None), ARG, "align_encoded: null tout")
        c.refused(lambda: c.align(kind, "_cs", csout=None), ARG, "align_cs: null csout")
        c.refused(lambda: c.align(kind, "_cs", mode=3), ARG, "align_cs: cs_mode must be AWV_CS_SHORT or AWV_CS_LONG")
    c.refused(lambda: c.align("pairs", "_bounded", bounds=None), ARG, "align_pairs_bounded: null max_penalty")
    c.refused(lambda: c.score("awv_score_pairs_bounded", bounds=None), ARG, "score_pairs_bounded: null max_penalty")


def test_ranges_bounded_and_the_richer_forms_accept_null_bounds(world, caller):
    from allwave_amd import ffi
    _, _, _, plain = world
    for kind, suffix in (("ranges", "_bounded"), ("pairs", "_clipped"), ("ranges", "_clipped"), ("pairs", "_encoded"), ("ranges", "_cs"), ("pairs", "_split")):
        caller.keep["res"][:] = 0
        assert caller.align(kind, suffix, bounds=None) == ffi.AWV_OK, (kind, suffix)
        assert caller.keep["res"].tobytes() == plain[kind][0].tobytes(), (kind, suffix)


def test_refusals_of_the_list(world, caller):
    from allwave_amd import ffi
    c, ARG = caller, ffi.AWV_ERR_ARG
    bad_pairs = c.lists["pairs"].copy()
    bad_pairs["t_idx"][3] = 4
    bad_ranges = c.lists["ranges"].copy()
    bad_ranges["t_end"][2] = len(world[1][2]) + 1
    for suffix in SIGNATURES:
        for n, lst in ((-1, {}), (1, {"list": None})):
            c.refused(lambda: c.align("pairs", suffix, n=n, **lst), ARG, "align_pairs: null pairs")
            c.refused(lambda: c.align("ranges", suffix, n=n, **lst), ARG, "align_ranges: null ranges")
        c.refused(lambda: c.align("pairs", suffix, list=bad_pairs), ARG, "align_pairs: sequence index out of range")
        c.refused(lambda: c.align("ranges", suffix, list=bad_ranges), ARG, "align_ranges: range 2 names a sequence index or an interval out of range")
    c.refused(lambda: c.score("awv_score_pairs", n=-1), ARG, "score_pairs: npairs < 0")
    c.refused(lambda: c.score("awv_score_pairs_bounded", n=-1), ARG, "score_pairs: npairs < 0")
    c.refused(lambda: c.score("awv_score_ranges", n=-1), ARG, "score_ranges: null ranges")
    c.refused(lambda: c.score("awv_score_pairs", n=1, list=None), ARG, "align_pairs: null pairs")
    c.refused(lambda: c.score("awv_score_ranges", n=1, list=None), ARG, "score_ranges: null ranges")
    c.refused(lambda: c.score("awv_score_pairs", list=bad_pairs), ARG, "align_pairs: sequence index out of range")
    c.refused(lambda: c.score("awv_score_ranges", list=bad_ranges), ARG, "score_ranges: range 2 names a sequence index or an interval out of range")


def test_every_call_is_refused_before_set_sequences(world, caller):
    from allwave_amd import ffi
    c = caller
    fresh = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE, max_batch_pairs=2)
    try:
        for suffix in SIGNATURES:
            for kind in ("pairs", "ranges"):
                c.refused(lambda: c.align(kind, suffix, engine=fresh), ffi.AWV_ERR_STATE, "align_%s before set_sequences" % kind, engine=fresh)
        for fn, who in (("awv_score_pairs", "score_pairs"), ("awv_score_pairs_bounded", "score_pairs"), ("awv_score_ranges", "score_ranges")):
            c.refused(lambda: c.score(fn, engine=fresh), ffi.AWV_ERR_STATE, who + " before set_sequences", engine=fresh)
    finally:
        fresh.close()
