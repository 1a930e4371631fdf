"""CPU tests of the aligning call forms: what all seventeen entry points answer to a null engine, and which
entry point, with which pointers, ffi.Engine._align_plain calls for every request it accepts."""
import ctypes as C
import itertools

import pytest

PEN = (0, 5, 8, 2, 24, 1)


def test_every_form_refuses_a_null_engine(hip_lib):
    """The fourteen aligning calls: AWV_ERR_ARG, "null engine".  The three score calls: what awv_score_pairs answers -- without
    a GPU there is no engine to pass, and they say that first."""
    import torch
    from allwave_amd import ffi
    L = hip_lib
    pen = C.byref(ffi.Penalties.from_scores(PEN))
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    sink, cs_sink = ffi.SINK_FN(), ffi.CS_SINK_FN()
    calls = {"": lambda f: f(None, pen, p, 1, p, sink, None),
             "_verified": lambda f: f(None, pen, p, 1, p, p, sink, None),
             "_bounded": lambda f: f(None, pen, p, 1, p, p, p, sink, None),
             "_clipped": lambda f: f(None, pen, p, 1, p, 3, p, p, p, sink, None),
             "_encoded": lambda f: f(None, pen, p, 1, p, 3, p, p, p, p, sink, None),
             "_cs": lambda f: f(None, pen, p, 1, p, 3, p, p, p, p, ffi.AWV_CS_SHORT, p, cs_sink, None),
             "_split": lambda f: f(None, pen, p, 1, p, 3, 5, p, p, p, p, p, sink, None)}
    for kind in ("pairs", "ranges"):
        for suffix, call in calls.items():
            assert call(getattr(L, "awv_align_" + kind + suffix)) == ffi.AWV_ERR_ARG, (kind, suffix)
            assert b"null engine" in L.awv_last_error(), (kind, suffix)
    want = L.awv_score_pairs(None, pen, p, 1, -1, p)
    assert want == (ffi.AWV_ERR_ARG if torch.cuda.is_available() else ffi.AWV_ERR_NO_DEVICE)
    assert L.awv_score_pairs_bounded(None, pen, p, 1, p, p) == want
    assert L.awv_score_ranges(None, pen, p, 1, p, p) == want


# (verify, max_penalty, clip, split, encode, cs) -> (the entry point's suffix; which of the arguments passed are non-null ("1"):
# engine, penalties, list, n, the form's own arguments, sink, user; the length of the tuple that comes back).  Written out, not
# computed: this is what the callers in host.py, dist.py, bench.py and the tests rely on.
FORMS = {
    (False, None, None, None  , False, None   ): (''         , '1111110'       , 2),
    (True , None, None, None  , False, None   ): ('_verified', '11111110'      , 3),
    (False, 7   , None, None  , False, None   ): ('_bounded' , '111111010'     , 2),
    (True , 7   , None, None  , False, None   ): ('_bounded' , '111111110'     , 3),
    (False, None, 3   , None  , False, None   ): ('_clipped' , '11110110110'   , 3),
    (True , None, 3   , None  , False, None   ): ('_clipped' , '11110111110'   , 4),
    (False, 7   , 3   , None  , False, None   ): ('_clipped' , '11111110110'   , 3),
    (True , 7   , 3   , None  , False, None   ): ('_clipped' , '11111111110'   , 4),
    (False, None, None, None  , True , None   ): ('_encoded' , '111101100110'  , 3),
    (True , None, None, None  , True , None   ): ('_encoded' , '111101110110'  , 4),
    (False, 7   , None, None  , True , None   ): ('_encoded' , '111111100110'  , 3),
    (True , 7   , None, None  , True , None   ): ('_encoded' , '111111110110'  , 4),
    (False, None, 3   , None  , True , None   ): ('_encoded' , '111101101110'  , 4),
    (True , None, 3   , None  , True , None   ): ('_encoded' , '111101111110'  , 5),
    (False, 7   , 3   , None  , True , None   ): ('_encoded' , '111111101110'  , 4),
    (True , 7   , 3   , None  , True , None   ): ('_encoded' , '111111111110'  , 5),
    (False, None, None, None  , False, 'short'): ('_cs'      , '11110110001110', 3),
    (True , None, None, None  , False, 'short'): ('_cs'      , '11110111001110', 4),
    (False, 7   , None, None  , False, 'short'): ('_cs'      , '11111110001110', 3),
    (True , 7   , None, None  , False, 'short'): ('_cs'      , '11111111001110', 4),
    (False, None, 3   , None  , False, 'short'): ('_cs'      , '11110110101110', 4),
    (True , None, 3   , None  , False, 'short'): ('_cs'      , '11110111101110', 5),
    (False, 7   , 3   , None  , False, 'short'): ('_cs'      , '11111110101110', 4),
    (True , 7   , 3   , None  , False, 'short'): ('_cs'      , '11111111101110', 5),
    (False, None, None, None  , True , 'short'): ('_cs'      , '11110110011110', 4),
    (True , None, None, None  , True , 'short'): ('_cs'      , '11110111011110', 5),
    (False, 7   , None, None  , True , 'short'): ('_cs'      , '11111110011110', 4),
    (True , 7   , None, None  , True , 'short'): ('_cs'      , '11111111011110', 5),
    (False, None, 3   , None  , True , 'short'): ('_cs'      , '11110110111110', 5),
    (True , None, 3   , None  , True , 'short'): ('_cs'      , '11110111111110', 6),
    (False, 7   , 3   , None  , True , 'short'): ('_cs'      , '11111110111110', 5),
    (True , 7   , 3   , None  , True , 'short'): ('_cs'      , '11111111111110', 6),
    (False, None, None, (3, 5), False, None   ): ('_split'   , '11110111011110', 3),
    (True , None, None, (3, 5), False, None   ): ('_split'   , '11110111111110', 4),
    (False, 7   , None, (3, 5), False, None   ): ('_split'   , '11111111011110', 3),
    (True , 7   , None, (3, 5), False, None   ): ('_split'   , '11111111111110', 4),
}


class RecordingLib:
    """Stands in for the loaded library: every call is recorded and answers AWV_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.mark.parametrize("fn", ["awv_align_pairs", "awv_align_ranges"])
def test_align_plain_chooses_the_entry_point(monkeypatch, fn):
    from allwave_amd import ffi
    lib = RecordingLib()
    monkeypatch.setattr(ffi, "load", lambda: lib)
    e = ffi.Engine()
    arr = e._pair_array([(0, 1), (1, 0)]) if fn == "awv_align_pairs" else e._range_array([(0, 1, 0, 0, 4, 0, 4), (1, 0, 0, 0, 4, 0, 4)])
    seen = 0
    for key in itertools.product((False, True), (None, 7), (None, 3), (None, (3, 5)), (False, True), (None, "short")):
        verify, bound, clip, split, encode, cs = key
        del lib.calls[:]
        try:
            out = e._align_plain(fn, PEN, arr, True, verify, bound, clip, None, split, encode, cs)
        except ValueError:  # split goes with none of clip, encode and cs
            assert key not in FORMS and split is not None and (clip is not None or encode or cs is not None), key
            continue
        suffix, non_null, length = FORMS[key]
        (name, args), = [c for c in lib.calls if c[0].startswith("awv_align_")]
        assert name == fn + suffix, key
        assert "".join("0" if a is None else "1" for a in args) == non_null, key
        assert len(out) == length, key
        seen += 1
    assert seen == len(FORMS) == 36
