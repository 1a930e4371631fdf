"""ctypes binding of liballwave_host.so -- the C++ mirror of allwave's host API (csrc/host/allwave.hpp).
Product path: no oracle, no CPU fallback (alignment entry points need the GPU)."""
import ctypes as C
import os

import numpy as np

from . import ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liballwave_host.so")
_LIB = None
ERRCAP = 512
_CAP = C.c_size_t(ERRCAP)  # size_t arguments are always passed as c_size_t (stack slots are 8 bytes wide)


class HostError(RuntimeError):
    pass


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        ffi.load()  # liballwave_hip.so first (same directory; also resolved through $ORIGIN)
        L = C.CDLL(LIB_PATH)
        L.awh_free.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def _err():
    return C.create_string_buffer(ERRCAP)


def parse_scores(s):
    """lib.rs:116-153: returns the 4 or 6 parsed scores; raises ValueError with the reference's message."""
    out = (C.c_int32 * 6)()
    n = C.c_int(0)
    e = _err()
    if load().awh_parse_scores(s.encode(), out, C.byref(n), e, _CAP) != 0:
        raise ValueError(e.value.decode())
    return tuple(out[:n.value])


def mode_and_penalties(s):
    """AlignmentMode::from_params (types.rs:107-116) + the penalties create_wfa_aligner passes down."""
    mode = C.c_int(0)
    pen = (C.c_int32 * 7)()
    e = _err()
    if load().awh_mode_from_scores(s.encode(), C.byref(mode), pen, e, _CAP) != 0:
        raise ValueError(e.value.decode())
    return ("EditDistance", "SinglePieceAffine", "TwoPieceAffine")[mode.value], tuple(pen)


def cigar_bytes_to_string(ops):
    ops = bytes(ops)
    buf = C.create_string_buffer(4 * len(ops) + 16)
    n = load().awh_cigar_to_string(ops, C.c_size_t(len(ops)), buf, C.c_size_t(len(buf)))
    if n < 0:
        raise HostError("buffer")
    return buf.value.decode()


def reverse_complement(seq):
    seq = bytes(seq)
    out = C.create_string_buffer(len(seq) + 1)
    load().awh_reverse_complement(seq, C.c_size_t(len(seq)), out)
    return out.raw[:len(seq)]


def format_paf(qid, qlen, tid, tlen, qs, qe, ts, te, is_reverse, num_matches, alignment_length, ops):
    ops = bytes(ops)
    buf = C.create_string_buffer(4 * len(ops) + 512)
    n = load().awh_format_paf(qid.encode(), C.c_size_t(qlen), tid.encode(), C.c_size_t(tlen), C.c_size_t(qs),
                              C.c_size_t(qe), C.c_size_t(ts), C.c_size_t(te), int(is_reverse),
                              C.c_size_t(num_matches), C.c_size_t(alignment_length), ops, C.c_size_t(len(ops)), buf,
                              C.c_size_t(len(buf)))
    if n < 0:
        raise HostError("buffer")
    return buf.value.decode()


def validate_cigar(ops, qlen, rlen):
    """wfa.rs:105-176: returns None when valid, else the reference's error text."""
    ops = bytes(ops)
    e = _err()
    rc = load().awh_validate_cigar(ops, C.c_size_t(len(ops)), C.c_size_t(qlen), C.c_size_t(rlen), e, _CAP)
    return None if rc == 0 else e.value.decode()


def set_engine_config(flags=0, first_row_cols=0, release=True):
    """awv_engine_config.flags / first_row_cols of the per-device engines the host library creates from now on; `release`
    destroys the cached engines first, so the next run gets a fresh one under this configuration."""
    load().awh_set_engine_config(int(flags), int(first_row_cols), int(bool(release)))


ORIENT = {"forward": 0, "wfa": 1, "mash": 2}

VERIFY_CODES = ("ok", "skipped", "bad_op", "overrun", "m_differs", "x_equal", "short", "counts", "penalty")  # ffi.AWV_VF_*


def last_verify():
    """What this thread's last all_pairs_paf / iterate / all_pairs_paf_count call left (zeros and no failures without verify=True):
    dict(pairs, failed, columns, kernel_ms -- last_verify_stats(), summed over the slots -- and failures: verify_failures(),
    one dict(index, query_idx, target_idx, is_reverse, code, class, column, penalty) per failed pair, by pair-list index)."""
    st = ffi.VerifyStats()
    out = C.c_void_p()
    n = C.c_size_t(0)
    if load().awh_last_verify(C.byref(st), C.byref(out), C.byref(n)) != 0:
        raise HostError("out of memory")
    k = n.value
    raw = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int64)), shape=(max(k, 1) * 7,))[:7 * k].reshape(k, 7).copy()
    load().awh_free(out)
    fails = [dict(index=int(r[0]), query_idx=int(r[1]), target_idx=int(r[2]), is_reverse=bool(r[3]), code=int(r[4]),
                  **{"class": VERIFY_CODES[int(r[4])] if 0 <= int(r[4]) < len(VERIFY_CODES) else "unknown"},
                  column=int(r[5]), penalty=int(r[6])) for r in raw]
    return dict(pairs=int(st.pairs), failed=int(st.failed), columns=int(st.columns), kernel_ms=float(st.kernel_ms), failures=fails)


def _set_bounds(max_penalty, max_divergence):
    """awh_set_bounds: the bounds of this thread's next alignment hook (None: none); that hook takes them."""
    if max_penalty is not None and int(max_penalty) < 0:
        raise ValueError("max_penalty must be >= 0 (None: no bound)")
    if max_divergence is not None and not 0.0 <= float(max_divergence) < 1.0:
        raise ValueError("max_divergence must be in [0, 1) (None: no bound)")
    load().awh_set_bounds(C.c_int64(-1 if max_penalty is None else int(max_penalty)),
                          C.c_double(-1.0 if max_divergence is None else float(max_divergence)))


def _check_clip(clip, clip_min_score):
    """(match bonus, least score) of clip= / clip_min_score=, (0, 1) for no clipping; ValueError before anything is set."""
    if clip is None:
        if clip_min_score is not None:
            raise ValueError("clip_min_score needs clip")
        return 0, 1
    if not 1 <= int(clip) <= 32767:
        raise ValueError("clip: the match bonus must be in [1, 32767] (None: no clipping)")
    if clip_min_score is not None and int(clip_min_score) < 1:
        raise ValueError("clip_min_score must be >= 1")
    return int(clip), 1 if clip_min_score is None else int(clip_min_score)


def _check_split(split, split_min_score, clip):
    """(match bonus, least score) of split= / split_min_score=, (0, 1) for no splitting; ValueError before anything is set."""
    if split is None:
        if split_min_score is not None:
            raise ValueError("split_min_score needs split")
        return 0, 1
    if clip is not None:
        raise ValueError("split and clip exclude each other")
    if not 1 <= int(split) <= 32767:
        raise ValueError("split: the match bonus must be in [1, 32767] (None: no splitting)")
    if split_min_score is None:
        raise ValueError("split needs split_min_score: no default can be derived")
    if int(split_min_score) < 1:
        raise ValueError("split_min_score must be >= 1")
    return int(split), int(split_min_score)


def _set_run_options(max_penalty, max_divergence, clip, clip_min_score, split=None, split_min_score=None, normalize=None, device_cigar=False,
                     cs=None, coverage=None, variants=False, liftover=None, liftover_from=None, ids=None, msa_targets=None, msa_max_bytes=None):
    """The bounds, the clipping, the splitting, the normalization, the device-side CIGAR text and the cs tag of this thread's next
    alignment hook, which takes them: every argument is checked before anything is set, and all settings are always written
    (awh_set_bounds, awh_set_clip, awh_set_split, awh_set_normalize, awh_set_device_cigar, awh_set_cs, awh_set_coverage,
    awh_set_variants, awh_set_liftover, awh_set_msa)."""
    bonus, least = _check_clip(clip, clip_min_score)
    sbonus, sleast = _check_split(split, split_min_score, clip)
    mode = ffi.norm_mode(normalize)
    if device_cigar and sbonus:
        raise ValueError("device_cigar and split exclude each other")
    cs_mode = ffi.cs_mode(cs)
    if cs_mode and sbonus:
        raise ValueError("cs and split exclude each other")
    roles = ffi.coverage_roles(coverage) if coverage is None or isinstance(coverage, str) else None
    if roles is None:
        raise ValueError("coverage: None, 'target', 'query' or 'both', not %r" % (coverage,))
    regions, side = _check_liftover(liftover, liftover_from, ids)
    msa_on, targets, bound = _check_msa(msa_targets, msa_max_bytes, ids, device_cigar)
    _set_bounds(max_penalty, max_divergence)
    load().awh_set_clip(bonus, C.c_int64(least))
    load().awh_set_split(sbonus, C.c_int64(sleast))
    load().awh_set_normalize(int(mode))
    load().awh_set_device_cigar(int(bool(device_cigar)))
    load().awh_set_cs(int(cs_mode))
    load().awh_set_coverage(int(roles))
    load().awh_set_variants(int(bool(variants)))
    load().awh_set_liftover.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    load().awh_set_liftover(regions.ctypes.data if len(regions) else None, len(regions), int(side))
    load().awh_set_msa.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64]
    load().awh_set_msa(int(msa_on), targets.ctypes.data if len(targets) else None, len(targets), int(bound))


def _check_msa(msa_targets, msa_max_bytes, ids, device_cigar):
    """(on, an int32 array of target indices -- empty: every sequence --, the bound or 0 for the default) of msa_targets= /
    msa_max_bytes=: msa_targets is None (off), "all" or an empty list (every sequence), or a list of indices or ids."""
    if msa_targets is None:
        if msa_max_bytes is not None:
            raise ValueError("msa_max_bytes requires msa_targets")
        return False, np.zeros(0, dtype=np.int32), 0
    if device_cigar:
        raise ValueError("msa_targets: not together with device_cigar (the sink then carries text, not op bytes)")
    if msa_max_bytes is not None and (isinstance(msa_max_bytes, bool) or int(msa_max_bytes) < 1):
        raise ValueError("msa_max_bytes: a positive number of bytes, not %r" % (msa_max_bytes,))
    if isinstance(msa_targets, str) and msa_targets == "all":
        msa_targets = []
    if isinstance(msa_targets, (str, bytes)):
        raise ValueError("msa_targets: 'all' or a list of indices or ids, not %r" % (msa_targets,))
    where = {name: k for k, name in enumerate(ids or [])}
    out = []
    for t in msa_targets:
        if isinstance(t, (str, bytes)):
            if t not in where:
                raise ValueError("msa_targets: no sequence named %r" % (t,))
            t = where[t]
        t = int(t)
        if t < 0 or t >= len(ids or []) or t in out:
            raise ValueError("msa_targets: index %d is out of range or named twice" % t)
        out.append(t)
    return True, np.array(out, dtype=np.int32), 0 if msa_max_bytes is None else int(msa_max_bytes)


def last_msa():
    """last_msa() of this thread's last all_pairs_paf / all_pairs_paf_count / iterate / align_ranges call with msa_targets=...:
    {target index: (names, block)} -- block the target's multiple alignment as a 2-D uint8 array (rows x width, '-' for a gap), names
    the rows' names: the target's id for row 0, `qname/qbeg-qend` and the strand sign for an item's row.  Built in one device call
    after the run, so several devices give the one-engine blocks exactly.  Empty for a call without msa_targets.
    last_msa.stats is not kept: last_msa_stats() returns the call's ffi.MsaStats."""
    return _last_msa()[0]


def last_msa_stats():
    """The ffi.MsaStats of the awv_msa_ranges call behind last_msa()."""
    return _last_msa(blocks=False)[1]


def _last_msa(blocks=True):
    L = load()
    st = ffi.MsaStats()
    L.awh_last_msa.argtypes = [C.c_void_p]
    L.awh_last_msa.restype = C.c_size_t
    L.awh_last_msa_block.argtypes = [C.c_size_t] + [C.c_void_p] * 6
    n = L.awh_last_msa(C.byref(st))
    out = {}
    for j in range(n if blocks else 0):
        t, rows, width, nlen = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_size_t(0)
        names, data = C.c_void_p(), C.c_void_p()
        if L.awh_last_msa_block(j, C.byref(t), C.byref(rows), C.byref(width), C.byref(names), C.byref(nlen), C.byref(data)) != 0:
            raise HostError("out of memory")
        try:
            nm = C.string_at(names, nlen.value).decode().split("\n")[:-1]
            nbytes = rows.value * width.value
            blk = np.frombuffer(C.string_at(data, nbytes), dtype=np.uint8).copy() if nbytes else np.zeros(0, dtype=np.uint8)
        finally:
            L.awh_free(names)
            L.awh_free(data)
        out[t.value] = (nm, blk.reshape(rows.value, width.value))
    return out, st


def _check_liftover(liftover, liftover_from, ids):
    """(an ffi.REGION_DTYPE array, the AWV_LIFT_FROM_* mask) of liftover= / liftover_from=: liftover is None (off), an
    ffi.REGION_DTYPE array or (seq, beg, end) rows, seq an index or one of `ids`; liftover_from "target" (the default), "query" or
    "both"."""
    if liftover is None:
        if liftover_from is not None:
            raise ValueError("liftover_from requires liftover")
        return np.zeros(0, dtype=ffi.REGION_DTYPE), 0
    side = ffi.lift_from("target" if liftover_from is None else liftover_from) if liftover_from is None or isinstance(liftover_from, str) else 0
    if not side:
        raise ValueError("liftover_from: 'target', 'query' or 'both', not %r" % (liftover_from,))
    if isinstance(liftover, np.ndarray) and liftover.dtype == ffi.REGION_DTYPE:
        return np.ascontiguousarray(liftover), side
    where = {name: k for k, name in enumerate(ids or [])}
    out = np.zeros(len(liftover), dtype=ffi.REGION_DTYPE)
    for k, row in enumerate(liftover):
        if len(row) != 3:
            raise ValueError("liftover: (seq, beg, end) rows")
        seq = row[0]
        if isinstance(seq, (str, bytes)):
            if seq not in where:
                raise ValueError("liftover: no sequence named %r" % (seq,))
            seq = where[seq]
        out[k] = (int(seq), int(row[1]), int(row[2]))
    return out, side


def last_liftover():
    """last_liftover() of this thread's last all_pairs_paf / all_pairs_paf_count / iterate / align_ranges call with liftover=...:
    dict(rows, stats) -- rows the lifted regions (ffi.LIFT_ROW_DTYPE, sorted by all fields, region first), the slots' rows
    concatenated and sorted, so several devices give the one-engine table exactly; stats an ffi.LiftStats summed over the slots.
    rows is empty for a call without liftover."""
    rows = C.c_void_p()
    n = C.c_size_t(0)
    st = ffi.LiftStats()
    L = load()
    L.awh_last_liftover.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if L.awh_last_liftover(C.byref(rows), C.byref(n), C.byref(st)) != 0:
        raise HostError("out of memory")
    try:
        nbytes = n.value * ffi.LIFT_ROW_DTYPE.itemsize
        out = np.frombuffer(C.string_at(rows, nbytes), dtype=ffi.LIFT_ROW_DTYPE).copy() if nbytes else np.zeros(0, dtype=ffi.LIFT_ROW_DTYPE)
    finally:
        L.awh_free(rows)
    return dict(rows=out, stats=st)


def last_coverage():
    """last_coverage() of this thread's last all_pairs_paf / all_pairs_paf_count / iterate / align_ranges call with coverage=...:
    dict(offsets, aligned, matched, items, failed, columns, boundaries, reads, kernel_ms) -- sequence s owns entries
    [offsets[s], offsets[s + 1]) of the two uint32 arrays, one per forward-strand base, summed over the slots; the counters are
    awv_cov_stats summed over the slots.  offsets is None, and the arrays are empty, for a call without coverage."""
    offs, al, ma = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    n = C.c_size_t(0)
    st = (C.c_uint64 * 5)()
    ms = C.c_double(0)
    L = load()
    L.awh_last_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.awh_last_coverage(C.byref(offs), C.byref(n), C.byref(al), C.byref(ma), st, C.byref(ms)) != 0:
        raise HostError("out of memory")
    try:
        k = n.value
        offsets = np.ctypeslib.as_array(offs, shape=(max(k, 1),))[:k].astype(np.int64) if k else None
        total = int(offsets[-1]) if k else 0
        aligned = np.ctypeslib.as_array(al, shape=(max(total, 1),))[:total].copy()
        matched = np.ctypeslib.as_array(ma, shape=(max(total, 1),))[:total].copy()
    finally:
        for p in (offs, al, ma):
            L.awh_free(C.cast(p, C.c_void_p))
    return dict(offsets=offsets, aligned=aligned, matched=matched, items=int(st[0]), failed=int(st[1]), columns=int(st[2]),
                boundaries=int(st[3]), reads=int(st[4]), kernel_ms=float(ms.value))


def last_variants():
    """last_variants() of this thread's last all_pairs_paf / all_pairs_paf_count / iterate / align_ranges call with variants=True:
    dict(rows, stats) -- rows the per-site allele table (ffi.VARIANT_DTYPE, in key order), the slots' tables merged by key (sum of
    count, min of rep), so several devices give the one-engine table exactly; stats an ffi.VariantsStats summed over the slots
    (rows: of the merged table).  rows is empty for a call without variants."""
    rows = C.c_void_p()
    n = C.c_size_t(0)
    st = ffi.VariantsStats()
    L = load()
    L.awh_last_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if L.awh_last_variants(C.byref(rows), C.byref(n), C.byref(st)) != 0:
        raise HostError("out of memory")
    try:
        nbytes = n.value * ffi.VARIANT_DTYPE.itemsize
        out = np.frombuffer(C.string_at(rows, nbytes), dtype=ffi.VARIANT_DTYPE).copy() if nbytes else np.zeros(0, dtype=ffi.VARIANT_DTYPE)
    finally:
        L.awh_free(rows)
    return dict(rows=out, stats=st)


def last_cs():
    """last_cs_stats() of this thread's last all_pairs_paf / all_pairs_paf_count / align_ranges call: dict(pairs, failed,
    text_bytes, columns, kernel_ms), summed over the slots (zeros for a call without cs, and for iterate, whose consumers hand
    out alignment records)."""
    out = (C.c_uint64 * 4)()
    ms = C.c_double(0)
    load().awh_last_cs(out, C.byref(ms))
    return dict(pairs=int(out[0]), failed=int(out[1]), text_bytes=int(out[2]), columns=int(out[3]), kernel_ms=float(ms.value))


def last_encode():
    """last_encode_stats() of this thread's last all_pairs_paf / all_pairs_paf_count / align_ranges call: dict(pairs, runs,
    text_bytes, columns, kernel_ms), summed over the slots (zeros for a call without device_cigar, and for iterate, whose
    consumers hand out op bytes)."""
    out = (C.c_uint64 * 4)()
    ms = C.c_double(0)
    load().awh_last_encode(out, C.byref(ms))
    return dict(pairs=int(out[0]), runs=int(out[1]), text_bytes=int(out[2]), columns=int(out[3]), kernel_ms=float(ms.value))


def last_normalize():
    """last_normalize_stats() of this thread's last all_pairs_paf / iterate / all_pairs_paf_count / align_ranges call:
    dict(pairs, records_moved, runs, runs_moved, columns_moved, columns, kernel_ms), summed over the slots (zeros for a call
    without normalize)."""
    out = (C.c_uint64 * 6)()
    ms = C.c_double(0)
    load().awh_last_normalize(out, C.byref(ms))
    return dict(pairs=int(out[0]), records_moved=int(out[1]), runs=int(out[2]), runs_moved=int(out[3]), columns_moved=int(out[4]),
                columns=int(out[5]), kernel_ms=float(ms.value))


def last_split():
    """last_split_stats() of this thread's last all_pairs_paf / iterate / all_pairs_paf_count / align_ranges call:
    dict(pairs, segments, empty, kernel_ms) -- finished pairs whose alignment was split, the segments they gave (one line or
    record each), and the pairs left out because no segment scores split_min_score (zeros for a call without split)."""
    out = (C.c_uint64 * 3)()
    ms = C.c_double(0)
    load().awh_last_split(out, C.byref(ms))
    return dict(pairs=int(out[0]), segments=int(out[1]), empty=int(out[2]), kernel_ms=float(ms.value))


def last_clip():
    """last_clip_stats() of this thread's last all_pairs_paf / iterate / all_pairs_paf_count / align_ranges call:
    dict(pairs, empty, below_min_score, kernel_ms) -- finished pairs whose alignment was clipped, and of them the ones left
    out because the clip is empty or scores below clip_min_score (zeros for a call without clip)."""
    out = (C.c_uint64 * 3)()
    ms = C.c_double(0)
    load().awh_last_clip(out, C.byref(ms))
    return dict(pairs=int(out[0]), empty=int(out[1]), below_min_score=int(out[2]), kernel_ms=float(ms.value))


def last_bounds():
    """last_bound_stats() of this thread's last all_pairs_paf / iterate / all_pairs_paf_count / align_ranges call:
    dict(pairs, above_penalty, above_divergence) -- pairs aligned under a bound, and of them the ones left out because their
    penalty is above max_penalty or their divergence above max_divergence (zeros for a call without bounds)."""
    out = (C.c_uint64 * 3)()
    load().awh_last_bounds(out)
    return dict(pairs=int(out[0]), above_penalty=int(out[1]), above_divergence=int(out[2]))


def verify_failure_path(ids, pairs, first, calls):
    """The way a failed check travels above the engine, without an engine (append_verify_failures per engine call,
    sort_verify_failures, report_verify_failures, the record packing of last_verify()).  pairs: the run's range of (q, t)
    pairs, which starts at pair-list index `first`; calls: one list per engine call, in the order the calls finish, of
    (place in the range, is_reverse, code, column, penalty) per entry.  Returns (exit status, report text); last_verify()
    then holds the failures."""
    p = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    flat = [e for c in calls for e in c]
    cuts = np.zeros(len(calls) + 1, dtype=np.uint64)
    cuts[1:] = np.cumsum([len(c) for c in calls], dtype=np.uint64)
    idx = np.array([e[0] for e in flat] + [0], dtype=np.int64)
    rev = np.array([1 if e[1] else 0 for e in flat] + [0], dtype=np.uint8)
    code = np.array([e[2] for e in flat] + [0], dtype=np.int32)
    col = np.array([e[3] for e in flat] + [0], dtype=np.int64)
    pen = np.array([e[4] for e in flat] + [0], dtype=np.int64)
    cids = (C.c_char_p * len(ids))(*[i.encode() for i in ids])
    buf = C.create_string_buffer(1 << 16)
    rc = load().awh_verify_failure_path(len(ids), cids, p.ctypes.data_as(C.c_void_p), C.c_size_t(len(p)), C.c_size_t(int(first)),
                                        idx.ctypes.data_as(C.c_void_p), rev.ctypes.data_as(C.c_void_p), code.ctypes.data_as(C.c_void_p),
                                        col.ctypes.data_as(C.c_void_p), pen.ctypes.data_as(C.c_void_p), cuts.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(len(calls)), buf, C.c_size_t(len(buf)))
    return rc, buf.value.decode()


def cigar_string_to_bytes(cg):
    """The op bytes of a PAF cg string: cigar_bytes_to_string undone ('=' -> M, X -> X, D -> I, I -> D).  ValueError for a
    string that is not <count><op>... over those letters."""
    cg = cg.encode() if isinstance(cg, str) else bytes(cg)
    cap = 16
    num = b""
    for ch in cg:  # (an upper bound of the op bytes: the sum of the counts)
        if 48 <= ch <= 57:
            num += bytes([ch])
        else:
            cap += int(num or b"0")
            num = b""
    if cap > (1 << 31):
        raise ValueError("malformed cg string")
    buf = C.create_string_buffer(cap)
    L = load()
    L.awh_cigar_string_to_bytes.restype = C.c_long
    n = L.awh_cigar_string_to_bytes(cg, buf, C.c_size_t(cap))
    if n < 0:
        raise ValueError("malformed cg string")
    return buf.raw[:n]


def check_paf(ids, seqs, paf_text, scores, optimal=False, device=0, partial=False):
    """Checks every line of a PAF (12 columns + cg:Z:) against the sequences on `device`; nothing is aligned (check_paf in
    allwave.hpp).  partial: a line over a proper interval of both sequences is checked as the global alignment of that interval
    pair instead of being reported not_end_to_end.  Returns dict(lines, checked, skipped, kernel_ms, failures): one dict(line, qname, tname, strand, class, column,
    penalty, optimum) per failing line, in line order; `class` as listed there; optimum is None unless `optimal` found one."""
    cids, data, offs = _seq_args(ids, seqs)
    txt = paf_text.encode() if isinstance(paf_text, str) else bytes(paf_text)
    out = C.c_void_p()
    n = C.c_size_t(0)
    counts = (C.c_uint64 * 4)()
    st = ffi.VerifyStats()
    e = _err()
    rc = load().awh_check_paf(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), scores.encode(), txt,
                              C.c_size_t(len(txt)), int(bool(optimal)), int(bool(partial)), int(device), C.byref(out), C.byref(n), counts, C.byref(st), e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    lines = C.string_at(out, n.value).decode().splitlines()
    load().awh_free(out)
    fails = []
    for ln in lines:
        f = ln.split("\t")
        fails.append({"line": int(f[0]), "qname": f[1], "tname": f[2], "strand": f[3], "class": f[4], "column": int(f[5]),
                      "penalty": int(f[6]), "optimum": int(f[7]) if len(f) > 7 else None})
    return dict(lines=int(counts[0]), checked=int(counts[1]), skipped=int(counts[2]), kernel_ms=float(st.kernel_ms), failures=fails)


def align_ranges(ids, seqs, ranges, scores, devices=None, device=0, verify=False, max_penalty=None, max_divergence=None, clip=None,
                 clip_min_score=None, split=None, split_min_score=None, normalize=None, device_cigar=False, cs=None, coverage=None, variants=False, liftover=None, liftover_from=None, msa_targets=None, msa_max_bytes=None):
    """allwave::align_ranges + alignment_to_paf: the interval pairs `ranges` -- rows (query_idx, target_idx, is_reverse,
    query_start, query_end, target_start, target_end), the query interval on its forward strand -- aligned globally on the
    engines `devices` names (default: [device]).  Returns the PAF lines in list order: columns 3-4 and 8-9 are the interval,
    2 and 7 the full lengths; a failed range prints its starts twice and an empty cg.  verify=True: every range is checked on
    the device; last_verify() then holds the counters and the failures (index = list index).  max_penalty / max_divergence: as
    for all_pairs_paf (the divergence bound's penalty bound comes from the rectangle's lengths); a range above a bound gives
    no line.  device_cigar: as for all_pairs_paf -- the same lines (in list order on one slot, in batch order on several).
    cs, coverage: as for all_pairs_paf."""
    cids, data, offs = _seq_args(ids, seqs)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 7))
    devs, nd = _device_args([device] if devices is None else devices)
    out = C.c_void_p()
    n = C.c_size_t(0)
    e = _err()
    rbuf = r if len(r) else np.zeros((1, 7), dtype=np.int64)
    _set_run_options(max_penalty, max_divergence, clip, clip_min_score, split, split_min_score, normalize, device_cigar, cs, coverage, variants, liftover, liftover_from, ids, msa_targets, msa_max_bytes)
    rc = load().awh_align_ranges_paf(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), scores.encode(),
                                     rbuf.ctypes.data_as(C.c_void_p), C.c_size_t(len(r)), devs, nd, int(bool(verify)), C.byref(out),
                                     C.byref(n), e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    lines = C.string_at(out, n.value).decode().splitlines()
    load().awh_free(out)
    return lines


def range_record_paf(qid, qlen, tid, tlen, rng, record, ops=b""):
    """The PAF line of one range's engine record (range_alignment_result + alignment_to_paf; needs no device).  rng: (0, 1,
    is_reverse, query_start, query_end, target_start, target_end); record: one ffi.RESULT_DTYPE record whose op bytes are `ops`."""
    rec = np.zeros(1, dtype=ffi.RESULT_DTYPE)
    rec[0] = record
    rec["cigar_off"], rec["cigar_len"] = 0, len(ops)
    r = np.ascontiguousarray(rng, dtype=np.int64)
    arena = bytes(ops) + b"\0"
    buf = C.create_string_buffer(4 * len(ops) + 512)
    n = load().awh_range_record_paf(qid.encode(), C.c_size_t(qlen), tid.encode(), C.c_size_t(tlen), r.ctypes.data_as(C.c_void_p),
                                    rec.ctypes.data_as(C.c_void_p), arena, buf, C.c_size_t(len(buf)))
    if n < 0:
        raise HostError("buffer")
    return buf.value.decode()


PAF_RANGE_CLASSES = ("", "bad_line", "unknown_name", "length_mismatch")


def parse_paf_ranges(ids, lengths, paf_text):
    """parse_paf_ranges (what --align-paf reads of a mapping file: columns 1-9): one (line, class, range) per non-empty line;
    class "" and the range's seven fields for a good line, else one of PAF_RANGE_CLASSES and None.  Needs no device."""
    txt = paf_text.encode() if isinstance(paf_text, str) else bytes(paf_text)
    cids = (C.c_char_p * len(ids))(*[i.encode() for i in ids])
    lens = np.ascontiguousarray(lengths, dtype=np.int64)
    out = C.c_void_p()
    n = C.c_size_t(0)
    if load().awh_parse_paf_ranges(len(ids), cids, lens.ctypes.data_as(C.c_void_p), txt, C.c_size_t(len(txt)), C.byref(out), C.byref(n)) != 0:
        raise HostError("out of memory")
    k = n.value
    raw = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int64)), shape=(max(k, 1) * 9,))[:9 * k].reshape(k, 9).copy()
    load().awh_free(out)
    return [(int(r[0]), PAF_RANGE_CLASSES[int(r[1])], tuple(int(v) for v in r[2:]) if r[1] == 0 else None) for r in raw]


def _orient_code(orientation, orientation_full):
    """the hooks' orientation argument: 3 = WFA orientation by two full alignments per pair (with_full_wfa_orientation)"""
    if orientation_full and orientation != "wfa":
        raise ValueError("orientation_full needs orientation='wfa'")
    return 3 if orientation_full else ORIENT[orientation]


def _seq_args(ids, seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    data = np.frombuffer(b"".join(bytes(s) for s in seqs) + b"\0", dtype=np.uint8)
    cids = (C.c_char_p * len(ids))(*[i.encode() for i in ids])
    return cids, data, offs


def _device_args(devices):
    """(int32 array, count) of a device list for the *_devices hooks (AllPairIterator::with_devices)."""
    devs = [int(d) for d in devices]
    if not devs:
        raise ValueError("devices: the device list is empty")
    return (C.c_int32 * len(devs))(*devs), len(devs)


def all_pairs_paf(ids, seqs, scores, orientation="wfa", exclude_self=True, device=0, sparsification="none", devices=None,
                  min_batch_pairs=0, orientation_full=False, verify=False, max_penalty=None, max_divergence=None, clip=None,
                  clip_min_score=None, split=None, split_min_score=None, normalize=None, device_cigar=False, cs=None, coverage=None, variants=False, liftover=None, liftover_from=None, msa_targets=None, msa_max_bytes=None):
    """AllPairIterator + alignment_to_paf per record; returns the list of PAF lines.  `devices`: a list of ordinals (one
    engine per entry, repeats allowed) to spread the pair list over in this call; None = [device].
    `min_batch_pairs` > 0 overrides the smallest batch of a multi-device run (default 16,384).  orientation_full: WFA
    orientation by two full alignments for every pair (the reference's method; the same strands) instead of bounded scores.
    verify: every alignment is checked on the device (with_verify); the lines are the same, last_verify() tells the outcome.
    max_penalty (an int >= 0) / max_divergence (0 <= d < 1): bounds on the final alignments (with_max_penalty /
    with_max_divergence) -- a pair whose penalty exceeds max_penalty, or whose alignment has (#X + #I + #D) > d * columns,
    is abandoned early where that can be proved and gives no line; the other lines are the unbounded call's; last_bounds()
    counts what was left out.
    clip (a match bonus, 1 .. 32767) / clip_min_score (default 1): every alignment is clipped to its best-scoring segment on
    the device (with_clip): each line is replaced by its segment's -- coordinates shifted by the bases skipped (a '-' line's
    query coordinates on the query's forward strand), columns 10 and 11, gi:f: and cg:Z: the segment's -- or dropped when the
    clip is empty or scores below clip_min_score; last_clip() counts what was left out.
    split (a match bonus) / split_min_score (required with it): every alignment is split into all its maximal segments that
    score at least split_min_score (with_split): each line is replaced by its segments' lines, in column order, or dropped;
    last_split() counts them.  Not together with clip.  iterate, all_pairs_paf_count and align_ranges take the same two.
    normalize ("left" / "right"): every alignment's gap runs are moved to their left- / right-normal place on the device
    (with_normalize) before the check, the clip and the split; only cg:Z: changes; last_normalize() tells what moved.
    iterate, all_pairs_paf_count and align_ranges take it too.
    device_cigar: the run-length text behind cg:Z: is made on the device (with_device_cigar) and the lines are formatted a
    batch at a time from it (for_each_paf_batch) instead of record by record from the op bytes: the same lines, byte for byte;
    last_encode() tells what was encoded.  Not together with split.  all_pairs_paf_count and align_ranges take it too;
    iterate accepts and ignores it (its consumers hand out op bytes).
    cs ("short" / "long"): every line gains minimap2's cs difference string, "\tcs:Z:<text>" after the cg:Z: field, made on the
    device (with_cs) from the op string -- normalized, and clipped, when those are set -- and the resident sequences; the line
    up to the tag is the line without it; last_cs() tells what was written.  Not together with split.
    coverage ("target" / "query" / "both"): the run also accumulates, on the device, the per-base depth of what it aligned
    (with_coverage: per base of every sequence, in how many alignments it is aligned and in how many it matches); the lines are
    those of the run without it, and last_coverage() returns the two tracks.  variants=True: the run also tallies, on the device, the
    per-site allele table of what it aligned (with_variants; last_variants() returns it).  liftover= ((seq, beg, end) rows, seq an
    index or an id, forward strand) with liftover_from= ("target", the default, "query" or "both"): the run also lifts those regions,
    on the device, through what it aligned (with_liftover; last_liftover() returns the rows).  msa_targets= ("all", or a list of
    indices or ids) with msa_max_bytes= (default 2^30): the run also lays every sequence out against each target as a multiple
    alignment, on the device, after the run (with_msa; last_msa() returns {target: (names, block)}); not with device_cigar.  iterate and align_ranges take them too.  all_pairs_paf_count and
    align_ranges take it too; iterate accepts and ignores it."""
    cids, data, offs = _seq_args(ids, seqs)
    devs, nd = _device_args([device] if devices is None else devices)
    out = C.c_void_p()
    n = C.c_size_t(0)
    e = _err()
    _set_run_options(max_penalty, max_divergence, clip, clip_min_score, split, split_min_score, normalize, device_cigar, cs, coverage, variants, liftover, liftover_from, ids, msa_targets, msa_max_bytes)
    rc = load().awh_all_pairs_paf_devices(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                          scores.encode(), sparsification.encode(), _orient_code(orientation, orientation_full), int(exclude_self),
                                          devs, nd, C.c_int64(int(min_batch_pairs)), int(bool(verify)), None, C.byref(out), C.byref(n), e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    txt = C.string_at(out, n.value).decode()
    load().awh_free(out)
    return txt.splitlines()


ITER_MODES = {"for_each": 0, "next": 1, "par_for_each": 2, "par_collect": 3, "process_alignments": 4}


def iterate(ids, seqs, scores, mode="for_each", sparsification="none", orientation="forward", threads=4, chunk=0,
            resparsify=False, fail_at=-1, device=0, devices=None, min_batch_pairs=0, shard=None, with_stats=False,
            orientation_full=False, verify=False, max_penalty=None, max_divergence=None, clip=None, clip_min_score=None, split=None,
            split_min_score=None, normalize=None, device_cigar=False, cs=None, coverage=None, variants=False, liftover=None, liftover_from=None, msa_targets=None, msa_max_bytes=None):
    """Every consumer of the pair list (iterator.rs:101-253, lib.rs:57-68) through one hook; returns the PAF lines in arrival
    order.  `fail_at` >= 0 makes the callback throw at that record: HostError carries its message.
    `devices`: a list of ordinals (one engine per entry, repeats allowed) to spread the pair list over; None = [device].
    `min_batch_pairs` > 0 overrides the smallest batch of a multi-device run, `shard` = (rank, world) keeps that shard of
    the list (with_shard; not "process_alignments").  with_stats: returns (lines, [ffi.Stats per slot]) --
    last_slot_stats(); all zeros for "process_alignments" without min_batch_pairs.  A HostError carries `.records`: how
    many records arrived before the error, and `.late_calls`: how many callback calls followed the first failure (with
    fail_at, each of those fails with a message of its own: "callback failed again, ...").  orientation_full: WFA
    orientation by two full alignments for every pair instead of bounded scores (the same strands).  verify: with_verify on the
    iterator, whichever consumer `mode` names; last_verify() tells the outcome.  max_penalty / max_divergence: as for
    all_pairs_paf -- no consumer is handed a pair above a bound.  device_cigar, cs: accepted and ignored -- every consumer here
    hands out alignment records with their op bytes."""
    cids, data, offs = _seq_args(ids, seqs)
    devs, nd = _device_args([device] if devices is None else devices)
    _set_run_options(max_penalty, max_divergence, clip, clip_min_score, split, split_min_score, normalize, device_cigar, cs, coverage, variants, liftover, liftover_from, ids, msa_targets, msa_max_bytes)
    st = (ffi.Stats * nd)()
    rank, world = shard if shard is not None else (0, 1)
    out = C.c_void_p()
    n, nrec, late = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    e = _err()
    rc = load().awh_iterate_devices(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), scores.encode(),
                                    sparsification.encode(), _orient_code(orientation, orientation_full), ITER_MODES[mode], int(threads), int(chunk),
                                    int(bool(resparsify)), C.c_long(int(fail_at)), devs, nd, C.c_int64(int(min_batch_pairs)),
                                    C.c_int64(int(rank)), C.c_int64(int(world)), int(bool(verify)), st, C.byref(out), C.byref(n), C.byref(nrec),
                                    C.byref(late), e, _CAP)
    if rc != 0:
        err = HostError(e.value.decode())
        err.records = nrec.value
        err.late_calls = late.value
        raise err
    txt = C.string_at(out, n.value).decode()
    load().awh_free(out)
    if with_stats:
        return txt.splitlines(), list(st)
    return txt.splitlines()


def all_pairs_paf_count(ids, seqs, scores, orientation="forward", device=0, format_threads=8, devices=None, min_batch_pairs=0,
                        sparsification=None, checksum=False, verify=False, max_penalty=None, max_divergence=None, clip=None,
                        clip_min_score=None, split=None, split_min_score=None, normalize=None, device_cigar=False, cs=None, coverage=None, variants=False, liftover=None, liftover_from=None, msa_targets=None, msa_max_bytes=None):
    """End to end: upload -> align -> D2H -> format into a counting sink. Returns (bytes, lines, secs, ffi.Stats) for
    every pair on `device`.  `devices`: a list of ordinals (one engine per entry, repeats allowed); the Stats are then
    summed over the slots, and the result gains a fifth element, each slot's Stats (last_slot_stats()), and a sixth, the
    sum of the lines' FNV-1a hashes when `checksum` (order-independent; else None).  With devices, `sparsification` plans
    the pair list (default: every pair).  verify: with_verify on the iterator; last_verify() tells the outcome.
    max_penalty / max_divergence: as for all_pairs_paf (the lines counted are the kept pairs').  device_cigar: as for
    all_pairs_paf; the Stats' d2h_ms then covers the text copy in the op bytes' place.  cs: as for all_pairs_paf; d2h_ms covers
    the cs text's copy too."""
    one = devices is None
    cids, data, offs = _seq_args(ids, seqs)
    devs, nd = _device_args([device] if one else devices)
    _set_run_options(max_penalty, max_divergence, clip, clip_min_score, split, split_min_score, normalize, device_cigar, cs, coverage, variants, liftover, liftover_from, ids, msa_targets, msa_max_bytes)
    nb, nl, secs, ck = C.c_uint64(0), C.c_uint64(0), C.c_double(0), C.c_uint64(0)
    st = ffi.Stats()
    slot = (ffi.Stats * nd)()
    e = _err()
    rc = load().awh_all_pairs_paf_count_devices(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                                scores.encode(), ORIENT[orientation],
                                                sparsification.encode() if sparsification and not one else None,
                                                devs, nd, C.c_int64(int(min_batch_pairs)), format_threads, int(bool(verify)), C.byref(nb), C.byref(nl),
                                                C.byref(ck) if checksum else None, C.byref(secs), C.byref(st), slot, e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    if one:
        return nb.value, nl.value, secs.value, st
    return nb.value, nl.value, secs.value, st, list(slot), (ck.value if checksum else None)


PAIR_SCORE_DTYPE = np.dtype([("query_idx", "<i8"), ("target_idx", "<i8"), ("is_reverse", "<i8"), ("penalty", "<i8"),
                             ("status", "<i8")])


def all_pairs_scores(ids, seqs, scores, orientation="mash", sparsification="none", devices=None, max_penalty=None, shard=None,
                     with_stats=False, orientation_full=False):
    """Score-only all-vs-all (AllPairIterator::scores): the optimal penalty of every planned pair without a CIGAR, in
    pair-list order, as a PAIR_SCORE_DTYPE array (query_idx, target_idx, is_reverse, penalty, status -- ffi.AWV_ST_*).
    The pair list is AllPairIterator::with_options(..., exclude_self=True, mash orientation, sparsification)'s; the strand of
    each pair comes from `orientation` ("mash", "wfa": bounded strand scores, two full alignments only for the pairs those
    leave open -- or for every pair with orientation_full -- or "forward").  `devices`: a list of
    ordinals (one engine per entry, repeats allowed; None = device 0), `shard` = (rank, world) keeps that shard of the list.
    max_penalty: None = no bound; else pairs proved above it come back AWV_ST_ABOVE_BOUND with penalty max_penalty + 1.
    with_stats: returns (array, ffi.Stats) -- last_stats(), summed over the slots."""
    if max_penalty is not None and int(max_penalty) < 0:
        raise ValueError("max_penalty must be >= 0 (None: no bound)")
    cids, data, offs = _seq_args(ids, seqs)
    devs, nd = _device_args([0] if devices is None else devices)
    rank, world = shard if shard is not None else (0, 1)
    out = C.c_void_p()
    n = C.c_size_t(0)
    st = ffi.Stats()
    e = _err()
    rc = load().awh_all_pairs_scores(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), scores.encode(),
                                     sparsification.encode(), _orient_code(orientation, orientation_full), devs, nd, C.c_int64(int(rank)), C.c_int64(int(world)),
                                     C.c_int64(-1 if max_penalty is None else int(max_penalty)), C.byref(out), C.byref(n),
                                     C.byref(st), e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    k = n.value
    raw = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int64)), shape=(max(k, 1) * 5,))[:5 * k].copy()
    load().awh_free(out)
    res = raw.view(PAIR_SCORE_DTYPE)
    return (res, st) if with_stats else res


def align_sequences(pattern, text, penalties, mode, device=0):
    """wfa.rs:178-258. penalties = (mismatch, o1, e1, o2, e2); mode in {"edit","affine","affine2p"}.
    Returns dict(score, cigar, matches, mismatches, insertions, deletions, alignment_length)."""
    pattern, text = bytes(pattern), bytes(text)
    pen = (C.c_int32 * 5)(*penalties)
    score = C.c_int32(0)
    cig = C.create_string_buffer(4 * (len(pattern) + len(text)) + 16)
    counts = (C.c_uint64 * 5)()
    e = _err()
    rc = load().awh_align_sequences(pattern, C.c_size_t(len(pattern)), text, C.c_size_t(len(text)), pen,
                                    {"edit": 0, "affine": 1, "affine2p": 2}[mode], device, C.byref(score), cig,
                                    C.c_size_t(len(cig)), counts, e, _CAP)
    if rc != 0:
        raise HostError(e.value.decode())
    return dict(score=score.value, cigar=cig.value.decode(), matches=counts[0], mismatches=counts[1],
                insertions=counts[2], deletions=counts[3], alignment_length=counts[4])


# ---- planner (host-only, no GPU) ---------------------------------------------------------------
def siphash(data, k0=0, k1=0, c=1, d=3):
    L = load()
    L.awh_siphash.restype = C.c_uint64
    data = bytes(data)
    return L.awh_siphash(data, C.c_size_t(len(data)), C.c_uint64(k0), C.c_uint64(k1), c, d)


def hash_bytes(data):
    """Rust: DefaultHasher over a `[u8]` (length prefix + bytes), as hash_kmer does."""
    L = load()
    L.awh_hash_bytes.restype = C.c_uint64
    data = bytes(data)
    return L.awh_hash_bytes(data, C.c_size_t(len(data)))


def hash_str(s):
    """Rust: DefaultHasher over a `str` (bytes + 0xFF), as the pair sparsifier does."""
    L = load()
    L.awh_hash_str.restype = C.c_uint64
    return L.awh_hash_str(s.encode())


def connectivity_probability(n, x):
    L = load()
    L.awh_connectivity_probability.restype = C.c_double
    return L.awh_connectivity_probability(C.c_size_t(n), C.c_double(x))


def _pairs_out(out, n):
    a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int64)), shape=(max(n, 1) * 2,))[:2 * n].reshape(n, 2).copy()
    load().awh_free(out)
    return [tuple(int(v) for v in r) for r in a]


def plan_pairs(ids, seqs, sparsification, exclude_self=True, resparsify=False, device=None):
    """Pair list AllPairIterator::with_options would align (iterator.rs:30-92); resparsify: planned with `-p none` first and
    then through with_sparsification (iterator.rs:101-110).  device: a HIP ordinal to plan on (the same list; HostError
    without that device), None: the host planner."""
    cids, data, offs = _seq_args(ids, seqs)
    out = C.c_void_p()
    n = C.c_size_t(0)
    e = _err()
    flags = int(bool(exclude_self)) | (2 if resparsify else 0)
    if device is None:
        rc = load().awh_plan_pairs(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                   sparsification.encode(), flags, C.byref(out), C.byref(n), e, _CAP)
        if rc != 0:
            raise ValueError(e.value.decode())
    else:
        rc = load().awh_plan_pairs_gpu(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                       sparsification.encode(), flags, int(device), C.byref(out), C.byref(n), e, _CAP)
        if rc != 0:
            raise (ValueError if rc == -1 else HostError)(e.value.decode())
    return _pairs_out(out, n.value)


def shard_assignment(pairs, lens, scores, world):
    """Shard of every pair under the cost-balanced (LPT) partition AllPairIterator::with_shard uses
    (planner::assign_shards_lpt) and the predicted per-pair costs.  pairs: int array [n, 2]; lens:
    sequence lengths; scores: "m,x,o,e[,o2,e2]"."""
    p = np.ascontiguousarray(np.asarray(pairs)[:, :2], dtype=np.int64)
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    shard = np.zeros(len(p), dtype=np.uint32)
    cost = np.zeros(len(p), dtype=np.float64)
    e = _err()
    rc = load().awh_shard_pairs(p.ctypes.data_as(C.c_void_p), C.c_size_t(len(p)), ln.ctypes.data_as(C.c_void_p), C.c_size_t(len(ln)), scores.encode(),
                                C.c_size_t(int(world)), shard.ctypes.data_as(C.c_void_p), cost.ctypes.data_as(C.c_void_p), e, _CAP)
    if rc != 0:
        raise ValueError(e.value.decode())
    return shard, cost


def device_batches(cost, slots, min_batch_pairs=16384):
    """Batches of a multi-device run (planner::device_batches): B = min(4 * slots, ceil(n / min_batch_pairs)), at least 1,
    cut by the LPT partition of the predicted costs `cost` (float array, one per pair; shard_assignment returns them).
    Returns a list of B lists of pair indices, each in list order."""
    c = np.ascontiguousarray(cost, dtype=np.float64)
    out = np.zeros(len(c), dtype=np.uint32)
    nb = C.c_size_t(0)
    e = _err()
    if load().awh_device_batches(c.ctypes.data_as(C.c_void_p), C.c_size_t(len(c)), C.c_size_t(int(slots)), C.c_size_t(int(min_batch_pairs)),
                                 out.ctypes.data_as(C.c_void_p), C.byref(nb), e, _CAP) != 0:
        raise HostError(e.value.decode())
    batches = [[] for _ in range(nb.value)]
    for i, b in enumerate(out.tolist()):
        batches[b].append(i)
    return batches


def knn_graph(dist, k, farthest=False):
    d = np.ascontiguousarray(dist, dtype=np.float64)
    out = C.c_void_p()
    n = C.c_size_t(0)
    load().awh_knn_graph(d.ctypes.data_as(C.c_void_p), len(d), int(k), int(farthest), C.byref(out), C.byref(n))
    return _pairs_out(out, n.value)


def mash_matrix(ids, seqs, k=15, device=None):
    """Mash distance matrix (mash.rs:135-166, sketch size 1,000); device: a HIP ordinal to sketch and intersect on (the same
    doubles, bit for bit; HostError without that device), None: the host planner."""
    cids, data, offs = _seq_args(ids, seqs)
    out = np.zeros((len(ids), len(ids)), dtype=np.float64)
    if device is None:
        load().awh_mash_matrix(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), int(k),
                               out.ctypes.data_as(C.c_void_p))
        return out
    e = _err()
    if load().awh_mash_matrix_gpu(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), int(k), int(device),
                                  out.ctypes.data_as(C.c_void_p), e, _CAP) != 0:
        raise HostError(e.value.decode())
    return out


def orient_mash(ids, seqs, pairs, device=None):
    """Mash orientation of every pair (alignment.rs:69-94): True = reverse.  device: a HIP ordinal (HostError without it)."""
    cids, data, offs = _seq_args(ids, seqs)
    p = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(max(len(p), 1), dtype=np.uint8)
    if device is None:
        load().awh_orient_mash(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                               p.ctypes.data_as(C.c_void_p), C.c_size_t(len(p)), out.ctypes.data_as(C.c_void_p))
    else:
        e = _err()
        if load().awh_orient_mash_gpu(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                      p.ctypes.data_as(C.c_void_p), C.c_size_t(len(p)), int(device), out.ctypes.data_as(C.c_void_p),
                                      e, _CAP) != 0:
            raise HostError(e.value.decode())
    return [bool(x) for x in out[:len(p)]]


def orient_wfa(ids, seqs, pairs, scores="0,1,1,1", full=False, device=0):
    """WFA orientation of every pair (alignment.rs:157-175) under the orientation penalties `scores` on `device`: True =
    reverse.  Decided from bounded strand scores where those prove which strand has fewer edits, from two full alignments
    where they do not; full=True: two full alignments for every pair (the same answers)."""
    p = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    eng = ffi.Engine(device=int(device))
    try:
        eng.set_sequences([s if isinstance(s, (bytes, bytearray)) else str(s).encode() for s in seqs])
        r = eng.orient_pairs(parse_scores(scores), p.astype(np.int32), full=full)
    except ffi.EngineError as err:
        raise HostError(str(err))
    finally:
        eng.close()
    return [bool(x) for x in r["is_reverse"]]


SKETCH_KINDS = {"canonical": 0, "forward": 1, "revcomp": 2}


def sketch(ids, seqs, k, s, kind="canonical", device=None):
    """Sketch of every sequence as a list of sorted hash lists: kind "canonical" (mash.rs:78-107), "forward" (stranded,
    alignment.rs:96-122) or "revcomp" (stranded, of reverse_complement(seq)).  device: a HIP ordinal (the engine's
    awv_sketch; HostError without it), None: the host code."""
    cids, data, offs = _seq_args(ids, seqs)
    po, ph = C.c_void_p(), C.c_void_p()
    e = _err()
    L = load()
    if L.awh_sketch(len(ids), cids, data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), int(k), int(s), SKETCH_KINDS[kind],
                    -1 if device is None else int(device), C.byref(po), C.byref(ph), e, _CAP) != 0:
        raise HostError(e.value.decode())
    n = len(ids)
    o = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    h = np.ctypeslib.as_array(C.cast(ph, C.POINTER(C.c_uint64)), shape=(int(o[n]) + 1,))[:int(o[n])].copy()
    L.awh_free(po)
    L.awh_free(ph)
    return [h[o[i]:o[i + 1]].tolist() for i in range(n)]


def keep_threshold(fraction):
    """(threshold, keep_all) of the hashed keep test: keep_pair's `h / u64::MAX < fraction` holds iff keep_all or h < threshold."""
    L = load()
    L.awh_keep_threshold.restype = C.c_uint64
    L.awh_keep_threshold.argtypes = [C.c_double, C.POINTER(C.c_int)]
    a = C.c_int(0)
    t = L.awh_keep_threshold(float(fraction), C.byref(a))
    return int(t), bool(a.value)
