"""GPU tests of what a persistent wave carries from one record to the next in the five newer record passes:
normalize.hip, encode.hip, cs.hip, coverage.hip and variants.hip.  Every list of tests/reuse_cases.py -- the scan lists and the
pass lists, whose record k + 1 is a trap for the state record k leaves (tests/test_reuse_cpu.py shows that a leaked carry changes
the answer) -- goes through each pass's own entry point with workgroups = 1, 2 and 0 and with one wave over several pieces of
the arena, every field and every byte against the *_one_host yardsticks; what equals the yardstick's on all four engines is
identical between them.  Each record is the pair (2 k, 2 k + 1) of its own sequences: a wrong slot names its record."""
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import coverage_cases as CV
import reuse_cases as RC
import split_cases as S
from test_gpu_reuse import engines, same_bytes, scan_engines  # noqa: F401  (engines: the module's fixture)
from util import DEFAULT_2P

pytestmark = pytest.mark.gpu

MODES = ("short", "long")
DIRECTIONS = ("left", "right")
TAIL = b"\x5a" * 9  # behind the last string of a normalize call's arena: comes back as it was
_WANT = {}


def want(key, make):
    """A reference, computed once and never changed."""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def inputs(name):
    """(sequences, pairs, RESULT_DTYPE records, arena) of a list: record k is the pair (2 k, 2 k + 1), the strings back to back."""
    return want(("inputs", name), lambda: RC.verify_inputs(RC.all_lists()[name], DEFAULT_2P))


def columns_of(recs):
    return sum(len(r.ops) for r in recs if r.status == 0)


def failed_of(codes):
    return int(((codes == 2) | (codes == 3)).sum())  # BAD_OP and LENGTHS, in every pass's codes


def same_texts(got, out, text, recs, where):
    """A text arena byte for byte; a difference is reported with the record it falls in and the one before it."""
    got = bytes(got)
    if got == text:
        return
    for i in range(len(recs)):
        lo, hi = int(out[i]["off"]), int(out[i]["off"]) + int(out[i]["len"])
        if got[lo:hi] != text[lo:hi]:
            at = next(j for j in range(lo, hi) if got[j:j + 1] != text[j:j + 1])
            assert False, (where, "the text of record %d of %d differs" % (i, len(recs)), recs[i].kind, len(recs[i].ops), "behind", recs[i - 1].kind if i else None,
                           got[at:at + 24], text[at:at + 24])
    assert False, (where, "the text arenas differ in size", len(got), len(text))


def same_rows(ffi, got, events, recs, where):
    """The events of a list record by record."""
    at = 0
    for i, ev in enumerate(events):
        if got[at:at + len(ev)].tobytes() != ev.tobytes():
            assert False, (where, "the events of record %d of %d differ" % (i, len(recs)), recs[i].kind, len(recs[i].ops), "behind", recs[i - 1].kind if i else None,
                           got[at:at + len(ev)][:2], ev[:2])
        at += len(ev)
    assert at == len(got), (where, at, len(got))


def same_tracks(got, wanted, recs, where, seqs=None):
    """(aligned, matched) of all sequences in set order; sequences 2 k and 2 k + 1 are record k's (seqs: the resident set, where
    it is not the records' own pattern and text).  A difference is reported with the record whose sequence it falls in."""
    lens = [len(s) for s in seqs] if seqs is not None else [len(s) for r in recs for s in (r.pattern, r.text)]
    ends = np.cumsum(lens)
    for track, g, w in zip(("aligned", "matched"), got, wanted):
        assert len(g) == len(w) == int(ends[-1]), (where, "the %s track has %d entries, not %d" % (track, len(g), len(w)))
        if np.array_equal(g, w):
            continue
        at = int(np.flatnonzero(g != w)[0])
        i = int(np.searchsorted(ends, at, side="right")) // 2
        assert False, (where, "the %s track differs at entry %d: record %d of %d" % (track, at, i, len(recs)), recs[i].kind, len(recs[i].ops),
                       "behind", recs[i - 1].kind if i else None, int(g[at]), int(w[at]))


def same_arena(got, wanted, recs, where):
    got = bytes(got)
    if got == wanted:
        return
    offs = RC.offsets_of(recs) + [sum(len(r.ops) for r in recs)]
    for i in range(len(recs)):
        if got[offs[i]:offs[i + 1]] != wanted[offs[i]:offs[i + 1]]:
            assert False, (where, "the string of record %d of %d differs" % (i, len(recs)), recs[i].kind, len(recs[i].ops), "behind", recs[i - 1].kind if i else None)
    assert False, (where, "the bytes behind the last string differ", got[offs[-1]:], wanted[offs[-1]:])


# ---- one call per pass, on one engine, against its reference ---------------------------------------------------------------------

def check_encode(ffi, e, recs, claimed, arena, ref, where):
    wout, wtext = ref
    text, tout, nbytes = e.encode_cigars(claimed, arena)
    same_bytes(tout, wout, recs, where)
    assert nbytes == len(wtext), where
    same_texts(text, wout, wtext, recs, where)
    st = e.encode_stats()
    assert (st.pairs, st.columns, st.runs, st.text_bytes) == (len(recs), columns_of(recs), int(wout["runs"].sum()), len(wtext)), (where, st.pairs, st.columns, st.runs)


def check_cs(ffi, e, mode, call, recs, claimed, arena, ref, where):
    wout, wtext = ref
    text, csout, nbytes = call(mode, claimed, arena)
    same_bytes(csout, wout, recs, where)
    assert nbytes == len(wtext), where
    same_texts(text, wout, wtext, recs, where)
    st = e.cs_stats()
    assert (st.pairs, st.failed, st.text_bytes) == (len(recs), failed_of(wout["code"]), len(wtext)), (where, st.pairs, st.failed)
    assert st.columns == columns_of(recs), (where, st.columns)


def check_coverage(ffi, e, roles, call, recs, claimed, arena, ref, where, seqs=None):
    witems, waligned, wmatched = ref
    e.coverage_begin(CV.ROLE_NAMES[roles])
    items = call(claimed, arena)
    same_bytes(items, witems, recs, where)
    _, aligned, matched = e.coverage_read()
    same_tracks((aligned, matched), (waligned, wmatched), recs, where, seqs)
    st = e.coverage_stats()
    assert (st.items, st.failed, st.columns) == (len(recs), failed_of(witems["code"]), columns_of(recs)), (where, st.items, st.failed, st.columns)
    assert st.boundaries == int(witems["boundaries"].sum()) * bin(roles).count("1"), where


def check_variants(ffi, e, call, recs, claimed, arena, ref, where):
    witems, events = ref
    b = e.variants_stats()
    before = (b.items, b.failed, b.columns, b.snv, b.ins, b.del_)
    items, rows = call(claimed, arena)
    same_bytes(items, witems, recs, where)
    same_rows(ffi, rows, events, recs, where)
    a = e.variants_stats()
    delta = tuple(x - y for x, y in zip((a.items, a.failed, a.columns, a.snv, a.ins, a.del_), before))
    assert delta == (len(recs), failed_of(witems["code"]), columns_of(recs)) + tuple(int(witems[f].sum()) for f in ("snv", "ins", "del")), (where, delta)


def check_normalize(ffi, e, direction, call, recs, claimed, arena, ref, where):
    warena, wres = ref
    got, nres = call(direction, claimed, arena + TAIL)
    same_bytes(nres, wres, recs, where)
    same_arena(got, warena, recs, where)
    ok = wres["code"] == 0
    st = e.normalize_stats()
    assert (st.pairs, st.columns) == (len(recs), columns_of(recs)), (where, st.pairs, st.columns)
    assert st.records_moved == int((ok & (wres["runs_moved"] > 0)).sum()) and st.runs_moved == int(wres["runs_moved"][ok].sum()), where
    assert st.columns_moved == int(wres["columns_moved"][ok].sum()), where
    assert st.runs == sum(len(re.findall(rb"I+|D+", r.ops)) for r, good in zip(recs, ok) if good and r.status == 0), (where, st.runs)


# ---- the lists through the five entry points ----------------------------------------------------------------------------------------

def test_encode_waves_take_record_after_record(engines):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, claimed, arena = inputs(name)
        ref = want(("encode", name), lambda: RC.encode_want(ffi, recs))
        for ename, e in scan_engines(engines):
            check_encode(ffi, e, recs, claimed, arena, ref, (name, ename))


@pytest.mark.parametrize("mode", MODES)
def test_cs_waves_take_record_after_record(engines, mode):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, claimed, arena = inputs(name)
        ref = want(("cs", name, mode), lambda: RC.cs_want(ffi, mode, recs))
        if name != "zero":
            assert 2 * int((ref[0]["code"] == 0).sum()) > len(recs), name
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            check_cs(ffi, e, mode, lambda m, c, a: e.cs_cigars(m, pairs, c, a), recs, claimed, arena, ref, (name, ename, mode))


@pytest.mark.parametrize("roles", CV.ROLES, ids=[CV.ROLE_NAMES[r] for r in CV.ROLES])
def test_coverage_waves_take_record_after_record(engines, roles):
    """An unsound record's sequences read back all zero: the reference holds them so."""
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, claimed, arena = inputs(name)
        ref = want(("coverage", name, roles), lambda: RC.coverage_want(ffi, roles, recs, seqs))
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            check_coverage(ffi, e, roles, lambda c, a: e.coverage_cigars(pairs, c, a), recs, claimed, arena, ref, (name, ename, roles))


def test_variants_waves_take_record_after_record(engines):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, claimed, arena = inputs(name)
        ref = want(("variants", name), lambda: RC.variants_want(ffi, recs, seqs))
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            check_variants(ffi, e, lambda c, a: e.variants_cigars(pairs, c, a), recs, claimed, arena, ref, (name, ename))


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_normalize_waves_take_record_after_record(engines, direction):
    """The result records and the whole arena that comes back, the bytes behind the last string among them."""
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs, pairs, claimed, arena = inputs(name)
        ref = want(("normalize", name, direction), lambda: RC.normalize_want(ffi, direction, recs, TAIL))
        for ename, e in scan_engines(engines):
            e.set_sequences(seqs)
            check_normalize(ffi, e, direction, lambda d, c, a: e.normalize_cigars(d, pairs, c, a), recs, claimed, arena, ref, (name, ename, direction))


def test_range_records_then_whole_forward_sequences(engines):
    """cs, coverage, variants and normalize on intervals that begin off the dword grid, on both strands, alternating with forward
    records on whole sequences (reuse_cases.verify_ranges_list)."""
    from allwave_amd import ffi
    recs, begs = RC.verify_ranges_list()
    seqs, ranges, claimed, arena = RC.verify_range_inputs(recs, begs, DEFAULT_2P, random.Random("reuse/ranges"))
    geometry = RC.range_geometry(seqs, ranges)
    cs = {mode: RC.cs_want(ffi, mode, recs) for mode in MODES}
    cov = RC.coverage_want(ffi, CV.BOTH, recs, seqs, geometry)
    var = RC.variants_want(ffi, recs, seqs, geometry)
    norm = {d: RC.normalize_want(ffi, d, recs, TAIL) for d in DIRECTIONS}
    assert all((ref[0]["code"] == 0).all() for ref in (cs["short"], cov, var)) and int(cov[1].max()) == 1 and sum(len(ev) for ev in var[1]) > 100
    for ename, e in scan_engines(engines):
        e.set_sequences(seqs)
        for mode in MODES:
            check_cs(ffi, e, mode, lambda m, c, a: e.cs_ranges(m, ranges, c, a), recs, claimed, arena, cs[mode], ("ranges", ename, mode))
        check_coverage(ffi, e, CV.BOTH, lambda c, a: e.coverage_ranges(ranges, c, a), recs, claimed, arena, cov, ("ranges", ename), seqs)
        check_variants(ffi, e, lambda c, a: e.variants_ranges(ranges, c, a), recs, claimed, arena, var, ("ranges", ename))
        for d in DIRECTIONS:
            check_normalize(ffi, e, d, lambda dd, c, a: e.normalize_ranges(dd, ranges, c, a), recs, claimed, arena, norm[d], ("ranges", ename, d))


def test_default_grid_takes_several_records_per_wave(hip_lib):
    """Nothing set: what production runs.  The 12,288 short records of reuse_cases.default_path_records through the five passes,
    each against its yardstick -- at 16 waves per CU every wave takes more than one.  The variants launch is the first whose
    placing scan (awv_text_scan_kernel<Place>) crosses its tiles of 1,024 records: items with and without events stand on both
    sides of every tile edge."""
    from allwave_amd import ffi
    n = 12288
    child = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)  # (as tests/test_gpu_reuse.py: torch in a process of its own)
    assert child.returncode == 0, child.stderr.decode(errors="replace")[-2000:]
    assert 2 * 16 * int(child.stdout.split()[-1]) <= n  # a device with more CUs would turn this into a run without reuse
    recs = RC.default_path_records(n)
    seqs, pairs, claimed, arena = RC.verify_inputs(recs, DEFAULT_2P)
    var = RC.variants_want(ffi, recs, seqs)
    counts = [len(ev) for ev in var[1]]
    for edge in range(1024, n, 1024):
        for side in (counts[edge - 26:edge], counts[edge:edge + 26]):
            assert any(c > 0 for c in side) and any(c == 0 for c in side), edge
    e = ffi.Engine()
    try:
        e.set_sequences(seqs)
        check_encode(ffi, e, recs, claimed, arena, RC.encode_want(ffi, recs), "encode")
        for mode in MODES:
            check_cs(ffi, e, mode, lambda m, c, a: e.cs_cigars(m, pairs, c, a), recs, claimed, arena, RC.cs_want(ffi, mode, recs), ("cs", mode))
        check_coverage(ffi, e, CV.BOTH, lambda c, a: e.coverage_cigars(pairs, c, a), recs, claimed, arena, RC.coverage_want(ffi, CV.BOTH, recs, seqs), "coverage")
        check_variants(ffi, e, lambda c, a: e.variants_cigars(pairs, c, a), recs, claimed, arena, var, "variants")
        assert e.variants_stats().items == n and e.variants_stats().items > 1024  # one launch (nothing set: no pieces) of more than one tile
        for d in DIRECTIONS:
            check_normalize(ffi, e, d, lambda dd, c, a: e.normalize_cigars(dd, pairs, c, a), recs, claimed, arena, RC.normalize_want(ffi, d, recs, TAIL), ("normalize", d))
    finally:
        e.close()


def test_aligning_calls_with_two_workgroups(engines):
    """The island set, aligned with workgroups = 2: normalized, encoded, with cs texts, and with the coverage and variants
    accumulators on -- records, op bytes, texts, tracks and table are the default engine's, byte for byte."""
    seqs, pairs = S.island_set()
    out = []
    for e in (engines("NO_ARENA_PROBE"), engines("NO_ARENA_PROBE", workgroups=2)):
        e.set_sequences(seqs)
        e.coverage_begin("both")
        e.variants_begin()
        res, cigs = e.align_pairs(DEFAULT_2P, pairs, normalize="left")
        res2, texts, tout = e.align_pairs(DEFAULT_2P, pairs, normalize="left", encode=True)
        res3, cigs3, (cs_texts, csout) = e.align_pairs(DEFAULT_2P, pairs, cs="short")
        assert (res["status"] == 0).all() and e.normalize_stats().pairs == e.encode_stats().pairs == e.cs_stats().pairs == len(pairs)
        _, aligned, matched = e.coverage_read()
        table = e.variants_read()
        assert e.coverage_stats().items == e.variants_stats().items >= len(pairs) and int(aligned.max()) >= 1 and len(table) > 0
        out.append((res.tobytes(), cigs, res2.tobytes(), texts, tout.tobytes(), res3.tobytes(), cigs3, cs_texts, csout.tobytes(), aligned.tobytes(), matched.tobytes(), table.tobytes()))
        e.variants_end()
        e.coverage_begin(None)
    assert out[0] == out[1]
