"""CPU tests of the allele table (csrc/variants_device.hpp): the host yardsticks awv_variants_one_host and awv_variants_fold_host
against the Python restatement (variants_cases.events_of, Table), the hash's combine identity, the fold's order independence, the
header's rule under sanitizers, and the ABI.  None of them needs a GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import variants_cases as R
from verify_cases import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return R.resident_set(), R.case_list()


@pytest.fixture(scope="module")
def items():
    return R.random_items()


def test_restatement_on_a_known_answer():
    # 2M 1X 2I 1M 3D 1X 2D over the rectangle [1, 11) x [2, 9) of query 3 (forward) and target 5
    pattern, ops, span = b"tACGTNacgtAC", b"MMXIIMDDDXDD", (1, 11, 2, 9)
    code, ev = R.events_of(3, 5, False, pattern, ops, span, (0, 0))
    h = R.hash_of
    assert code == R.OK and ev == [(5, 4, R.SNV, 1, ord("G"), (3 << 32) | 3), (5, 5, R.DEL, 2, 0, (3 << 32) | 4), (5, 8, R.INS, 3, h(b"NAC"), (3 << 32) | 5),
                                   (5, 8, R.SNV, 1, ord("G"), (3 << 32) | 8), (5, 9, R.INS, 2, h(b"TA"), (3 << 32) | 9)]
    assert h(b"") == 0 and h(b"a") == ord("A") and h(b"NAC") == ((ord("N") * R.BASE + ord("A")) * R.BASE + ord("C")) % R.MOD == h(b"nac")
    assert R.counts_of(ev) == (2, 2, 1)
    # the reverse strand only changes the representative; the last insertion sits before tlen of the rectangle's end
    assert [e[5] for e in R.events_of(3, 5, True, pattern, ops, span, (0, 0))[1]] == [(3 << 32) | (1 << 31) | p for p in (3, 4, 5, 8, 9)]
    assert R.events_of(3, 5, False, pattern, ops, (1, 10, 2, 9), (0, 0)) == (R.LENGTHS, [])
    assert R.events_of(3, 5, False, pattern, b"MM=", span, (0, 0)) == (R.BAD_OP, [])
    # a slice that cuts a run cuts the event
    assert R.events_of(3, 5, False, pattern, ops[4:8], span, (3, 4))[1] == [(5, 6, R.DEL, 1, 0, (3 << 32) | 4), (5, 8, R.INS, 2, h(b"NA"), (3 << 32) | 5)]
    tb = R.Table()
    tb.add_events(ev)
    tb.add_events(R.events_of(2, 5, True, pattern, ops, span, (0, 0))[1])
    rows = tb.array()
    assert rows["count"].tolist() == [2] * 5 and rows["rep"].tolist() == [(2 << 32) | (1 << 31) | p for p in (3, 4, 8, 5, 9)]
    assert rows["type"].tolist() == [R.SNV, R.DEL, R.SNV, R.INS, R.INS] and rows["pos"].tolist() == [4, 5, 8, 8, 9]


def test_paf_reading_agrees_with_the_restatement():
    seqs = [b"ACGTACGTAC", b"TTGCATGCA"]
    line = "q\t10\t2\t8\t-\tt\t9\t1\t8\t5\t8\t60\tcg:Z:2=1X1I2=2D"
    tb = R.table_from_paf([line], ["q", "t"], seqs)
    want = R.Table()
    assert want.add(seqs, 0, 1, True, b"MMXDMMII", span=(2, 8, 1, 8)) == R.OK
    assert R.same(tb.array(), want.array()) and len(tb.rows) == 3
    assert R.format_table(["q", "t"], seqs, tb.array()) == ["t\t3\tsnv\t1\tC\tG\t1", "t\t4\tins\t1\t.\tT\t1", "t\t6\tdel\t2\tGC\t.\t1"]


def one_host(ffi, seqs, case):
    name, q, t, rev, ops, sl, status, _ = case
    return ffi.variants_one_host(q, t, rev, revcomp(seqs[q]) if rev else seqs[q], len(seqs[t]), ops, slice=sl)


def test_yardsticks_on_the_case_list(hip_lib, cases):
    from allwave_amd import ffi
    seqs, cl = cases
    assert ffi.VARIANT_DTYPE == R.ROW_DTYPE
    codes, everything = set(), []
    for case in cl:
        if case[6] != 0:
            continue
        code, events = R.case_events(seqs, case)
        item, got = one_host(ffi, seqs, case)
        assert (int(item["code"]), int(item["snv"]), int(item["ins"]), int(item["del"])) == (code,) + R.counts_of(events), case[0]
        assert R.same(got, R.as_rows(events)), case[0]
        codes.add(code)
        everything.append(got)
    assert codes == {R.OK, R.BAD_OP, R.LENGTHS}
    want = R.expected_table(seqs, cl)
    folded = ffi.variants_fold_host(np.concatenate(everything))
    assert R.same(folded, want.array()) and int(folded["count"].sum()) == want.events
    # the properties the list was built for
    rows = want.rows
    site = [k for k in rows if k[:4] == (3, 10, R.INS, 3)]
    assert len(site) == 2 and seqs[1][10:13] != seqs[2][10:13]  # two different insertions of equal length at one site: two rows
    shared = [c for c in cl if c[0].startswith(("an alignment of query 4", "the same alignment of query 5"))]
    two = R.expected_table(seqs, shared).rows  # the same alleles through a forward and a q_revcomp query: one row, the smaller rep
    for ev in R.case_events(seqs, shared[0])[1]:
        assert two[ev[:5]] == [2, ev[5]] and ev[5] >> 32 == 4 and rows[ev[:5]][0] >= 2 and rows[ev[:5]][1] <= ev[5]
    assert len(two) == len(R.case_events(seqs, shared[0])[1]) >= 6
    assert [e[:5] for e in R.case_events(seqs, shared[0])[1]] == [e[:5] for e in R.case_events(seqs, shared[1])[1]]
    assert any(k[1] == R.SET_LENS[0] and k[2] == R.INS for k in rows if k[0] == 0)  # an insertion before tlen
    assert any(c in b"acgtNn" for c in seqs[4][:200])


def test_yardsticks_on_random_items(hip_lib, items):
    from allwave_amd import ffi
    assert len(items) == 300
    tb, everything = R.Table(), []
    n_range = n_slice = n_rev = 0
    for k, (q, t, rev, pattern, tlen, span, ops, sl) in enumerate(items):
        item_ops, skips = (ops, (0, 0)) if sl is None else (ops[sl[0]:sl[1]], (sl[2], sl[3]))
        code, events = R.events_of(q, t, rev, pattern, item_ops, span, skips)
        item, got = ffi.variants_one_host(q, t, rev, pattern, tlen, ops, span=span, slice=sl)
        assert code == R.OK == int(item["code"]) and (int(item["snv"]), int(item["ins"]), int(item["del"])) == R.counts_of(events)
        assert R.same(got, R.as_rows(events)), k
        tb.add_events(events)
        everything.append(got)
        n_range += span != (0, len(pattern), 0, tlen)
        n_slice += sl is not None
        n_rev += rev
    assert n_range >= 50 and n_slice >= 50 and n_rev >= 100
    folded = ffi.variants_fold_host(np.concatenate(everything))
    assert R.same(folded, tb.array()) and len(folded) < tb.events  # rows were shared
    # folding is idempotent, and rows fold like events: a table and more events
    assert R.same(ffi.variants_fold_host(folded), folded)
    half = ffi.variants_fold_host(np.concatenate(everything[:150]))
    assert R.same(ffi.variants_fold_host(np.concatenate([half] + everything[150:])), folded)


def test_unsound_items_have_no_events(hip_lib):
    from allwave_amd import ffi
    pattern = b"ACGT" * 5
    for ops, sl, code in ((b"XXXX?", None, R.BAD_OP), (b"?XXXX", None, R.BAD_OP), (b"X" * 21, None, R.LENGTHS), (b"X" * 20 + b"D", None, R.LENGTHS),
                          (b"X" * 20 + b"I", None, R.LENGTHS), (b"XXXX", (0, 4, 17, 0), R.LENGTHS), (b"X" * 30 + b"?", None, R.BAD_OP)):
        for rev in (False, True):
            item, ev = ffi.variants_one_host(0, 1, rev, pattern, 20, ops, slice=sl)
            assert (int(item["code"]), int(item["snv"]), int(item["ins"]), int(item["del"])) == (code, 0, 0, 0) and len(ev) == 0
    for kw in (dict(slice=(3, 2, 0, 0)), dict(slice=(0, 5, 0, 0)), dict(slice=(0, 4, -1, 0)), dict(span=(0, 21, 0, 20)), dict(span=(5, 4, 0, 20))):
        with pytest.raises(ffi.EngineError) as err:
            ffi.variants_one_host(0, 1, False, pattern, 20, b"XXXX", **kw)
        assert err.value.code == ffi.AWV_ERR_ARG
    # a buffer too small is not written past: the count says what it takes
    L = ffi.load()
    out = np.zeros(1, dtype=ffi.VAR_ITEM_DTYPE)
    ev = np.zeros(3, dtype=ffi.VARIANT_DTYPE)
    n = C.c_uint64(0)
    assert L.awv_variants_one_host(0, 1, 0, pattern, 20, 20, 0, 20, 0, 20, b"XXXXX", 5, None, ev.ctypes.data, 2, C.byref(n), out.ctypes.data) == ffi.AWV_OK
    assert n.value == 5 and ev["count"].tolist() == [1, 1, 0]
    assert L.awv_variants_one_host(0, 1, 0, pattern, 20, 20, 0, 20, 0, 20, b"XXXXX", 5, None, None, 0, C.byref(n), None) == ffi.AWV_ERR_ARG
    assert L.awv_variants_fold_host(None, 0, C.byref(n)) == ffi.AWV_OK and n.value == 0
    assert L.awv_variants_fold_host(None, 1, C.byref(n)) == ffi.AWV_ERR_ARG


def test_the_fold_does_not_depend_on_the_order(hip_lib, cases):
    from allwave_amd import ffi
    seqs, cl = cases
    sound = [c for c in cl if c[6] == 0][::3]
    want = R.expected_table(seqs, sound).array()
    assert int(want["count"].max()) >= 3
    events = np.concatenate([R.as_rows(R.case_events(seqs, c)[1]) for c in sound])
    for seed in (1, 2, 3):
        order = np.random.RandomState(seed).permutation(len(events))
        assert R.same(ffi.variants_fold_host(events[order]), want)
        cut = len(events) // (seed + 1)  # folded in two parts, the parts folded together
        parts = [ffi.variants_fold_host(events[order][:cut]), ffi.variants_fold_host(events[order][cut:])]
        assert R.same(ffi.variants_fold_host(np.concatenate(parts[::-1])), want)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/variants_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("variants") / "variants_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "variants_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def fnv(rows):
    h = 1469598103934665603
    for r in rows:
        for f in ("t_idx", "pos", "type", "len", "hash", "rep", "count"):
            h = ((h ^ int(r[f])) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_combine_identity_and_host_rule_under_sanitizers(driver, cases, items):
    """hash_push, hash_combine and hash_pow, var_one and fold_rows of csrc/variants_device.hpp with the slice rule of the cs text as
    a program of their own, on exact-size arrays: h(a.b) = h(a) * B^|b| + h(b) on random splits, every case is what events_of
    says -- and the sanitizers report nothing."""
    seqs, cl = cases
    rng = random.Random(533)
    splits = [(b"", b""), (b"A", b""), (b"", b"c"), (b"acgtn", b"ACGTN")]
    for _ in range(60):
        s = bytes(rng.choice(b"ACGTacgtNn") for _ in range(rng.choice([1, 2, 15, 16, 17, 64, 300, 1100, 2500])))
        cut = rng.randint(0, len(s))
        splits.append((s[:cut], s[cut:]))
    lines = []  # (q, t, rev, tlen, span, pattern, ops, slice)
    for name, q, t, rev, ops, sl, status, _ in cl:
        if status == 0 and len(ops) <= 1200:
            lines.append((q, t, rev, len(seqs[t]), (0, len(seqs[q]), 0, len(seqs[t])), revcomp(seqs[q]) if rev else seqs[q], ops, sl or (0, len(ops), 0, 0)))
    for q, t, rev, pattern, tlen, span, ops, sl in items[::3]:
        lines.append((q, t, rev, tlen, span, pattern, ops, sl or (0, len(ops), 0, 0)))  # rectangles that end on the pattern's last base
    refused = [(0, 1, 0, 4, (0, 4, 0, 4), b"ACGT", b"MMXM", (3, 2, 0, 0)), (0, 1, 0, 4, (0, 4, 0, 4), b"ACGT", b"MMXM", (0, 5, 0, 0)),
               (0, 1, 1, 4, (0, 4, 0, 4), b"ACGT", b"MMXM", (0, 4, -1, 0))]
    lines += refused
    text_in = "".join("H %s %s\n" % (a.hex() or "-", b.hex() or "-") for a, b in splits)
    text_in += "".join("V %d %d %d %d %d %d %d %d %s %s %d %d %d %d\n" % ((q, t, rev, tl) + tuple(sp) + (p.hex() or "-", o.hex() or "-") + tuple(sl))
                       for q, t, rev, tl, sp, p, o, sl in lines)
    r = subprocess.run([driver], input=text_in, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(splits) + len(lines)
    for (a, b), line in zip(splits, got):
        assert [int(v) for v in line.split()] == [R.hash_of(a), R.hash_of(b), R.hash_of(a + b), R.hash_of(a + b)], (a, b)
        assert R.hash_of(a + b) == (R.hash_of(a) * pow(R.BASE, len(b), R.MOD) + R.hash_of(b)) % R.MOD
    codes = set()
    for case, line in zip(lines, got[len(splits):]):
        q, t, rev, tl, sp, p, o, sl = case
        if case in refused:
            assert line.split()[:6] == ["0", str(R.SKIPPED), "0", "0", "0", "0"], line
            continue
        code, events = R.events_of(q, t, rev, p, o[sl[0]:sl[1]], sp, (sl[2], sl[3]))
        tb = R.Table()
        tb.add_events(events, 2)
        assert line == "1 %d %d %d %d %d %d %d %d" % ((code,) + R.counts_of(events) + (len(events), fnv(R.as_rows(events)), len(tb.rows), fnv(tb.array()))), (line, sl)
        codes.add(code)
    assert codes == {R.OK, R.BAD_OP, R.LENGTHS}


def test_exports_struct_sizes_and_constants(hip_lib):
    from allwave_amd import ffi
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for name in ("awv_variants_one_host", "awv_variants_fold_host"):
        assert name in ffi.EXPORTS and getattr(hip_lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr), name
    assert ffi.VARIANT_DTYPE.itemsize == 40 and "} awv_variant; /* 40 bytes */" in hdr
    names = ("t_idx", "pos", "type", "len", "hash", "rep", "count", "reserved")
    assert [ffi.VARIANT_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 24, 32, 36]
    assert [str(ffi.VARIANT_DTYPE.fields[n][0]) for n in names] == ["int32"] * 4 + ["uint64"] * 2 + ["uint32"] * 2
    assert ffi.VAR_ITEM_DTYPE.itemsize == 16 and "} awv_var_item; /* 16 bytes */" in hdr and list(ffi.VAR_ITEM_DTYPE.names) == ["code", "snv", "ins", "del"]
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AWV_V(?:AR|R)_[A-Z_]*)\s+(\d+)\s", hdr)}
    assert defs == dict(AWV_VAR_SNV=0, AWV_VAR_DEL=1, AWV_VAR_INS=2, AWV_VR_OK=0, AWV_VR_SKIPPED=1, AWV_VR_BAD_OP=2, AWV_VR_LENGTHS=3)
    assert all(getattr(ffi, k) == v for k, v in defs.items())
    assert "#define AWV_VAR_HASH_BASE %dull /* B = 0x%x," % (R.BASE, R.BASE) in hdr and ffi.AWV_VAR_HASH_BASE == R.BASE < R.MOD == ffi.AWV_VAR_HASH_MOD
    assert (R.OK, R.SKIPPED, R.BAD_OP, R.LENGTHS) == (ffi.AWV_VR_OK, ffi.AWV_VR_SKIPPED, ffi.AWV_VR_BAD_OP, ffi.AWV_VR_LENGTHS)
    assert (R.SNV, R.DEL, R.INS) == (ffi.AWV_VAR_SNV, ffi.AWV_VAR_DEL, ffi.AWV_VAR_INS)
    assert hip_lib.awv_abi_version() == 3 and "#define AWV_ABI_VERSION 3" in hdr
