"""CPU tests of the target-anchored multiple alignment (csrc/msa_device.hpp): the host yardstick awv_msa_host against the Python
restatement (msa_cases.msa_of), the known answer, properties on random strings, what the case list holds, the header's rule as a
program of its own under the sanitizers, the ABI of the new structs and the command-line tool's usage errors.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import cs_cases as X
import msa_cases as M
import normalize_cases as N
from util import rand_seq
from verify_cases import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text_of(row):
    return bytes(bytearray(int(b) for b in row))


def host_of(seqs, s, items):
    """ffi.msa_host on the items of target s, as msa_of's items."""
    from allwave_amd import ffi
    mine = [(revcomp(seqs[q]) if rev else bytes(seqs[q]), None if status != 0 else ops, span, sl) for q, t, rev, ops, span, sl, status in items if t == s]
    return ffi.msa_host(seqs[s], mine)


def test_known_answer(hip_lib):
    K = M.KNOWN
    seqs = [K["text"], K["pattern"], K["pattern2"]]
    one = [(1, 0, 0, K["ops"], None, None, 0)]
    two = one + [(2, 0, 0, K["ops2"], None, None, 0)]
    w = M.msa_of(seqs, [0], one)
    assert w["targets"] == [(0, 2, 30, 0)] and [text_of(r) for r in w["blocks"][0]] == [K["row0"], K["row1"]]
    assert w["items"] == [(M.OK, 0, 1, 27, 0, 30)] and w["runs"] == 1 and w["bases"] == 27 and w["bytes"] == 60
    w2 = M.msa_of(seqs, [0], two)
    assert [text_of(r) for r in w2["blocks"][0]] == [K["row0"], K["row1"], K["row2"]] and w2["targets"] == [(0, 3, 30, 0)]
    assert w2["items"][1] == (M.OK, 0, 2, 28, 0, 30)
    for items, want in ((one, w), (two, w2)):
        ins, width, codes, block = host_of(seqs, 0, items)
        assert width == 30 and list(codes) == [M.OK] * len(items) and list(ins) == want["ins"][0] and np.array_equal(block, want["blocks"][0])
    assert sum(w2["ins"][0]) == 3 and w2["ins"][0][19] == 3


@pytest.fixture(scope="module")
def cases():
    return M.case_list(), M.resident_set()


@pytest.fixture(scope="module")
def wanted(cases):
    cl, seqs = cases
    return M.msa_of(seqs, list(M.TARGETS), M.case_items(cl))


def test_the_case_list_holds_what_it_names(cases, wanted):
    cl, seqs = cases
    assert [len(s) for s in seqs] == list(M.SET_LENS) and seqs[4].islower() and b"N" in seqs[5] and b"n" in seqs[10] and min(M.SET_LENS) == 10 and max(M.SET_LENS) == 2200
    by = {c[0]: (k, c) for k, c in enumerate(cl)}
    assert len(by) == len(cl)
    items, ins, blocks = wanted["items"], wanted["ins"], wanted["blocks"]
    tj = {s: j for j, s in enumerate(M.TARGETS)}
    assert {i[0] for i in items} == {M.OK, M.SKIPPED, M.BAD_OP, M.LENGTHS, M.NOT_CHOSEN}
    for res in M.RESIDUES:  # 'D' runs at the named arena bytes
        for name, want in (("D on a lane's last byte, on the next lane's first, a run across the two, and on a chunk's last byte, residue %d", [15, 32, 47, 48, 1023]),
                           ("D on a chunk's first byte and a run across two chunks, residue %d", [1024, 2047, 2048])):
            k, c = by[name % res]
            assert c[7] == res and [res + p for p in range(len(c[4])) if c[4][p:p + 1] == b"D"] == want and items[k][0] == M.OK
    k, c = by["a D run of 60 across byte 1024"]
    assert c[7] == 0 and c[4].index(b"D") == 1000 and c[4].count(b"D") == 60
    assert by["a D run longer than a chunk"][1][4].count(b"D") == 1100 > 1024 and ins[tj[6]][10] == 1100 and ins[tj[6]][1000] == 60
    assert ins[tj[0]][0] >= 3 and ins[tj[0]][10] == 2  # slot 0 and slot L
    (ka, _), (kb, _) = by["DI at one place"], by["ID at the same place"]
    ra, rb = blocks[tj[9]][items[ka][2]], blocks[tj[9]][items[kb][2]]
    assert items[ka][0] == items[kb][0] == M.OK and not np.array_equal(ra, rb) and items[ka][3] == items[kb][3]
    rows3 = [text_of(blocks[tj[10]][items[by["one of three at a slot: %d D" % n][0]][2]]) for n in (1, 3, 2)]
    c0 = wanted["ins"][tj[10]][30] == 3 and sum(wanted["ins"][tj[10]][:30]) + 30
    assert c0 and [r[c0:c0 + 3].count(b"-") for r in rows3] == [2, 0, 1] and all(r[c0] != ord("-") for r in rows3)  # the maximum, left-justified
    k, c = by["a slice that cuts a D run at either end"]
    assert c[4][c[5][0] - 1:c[5][0] + 1] == b"DD" and c[4][c[5][1] - 1:c[5][1] + 1] == b"DD" and items[k][0] == M.OK and items[k][3] == 18
    assert by["a slice with skips of its own"][1][5][2:] == (7, 9) and by["a q_revcomp item"][1][3] == 1
    assert items[by["an item whose target is not chosen"][0]] == (M.NOT_CHOSEN, -1, 0, 0, 0, 0)
    assert items[by["a record that is not completed, target not chosen"][0]][0] == M.NOT_CHOSEN
    assert 12 in M.TARGETS and all(c[2] != 12 for c in cl) and wanted["targets"][tj[12]][1:3] == (1, M.SET_LENS[12])  # a target without items
    assert by["an empty op string"][1][4] == b"" and items[by["an empty op string"][0]][:2] == (M.OK, tj[10]) and items[by["only I"][0]][3:] == (0, 0, 0)
    assert items[by["a record that is not completed"][0]] == (M.SKIPPED, tj[10], 0, 0, 0, 0)
    assert items[by["a string one base too long"][0]][0] == M.LENGTHS == items[by["a string one base too long for the query"][0]][0]
    k, c = by["a stray byte behind a D run longer than every other item's"]
    assert items[k][0] == M.BAD_OP and c[4].index(b"=") > c[4].index(b"D") and c[4].count(b"D") == 9 > max(ins[tj[10]])
    k, c = by["a stray byte behind a long D run, second chunk"]
    assert items[k][0] == M.BAD_OP and c[4].count(b"D") == 1200 > max(ins[tj[6]]) and len(c[4]) > 1024
    assert len(cl) > 2 * 2 + 8 and len({c[2] for c in cl}) >= 6  # more items than two workgroups take in a trip each; targets mixed
    assert wanted["failed"] == sum(1 for i in items if i[0] in (M.BAD_OP, M.LENGTHS)) >= 4


def test_msa_host_on_the_case_list(hip_lib, cases, wanted):
    cl, seqs = cases
    its = M.case_items(cl)
    for j, s in enumerate(M.TARGETS):
        ins, width, codes, block = host_of(seqs, s, its)
        assert list(ins) == wanted["ins"][j] and width == wanted["targets"][j][2], s
        assert list(codes) == [w[0] for w, it in zip(wanted["items"], its) if it[1] == s], s
        assert np.array_equal(block, wanted["blocks"][j]), s


def random_call(rng, n_items, long_ops):
    """One target and n_items random items on it: [(q, 0, rev, ops, span, slice, 0)] over seqs (the target is sequence 0)."""
    tlen = rng.randint(1, 400)
    seqs = [rand_seq(rng, tlen, b"ACGTacgtN")]
    items = []
    for k in range(n_items):
        n = rng.randint(0, 300)
        ops = N.random_ops_long(rng, n) if long_ops else X.random_ops(rng, n)
        while len(ops) - ops.count(b"D") > tlen:
            ops = ops[:len(ops) // 2]
        need_q, need_t = len(ops) - ops.count(b"I"), len(ops) - ops.count(b"D")
        pb, tb = rng.randint(0, 5), rng.randint(0, tlen - need_t)
        seqs.append(rand_seq(rng, pb + need_q + rng.randint(0, 5), b"ACGTacgtN"))
        sl = None
        if k % 3 == 0 and ops:
            b = rng.randint(0, len(ops))
            e = rng.randint(b, len(ops))
            sl = (b, e, b - ops[:b].count(b"I"), b - ops[:b].count(b"D"))
        items.append((len(seqs) - 1, 0, k % 2, ops, (pb, pb + need_q, tb, tb + need_t), sl, 0))
    return seqs, items


def test_properties_on_random_strings(hip_lib):
    rng = random.Random(720)
    gaps = 0
    for trial in range(40):
        seqs, items = random_call(rng, rng.randint(1, 6), trial % 2)
        w = M.msa_of(seqs, [0], items)
        blk, row0 = w["blocks"][0], w["blocks"][0][0]
        ins, width, codes, block = host_of(seqs, 0, items)
        assert np.array_equal(block, blk) and list(ins) == w["ins"][0] and list(codes) == [i[0] for i in w["items"]] == [M.OK] * len(items)
        assert text_of(row0).replace(b"-", b"") == seqs[0].upper()
        used = np.zeros(blk.shape[1], dtype=bool)
        for (q, _, rev, ops, span, sl, _), it in zip(items, w["items"]):
            row = blk[it[2]]
            pattern = revcomp(seqs[q]) if rev else seqs[q]
            x0 = span[0] if sl is None else span[0] + sl[2]
            own = ops if sl is None else ops[sl[0]:sl[1]]
            consumed = len(own) - own.count(b"I")
            assert text_of(row).replace(b"-", b"") == pattern[x0:x0 + consumed].upper()  # exactly the pattern bases the item consumes
            lead, trail = len(own) - len(own.lstrip(b"I")), len(own) - len(own.rstrip(b"I"))
            core = own[lead:len(own) - trail] if consumed else b""
            assert M.ops_from_rows(row0, row) == core.replace(b"X", b"M")  # the op string back, order included
            assert (it[4], it[5]) == ((int(np.flatnonzero(row != 45)[0]), int(np.flatnonzero(row != 45)[-1]) + 1) if consumed else (0, 0)) and it[3] == consumed
            used |= row != 45
        inscol = row0 == 45
        assert (used[inscol]).all()  # every insertion column holds a base of some item
        gaps += int(inscol.sum())
        perm = list(range(len(items)))
        rng.shuffle(perm)
        w2 = M.msa_of(seqs, [0], [items[p] for p in perm])
        assert w2["ins"] == w["ins"] and np.array_equal(w2["blocks"][0][0], row0)
        for new, old in enumerate(perm):  # permuting the items permutes the rows and changes nothing else
            assert np.array_equal(w2["blocks"][0][w2["items"][new][2]], blk[w["items"][old][2]])
            assert w2["items"][new][3:] == w["items"][old][3:]
    assert gaps > 200


def test_msa_host_refuses(hip_lib):
    from allwave_amd import ffi
    t, p = b"ACGTACGTAC", b"ACGTAC"
    for item in ((p, b"MMMM", (0, 7, 0, 10), None), (p, b"MMMM", (0, 6, 0, 11), None), (p, b"MMMM", (3, 2, 0, 10), None), (p, b"MMMM", None, (0, 5, 0, 0)),
                 (p, b"MMMM", None, (3, 2, 0, 0)), (p, b"MMMM", None, (0, 4, -1, 0))):
        with pytest.raises(ffi.EngineError) as err:
            ffi.msa_host(t, [item])
        assert err.value.code == ffi.AWV_ERR_ARG
    ins, width, codes, block = ffi.msa_host(t, [(p, None, None, None), (p, b"MMDDDD", None, None), (p, b"MMMMMMM", None, None), (p, b"MM?", None, None)])
    assert list(codes) == [M.SKIPPED, M.OK, M.LENGTHS, M.BAD_OP] and width == 14 and block.shape == (2, 14) and text_of(block[1]) == b"ACGTAC--------"
    ins, width, codes, block = ffi.msa_host(b"", [])
    assert width == 0 and list(ins) == [0] and block.size == 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/msa_driver.cpp, compiled for the host only under the address and undefined-behaviour sanitizers (host options:
    nothing is built for or run on a GPU)."""
    from allwave_amd import build
    exe = str(tmp_path_factory.mktemp("msa") / "msa_driver")
    cmd = [build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, "-I" + build.HOST_DIR,
           os.path.join(ROOT, "tests", "msa_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return exe


def test_host_rule_under_sanitizers(driver, cases, wanted):
    """msa_target of csrc/msa_device.hpp behind the slice rule of the cs text as a program of its own, on exact-size copies of the
    case list's bytes: it must print msa_of's answers."""
    cl, seqs = cases
    its = M.case_items(cl)
    lines, want = [], []
    for j, s in enumerate(M.TARGETS):
        lines.append("T " + (seqs[s].hex() or "-"))
        mine = [(it, w) for it, w in zip(its, wanted["items"]) if it[1] == s]
        for (q, t, rev, ops, span, sl, status), _ in mine:
            pattern = revcomp(seqs[q]) if rev else seqs[q]
            cb, ce, qs, ts = sl if sl is not None else (0, len(ops), 0, 0)
            lines.append("I %s 0 %d 0 %d %s %d %d %d %d" % (pattern.hex() or "-", len(pattern), len(seqs[s]), "!" if status else (ops.hex() or "-"), cb, ce, qs, ts))
        lines.append("E")
        blk = wanted["blocks"][j]
        want += ["W %d %d" % (blk.shape[1], blk.shape[0]), "C" + "".join(" %d" % w[0] for _, w in mine), "N" + "".join(" %d" % v for v in wanted["ins"][j])]
        want += [text_of(r).decode() for r in blk]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want) > 40
    for g, w in zip(got, want):
        assert g == w, (g[:200], w[:200])


def test_abi_of_the_new_structs(hip_lib):
    from allwave_amd import ffi
    assert ffi.MSA_ITEM_DTYPE.itemsize == 32 and ffi.MSA_TARGET_DTYPE.itemsize == 24 and C.sizeof(ffi.MsaStats) == 72
    hdr = open(os.path.join(ROOT, "include", "allwave_hip.h")).read()
    for text in ("} awv_msa_item; /* 32 bytes */", "} awv_msa_target; /* 24 bytes */", "} awv_msa_stats; /* 72 bytes */"):
        assert text in hdr
    assert ffi.MSA_ITEM_DTYPE.names == M.ITEM_FIELDS and ffi.MSA_TARGET_DTYPE.names == M.TARGET_FIELDS
    assert (ffi.AWV_MS_OK, ffi.AWV_MS_SKIPPED, ffi.AWV_MS_BAD_OP, ffi.AWV_MS_LENGTHS, ffi.AWV_MS_NOT_CHOSEN) == (M.OK, M.SKIPPED, M.BAD_OP, M.LENGTHS, M.NOT_CHOSEN)
    for name, value in (("OK", 0), ("SKIPPED", 1), ("BAD_OP", 2), ("LENGTHS", 3), ("NOT_CHOSEN", 4)):
        assert "#define AWV_MS_%s %d" % (name, value) in hdr
    assert [n for n, _ in ffi.MsaStats._fields_] == ["width_ms", "scan_ms", "emit_ms", "items", "failed", "columns", "runs", "bases", "bytes"]
    # the yardstick needs no device and is no product path: nothing but the C entry point names it
    for dirpath, _, files in os.walk(os.path.join(ROOT, "allwave_amd", "csrc")):
        for f in files:
            txt = open(os.path.join(dirpath, f), errors="replace").read()
            assert f == "msa.hip" or ("awv_msa_host(" not in txt and "msa_target(" not in txt) or f == "msa_device.hpp", f
    assert "awv_msa_host(" not in open(os.path.join(ROOT, "allwave_amd", "csrc", "msa_device.hpp")).read()
    assert open(os.path.join(ROOT, "allwave_amd", "csrc", "msa.hip")).read().count("msa_target(") == 1


def test_cli_usage_errors_and_help(hip_lib, tmp_path):
    from allwave_amd import build
    build.build_host()
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTTCGTAC\n")
    paf = tmp_path / "x.paf"
    paf.write_text("")
    out = tmp_path / "msa.fa"

    def usage(args, *words):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa)] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "" and all(w in r.stderr for w in words), (args, r.stderr)

    for extra, word in ((["--score-only"], "--score-only"), (["--check-paf", str(paf)], "--check-paf"), (["--mash-matrix"], "--mash-matrix"),
                        (["--device-cigar"], "--device-cigar")):
        usage(["--msa", str(out), "--msa-target", "a"] + extra, "--msa", word)
    usage(["--msa", str(out)], "'--msa' requires '--msa-target'")
    usage(["--msa-target", "a"], "'--msa-target' requires '--msa'")
    usage(["--msa-max-bytes", "5"], "'--msa-max-bytes' requires '--msa'")
    usage(["--msa", str(out), "--msa-target", "nobody"], "no sequence named 'nobody'")
    usage(["--msa", str(out), "--msa-target", "a", "--msa-target", "b"], "must contain {}")
    usage(["--msa", str(out), "--msa-target", "a", "--msa-target", "a"], "named twice")
    for value in ("0", "-1", "x", ""):
        usage(["--msa", str(out), "--msa-target", "a", "--msa-max-bytes", value], "--msa-max-bytes expects a number of bytes N >= 1")
    assert not out.exists()
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--msa FILE" in r.stdout and "--msa-target NAME" in r.stdout and "--msa-max-bytes N" in r.stdout
    assert "msa T targets, R rows, B bytes, K ms" in r.stdout and "--shard every process writes" in r.stdout and "{}" in r.stdout
