"""CPU tests of the reuse lists as lift.hip and msa.hip take them (tests/reuse_cases.py, the builders at its end): that the traps
are traps, from the restatements alone.  The processing order at one workgroup is the list order (msa) and the list order
restricted to the records that have a query (lift); for every carry of the two kernels a plain model of the leak -- B walked
from the state A left, built on msa_cases.msa_of's and lift_cases.lift_of's reading of the contract -- gives the clean answer
without the leak and another one with it, which is what makes tests/test_gpu_reuse_lift_msa.py fail on a kernel that forgets a
reset; most records of every list are sound under both passes' rule; the C yardsticks are the restatements on these lists; and
the launch-geometry set holds what the GPU test relies on.  What each list traps:

  main-D, pass-D   gap_tail -> gap_head: msa's run0 (B's leading 'D' run comes out too narrow, or is dropped), lift's last_a from
                   the query side; all_gaps -> plain: msa's prev_d (B on a 16-byte boundary: one run too many in the stats)
  main-I, pass-I   gap_tail -> gap_head: lift's last_a from the target side; all_gaps -> plain: prev_d
  every list       a record with columns, then one with a base: msa's cq / ct, lift's four counts; the records with 200 queries,
                   then the next one: lift's probe cursors
  zero             SKIPPED and column-free records behind two plain ones: nothing of a walked record may reach them"""
import numpy as np

import lift_cases as L
import msa_cases as M
import reuse_cases as RC
from test_reuse_cpu import consumed, instances, op_runs, spread

D, I = ord("D"), ord("I")
MSA_LISTS_D = ("main-D", "pass-D")
OKC = 0  # AWV_LF_OK = AWV_MS_OK
_MADE = {}


def made(key, make):
    """Built once and never changed."""
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


def inputs(name):
    return made(("inputs", name), lambda: RC.lift_msa_inputs(RC.all_lists()[name]))


def queries(name):
    return made(("queries", name), lambda: RC.lift_queries(RC.all_lists()[name], inputs(name)[0], name))


def own(name):
    """msa_of's answer in the own-targets layout."""
    def make():
        recs = RC.all_lists()[name]
        seqs, pairs, targets = RC.msa_layout(recs, inputs(name)[0], False, name)
        return RC.msa_want(seqs, targets, RC.msa_items(recs, pairs))
    return made(("own", name), make)


def queried_pairs(recs, qs):
    """[(k, A, B)]: record k and the record lift.hip walks before it at one workgroup -- the one before it among those with a query."""
    ks = sorted({q[0] for q in qs})
    return [(b, recs[a], recs[b]) for a, b in zip(ks, ks[1:])]


# ---- the processing order ------------------------------------------------------------------------------------------------------

def test_lift_and_msa_take_the_lists_in_list_order():
    for name, recs in RC.all_lists().items():
        seqs, pairs, results, arena = inputs(name)
        keys = [int(r["cigar_len"]) if r["status"] == 0 else 0 for r in results]
        assert keys == [RC.scan_key(r) for r in recs] and RC.dispatch_order(keys) == list(range(len(recs))), name  # msa: every record
        if name != "zero":
            assert all(x > y for x, y in zip(keys, keys[1:])), name
        # lift: the records with a query, compacted in list order, then the same stable sort
        ks = sorted({q[0] for q in queries(name)})
        assert [ks[i] for i in RC.dispatch_order([keys[k] for k in ks])] == ks, name
        assert all(RC.has_query(k) for k in ks) and not any(RC.has_query(k) for k in range(1, len(recs), 3)), name
        missing = [k for k in range(len(recs)) if RC.has_query(k) and k not in ks]
        assert all(recs[k].kind == "len0" for k in missing), (name, missing)  # no base on either side: no interval to ask for
        assert len(ks) >= (2 * len(recs)) // 3 - 12, name
        # the strings: inside the arena, in order, none over another, every residue modulo 16
        offs = [int(r["cigar_off"]) for r in results]
        assert all(offs[k] + len(recs[k].ops) <= offs[k + 1] for k in range(len(recs) - 1)) and offs[-1] + len(recs[-1].ops) == len(arena), name
        assert all(arena[o:o + len(r.ops)] == r.ops for o, r in zip(offs, recs)), name
        if name != "zero":
            assert sorted(set(o % 16 for o in offs)) == list(range(16)), name
    recs, begs = RC.verify_ranges_list()
    keys = [RC.scan_key(r) for r in recs]
    assert all(x > y for x, y in zip(keys, keys[1:]))


def test_heavy_records_fill_more_than_a_step_of_probes():
    """The records with 200 queries: 130 or more from one side; the probes of that side that one chunk answers are more than 64, and
    others are answered in a later chunk -- they stay pending behind the first."""
    for name, recs in RC.all_lists().items():
        seqs, pairs, results, arena = inputs(name)
        heavy = RC.heavy_records(recs)
        assert heavy[0] == 0 and (name == "zero" or len(heavy) == 2), name
        for k in heavy:
            mine = [q for q in queries(name) if q[0] == k]
            assert len(mine) >= 200 and sum(1 for q in mine if q[1] == RC.FROM_TARGET) >= 130 and RC.has_query(k), (name, k)
            sh = int(results[k]["cigar_off"]) % 16
            ops = recs[k].ops
            ys, y = [], 0
            for op in ops:
                ys.append(y)
                y += op != D
            aligned = [c for c in range(len(ops)) if ops[c] in b"MX"]
            by_chunk = {}
            for _, frm, beg, end in mine:
                if frm != RC.FROM_TARGET:
                    continue
                for r in (beg, end):  # a probe: the first aligned column whose text offset is r or more
                    col = next((c for c in aligned if ys[c] >= r), None)
                    if col is not None:
                        by_chunk[(sh + col) // RC.CHUNK] = by_chunk.get((sh + col) // RC.CHUNK, 0) + 1
            if name != "zero":
                assert max(by_chunk.values()) > 2 * 64 and len(by_chunk) >= 2 and max(by_chunk) > max(by_chunk, key=by_chunk.get), (name, k, by_chunk)
                assert (sh + len(ops) - 1) // RC.CHUNK >= 1, (name, k)
            else:
                assert max(by_chunk.values()) > 2 * 64, (name, by_chunk)
        if name != "zero":  # the second heavy record has two chunks at every residue, and a shorter record behind it
            k = heavy[1]
            nxt = next(b for b, _, _ in queried_pairs(recs, queries(name)) if b > k)
            assert RC.CHUNK + 16 <= len(recs[k].ops) < 2 * RC.CHUNK - 16 and len(recs[nxt].ops) < len(recs[k].ops) and len(recs[0].ops) > 4 * RC.CHUNK, name


# ---- msa.hip: models of the walk ------------------------------------------------------------------------------------------------

def msa_walk(ops, y0, run0=0, prev_d=False):
    """msa.hip's widening walk of a sound string, column by column: ([(slot, run)] in column order, the runs counted).  A 'D' run
    is owned by the column that ends it (or the string's end); its width is that column less "one past the last column so far that
    is no 'D'" -- run0, 0 in a fresh wave -- and a width of 0 or less widens nothing.  prev_d: the column before column 0 counts as
    a 'D' (it can only where the string begins on a 16-byte boundary)."""
    out, runs = [], 0
    y, last_nd, was_d = y0, run0, prev_d
    for k, op in enumerate(ops):
        if op != D:
            if was_d:
                runs += 1
                if k - last_nd > 0:
                    out.append((y, k - last_nd))
            last_nd = max(last_nd, k + 1)
            y += 1
        was_d = op == D
    if was_d and ops:
        runs += 1
        if len(ops) - last_nd > 0:
            out.append((y, len(ops) - last_nd))
    return out, runs


def ins_of(widened, tlen):
    ins = [0] * (tlen + 1)
    for y, run in widened:
        if 0 <= y <= tlen:
            ins[y] = max(ins[y], run)
    return ins


def cols_of(ins):
    acc, out = 0, []
    for p, w in enumerate(ins):
        acc += w
        out.append(p + acc)
    return out


def msa_place(ops, pattern, tlen, ins, cq=0, ct=0):
    """msa.hip's emit walk: {column: byte} of an item's row over its target's widths, from pattern position cq and text position
    ct (0, 0 in a fresh wave); a base is stored only where both positions are inside their sequences."""
    cols = cols_of(ins)
    at, x, y, j = {}, cq, ct, 0
    for op in ops:
        j = j + 1 if op == D else 0
        if op != I and x < len(pattern) and y <= tlen and (op == D or y < tlen):
            at[cols[y] - ins[y] + j - 1 if op == D else cols[y]] = M.upper(pattern[x])
        x += op != I
        y += op != D
    return at


def columns_of_item(ops, ins):
    """(col_beg, col_end) of a whole-span item over the widths `ins`, as msa_device.hpp's item_columns makes them from the ends."""
    cols = cols_of(ins)
    cs = [k for k in range(len(ops)) if ops[k] != I]
    if not cs:
        return 0, 0
    ys, y = {}, 0
    for k, op in enumerate(ops):
        ys[k] = y
        y += op != D
    kf, kl = cs[0], cs[-1]
    beg = cols[ys[kf]] - ins[ys[kf]] if ops[kf] == D else cols[ys[kf]]
    if ops[kl] == D:
        run = kl + 1 - max([k + 1 for k in range(kl) if ops[k] != D], default=0)
        end = cols[ys[kl]] - ins[ys[kl]] + run
    else:
        end = cols[ys[kl]] + 1
    return beg, end


def sound_msa(name, k):
    return own(name)["items"][k][0] == OKC


def test_msa_models_without_a_leak_are_msa_of():
    """The three models from a fresh state, on every sound record of every list in the own-targets layout: the widths, the run
    count, the row and the column interval are msa_of's."""
    for name, recs in RC.all_lists().items():
        w = own(name)
        runs = 0
        for k, r in enumerate(recs):
            if not sound_msa(name, k):
                continue
            tlen = len(r.text)
            widened, n = msa_walk(r.ops, 0)
            runs += n
            ins = ins_of(widened, tlen)
            assert ins == w["ins"][k], (name, k)
            row = w["blocks"][k][1]
            assert msa_place(r.ops, r.pattern, tlen, ins) == {c: int(b) for c, b in enumerate(row) if b != ord("-")}, (name, k)
            assert columns_of_item(r.ops, ins) == w["items"][k][4:6] and w["items"][k][3] == len(r.ops) - r.ops.count(b"I"), (name, k)
        assert runs == w["runs"], name


def test_leaked_msa_positions_move_the_bases():
    """cq / ct from A into B (width and emit kernels): B's row would be filled from where A's walk ended -- other bases at other
    columns, or none at all, its own sequences being as long as it needs."""
    n = 0
    for name, recs in RC.all_lists().items():
        w = own(name)
        found = []
        for k, (x, y) in enumerate(zip(recs, recs[1:])):
            if x.status != 0 or not x.ops or not sound_msa(name, k + 1) or not w["items"][k + 1][3]:
                continue
            cq, ct = consumed(x.ops)
            ins = w["ins"][k + 1]
            assert msa_place(y.ops, y.pattern, len(y.text), ins, cq, ct) != msa_place(y.ops, y.pattern, len(y.text), ins), (name, k)
            found.append((k, x, y))
        assert name == "zero" or (spread(found, 100) and len(found) > len(recs) // 2), (name, len(found))
        n += len(found)
    assert n >= 1000


def test_leaked_run_start_narrows_the_leading_run():
    """run0 from A into B: A's last column that is no 'D' lies far behind B's leading 'D' run, so the run's width comes out 0 or
    less and widen_slot drops it without any error -- the slot stays 0, the block is narrower, B's column interval ends earlier.
    (Its first column is 0 with and without the leak: a run at slot 0 begins the block.)"""
    n = 0
    for name in MSA_LISTS_D:
        recs = RC.all_lists()[name]
        w = own(name)
        found = instances(recs, "gap_tail", "gap_head")
        assert spread(found, 8), (name, len(found))
        for k, x, y in found:
            assert sound_msa(name, k + 1) and y.ops[:1] == b"D" and len(x.ops) >= 2
            run0 = max([c + 1 for c in range(len(x.ops)) if x.ops[c] != D], default=0)  # what run0 holds behind A
            first = op_runs(y.ops)[0][2]
            tlen = len(y.text)
            clean, leaked = ins_of(msa_walk(y.ops, 0)[0], tlen), ins_of(msa_walk(y.ops, 0, run0=run0)[0], tlen)
            assert clean == w["ins"][k + 1] and clean[0] == first > 0
            if run0 == 0:
                continue  # (A is one 'D' run: nothing to carry)
            assert leaked[0] == max(first - run0, 0) < clean[0], (name, k)
            assert run0 >= first or len(x.ops) < 40, (name, k)  # dropped altogether, silently
            if len(op_runs(y.ops)) == 1:
                continue  # (B is that run alone: its ends are the run's own)
            cb, ce = columns_of_item(y.ops, clean)
            lb, le = columns_of_item(y.ops, leaked)
            assert (cb, ce) == w["items"][k + 1][4:6] and cb == lb == 0 and le < ce and cols_of(leaked)[-1] < cols_of(clean)[-1], (name, k)
            n += 1
    assert n >= 16


def test_leaked_prev_d_counts_a_run_that_is_none():
    """prev_d from A into B: A ends in 'D' and B begins with another op on a 16-byte boundary (lane 0's byte 0 is then a column, and
    the bit before it is the carried one): B's first column would close a run of width 0 -- nothing widens, stats.runs is one more."""
    n = 0
    for name, recs in RC.all_lists().items():
        if name in ("zero", "norm-left", "norm-right"):
            continue
        seqs, pairs, results, arena = inputs(name)
        found = instances(recs, "all_gaps", "plain")
        assert spread(found), (name, len(found))
        for k, x, y in found:
            assert x.ops[-1:] == b"D" and y.ops[:1] in (b"M", b"X", b"I") and int(results[k + 1]["cigar_off"]) % 16 == 0, (name, k)
            if not sound_msa(name, k + 1):
                continue
            clean, leaked = msa_walk(y.ops, 0), msa_walk(y.ops, 0, prev_d=True)
            assert leaked[0] == clean[0] and leaked[1] == clean[1] + 1, (name, k)
            n += 1
    assert n >= 32
    for name, recs in RC.all_lists().items():  # and every other such adjacency lies on a boundary too
        results = inputs(name)[2]
        for k, (x, y) in enumerate(zip(recs, recs[1:])):
            if x.ops[-1:] == b"D" and y.ops and y.ops[:1] != b"D":
                assert int(results[k + 1]["cigar_off"]) % 16 == 0, (name, k)


# ---- lift.hip: models of the walk -----------------------------------------------------------------------------------------------

def lift_core(ops, frm, a, b, carried_end=0):
    """The two columns of lift_device.hpp for a whole forward item whose source begins at 0: the first aligned column whose source
    position is a or more (none: the string's length), and one past the last aligned column whose position is below b -- none: one
    past the last aligned column so far, last_a, which is 0 in a fresh wave."""
    src, s = [], 0
    for op in ops:
        src.append(s)
        s += op != (D if frm == RC.FROM_TARGET else I)
    aligned = [k for k in range(len(ops)) if ops[k] in b"MX"]
    return min([k for k in aligned if src[k] >= a], default=len(ops)), max([k + 1 for k in aligned if src[k] < b], default=carried_end)


def whole(r):
    return (0, len(r.pattern), 0, len(r.text))


def forward_query(r, q):
    """(a, b) of a query in the item's own coordinates."""
    _, frm, beg, end = q
    return (len(r.pattern) - end, len(r.pattern) - beg) if frm == RC.FROM_QUERY and r.rc else (beg, end)


def lift_clean(r, q):
    _, frm, beg, end = q
    return L.lift_of(r.ops, whole(r), "-" if r.rc else "+", frm, beg, end, len(r.pattern), status=r.status)


def test_the_lift_yardstick_is_the_restatement(hip_lib):
    """ffi.lift_one_host against lift_of on every query of the shorter records and of every eighth record, and on all of the
    key-0 list's."""
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        qs = queries(name)
        want = made(("lift", name), lambda: RC.lift_want(ffi, recs, qs, inputs(name)[0]))
        codes = set()
        for j, q in enumerate(qs):
            r = recs[q[0]]
            if len(r.ops) <= 400 or (q[0] % 8 == 0 and q[0]):
                assert tuple(int(want[j][f]) for f in L.FIELDS) == lift_clean(r, q), (name, q)
            codes.add(int(want[j]["code"]))
        assert codes >= ({L.OK, L.UNALIGNED} if name.startswith("norm") else {L.OK, L.SKIPPED, L.UNALIGNED} if name == "zero" else {L.OK, L.BAD_OP, L.LENGTHS, L.UNALIGNED}), (name, codes)


def test_leaked_lift_counts_change_the_result():
    """tm / tx / ti / td from A into B: B's prefixes, skips and consumed lengths would go on from A's totals -- its own sequences
    are as long as it needs, so the totals no longer fit them: the result of its whole-interval query loses its four counts."""
    n = 0
    for name, recs in RC.all_lists().items():
        qs = queries(name)
        found = []
        for k, x, y in queried_pairs(recs, qs):
            if x.status != 0 or not x.ops or y.status != 0 or not (len(y.ops) <= 1200 or k % 8 == 0):
                continue
            q = (k, RC.FROM_TARGET, 0, min(consumed(y.ops)[1], len(y.text)))  # the whole source interval: in the list too
            if q[3] == 0:
                continue  # (no text base: no query from the target)
            assert q in qs, (name, k)
            clean = lift_clean(y, q)
            if clean[0] != L.OK:
                continue
            cq, ct = consumed(x.ops)
            leaked = L.lift_of(y.ops, whole(y), "-" if y.rc else "+", RC.FROM_TARGET, 0, q[3], len(y.pattern), sl=(0, len(y.ops), cq, ct))
            assert sum(clean[9:13]) > 0 and leaked[9:13] != clean[9:13] and leaked != clean, (name, k)
            found.append((k, x, y))
        assert name == "zero" or (spread(found, 40)), (name, len(found))
        n += len(found)
    assert n >= 300


def test_leaked_last_aligned_column_turns_unaligned_into_a_lift():
    """last_a from A into B: a query that ends inside B's leading run of source-only columns has no aligned column before its end --
    UNALIGNED.  With A's last aligned column carried, its end would be that column, far behind its begin: a lift that is none."""
    n = 0
    for name in ("main-I", "main-D", "pass-I", "pass-D"):
        recs = RC.all_lists()[name]
        qs = queries(name)
        frm = RC.FROM_TARGET if name.endswith("I") else RC.FROM_QUERY
        g = name[-1].encode()
        found = []
        for k, x, y in queried_pairs(recs, qs):
            if y.kind != "gap_head":
                continue
            head = op_runs(y.ops)[0][2]
            assert y.ops[:1] == g and y.rc == 0
            q = (k, frm, 0, (head + 1) // 2)
            assert q in qs, (name, k)
            a_end = max([c + 1 for c in range(len(x.ops)) if x.ops[c] in b"MX"], default=0)  # what last_a.col holds behind A
            beg, end = lift_core(y.ops, frm, 0, q[3])
            clean = lift_clean(y, q)
            if clean[0] != L.UNALIGNED:
                continue  # (a stray byte, or a string that is one gap run)
            assert end == 0 and beg >= head
            lbeg, lend = lift_core(y.ops, frm, 0, q[3], carried_end=a_end)
            if a_end > beg:
                assert (lbeg, lend) == (beg, a_end) and lbeg < lend, (name, k)  # compose() makes an OK result of it
                found.append((k, x, y))
        assert spread(found), (name, len(found))
        n += len(found)
    assert n >= 20


def test_leaked_probe_cursor_leaves_the_next_record_unanswered(hip_lib):
    """pp from A into B behind a record with 200 queries: the cursors stand behind A's probes, which lie before B's, so B's walk
    would answer A's offsets again, or nothing, and B's queries would read answers nobody wrote for them -- zero prefixes make
    every one UNALIGNED.  B has queries that are OK."""
    from allwave_amd import ffi
    n = 0
    for name, recs in RC.all_lists().items():
        qs = queries(name)
        want = made(("lift", name), lambda: RC.lift_want(ffi, recs, qs, inputs(name)[0]))
        pairs = {a: b for a, b in zip(sorted({q[0] for q in qs}), sorted({q[0] for q in qs})[1:])}
        for k in RC.heavy_records(recs):
            b = pairs[k]
            if name == "zero":  # (behind its one heavy record comes a SKIPPED one, which reads no answer)
                assert all(int(want[j]["code"]) == L.SKIPPED for j, q in enumerate(qs) if q[0] == b)
                continue
            ok = [j for j, q in enumerate(qs) if q[0] == b and int(want[j]["code"]) == L.OK]
            assert len(ok) >= 4 and sum(1 for q in qs if q[0] == k) > 3 * 64 > sum(1 for q in qs if q[0] == b), (name, k, b)
            n += 1
    assert n >= 12


# ---- the share of sound records ---------------------------------------------------------------------------------------------------

def test_most_records_are_sound_under_both_passes(hip_lib):
    from allwave_amd import ffi
    for name, recs in RC.all_lists().items():
        seqs = inputs(name)[0]
        cs = RC.cs_want(ffi, "short", recs)[0]["code"]  # the rule both passes use: awvcs::whole_code
        w = own(name)
        codes = [i[0] for i in w["items"]]
        assert [int(c) for c in cs] == codes, name  # (the codes' numbers are the same: OK, SKIPPED, BAD_OP, LENGTHS)
        if name != "zero":
            assert 2 * codes.count(OKC) > len(recs), name
        s2, pairs, targets = RC.msa_layout(recs, seqs, True, name)
        shared = made(("shared", name), lambda: RC.msa_want(s2, targets, RC.msa_items(recs, pairs)))
        assert all(len(s2[t]) >= max(len(r.ops) for r in recs) for t in targets) and len(targets) == 3
        for k, (r, it) in enumerate(zip(recs, shared["items"])):
            stray = any(b not in b"MXID" for b in r.ops)
            # (an `overrun` string consumes more than its own query holds: LENGTHS in either layout -- the query is the record's own)
            want = M.SKIPPED if r.status != 0 else M.BAD_OP if stray else M.LENGTHS if consumed(r.ops)[0] > len(r.pattern) else M.OK
            assert it[0] == want and it[1] == k % 3 and (want != M.LENGTHS or r.kind == "overrun"), (name, k, r.kind)
        rows = [t[1] - 1 for t in shared["targets"]]
        assert name == "zero" or min(rows) >= 50, (name, rows)
        assert max(shared["ins"][0][:40]) >= 2 or name == "zero", name  # the leading slots are widened
        # the C yardstick on one target of each layout
        k = next(k for k in range(len(recs) - 1, -1, -1) if codes[k] == OKC and recs[k].ops.count(b"D") and len(recs[k].ops) >= 300)
        for want, s, j in ((w, 2 * k + 1, k), (shared, targets[0], 0)):
            set_, items = (seqs, RC.msa_items(recs, RC.msa_layout(recs, seqs, False)[1])) if want is w else (s2, RC.msa_items(recs, pairs))
            ins, width, hc, block = RC.msa_host_of(ffi, set_, s, items)
            assert list(ins) == want["ins"][j] and width == want["targets"][j][2] and np.array_equal(block, want["blocks"][j]), (name, s)
            assert list(hc) == [i[0] for i, it in zip(want["items"], items) if it[1] == s], (name, s)


# ---- the launch-geometry set ------------------------------------------------------------------------------------------------------

def test_geometry_set_reaches_the_tile_edges_and_the_second_trip():
    seqs, ranges, strings, items, targets = RC.geometry_set()
    assert [len(seqs[t]) + 1 for t in targets] == [1024, 1025, 2048, 2049, 16501] and max(len(s) for s in strings) <= 60
    w = M.msa_of(seqs, targets, items)
    assert all(i[0] == M.OK for i in w["items"]) and sum(r[2] for r in ranges.tolist()) >= len(items) // 3
    for j, t in enumerate(targets):
        length = len(seqs[t])
        ins = w["ins"][j]
        slots = RC.geometry_slots(length)
        assert {0, length - 1, length} <= set(slots) and [s for s in range(length + 1) if ins[s]] == slots, (t, slots)
        for s in slots:  # two items or more, of different widths: the slot holds the widest
            widths = sorted(it[3].count(b"D") for it in items if it[1] == t and it[4][2] + it[3].index(b"D") == s)
            assert len(widths) >= 2 and len(set(widths)) == len(widths) and ins[s] == widths[-1] >= 4, (t, s, widths)
        assert w["targets"][j][2] == length + sum(ins)
        # a run on both sides of every tile edge of the scan the target has, and one at its last slot
        for edge in range(1024, length + 1, 1024):
            if edge in RC.GEOMETRY_SLOTS:
                assert ins[edge - 1] and ins[edge], (t, edge)
    long_ = w["blocks"][4]
    assert len(seqs[4]) > 64 * 256 and {16383, 16384} <= set(RC.geometry_slots(len(seqs[4])))
    assert (long_[0, 16384 + sum(w["ins"][4][:16385]):] != ord("-")).sum() == len(seqs[4]) - 16384  # row 0's bases of the second trip
    assert any(i[5] > 16384 for i in w["items"])  # and items that end behind it
