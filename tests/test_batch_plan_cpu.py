"""CPU test of the routing rules of an aligning call (allwave_amd/csrc/batch_plan.hpp): a stand-alone driver,
built with the system C++ compiler under AddressSanitizer and UBSan, prints the plan the header makes of penalty sets and of
lists of lengths.  Its output is checked against the rules restated here -- penalty_space.derive, carve(), order(), groups(),
rows() -- and against the properties the engine relies on.  Only lengths are needed, so 500-Mbp "sequences" cost nothing.

About the LDS property: the sequence staging never pushes a workgroup's dynamic LDS past its share of the CU (dyn <= budget
whenever anything is staged); the ring metadata alone may exceed the share (ring 256, one wave per pair) and then nothing is
staged."""
import os
import re
import shutil
import subprocess

import pytest

import penalty_space as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# allwave_amd/csrc/biwfa_device.hpp (test_limits_mirror_the_device_header)
COL_PAD, WAVES_PER_SIMD, STATIC_LDS_RESERVE, STACK_CAP = 576, 4, 1024, 48
EV_STACK_WORDS, EV_TWIN_WORDS = (STACK_CAP * 32 + 3) // 4 + 16, ps.MAX_SCOPE * ps.NCOMP
ROW_META, ROW_META16, BREAKPOINT = 8, 4, 32
LIMITS = (ps.TMAX, ps.TMAX32, ps.CHAIN_MAX, ps.MAX_RING, ps.MAX_SCOPE, ps.NCOMP, COL_PAD, ps.FALLBACK_MIN_SCORE, ps.FALLBACK_MIN_LENGTH,
          WAVES_PER_SIMD, STATIC_LDS_RESERVE, EV_STACK_WORDS, EV_TWIN_WORDS, ROW_META, ROW_META16, BREAKPOINT)
F_FORCE_INT32, F_NO_PACKED_SEQ, F_ONE_WAVE, F_FOUR_WAVES, F_NO_WIDE16 = 2, 4, 8, 16, 256
AWV_ERR_PENALTIES = -4
NG = 9
NUM_CUS = 2   # thresholds of 8, 16 and 32 pairs: tiny lists reach them


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "allwave_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "batch_plan_driver.cpp"), "-o", exe])
    return exe


def run(driver, lines):
    text = "limits " + " ".join(str(v) for v in LIMITS) + "\n" + "".join(ln + "\n" for ln in lines)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def lens_text(lens):
    return "%d %s" % (len(lens), " ".join("%d %d" % l for l in lens))


def pen_text(scores, flags=0):
    s = list(scores) + ([0, 0, 0] if len(scores) == 4 else [1])
    return "%d %s" % (flags, " ".join(str(v) for v in s))


def test_limits_mirror_the_device_header():
    text = open(os.path.join(ROOT, "allwave_amd", "csrc", "biwfa_device.hpp")).read()

    def const(name):
        m = re.search(r"constexpr int %s = (\d+);" % name, text) or re.search(r"#define AWV_%s (\d+)" % name, text)
        return int(m.group(1))
    for name, v in (("TMAX", ps.TMAX), ("TMAX32", ps.TMAX32), ("CHAIN_MAX", ps.CHAIN_MAX), ("MAX_RING", ps.MAX_RING), ("MAX_SCOPE", ps.MAX_SCOPE),
                    ("NCOMP", ps.NCOMP), ("COL_PAD", COL_PAD), ("FALLBACK_MIN_SCORE", ps.FALLBACK_MIN_SCORE),
                    ("FALLBACK_MIN_LENGTH", ps.FALLBACK_MIN_LENGTH), ("WAVES_PER_SIMD", WAVES_PER_SIMD),
                    ("STATIC_LDS_RESERVE", STATIC_LDS_RESERVE), ("STACK_CAP", STACK_CAP)):
        assert const(name) == v, name
    assert "EV_STACK_WORDS = (STACK_CAP * 32 + 3) / 4 + 16;" in text and "EV_TWIN_WORDS = MAX_SCOPE * NCOMP;" in text
    assert "struct RowMeta { int lo, hi; };" in text and "RowMeta16 { int16_t lo, hi; };" in text
    assert "struct Breakpoint { int score, sf, sr, kf, kr, off_f, off_r, comp; };" in text


# ---- penalties ----
def test_penalty_plan_equals_derive(driver):
    cases = [(name, s, fl) for name, s in ps.PENALTY_SPACE for fl in (0, ps.AWV_F_SINGLE_STEP, ps.AWV_F_NO_CHAIN)]
    out = run(driver, ["pen " + pen_text(s, fl) for _, s, fl in cases])
    assert len(out) == len(cases)
    seen = set()
    for (name, s, fl), ln in zip(cases, out):
        f = ln.split(None, 15)
        code, late, two, x, o1, e1, o2, e2, scope, multi_T, chain, ring, sb, wb = (int(v) for v in f[1:15])
        d = ps.derive(s, fl)
        assert (code == 0) == d.accepted, (name, fl, ln)
        if d.reason in ("match != 0", "need x > 0, o >= 0, e > 0", "need o2 >= 0, e2 > 0"):   # the sign rules: nothing is derived
            assert code == AWV_ERR_PENALTIES and not late and (d.reason.split()[0] in f[15] or d.reason in f[15]), (name, ln)
            seen.add("signs" if d.reason != "match != 0" else "match")
            continue
        assert (bool(two), x, o1, e1, o2, e2, scope) == (d.two_piece, d.x, d.o1, d.e1, d.o2, d.e2, d.scope), (name, fl, ln)
        if d.reason == "scope":
            assert code == AWV_ERR_PENALTIES and not late and scope == 127, (name, ln)
            seen.add("scope")
            continue
        assert (multi_T, chain, ring, sb) == (d.multi_T, d.chain_max, d.ring, d.sb), (name, fl, ln)
        if d.reason == "sb":
            assert code == AWV_ERR_PENALTIES and late and sb > ps.MAX_SB, (name, ln)   # (reported after the call's pairs are checked)
            seen.add("sb")
            continue
        assert wb == (2 * sb + 9 + 2 * COL_PAD + 63) // 64 * 64 and f[15] == "-", (name, ln)
        if tuple(s) == (0, 5, 121, 1) and fl == 0:
            assert ring == 256
            seen.add("ring256")
    assert seen == {"signs", "match", "scope", "sb", "ring256"}


# ---- carving ----
def carve(lens, max_batch, max_arena, score_only):
    out, first = [], 0
    while first < len(lens):
        arena, offs = 0, []
        while first + len(offs) < len(lens) and len(offs) < max_batch:
            ql, tl = lens[first + len(offs)]
            need = 0 if score_only else (ql + tl + 7) // 8 * 8
            if offs and arena + need > max_arena:
                break
            offs.append(arena)
            arena += need
        out.append((first, len(offs), arena, offs))
        first += len(offs)
    return out


CARVE_LENS = (0, 1, 7, 8, 9, 100, 32759, 32760)


def test_carving(driver):
    lens = [(a, b) for a in CARVE_LENS for b in CARVE_LENS]   # 64 pairs, every combination
    cases = [(mb, ma, so) for mb in (1, 3, 1 << 20) for ma in (8, 64, 1 << 33) for so in (0, 1)]
    out = iter(run(driver, ["carve %d %d %d %s" % (mb, ma, so, lens_text(lens)) for mb, ma, so in cases]))
    shapes = set()
    for mb, ma, so in cases:
        got = []
        for ln in out:
            if ln == "end":
                break
            f = ln.split()
            ents = [tuple(int(v) for v in e.split(":")) for e in f[4:]]
            got.append((int(f[1]), int(f[2]), int(f[3]), ents))
        assert [(a, n, ar, [e[0] for e in ents]) for a, n, ar, ents in got] == carve(lens, mb, ma, so), (mb, ma, so)
        at = 0
        for first, n, arena, ents in got:
            assert first == at and 1 <= n <= mb and len(ents) == n   # the batches partition the list in order
            run_off = 0
            for k, (off, bi, ql, tl) in enumerate(ents):
                assert (bi, ql, tl) == (k, *lens[first + k]) and off == run_off and off % 8 == 0   # cumulative, 8-aligned
                run_off += 0 if so else (ql + tl + 7) // 8 * 8
            assert arena == run_off and (arena <= ma or n == 1) and (not so or arena == 0)
            shapes.add((n == 1 and arena > ma, n > 1))
            at += n
        assert at == len(lens)
    assert shapes == {(True, False), (False, False), (False, True)}


# ---- dispatch order ----
def cost(ql, tl):
    return ql + tl + 4 * abs(ql - tl)


def order(lens):
    c = [cost(*l) for l in lens]
    if len(set(c)) <= 1:
        return list(range(len(lens))), False
    o = sorted(range(len(lens)), key=lambda i: -c[i])   # (stable)
    return o, c[o[0]] >= 3 * c[o[len(o) // 2]]


def test_dispatch_order(driver):
    med = (100, 100)    # cost 200: the median of each skew list
    cases = {
        "uniform": [(100, 100), (75, 85), (85, 75), (50, 70)],                 # all of cost 200, lengths differ
        "ties": [(10, 10), (100, 100), (50, 50), (98, 90), (50, 50), (90, 98), (500000000, 1)],
        "skew_at": [med, (300, 300), med, (5, 5), (7, 7)],                     # 600 = 3 x 200
        "skew_below": [med, (297, 298), med, (5, 5), (7, 7)],                  # 595 + 4 x 1 = 599
        "one": [(5, 9)],
        "empty": [],
    }
    out = run(driver, ["order " + lens_text(l) for l in cases.values()])
    res = {}
    for (name, lens), ln in zip(cases.items(), out):
        f = [int(v) for v in ln.split()[1:]]
        res[name] = (f[1:], bool(f[0]))
        assert res[name] == order(lens), name
        assert sorted(f[1:]) == list(range(len(lens)))
    assert res["uniform"] == ([0, 1, 2, 3], False)                             # identity order
    assert res["ties"][0] == [6, 3, 5, 1, 2, 4, 0]                             # equal costs keep caller order
    assert cost(300, 300) == 3 * cost(*med) and res["skew_at"][1] and cost(297, 298) == 3 * cost(*med) - 1 and not res["skew_below"][1]


# ---- groups ----
def groups(lens, flags, num_cus, skewed):
    n = len(lens)
    never_wide = bool(flags & F_ONE_WAVE)
    all_wide = not never_wide and (bool(flags & F_FOUR_WAVES) or n <= WAVES_PER_SIMD * num_cus or (skewed and n <= 4 * WAVES_PER_SIMD * num_cus))
    n_huge = sum(abs(a - b) >= 16384 for a, b in lens)
    use_sixteen = not never_wide and not flags & F_FOUR_WAVES and 0 < n_huge <= num_cus
    fl = []
    for a, b in lens:
        f = 1 if all_wide or (not never_wide and (abs(a - b) >= 4096 or max(a, b) >= 32760)) else 0
        if use_sixteen and abs(a - b) >= 16384:
            f = 2
        fl.append(f)
    ones = [i for i, f in enumerate(fl) if f == 0]
    if not never_wide and ones and fl.count(1) and len(ones) <= (WAVES_PER_SIMD * 256 // 64) * num_cus:
        if 2 * cost(*lens[ones[0]]) >= 3 * cost(*lens[ones[len(ones) // 2]]):
            fl = [1 if f == 0 else f for f in fl]
    g = []
    for (a, b), f in zip(lens, fl):
        w = 1 if flags & F_FORCE_INT32 or max(a, b) >= 32760 else 0
        if w == 1 and not flags & F_FORCE_INT32 and not flags & F_NO_WIDE16 and f >= 1 and min(a, b) < 32760:
            w = 2
        g.append(f * 3 + w)
    return g, demand_of(g, lens, num_cus)


def demand_of(g, lens, num_cus):
    d = []
    for k in range(NG):
        mem = [a + b for (a, b), gi in zip(lens, g) if gi == k]
        slots = min((WAVES_PER_SIMD * 256 // (64 * (1, 4, 16)[k // 3])) * num_cus, len(mem))
        d.append(slots * max(mem) * (4 if k % 3 == 1 else 2) if mem else 0)
    return d


def group_cases():
    small, S = (1000, 1000), 39
    c = {}
    for n in (8, 9, 16, 17, 32, 33):
        c["n%d" % n] = ([small] * n, 0, False)
        c["n%d_skewed" % n] = ([(3000, 3000)] + [small] * (n - 1), 0, True)
    for d in (4095, 4096):
        c["delta%d" % d] = ([(5000 + d, 5000)] + [small] * S, 0, False)
    for d in (16383, 16384):
        c["delta%d" % d] = ([(616 + d, 616)] + [small] * S, 0, False)
    for a, b in ((32759, 32759), (32760, 32759), (32760, 32760), (40000, 32759), (500000000, 32760), (500000000, 20)):
        for fl in (0, F_NO_WIDE16, F_FORCE_INT32, F_ONE_WAVE, F_FOUR_WAVES):
            c["len%d_%d_f%d" % (a, b, fl)] = ([(a, b)] + [small] * S, fl, False)
    # the median rule: eleven pairs, one four-wave; the one-wave pairs' first against their median (the sixth of ten)
    c["median_at"] = ([(9096, 5000), (1500, 1500)] + [small] * 9, 0, False)       # 2 x 3000 = 3 x 2000
    c["median_below"] = ([(9096, 5000), (1499, 1500)] + [(1000, 1001)] * 9, 0, False)   # 2 x 3003 = 6006 < 3 x 2005
    c["median_many"] = ([(9096, 5000), (1500, 1500)] + [small] * 32, 0, False)    # 33 one-wave pairs: more than fill the machine
    for k in (NUM_CUS, NUM_CUS + 1):
        c["huge%d" % k] = ([(20000, 100)] * k + [small] * S, 0, False)
        c["huge%d_four" % k] = ([(20000, 100)] * k + [small] * S, F_FOUR_WAVES, False)
    c["empty"] = ([], 0, False)
    return c


def test_groups(driver):
    cases = group_cases()
    out = run(driver, ["groups %d %d %d %s" % (fl, NUM_CUS, sk, lens_text(lens)) for lens, fl, sk in cases.values()])
    res = {}
    for (name, (lens, fl, sk)), ln in zip(cases.items(), out):
        a, b, c = ln[len("groups"):].split("|")
        g, dorder = [int(v) for v in a.split()], [int(v) for v in b.split()]
        counts = [tuple(int(v) for v in e.split(":")) for e in c.split()]
        want, demand = groups(lens, fl, NUM_CUS, sk)
        assert g == want, name
        # every pair lands in exactly one group; the demand order covers every group, descending
        assert len(g) == len(lens) and all(0 <= k < NG for k in g) and [n for n, _ in counts] == [g.count(k) for k in range(NG)], name
        assert sorted(dorder) == list(range(NG)) and dorder == sorted(range(NG), key=lambda k: -demand[k]), name
        assert all(demand[x] >= demand[y] for x, y in zip(dorder, dorder[1:])), name
        res[name] = g
    first = {k: v[0] if v else None for k, v in res.items()}
    assert set(res["n8"]) == {3} and set(res["n9"]) == {0} and set(res["n32"]) == {0}
    assert set(res["n32_skewed"]) == {3} and set(res["n33_skewed"]) == {0} and set(res["n9_skewed"]) == {3}
    assert (first["delta4095"], first["delta4096"], first["delta16383"], first["delta16384"]) == (0, 3, 3, 6)
    assert set(res["delta4096"][1:]) == {0}
    assert [first["len%d_%d_f0" % ab] for ab in ((32759, 32759), (32760, 32759), (32760, 32760), (40000, 32759))] == [0, 5, 4, 5]
    assert first["len500000000_32760_f0"] == 7 and first["len500000000_20_f0"] == 8
    assert first["len32760_32759_f%d" % F_NO_WIDE16] == 4 and first["len32760_32759_f%d" % F_FORCE_INT32] == 4
    assert set(res["len32759_32759_f%d" % F_FORCE_INT32]) == {1} and first["len32760_32759_f%d" % F_ONE_WAVE] == 1
    assert set(res["len500000000_20_f%d" % F_ONE_WAVE]) <= {0, 1} and set(res["len32759_32759_f%d" % F_FOUR_WAVES]) == {3}
    assert set(res["median_at"]) == {3} and res["median_below"] == [3] + [0] * 10 and res["median_many"] == [3] + [0] * 33
    assert res["huge2"][:2] == [6, 6] and res["huge3"][:3] == [3, 3, 3] and res["huge2_four"][:2] == [3, 3]


# ---- rows ----
def rows(lens, flags, num_cus, workgroups, max_scratch, first_row_cols, twin_ok, waves, width, d):
    esz = 4 if width == 1 else 2
    wc_2g = (2 ** 31 - 1) // (2 * ps.NCOMP * d.ring * esz) // 256 * 256
    span = 2 * ((wc_2g - 2 * COL_PAD - 9 - 256) // 2) + 2 * COL_PAD
    mask = [a > 0 and b > 0 and abs(a - b) > span for a, b in lens]
    kept = [l for l, m in zip(lens, mask) if not m]
    wg = 64 * waves
    nslots_g = max(1, workgroups // waves) if workgroups > 0 else (WAVES_PER_SIMD * 256 // wg) * num_cus
    maxsum, maxlen = max([a + b for a, b in kept] + [0]), max([max(l) for l in kept] + [0])
    maxdelta = max([abs(a - b) for a, b in kept] + [0])
    wcap_full = (maxsum + 9 + 256 + 2 * COL_PAD + 255) // 256 * 256
    want = min(nslots_g, len(kept))
    twin = bool(twin_ok) and waves == 1 and width == 0
    ev_extra = EV_STACK_WORDS + (EV_TWIN_WORDS if twin else 0)
    lds_meta = (2 * ps.NCOMP * d.ring * (ROW_META16 if width == 0 else ROW_META) + 4 * d.ring * 4 + d.scope * ps.NCOMP * 4 +
                (BREAKPOINT if twin else 0) + 15) // 16 * 16
    seq_need = (((maxlen + 15) // 16 + 2) * 2 + 10) * 4
    lds_budget = 160 * 1024 // (WAVES_PER_SIMD * 256 // wg) - STATIC_LDS_RESERVE
    lds_seq = 0 if flags & F_NO_PACKED_SEQ or lds_meta >= lds_budget else min(seq_need, lds_budget - lds_meta)
    lds_seq = lds_seq // 16 * 16
    wb = (2 * d.sb + 9 + 2 * COL_PAD + 63) // 64 * 64
    hist_rows = ((d.sb + 1) * ps.NCOMP * wb * esz + 63) // 64 * 64
    hist_stride = hist_rows + ((d.sb + 1) * ps.NCOMP * ROW_META + 63) // 64 * 64
    budget = max_scratch if max_scratch > 0 else 160 << 30

    def per_slot(wc):
        return 2 * ps.NCOMP * d.ring * wc * esz + hist_stride + (wc + ev_extra) * 4
    wcap = min(wcap_full, max(8192, (wcap_full // 2 + 255) // 256 * 256, (2 * maxdelta + 4096 + 255) // 256 * 256))
    if per_slot(wcap) * want > budget:
        fixed, per_col, share = hist_stride + ev_extra * 4, 2 * ps.NCOMP * d.ring * esz + 4, budget // want
        wc = (share - fixed) // per_col if share > fixed else 0
        wcap = min(wcap, max(wc // 256 * 256, 8192))
    if first_row_cols > 0:
        wcap = min(wcap, max(2048, (first_row_cols + 255) // 256 * 256))
    wcap = min(wcap, wc_2g)
    wc_last = min(wcap_full, wc_2g)
    attempts, wc = [], wcap
    while True:
        attempts.append((wc, min(want, max(1, budget // per_slot(wc))), per_slot(wc), 2 * ps.NCOMP * d.ring * wc * esz, wc + ev_extra))
        if wc >= wc_last:
            break
        wc = min(wc_last, 4 * wc)
    return dict(wc_2g=wc_2g, span=span, mask=mask, waves=waves, wg=wg, esz=esz, nslots_g=nslots_g, wcap_full=wcap_full, wcap=wcap, wc_last=wc_last,
                twin=twin, ev_extra=ev_extra, lds_meta=lds_meta, lds_seq=lds_seq, dyn_lds=lds_meta + lds_seq, lds_budget=lds_budget,
                hist_rows=hist_rows, hist_stride=hist_stride, budget=budget, attempts=attempts)


RING64, RING128, RING256 = (0, 5, 8, 2, 24, 1), (0, 3, 90, 1), (0, 5, 121, 1)
SPAN16_64 = 2 * ((1677568 - 2 * COL_PAD - 9 - 256) // 2) + 2 * COL_PAD


def row_cases():
    # name -> (lens, flags, workgroups, max_scratch, first_row_cols, twin_ok, waves, width, scores)
    c = {}
    for ring, s in ((64, RING64), (128, RING128), (256, RING256)):
        for waves, width in ((1, 0), (1, 1), (4, 0), (4, 1), (4, 2), (16, 0), (16, 1), (16, 2)):
            for twin_ok in (0, 1):
                c["r%d_w%d_x%d_t%d" % (ring, waves, width, twin_ok)] = ([(30000, 29000)] * 40 + [(7, 9), (0, 5)], 0, 0, 0, 0, twin_ok, waves, width, s)
    c["filter"] = ([(10, 10 + SPAN16_64), (10, 11 + SPAN16_64), (11 + SPAN16_64, 10), (0, 500000000), (500000000, 0), (500000000, 500000000)],
                   0, 0, 0, 0, 0, 4, 0, RING64)
    c["all_filtered"] = ([(1, 400000000)] * 3, 0, 0, 0, 0, 0, 16, 2, RING64)
    for frc in (1, 2048, 2049, 2304, 100000):
        c["first_row_cols%d" % frc] = ([(30000, 30000)] * 5, 0, 0, 0, frc, 1, 1, 0, RING64)
    c["small_scratch"] = ([(30000, 30000)] * 40, 0, 0, 1 << 20, 0, 1, 1, 0, RING64)
    c["mid_scratch"] = ([(30000, 30000)] * 40, 0, 0, 3 << 30, 0, 1, 1, 0, RING64)
    c["wide_rerun"] = ([(300000000, 299500000), (5, 5)], 0, 0, 0, 0, 0, 16, 1, RING64)     # re-runs stop at the 2 GiB limit
    c["workgroups"] = ([(5000, 5000)] * 40, 0, 10, 0, 0, 0, 4, 0, RING64)
    c["workgroups_few"] = ([(5000, 5000)] * 40, 0, 3, 0, 0, 0, 16, 0, RING64)
    c["no_packed"] = ([(5000, 5000)] * 40, F_NO_PACKED_SEQ, 0, 0, 0, 0, 1, 0, RING64)
    c["short"] = ([(50, 60)] * 3, 0, 0, 0, 0, 1, 1, 0, RING64)
    return c


def test_rows(driver):
    cases = row_cases()
    out = run(driver, ["rows %d %d %d %d %d %d %d %d %s %s" % (fl, NUM_CUS, wgs, ms, frc, tw, waves, width, pen_text(s), lens_text(lens))
                       for lens, fl, wgs, ms, frc, tw, waves, width, s in cases.values()])
    keys = ("waves wg esz wc_2g nslots_g wcap_full wcap wc_last twin ev_extra lds_meta lds_seq dyn_lds lds_budget hist_rows hist_stride budget").split()
    res = {}
    for (name, (lens, fl, wgs, ms, frc, tw, waves, width, s)), ln in zip(cases.items(), out):
        head, tail = ln.split("|")
        f = head.split()
        got = dict(zip(keys, (int(v) for v in f[4:])), span=int(f[2]), mask=[ch == "1" for ch in f[3]],
                   attempts=[tuple(int(v) for v in a.split(":")) for a in tail.split()])
        assert int(f[1]) == got["wc_2g"]
        got["twin"] = bool(got["twin"])
        assert got == rows(lens, fl, NUM_CUS, wgs, ms, frc, tw, waves, width, ps.derive(s)), name
        res[name] = got
        # the re-run sequence ends at wc_last and never exceeds the 2 GiB limit; a row's ring stays below 2 GiB
        wcs = [a[0] for a in got["attempts"]]
        assert wcs[0] == got["wcap"] and wcs[-1] == got["wc_last"] and all(w <= got["wc_2g"] for w in wcs), name
        assert all(b == min(got["wc_last"], 4 * a) for a, b in zip(wcs, wcs[1:])) and all(a[3] < 2 ** 31 for a in got["attempts"]), name
        # arenas inside the scratch budget whenever more than one workgroup runs
        kept = got["mask"].count(False)   # (the engine plans no rows for a group the pre-filter emptied)
        assert all(slots >= min(1, kept) and (slots <= 1 or slots * per <= got["budget"]) for _, slots, per, _, _ in got["attempts"]), name
        assert got["lds_meta"] % 16 == 0 and got["lds_seq"] % 16 == 0 and got["dyn_lds"] == got["lds_meta"] + got["lds_seq"], name
        assert got["dyn_lds"] <= got["lds_budget"] or got["lds_seq"] == 0, name
        if ps.derive(s).ring == 64:
            assert got["dyn_lds"] <= got["lds_budget"], name
    # the five limits the source comment states
    assert [res["r%d_w4_x1_t0" % r]["wc_2g"] for r in (64, 128, 256)] == [838656, 419328, 209664]
    assert [res["r%d_w4_x0_t0" % r]["wc_2g"] for r in (64, 128)] == [1677568, 838656]
    assert res["r64_w4_x2_t0"]["wc_2g"] == 1677568
    # the pre-filter: CAPACITY exactly beyond the span; empty sequences are exempt
    assert res["filter"]["span"] == SPAN16_64 and res["filter"]["mask"] == [False, True, True, False, False, False]
    assert res["all_filtered"]["mask"] == [True] * 3
    assert [res["first_row_cols%d" % v]["wcap"] for v in (1, 2048, 2049, 2304)] == [2048, 2048, 2304, 2304]
    assert res["first_row_cols100000"]["wcap"] == res["r64_w1_x0_t1"]["wcap"] or res["first_row_cols100000"]["wcap"] < 100000
    # a small budget keeps rows of 8192 columns and sheds workgroups instead
    assert res["small_scratch"]["wcap"] == 8192 and res["small_scratch"]["attempts"][0][1] == 1
    assert res["mid_scratch"]["wcap"] >= 8192 and 1 < res["mid_scratch"]["attempts"][0][1] <= 32
    assert res["wide_rerun"]["wc_last"] == 838656 < res["wide_rerun"]["wcap_full"] and len(res["wide_rerun"]["attempts"]) == 1
    assert res["workgroups"]["nslots_g"] == 2 and res["workgroups_few"]["nslots_g"] == 1 and res["r64_w16_x0_t0"]["nslots_g"] == 2
    assert res["no_packed"]["lds_seq"] == 0 and res["short"]["lds_seq"] > 0
    # twin groups (one wave, 16-bit rows, twin units allowed) add exactly the twin record and the twin event words
    for ring in (64, 128, 256):
        for waves, width in ((1, 0), (1, 1), (4, 0), (4, 2), (16, 1)):
            a, b = res["r%d_w%d_x%d_t0" % (ring, waves, width)], res["r%d_w%d_x%d_t1" % (ring, waves, width)]
            if (waves, width) == (1, 0):
                assert b["twin"] and not a["twin"]
                assert b["lds_meta"] - a["lds_meta"] == BREAKPOINT and b["ev_extra"] - a["ev_extra"] == EV_TWIN_WORDS
                assert all(y[4] - x[4] == EV_TWIN_WORDS for x, y in zip(a["attempts"], b["attempts"]))
            else:
                assert a == b
