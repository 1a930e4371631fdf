"""GPU tests (-m gpu) of twin units: an entry (q, t) of a pair list and its swapped entry (t, q) are aligned as one unit that
shares their breakpoint searches (in the one-wave kernels with 16-bit rows -- under AWV_F_FOUR_WAVES or
AWV_F_FORCE_INT32 no unit is formed and the same comparisons must still hold).  Every case compares every result field and every CIGAR byte three ways:
the default path, AWV_F_NO_TWIN (every entry on its own: the path as it was) and the CPU oracle."""
import random

import pytest

import repeats as R
import twin_cases as TC
from util import DEFAULT_2P, PENALTY_SETS, check_against_oracle

pytestmark = pytest.mark.gpu

_SWAP = TC.SWAP
rc, same_records, oracle_records, check_records = TC.rc, TC.same_records, TC.oracle_records, TC.check_records


@pytest.fixture(scope="module")
def engines(hip_lib):
    """One engine per kernel flavour x row width x sharing depth, and per flavour x row width with AWV_F_NO_TWIN."""
    from allwave_amd import ffi
    made = {}

    def get(waves, width, twin):
        key = (waves, width, twin)
        if key not in made:
            made[key] = ffi.Engine(flags=waves | width | {"all": 0, "top": ffi.AWV_F_TWIN_TOP_ONLY, "off": ffi.AWV_F_NO_TWIN}[twin])
        return made[key]

    yield get
    for e in made.values():
        e.close()


def variants():
    from allwave_amd import ffi
    return [(w, b) for w in (ffi.AWV_F_ONE_WAVE, ffi.AWV_F_FOUR_WAVES) for b in (0, ffi.AWV_F_FORCE_INT32)]


def forms_twins(waves, width):
    """Twin units are built into the one-wave kernel with 16-bit rows only (the multi-wave kernels with them
    faulted on the GPU and went back to the code they had; the one-wave 32-bit search grew scratch reloads in its step code
    and was left as it was).  For the other three variants the comparisons below therefore only show that nothing changed:
    they must form no unit and return the same bytes.  When units come back there, the asserts on 66 units and on shared
    searches below the top level apply to them again as the issue states them."""
    from allwave_amd import ffi
    return waves == ffi.AWV_F_ONE_WAVE and width == 0


@pytest.fixture(scope="module")
def twelve():
    """twin_cases.twelve: 66 twin units and one single entry."""
    return TC.twelve()


@pytest.mark.parametrize("scores", PENALTY_SETS)
def test_all_directed_pairs(engines, oracle, twelve, scores):
    """The oracle is run once per penalty set (util.check_against_oracle, on the default path under one wave per pair);
    every other variant, AWV_F_NO_TWIN included, must return the same records and bytes as that run."""
    from allwave_amd import ffi
    seqs, pairs = twelve
    first = engines(ffi.AWV_F_ONE_WAVE, 0, "all")
    check_against_oracle(first, oracle, seqs, pairs, scores)
    ref = first.align_pairs(scores, pairs)
    assert [len(c) for c in ref[1]] == list(ref[0]["cigar_len"])
    for waves, width in variants():
        off = engines(waves, width, "off")
        off.set_sequences(seqs)
        same_records(off.align_pairs(scores, pairs), ref)
        assert off.twin_stats() == (0, 0, 0, 0)
        for depth in ("top", "all"):
            e = engines(waves, width, depth)
            e.set_sequences(seqs)
            got = e.align_pairs(scores, pairs)
            units, shared, solo, nonmirror = e.twin_stats()
            print("%s waves %d width %d %s: units %d shared %d per-orientation %d non-mirror %d" %
                  (scores, waves, width, depth, units, shared, solo, nonmirror))
            same_records(got, ref)
            if not forms_twins(waves, width):
                assert (units, shared, solo, nonmirror) == (0, 0, 0, 0)
                continue
            assert units == 66
            if depth == "top":
                assert 0 < shared <= 66
            else:
                assert shared > 66, "no search below the top level ran shared"
            st = e.stats()
            assert st.pairs_completed == 133 and st.aligned_bp == sum(len(seqs[a]) for a, _ in pairs)


def repeat_pairs():
    """Microsatellites, tandem arrays and homopolymer ends: many optimal alignments, so ties decide the CIGAR and the two
    orientations of a pair often break them differently."""
    rng = random.Random("twin-repeats/8")  # (seed chosen for the condition the test checks: 7 of the 20 pairs)
    ab = [R.microsatellite(rng) for _ in range(8)] + [R.tandem(rng, total=(1500, 4000)) for _ in range(3)]
    ab += [R.end_runs(rng) for _ in range(9)]
    seqs, pairs = [], []
    for a, b in ab:
        seqs += [a, b]
        pairs += [(len(seqs) - 2, len(seqs) - 1), (len(seqs) - 1, len(seqs) - 2)]
    return seqs, pairs


def test_repeat_rich_pairs_break_ties_per_orientation(engines, oracle):
    from allwave_amd import ffi
    seqs, pairs = repeat_pairs()
    want = oracle_records(oracle, seqs, pairs, DEFAULT_2P)
    # the condition on the inputs, from the oracle alone: for at least a quarter of the unordered pairs the CIGAR of (j, i)
    # is not the I/D swap of the CIGAR of (i, j)
    differ = sum(1 for k in range(0, len(pairs), 2) if want[k + 1][1] != want[k][1].translate(_SWAP))
    print("%d of %d unordered pairs: the swapped pair's CIGAR is not the I/D swap" % (differ, len(pairs) // 2))
    assert 4 * differ >= len(pairs) // 2
    nonmirror_seen = 0
    for waves, width in variants():
        off = engines(waves, width, "off")
        off.set_sequences(seqs)
        plain = off.align_pairs(DEFAULT_2P, pairs)
        check_records(plain, want, seqs, pairs)
        for depth in ("top", "all"):
            e = engines(waves, width, depth)
            e.set_sequences(seqs)
            got = e.align_pairs(DEFAULT_2P, pairs)
            units, shared, solo, nonmirror = e.twin_stats()
            print("waves %d width %d %s: units %d shared %d per-orientation %d non-mirror %d" % (waves, width, depth, units, shared, solo, nonmirror))
            same_records(got, plain)
            check_records(got, want, seqs, pairs)
            if not forms_twins(waves, width):
                assert (units, shared, solo, nonmirror) == (0, 0, 0, 0)
                continue
            assert units == len(pairs) // 2
            if depth == "all":
                assert nonmirror >= 1, "no shared search found two different breakpoints"
                nonmirror_seen += nonmirror
    check_against_oracle(engines(ffi.AWV_F_ONE_WAVE, 0, "all"), oracle, seqs, pairs, DEFAULT_2P)
    assert nonmirror_seen > 0


@pytest.mark.parametrize("scores", [DEFAULT_2P, (0, 4, 6, 2)])
def test_pairing_list(engines, oracle, scores):
    """Missing twins, (i, i), duplicates, q_revcomp entries, an empty sequence, identical sequences, pairs of <= 100 bases."""
    seqs, pairs = TC.pairing_sequences(), TC.PAIRING_LIST
    want = oracle_records(oracle, seqs, pairs, scores)
    qt = [(rc(seqs[q]) if r else seqs[q], seqs[t]) for q, t, r in pairs]
    flat = [s for ab in qt for s in ab]
    for waves, width in variants():
        off = engines(waves, width, "off")
        off.set_sequences(seqs)
        plain = off.align_pairs(scores, pairs)
        for depth in ("top", "all"):
            e = engines(waves, width, depth)
            e.set_sequences(seqs)
            got = e.align_pairs(scores, pairs)
            same_records(got, plain)
            check_records(got, want, flat, [(2 * i, 2 * i + 1) for i in range(len(pairs))])
            assert e.twin_stats()[0] == (8 if forms_twins(waves, width) else 0)
            assert e.stats().pairs_completed == len(pairs)


def test_other_entry_points_are_unchanged(engines, twelve):
    """The bounded and the range entry points never form twin units; an unbounded awv_score_pairs does (one top-level search
    gives both entries their penalty).  All of them: same answers as under AWV_F_NO_TWIN."""
    from allwave_amd import ffi
    seqs, pairs = twelve
    on, off = engines(ffi.AWV_F_ONE_WAVE, 0, "all"), engines(ffi.AWV_F_ONE_WAVE, 0, "off")
    ranges = [(q, t, 0, 100, len(seqs[q]) - 50, 80, len(seqs[t]) - 20) for q, t in pairs]
    bounds = [300 if i % 3 else -1 for i in range(len(pairs))]
    outs = []
    for e in (on, off):
        e.set_sequences(seqs)
        o = [e.score_pairs(DEFAULT_2P, pairs)]
        assert e.twin_stats() == ((66, 66, 0, 0) if e is on else (0, 0, 0, 0))
        o.append(e.score_pairs(DEFAULT_2P, pairs, max_penalty=400))
        assert e.twin_stats() == (0, 0, 0, 0)
        o.append(e.align_pairs(DEFAULT_2P, pairs, max_penalty=400))
        assert e.twin_stats() == (0, 0, 0, 0)
        o.append(e.align_pairs(DEFAULT_2P, pairs, max_penalty=bounds))
        o.append(e.align_ranges(DEFAULT_2P, ranges))
        assert e.twin_stats() == (0, 0, 0, 0)
        o.append(e.score_ranges(DEFAULT_2P, ranges))
        o.append(e.align_pairs(DEFAULT_2P, pairs, verify=True))
        o.append(e.align_pairs(DEFAULT_2P, pairs, clip=2))
        outs.append(o)
    a, b = outs
    for k in (0, 1, 5):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in (2, 3, 4):
        same_records(a[k], b[k])
    same_records(a[6][:2], b[6][:2])
    assert a[6][2].tobytes() == b[6][2].tobytes() and (a[6][2]["code"] == ffi.AWV_VF_OK).all()
    same_records(a[7][:2], b[7][:2])
    assert a[7][2].tobytes() == b[7][2].tobytes()
    on.align_pairs(DEFAULT_2P, pairs, verify=True)
    assert on.twin_stats()[0] == 66  # the verified entry point forms twin units too
