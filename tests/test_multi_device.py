"""One pair list over several engines in one call (AllPairIterator::with_devices, host.iterate(..., devices=[...]),
allwave_hip --devices).  CPU tests: the batch planner (planner::device_batches), the CLI's --devices parsing and error
propagation across the submitter threads on a box without a GPU.  GPU tests: every consumer, both orientations and
several penalty classes on two or three slots of device 0 give the one-device output, which is the oracle's."""
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from util import DEFAULT_2P, EDIT, mutate, rand_seq, rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(hip_lib):
    from allwave_amd import build, host as H
    build.build_host()
    H.load()
    return H


def _lpt_loads(batches, cost):
    return [float(sum(cost[i] for i in b)) for b in batches]


def _skewed_costs(rng, n):
    """Predicted costs with a config-5-like spread (largest / smallest above 100x): a few long pairs among many short ones."""
    lens = rng.integers(100, 1000, size=40).tolist() + rng.integers(20000, 60000, size=4).tolist()
    pairs = [(int(rng.integers(len(lens))), int(rng.integers(len(lens)))) for _ in range(n)]
    return np.asarray(pairs, dtype=np.int64), np.asarray(lens, dtype=np.int64)


def test_device_batches_partition_and_rule(host):
    """Every pair in exactly one batch, in list order inside it; B = min(4 * slots, ceil(n / min_batch_pairs)), at least 1;
    the LPT bound (heaviest batch - lightest <= the largest pair) holds; the result is the same on every call."""
    rng = np.random.default_rng(5)
    cases = []
    for n in (0, 1, 7, 100, 1000, 5000):
        pairs, lens = _skewed_costs(rng, max(n, 1))
        _, cost = host.shard_assignment(pairs[:n], lens, "0,5,8,2,24,1", 1)
        if n >= 100:
            assert cost.max() / cost.min() > 100, n  # (the skew the rule is meant for)
        cases.append(cost)
        cases.append(np.full(n, 7.0))  # equal costs (config 2 / 3)
    for cost in cases:
        n = len(cost)
        for slots in (1, 2, 3, 8):
            for mb in (1, 5, 64, 16384):
                b = host.device_batches(cost, slots, mb)
                want = max(1, min(4 * slots, -(-n // mb)))
                assert len(b) == want, (n, slots, mb)
                flat = sorted(i for x in b for i in x)
                assert flat == list(range(n)), (n, slots, mb)
                for x in b:
                    assert x == sorted(x)
                if n:
                    loads = _lpt_loads(b, cost)
                    assert max(loads) - min(loads) <= cost.max() * (1 + 1e-12), (n, slots, mb)
                assert host.device_batches(cost, slots, mb) == b
        if n >= 8:  # min_batch_pairs = 1 gives 4 * slots batches when n allows
            assert len(host.device_batches(cost, 2, 1)) == 8
    # equal costs come out strided, like the shards
    assert host.device_batches(np.ones(10), 2, 1) == [[0, 8], [1, 9], [2], [3], [4], [5], [6], [7]]
    assert host.device_batches(np.ones(10), 2) == [list(range(10))]  # default: 16,384 pairs per batch at the least


@pytest.mark.parametrize("argv, msg", [
    (["--devices", "0,x"], "'x' is not a device ordinal"),
    (["--devices", "3-1"], "empty range '3-1'"),
    (["--devices", ""], "the device list is empty"),
    (["--devices", "0-99999"], "more than 256 entries"),
    (["--device", "0", "--devices", "0,1"], "'--device' cannot be used with '--devices'"),
])
def test_cli_devices_rejects(host, tmp_path, argv, msg):
    """--devices parse errors and --device with --devices: exit 1 with a message, before any device is opened (no PAF)."""
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTACCTAC\n")
    out = tmp_path / "out.paf"
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-p", "none", "-o", str(out)] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r
    assert msg in r.stderr
    assert not out.exists()
    assert r.stdout == ""


def test_cli_devices_all_without_gpu(host, tmp_path):
    """--devices all asks the HIP runtime for the visible devices: on a box without a GPU, exit 1 with its message."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from allwave_amd import build
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTAC\n>b\nACGTACCTAC\n")
    r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-p", "none", "-o", str(tmp_path / "o.paf"), "--devices", "all"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--devices all: no HIP device available" in r.stderr, r
    assert not (tmp_path / "o.paf").exists()


def test_cli_usage_names_devices(host):
    from allwave_amd import build
    r = subprocess.run([build.CLI_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--devices LIST" in r.stdout


def test_empty_device_list_is_refused(host):
    with pytest.raises(ValueError, match="empty"):
        host.iterate(["a", "b"], [b"ACGT", b"ACGA"], "0,1,1,1", devices=[])


def test_no_gpu_multi_slot_fails_promptly(host):
    """On a box without a GPU every slot's engine creation fails: the first error crosses the submitter threads and is
    raised once, promptly, with the engine's no-device message; the one-device form (devices=None) fails the same way --
    in a child process, so that a hang would end at its time limit instead of stopping the suite."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    code = (
        "import sys, time; sys.path.insert(0, %r)\n"
        "from allwave_amd import host as H\n"
        "t = time.time()\n"
        "for kw in (dict(devices=[0, 0], min_batch_pairs=1), dict(devices=None)):\n"
        "    for mode in ('for_each', 'next', 'par_for_each', 'par_collect', 'process_alignments'):\n"
        "        try:\n"
        "            H.iterate(['a', 'b', 'c'], [b'ACGT' * 9, b'ACGA' * 9, b'TTGA' * 9], '0,5,8,2,24,1', mode=mode, chunk=2, **kw)\n"
        "            print('no error', mode, kw); sys.exit(1)\n"
        "        except H.HostError as e:\n"
        "            assert 'no HIP device' in str(e) and 'no CPU fallback' in str(e), (kw, str(e))\n"
        "            assert e.records == 0, (kw, e.records)\n"
        "print('ok %%.3f' %% (time.time() - t))\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
    assert float(r.stdout.split()[1]) < 30


# ---------------------------------------------------------------------------------------------------------------- GPU
def _revcomp(s):
    comp = {65: 84, 84: 65, 67: 71, 71: 67}
    return bytes(comp.get(b, 78) for b in reversed(s))


def _mixed_list(seed, with_rc=False):
    """0.1-6 kbp, divergences 2-12 %, unequal-length pairs (prefixes), optionally reverse-complemented copies."""
    rng = random.Random(seed)
    a, d = rand_seq(rng, 6000), rand_seq(rng, 2000)
    seqs = [a, mutate(a, 0.02, rng), mutate(a[:4700], 0.05, rng), d, mutate(d, 0.12, rng), mutate(d[300:400], 0.03, rng),
            mutate(d[:1500], 0.08, rng)]
    if with_rc:
        seqs[2] = _revcomp(seqs[2])
        seqs[4] = _revcomp(seqs[4])
        seqs.append(_revcomp(mutate(d[200:1800], 0.04, rng)))
    return ["m%d" % i for i in range(len(seqs))], seqs


def _oracle_line(oracle, ids, seqs, i, j, scores, rev):
    q = _revcomp(seqs[i]) if rev else seqs[i]
    pen, ops = oracle.Aligner(scores).align(q, seqs[j])
    m, x = ops.count(b"M"), ops.count(b"X")
    qe, te = m + x + ops.count(b"D"), m + x + ops.count(b"I")
    ident = (m / (m + x)) if (m + x) else 0.0
    return "%s\t%d\t0\t%d\t%s\t%s\t%d\t0\t%d\t%d\t%d\t60\tgi:f:%.6f\tcg:Z:%s" % (
        ids[i], len(seqs[i]), qe, "-" if rev else "+", ids[j], len(seqs[j]), te, m, max(qe, te), ident, rle(ops))


def _check_lines_against_oracle(oracle, ids, seqs, lines, scores):
    """Every line is the oracle's alignment of its pair on the strand the line names."""
    for ln in lines:
        f = ln.split("\t")
        i, j = ids.index(f[0]), ids.index(f[5])
        assert ln == _oracle_line(oracle, ids, seqs, i, j, scores, f[4] == "-"), (f[0], f[5])


def _fnv_sum(lines):
    tot = 0
    for ln in lines:
        h = 14695981039346656037
        for c in ln.encode():
            h = ((h ^ c) * 1099511628211) % (1 << 64)
        tot = (tot + h) % (1 << 64)
    return tot


def _assert_slots_worked(stats, npairs):
    assert len(stats) >= 2
    assert all(s.pairs_completed > 0 for s in stats), [s.pairs_completed for s in stats]
    assert sum(s.pairs_completed for s in stats) == npairs


@pytest.mark.gpu
def test_two_slots_every_consumer(host, oracle):
    """devices=[0, 0] with one-pair batches: each consumer of host.iterate gives the one-device output and the oracle's --
    the same list for the ordered consumers (par_collect, next), the same lines otherwise; both slots align pairs."""
    ids, seqs = _mixed_list(11)
    sc = "0,5,8,2,24,1"
    n = len(seqs)
    want = [_oracle_line(oracle, ids, seqs, i, j, DEFAULT_2P, False) for i in range(n) for j in range(n) if i != j]
    assert host.iterate(ids, seqs, sc, mode="par_collect") == want
    kw = dict(devices=[0, 0], min_batch_pairs=1, with_stats=True)
    got, st = host.iterate(ids, seqs, sc, mode="par_collect", **kw)
    assert got == want
    _assert_slots_worked(st, len(want))
    got, st = host.iterate(ids, seqs, sc, mode="for_each", **kw)
    assert sorted(got) == sorted(want)
    _assert_slots_worked(st, len(want))
    got, st = host.iterate(ids, seqs, sc, mode="par_for_each", threads=3, **kw)
    assert sorted(got) == sorted(want)
    _assert_slots_worked(st, len(want))
    got, _ = host.iterate(ids, seqs, sc, mode="next", chunk=9, **kw)   # several runs of 9 pairs, each over both slots
    assert got == want
    got, _ = host.iterate(ids, seqs, sc, mode="next", **kw)            # one run
    assert got == want
    # process_alignments_with_callback: mash orientation (all '+' here), through the devices overload and with small batches
    single = host.iterate(ids, seqs, sc, mode="process_alignments")
    assert sorted(single) == sorted(want)
    assert sorted(host.iterate(ids, seqs, sc, mode="process_alignments", devices=[0, 0])) == sorted(want)
    got, st = host.iterate(ids, seqs, sc, mode="process_alignments", **kw)
    assert sorted(got) == sorted(want)
    _assert_slots_worked(st, len(want))
    # all_pairs_paf and the counting path
    assert sorted(host.all_pairs_paf(ids, seqs, sc, orientation="forward", devices=[0, 0], min_batch_pairs=1)) == sorted(want)
    nb1, nl1, _, _ = host.all_pairs_paf_count(ids, seqs, sc)
    nb2, nl2, _, tot, slots, ck2 = host.all_pairs_paf_count(ids, seqs, sc, devices=[0, 0], min_batch_pairs=1, checksum=True)
    assert (nb2, nl2) == (nb1, nl1) == (sum(len(x) + 1 for x in want), len(want))
    assert ck2 == _fnv_sum(want)
    nb3, nl3, _, _, slots3, ck3 = host.all_pairs_paf_count(ids, seqs, sc, devices=[0], checksum=True)
    assert (nb3, nl3, ck3) == (nb1, nl1, ck2) and len(slots3) == 1 and slots3[0].pairs_completed == len(want)
    _assert_slots_worked(slots, len(want))
    assert tot.pairs_completed == len(want)
    assert tot.cell_steps == sum(s.cell_steps for s in slots)


@pytest.mark.gpu
@pytest.mark.parametrize("scores, tup", [("0,3,5,1,20,1", (0, 3, 5, 1, 20, 1)), ("0,1,1,1", EDIT)])
@pytest.mark.parametrize("orientation", ["wfa", "mash"])
def test_two_slots_orientation(host, oracle, orientation, scores, tup):
    """WFA orientation (per batch, on the engine that takes it) and mash orientation (once, on host threads) on reads
    with reverse-complemented copies, under a 2-piece and an edit penalty set: the one-device lines, each the oracle's."""
    ids, seqs = _mixed_list(12, with_rc=True)
    single = host.iterate(ids, seqs, scores, mode="par_collect", orientation=orientation)
    assert any(ln.split("\t")[4] == "-" for ln in single)
    _check_lines_against_oracle(oracle, ids, seqs, single, tup)
    got, st = host.iterate(ids, seqs, scores, mode="par_collect", orientation=orientation, devices=[0, 0], min_batch_pairs=1,
                           with_stats=True)
    assert got == single
    _assert_slots_worked(st, len(single))
    got = host.iterate(ids, seqs, scores, mode="for_each", orientation=orientation, devices=[0, 0], min_batch_pairs=1)
    assert sorted(got) == sorted(single)


@pytest.mark.gpu
def test_three_slots_compose_with_shards(host):
    """devices=[0, 0, 0] on shard r of 2: the two shards' lines together are the whole list's, each line once."""
    ids, seqs = _mixed_list(13)
    sc = "0,5,8,2,24,1"
    whole = host.iterate(ids, seqs, sc, mode="par_collect")
    parts = []
    for r in (0, 1):
        got, st = host.iterate(ids, seqs, sc, mode="par_collect", devices=[0, 0, 0], min_batch_pairs=1, shard=(r, 2), with_stats=True)
        assert 0 < len(got) < len(whole)
        assert sum(s.pairs_completed for s in st) == len(got)
        assert sum(1 for s in st if s.pairs_completed > 0) == 3
        parts += got
    assert sorted(parts) == sorted(whole)


@pytest.mark.gpu
def test_multi_slot_callback_error(host):
    """The callback's first error wins on the multi-slot path: it is what the caller sees, fewer records than the list
    arrive, and the call returns promptly.  Every call after the first failure fails with a message of its own ("failed
    again"), so a later error reported in its place, or a slot that goes on calling the callback, shows: the serial
    consumers make no call after the first failure; the parallel one at most the one already under way on the other slot."""
    ids, seqs = _mixed_list(14)
    npairs = len(seqs) * (len(seqs) - 1)
    for mode, kw in (("for_each", {}), ("par_for_each", {"threads": 3}), ("process_alignments", {"orientation": "mash"})):
        t0 = time.time()
        with pytest.raises(host.HostError) as ei:
            host.iterate(ids, seqs, "0,5,8,2,24,1", mode=mode, fail_at=6, devices=[0, 0], min_batch_pairs=1, **kw)
        assert time.time() - t0 < 120, mode
        assert 6 <= ei.value.records < npairs, (mode, ei.value.records)
        if mode == "par_for_each":  # (callback calls on two slots' threads at once: either may be recorded first)
            assert str(ei.value).startswith("callback failed"), str(ei.value)
            assert ei.value.late_calls <= 1, ei.value.late_calls
        else:
            assert str(ei.value) == "callback failed at record 6", (mode, str(ei.value))
            assert ei.value.late_calls == 0, (mode, ei.value.late_calls)


@pytest.mark.gpu
def test_invalid_ordinal_fails_before_any_launch(host):
    """devices=[0, 99]: slot 1's engine cannot be created; the run ends before any batch is taken -- the engine's error,
    no record reported."""
    ids, seqs = _mixed_list(15)
    for mode in ("for_each", "par_collect"):
        with pytest.raises(host.HostError, match="device ordinal out of range") as ei:
            host.iterate(ids, seqs, "0,5,8,2,24,1", mode=mode, devices=[0, 99], min_batch_pairs=1)
        assert ei.value.records == 0


@pytest.mark.gpu
def test_cli_devices_matches_device(host, tmp_path):
    """allwave_hip --devices 0,0 and --devices all write the lines --device 0 writes (order aside)."""
    from allwave_amd import build
    ids, seqs = _mixed_list(16, with_rc=True)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    outs = {}
    for flag in (["--device", "0"], ["--devices", "0,0"], ["--devices", "all"]):
        o = tmp_path / ("o%s.paf" % flag[1].replace(",", "_"))
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "-p", "none", "--no-progress", "-o", str(o)] + flag,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[flag[1]] = o.read_text().splitlines()
    n = len(seqs)
    assert len(outs["0"]) == len(outs["0,0"]) == len(outs["all"]) == n * (n - 1)
    assert sorted(outs["0,0"]) == sorted(outs["0"])
    assert sorted(outs["all"]) == sorted(outs["0"])
