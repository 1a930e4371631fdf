"""Device pair planning (csrc/planner.hip) against the host planner: sketches, mash matrices, planned pair lists, mash
orientation and the CLI must be identical, byte for byte."""
import random
import subprocess

import numpy as np
import pytest

import repeats
from util import mutate, rand_seq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(hip_lib):
    from allwave_amd import build, host as H
    build.build_host()
    H.load()
    return H


def _ids(seqs):
    return ["s%d" % i for i in range(len(seqs))]


def _sketch_inputs():
    rng = random.Random(17)
    seqs = [rand_seq(rng, 5000), bytes(rng.choice(b"ACGTacgt") for _ in range(3000)), rand_seq(rng, 4000).lower()]
    # runs of N and IUPAC codes inside otherwise valid sequence
    s = bytearray(rand_seq(rng, 6000))
    for _ in range(30):
        p = rng.randrange(len(s) - 40)
        s[p:p + rng.randint(1, 30)] = bytes(rng.choice(b"NNNRYKMSWBDHVn-") for _ in range(rng.randint(1, 30)))[:len(s[p:p + 30])]
    seqs.append(bytes(s))
    seqs.append(b"N" * 500)
    # lengths around every k of the sweep
    for ln in (0, 1, 2, 10, 11, 12, 14, 15, 16, 20, 21, 22, 31, 32, 33, 63, 64, 65):
        seqs.append(rand_seq(rng, ln))
    seqs.append(rand_seq(rng, 100_000))
    seqs += [b"A" * 3000, b"c" * 700, b"AC" * 1500]
    for gen in (repeats.microsatellite, repeats.tandem, repeats.low_complexity, repeats.cnv):
        for _ in range(2):
            seqs += list(gen(rng))
    # a ~600 bp unit repeated: every hash comes 20 times, so duplicates straddle the s-th position
    unit = rand_seq(rng, 600)
    seqs.append(unit * 20)
    seqs.append(mutate(unit * 12, 0.002, rng))
    seqs.append(unit[:599] * 9 + unit.lower() * 5)
    return seqs


@pytest.mark.parametrize("kind", ["canonical", "forward", "revcomp"])
def test_sketches_equal_host(host, kind):
    seqs = _sketch_inputs()
    ids = _ids(seqs)
    small_seen = False
    for k in (1, 11, 15, 21, 32, 64):
        for s in (1, 1000, 4096):
            want = host.sketch(ids, seqs, k, s, kind)
            got = host.sketch(ids, seqs, k, s, kind, device=0)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, "kind %s k %d s %d sequence %d (length %d): %d hashes against %d" % (kind, k, s, i, len(seqs[i]), len(g), len(w))
            small_seen = small_seen or (s == 1000 and k == 15 and 0 < len(want[-3]) < 200)
    assert small_seen  # the repeated unit's sketch is far smaller than s


def test_sketch_limits_run_host_code(host):
    seqs = _sketch_inputs()[:6]
    ids = _ids(seqs)
    for k, s in ((65, 100), (15, 4097), (0, 100)):
        assert host.sketch(ids, seqs, k, s, "canonical", device=0) == host.sketch(ids, seqs, k, s, "canonical")


def _matrix_sets():
    rng = random.Random(3)
    base = rand_seq(rng, 3000)
    a = [base, base, mutate(base, 0.02, rng), mutate(base, 0.2, rng), rand_seq(rng, 3000), rand_seq(rng, 2500), b"ACGTACG", b"",
         base.lower(), base[:1500] + b"N" * 10 + base[1500:]]
    b = [rand_seq(rng, 2000) for _ in range(40)]  # unrelated: all distances 1.0
    c = [mutate(base, 0.05, rng) for _ in range(25)] + [rand_seq(rng, 14)]
    return [a, b, c, [base], []]


@pytest.mark.parametrize("k", [15, 21, 9])
def test_mash_matrix_bytewise(host, k):
    for seqs in _matrix_sets():
        ids = _ids(seqs)
        want = host.mash_matrix(ids, seqs, k=k)
        got = host.mash_matrix(ids, seqs, k=k, device=0)
        assert got.tobytes() == want.tobytes()  # (the sign of zero included)
    seqs = _matrix_sets()[0]
    got = host.mash_matrix(_ids(seqs), seqs, device=0)
    assert np.signbit(got[0, 1]) and got[0, 1] == 0.0  # identical copies: -0.0, as the host prints it


def _tree_sets(rng):
    base = rand_seq(rng, 2000)
    ties = [base] * 5 + [mutate(base, 0.03, rng) for _ in range(4)] + [rand_seq(rng, 1500) for _ in range(8)]
    fam = []
    for _ in range(6):
        r = rand_seq(rng, 1500)
        fam += [mutate(r, rng.uniform(0.0, 0.1), rng) for _ in range(rng.randint(1, 5))]
    return {"ties": ties, "families": fam}


def test_plan_tree_equal_host(host):
    rng = random.Random(11)
    sets = _tree_sets(rng)
    specs = ["tree:%d:%d:0.0" % (n, f) for n in (0, 1, 3, 64, 65) for f in (0, 1, 3) if n or f] + \
            ["tree:3:1:0.1", "tree:2:0:0.5", "tree:0:1:0.3", "tree:1:64:0.0", "tree:65:65:0.2", "tree:3:2:0.1:21", "tree:2:2:0.0:11",
             "tree:2:1:0.0:6", "tree:3:1:1.0"]
    for name, seqs in sets.items():
        ids = _ids(seqs)
        for spec in specs:
            want = host.plan_pairs(ids, seqs, spec)
            assert host.plan_pairs(ids, seqs, spec, device=0) == want, (name, spec)
    # every sequence unrelated: all distances 1.0, the k-th neighbour decided by index alone
    seqs = [rand_seq(rng, 1200) for _ in range(30)]
    for spec in ("tree:3:2:0.0", "tree:1:1:0.05"):
        assert host.plan_pairs(_ids(seqs), seqs, spec, device=0) == host.plan_pairs(_ids(seqs), seqs, spec)


@pytest.mark.parametrize("n", [2, 3, 11, 300])
def test_plan_sizes_equal_host(host, n):
    rng = random.Random(n)
    base = rand_seq(rng, 1500)
    seqs = [mutate(base, rng.uniform(0.0, 0.15), rng) if rng.random() < 0.7 else rand_seq(rng, 1000) for _ in range(n)]
    ids = ["seq_%d#%s" % (i, "x" * (i % 13)) for i in range(n)]
    specs = ["tree:3:1:0.1", "tree:1:0:0.0", "random:0.3", "tree:1:0:1.0", "random:1", "random:1.0", "giant:0.9", "connectivity:0.5",
             "auto"]
    for spec in specs:
        for exclude_self in (True, False):
            want = host.plan_pairs(ids, seqs, spec, exclude_self=exclude_self)
            got = host.plan_pairs(ids, seqs, spec, exclude_self=exclude_self, device=0)
            assert got == want, (n, spec, exclude_self)
    assert host.plan_pairs(ids, seqs, "random:0.4", resparsify=True, device=0) == host.plan_pairs(ids, seqs, "random:0.4", resparsify=True)


def test_orient_mash_equal_host(host):
    rng = random.Random(9)
    ref = rand_seq(rng, 2000)
    fwd = mutate(ref, 0.05, rng)
    rc = host.reverse_complement(mutate(ref, 0.05, rng))
    seqs = [ref, fwd, rc, rand_seq(rng, 2000), b"ACGT", ref.lower()]
    ids = _ids(seqs)
    pairs = [(1, 0), (2, 0), (3, 0), (4, 0), (0, 2), (5, 0)]
    assert host.orient_mash(ids, seqs, pairs, device=0) == host.orient_mash(ids, seqs, pairs) == [False, True, False, False, True, False]
    # repeat-rich sequences, both strands, 10,000 random pairs
    seqs = []
    for gen in (repeats.microsatellite, repeats.tandem, repeats.low_complexity, repeats.cnv):
        for _ in range(6):
            a, b = gen(rng)
            seqs += [a, host.reverse_complement(b) if rng.random() < 0.5 else b]
    seqs += [rand_seq(rng, 3000) for _ in range(8)] + [b"", b"ACG"]
    ids = _ids(seqs)
    pairs = [(rng.randrange(len(seqs)), rng.randrange(len(seqs))) for _ in range(10_000)]
    got = host.orient_mash(ids, seqs, pairs, device=0)
    assert got == host.orient_mash(ids, seqs, pairs)
    assert any(got) and not all(got)


def _write_fasta(path, ids, seqs):
    path.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))


def test_cli_plan_device_output_identical(host, tmp_path):
    from allwave_amd import build
    rng = random.Random(21)
    base = rand_seq(rng, 1200)
    seqs = [base, base] + [mutate(base, 0.04, rng) for _ in range(6)] + [host.reverse_complement(mutate(base, 0.04, rng)) for _ in range(3)] + \
           [rand_seq(rng, 900), b"ACGT"]
    ids = ["c%d" % i for i in range(len(seqs))]
    fa = tmp_path / "in.fa"
    _write_fasta(fa, ids, seqs)

    def run(*extra):
        r = subprocess.run([build.CLI_BIN, "-i", str(fa), "--no-progress"] + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    assert run("--mash-matrix", "--plan-device", "0") == run("--mash-matrix")
    assert run("--mash-matrix", "-p", "tree:1:1:0:21", "--plan-device", "0") == run("--mash-matrix", "-p", "tree:1:1:0:21")
    want = sorted(run("-p", "tree:2:1:0.1").splitlines())
    assert want and sorted(run("-p", "tree:2:1:0.1", "--plan-device", "0").splitlines()) == want
    # with --shard every rank plans the same list on its plan device
    shards = sorted(run("-p", "tree:2:1:0.1", "--plan-device", "0", "--shard", "0/2").splitlines() +
                    run("-p", "tree:2:1:0.1", "--plan-device", "0", "--shard", "1/2").splitlines())
    assert shards == want
    assert sorted(run("-p", "giant:0.9", "--plan-device", "0", "--devices", "0,0").splitlines()) == sorted(run("-p", "giant:0.9").splitlines())


def test_tree_scale_1024(host):
    """Config 3 style: 1,024 x 10 kbp at 5 % divergence from synth.generate, tree:3:1:0.1."""
    from allwave_amd import synth
    data, offs, ids = synth.generate(1024, 10_000, 0.05, 3)
    seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i in ids]
    want = host.plan_pairs(ids, seqs, "tree:3:1:0.1")
    got = host.plan_pairs(ids, seqs, "tree:3:1:0.1", device=0)
    assert len(want) > 1024 * 3 and got == want
