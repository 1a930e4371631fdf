"""CPU tests of device pair planning's host side: the integer keep threshold, the exported entry points, and that asking for
a plan device never quietly plans on the host when there is no GPU."""
import ctypes as C
import random
import subprocess

import pytest

U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def host(hip_lib):
    from allwave_amd import build, host as H
    build.build_host()
    H.load()
    return H


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def _kept(h, f):
    # keep_pair's predicate as Rust and C evaluate it: (h as f64) / (u64::MAX as f64) < f, both correctly rounded
    return float(h) / float(U64_MAX) < f


FRACTIONS = [1e-9, 1e-6, 1e-3, 0.01, 0.1, 1 / 3, 0.5, 0.9, 0.99, 0.999999, 1 - 1e-9, 1 - 1e-12, 0.0, 1.0, 1.5, 2.0, -0.5]


@pytest.mark.parametrize("f", FRACTIONS)
def test_keep_threshold_matches_float_predicate(host, f):
    t, keep_all = host.keep_threshold(f)
    assert keep_all == _kept(U64_MAX, f)
    if keep_all:
        assert f >= 1.0
        for h in (0, 1, U64_MAX // 2, U64_MAX - 1, U64_MAX):
            assert _kept(h, f)
        return
    # the boundary itself and its neighbours
    for h in (t - 2, t - 1, t, t + 1, t + 2):
        if 0 <= h <= U64_MAX:
            assert _kept(h, f) == (h < t), (f, h, t)
    rng = random.Random(hash(f) & 0xFFFF)
    for _ in range(2000):
        h = rng.getrandbits(64)
        assert _kept(h, f) == (h < t), (f, h, t)
    for _ in range(500):  # near the boundary, where rounding of (double)h decides
        h = min(U64_MAX, max(0, t + rng.randint(-(1 << 12), 1 << 12)))
        assert _kept(h, f) == (h < t), (f, h, t)


def test_keep_threshold_edges(host):
    assert host.keep_threshold(0.0) == (0, False)
    assert host.keep_threshold(float("nan"))[1] is False and host.keep_threshold(float("nan"))[0] == 0
    # u64::MAX as f64 is 2^64, and so is every h >= 2^64 - 1024 (rounded to the nearest double, ties to even): h / 2^64 < 1
    # fails for exactly those, so a fraction of 1 keeps all but the top 1,024 hashes
    assert host.keep_threshold(1.0) == ((1 << 64) - 1024, False)
    assert host.keep_threshold(1.0 + 2 ** -52)[1] is True
    assert host.keep_threshold(3.0)[1] is True


def test_device_planner_entry_points_exported(hip_lib, host):
    from allwave_amd import ffi
    for name in ("awv_sketch", "awv_sketch_copy", "awv_sketch_pair_counts", "awv_sketch_rows", "awv_sketch_knn", "awv_keep_pairs"):
        assert name in ffi.EXPORTS
        assert getattr(hip_lib, name) is not None
    L = host.load()
    for name in ("awh_mash_matrix_gpu", "awh_plan_pairs_gpu", "awh_orient_mash_gpu", "awh_sketch", "awh_keep_threshold"):
        assert getattr(L, name) is not None


def test_device_entry_points_refuse_null_engine_without_gpu(hip_lib):
    """A null engine: AWV_ERR_NO_DEVICE on a box without a GPU (no CPU fallback), AWV_ERR_ARG with one."""
    from allwave_amd import ffi
    hip_lib.awv_sketch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    rc = hip_lib.awv_sketch(None, 0, 15, 1000, None)
    assert rc == (ffi.AWV_ERR_ARG if _gpu_present() else ffi.AWV_ERR_NO_DEVICE)
    hip_lib.awv_keep_pairs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p]
    rc = hip_lib.awv_keep_pairs(None, 0, None, None, 0, 0, 0, None)
    assert rc == (ffi.AWV_ERR_ARG if _gpu_present() else ffi.AWV_ERR_NO_DEVICE)


def _seqs():
    rng = random.Random(5)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(800)) for _ in range(4)]
    return ["q%d" % i for i in range(len(seqs))], seqs


def test_device_planning_without_gpu_is_an_error(host):
    """device=0 plans on the device or fails with a clear error; it never quietly runs the host planner."""
    ids, seqs = _seqs()
    calls = [
        lambda d: host.mash_matrix(ids, seqs, device=d),
        lambda d: host.plan_pairs(ids, seqs, "tree:1:1:0.5", device=d),
        lambda d: host.plan_pairs(ids, seqs, "random:0.5", device=d),
        lambda d: host.plan_pairs(ids, seqs, "tree:65:1:0.5", device=d),  # (beyond the device's kNN limit: the host code runs on a GPU box)
        lambda d: host.orient_mash(ids, seqs, [(0, 1), (2, 3)], device=d),
        lambda d: host.sketch(ids, seqs, 15, 1000, "canonical", device=d),
    ]
    for call in calls:
        if _gpu_present():
            got, want = call(0), call(None)
            assert (got.tobytes() == want.tobytes()) if hasattr(got, "tobytes") else got == want
        else:
            with pytest.raises(host.HostError, match="no HIP device"):
                call(0)


def test_cli_plan_device_without_gpu_is_an_error(host, tmp_path):
    from allwave_amd import build
    ids, seqs = _seqs()
    fa = tmp_path / "x.fa"
    fa.write_text("".join(">%s\n%s\n" % (i, s.decode()) for i, s in zip(ids, seqs)))
    out = subprocess.run([build.CLI_BIN, "-i", str(fa), "--mash-matrix", "--plan-device", "0"], capture_output=True, text=True, timeout=120)
    ref = subprocess.run([build.CLI_BIN, "-i", str(fa), "--mash-matrix"], capture_output=True, text=True, timeout=120)
    assert ref.returncode == 0
    if _gpu_present():
        assert out.returncode == 0 and out.stdout == ref.stdout
    else:
        assert out.returncode != 0 and "no HIP device" in out.stderr and out.stdout == ""
    bad = subprocess.run([build.CLI_BIN, "-i", str(fa), "--mash-matrix", "--plan-device", "x"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--plan-device expects a device ordinal" in bad.stderr
