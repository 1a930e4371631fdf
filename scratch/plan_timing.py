"""Host against device pair planning: wall time of --mash-matrix, tree:3:1:0.1 and mash orientation of config 2's pair list,
each planned once on the host (planner.cpp) and once on a GPU (planner.hip through the same entry points), outputs asserted
equal.  Wall times include everything the call does (device: engine creation, sequence upload, sketches, copies back).

    python scratch/plan_timing.py [--sizes 1024,2048,4096] [--length 10000] [--device 0] [--out results.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allwave_amd import host as H, synth  # noqa: E402


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H.load()
    rows = []

    def emit(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    # device warm-up (HIP runtime initialisation is not planning time)
    H.sketch(["w"], [b"ACGT" * 10], 15, 10, device=a.device)
    # mash orientation of config 2's pair list: 256 x 10 kbp, every ordered pair i != j
    data, offs, ids = synth.generate(256, a.length, 0.05, 2)
    seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(len(ids))]
    pairs = [(i, j) for i in range(256) for j in range(256) if i != j]
    want, th = timed(lambda: H.orient_mash(ids, seqs, pairs))
    got, td = timed(lambda: H.orient_mash(ids, seqs, pairs, device=a.device))
    assert got == want
    emit(dict(what="orient_mash", n=256, pairs=len(pairs), host_s=round(th, 3), device_s=round(td, 3), equal=True))
    for n in [int(x) for x in a.sizes.split(",")]:
        data, offs, ids = synth.generate(n, a.length, 0.05, 3)
        seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(n)]
        want, th = timed(lambda: H.mash_matrix(ids, seqs))
        got, td = timed(lambda: H.mash_matrix(ids, seqs, device=a.device))
        assert got.tobytes() == want.tobytes()
        del want, got
        emit(dict(what="mash_matrix", n=n, host_s=round(th, 3), device_s=round(td, 3), equal=True))
        want, th = timed(lambda: H.plan_pairs(ids, seqs, "tree:3:1:0.1"))
        got, td = timed(lambda: H.plan_pairs(ids, seqs, "tree:3:1:0.1", device=a.device))
        assert got == want
        emit(dict(what="tree:3:1:0.1", n=n, pairs=len(want), host_s=round(th, 3), device_s=round(td, 3), equal=True))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
