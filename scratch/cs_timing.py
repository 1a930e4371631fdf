"""The cs tag measured: the end-to-end PAF path on config 2 with cs off, short and long, alternating in one
process on warm engines (16 format threads, forward orientation, device_cigar on throughout so that the cs kernels stand next to
the encode kernels), and the text's size against the op bytes'.
usage: python scratch/cs_timing.py [runs of each kind, default 3]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allwave_amd import synth, host as H

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cfg = synth.CONFIGS["c2"]
data, offs, _ = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"])
seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(cfg["nseq"])]
ids = ["s%05d" % i for i in range(cfg["nseq"])]
sc = ",".join(map(str, cfg["scores"]))
KINDS = (None, "short", "long")


def one(cs):
    t0 = time.time()
    nb, nl, secs, st, _, ck = H.all_pairs_paf_count(ids, seqs, sc, orientation="forward", devices=[0], format_threads=16, checksum=True, device_cigar=True, cs=cs)
    wall = time.time() - t0
    le, lc = H.last_encode(), H.last_cs()
    dev_ms = st.kernel_ms + st.d2h_ms + st.h2d_ms + le["kernel_ms"] + lc["kernel_ms"]
    return dict(wall=wall, inside=secs, kernel_ms=st.kernel_ms, d2h_ms=st.d2h_ms, h2d_ms=st.h2d_ms, encode_ms=le["kernel_ms"], cs_ms=lc["kernel_ms"],
                rest_ms=1000 * secs - dev_ms, bytes=nb, lines=nl, checksum=ck, cs=lc)


print("c2: %d sequences, all pairs, scores %s, forward orientation, 16 format threads, device_cigar on" % (cfg["nseq"], sc), flush=True)
for cs in KINDS:  # warm: engines, arenas, host buffers
    r = one(cs)
    print("warm-up, cs %-5s: wall %.3f s" % (cs, r["wall"]), flush=True)
acc = {cs: [] for cs in KINDS}
for rep in range(runs):
    for cs in KINDS:
        r = one(cs)
        acc[cs].append(r)
        print("run %d, cs %-5s: wall %.3f s, inside %.3f s, align kernels %.1f ms, d2h %.2f ms, h2d %.2f ms, encode kernels %.2f ms, cs kernels %.2f ms, "
              "rest of the call (formatting, hand-over) %.1f ms; %d lines, %d bytes, checksum %016x"
              % (rep, cs, r["wall"], r["inside"], r["kernel_ms"], r["d2h_ms"], r["h2d_ms"], r["encode_ms"], r["cs_ms"], r["rest_ms"], r["lines"], r["bytes"],
                 r["checksum"]), flush=True)
for cs in KINDS:
    assert len({r["checksum"] for r in acc[cs]}) == 1 and len({r["bytes"] for r in acc[cs]}) == 1
for cs in KINDS[1:]:
    x = acc[cs][-1]["cs"]
    print("cs %-5s: %d pairs, %d failed, %d columns (op bytes), %d text bytes: text / op bytes = %.4f; the PAF grows by %d bytes"
          % (cs, x["pairs"], x["failed"], x["columns"], x["text_bytes"], x["text_bytes"] / x["columns"], acc[cs][-1]["bytes"] - acc[None][-1]["bytes"]), flush=True)
for key in ("wall", "inside", "d2h_ms", "encode_ms", "cs_ms", "rest_ms"):
    m = {cs: np.mean([r[key] for r in acc[cs]]) for cs in KINDS}
    print("mean %-9s off %.4f  short %.4f  long %.4f" % (key, m[None], m["short"], m["long"]), flush=True)
H.set_engine_config(release=True)
