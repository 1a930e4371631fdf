"""Gap-run normalization measured: its kernel against the alignment, verify and clip kernels on config 2's
pair list, and what it buys -- how many (q, t) / (t, q) twins place their gaps alike before and after.
One warm engine, one process; kernel times from awv_engine_*_stats.
usage: python scratch/normalize_timing.py [config, default c2] [sequences of it whose twins are compared, default 64]"""
import os, random, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from allwave_amd import ffi, synth

SWAP = bytes.maketrans(b"ID", b"DI")


def twins_agree(cigs, pairs):
    """(twin units, units whose two op strings are equal once one has I and D exchanged)"""
    at = {(int(q), int(t)): k for k, (q, t) in enumerate(pairs[:, :2])}
    units = same = 0
    for (q, t), k in at.items():
        if q < t and (t, q) in at and cigs[k] is not None and cigs[at[(t, q)]] is not None:
            units += 1
            same += cigs[k] == cigs[at[(t, q)]].translate(SWAP)
    return units, same


cname = sys.argv[1] if len(sys.argv) > 1 else "c2"
cfg = synth.CONFIGS[cname]
kw = {"mixed_lengths": cfg["mixed_lengths"]} if "mixed_lengths" in cfg else {}
data, offs, ids = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"], **kw)
pairs = np.ascontiguousarray(synth.all_pairs(cfg["nseq"]))
scores = cfg["scores"]
print("%s: %d pairs, scores %s" % (cname, len(pairs), scores), flush=True)
e = ffi.Engine(device=0, flags=ffi.AWV_F_KEEP_ON_DEVICE)
e.set_sequences((data, offs))
ref, _ = e.align_pairs(scores, pairs, want_cigars=False)  # (warm: the arenas are allocated here)
assert (ref["status"] == 0).all()
print("align_pairs: kernel %.1f ms, %d columns" % (e.stats().kernel_ms, int(ref["cigar_len"].sum())), flush=True)
for rep in range(3):
    res, _, vres = e.align_pairs(scores, pairs, want_cigars=False, verify=True)
    vs = e.verify_stats()
    assert res.tobytes() == ref.tobytes() and (vres["code"] == 0).all()
    res, _, cres = e.align_pairs(scores, pairs, want_cigars=False, clip=2)
    cs = e.clip_stats()
    res, _, vres = e.align_pairs(scores, pairs, want_cigars=False, normalize="left", verify=True)
    ns, a_ms = e.normalize_stats(), e.stats().kernel_ms
    assert res.tobytes() == ref.tobytes() and (vres["code"] == 0).all() and ns.columns == vs.columns and ns.pairs == vs.pairs
    print("run %d: normalize kernel %8.3f ms  verify kernel %8.3f ms  clip kernel %8.3f ms  normalize / verify = %.3f  (alignment kernels %.1f ms)"
          % (rep, ns.kernel_ms, vs.kernel_ms, cs.kernel_ms, ns.kernel_ms / vs.kernel_ms, a_ms), flush=True)
print("normalized: %d pairs, %d of them moved; %d gap runs, %d moved, %d columns moved in all (%.2f per moved run), %d columns"
      % (ns.pairs, ns.records_moved, ns.runs, ns.runs_moved, ns.columns_moved, ns.columns_moved / max(ns.runs_moved, 1), ns.columns), flush=True)
e.close()

# ---- what it buys: twins that place their gaps alike
nsub = int(sys.argv[2]) if len(sys.argv) > 2 else 64
sub = np.ascontiguousarray(synth.all_pairs(nsub))
e = ffi.Engine(device=0)
e.set_sequences((data[:int(offs[nsub])], offs[:nsub + 1]))
for flags_name, norm in (("off", None), ("left", "left"), ("right", "right")):
    res, cigs = e.align_pairs(scores, sub, normalize=norm)
    units, same = twins_agree(cigs, sub)
    print("%s, first %d sequences, normalize %s: %d twin units, %d with equal gap placement (%.1f %%)"
          % (cname, nsub, flags_name, units, same, 100.0 * same / max(units, 1)), flush=True)

import repeats
rng = random.Random(2024)
seqs, rp = [], []
for name in ("microsatellite", "tandem", "cnv", "low_complexity", "end_runs"):
    for _ in range(40):
        p, t = repeats.SMALL[name](rng)
        seqs += [p, t]
        rp += [(len(seqs) - 2, len(seqs) - 1), (len(seqs) - 1, len(seqs) - 2)]
rp = np.array(rp, dtype=np.int32)
e.set_sequences(seqs)
for scores_r in ((0, 5, 8, 2, 24, 1), (0, 4, 6, 2)):
    for norm in (None, "left"):
        res, cigs = e.align_pairs(scores_r, rp, normalize=norm)
        units, same = twins_agree(cigs, rp)
        print("repeat-rich list (200 pairs and their swapped twins, tests/repeats.py SMALL), scores %s, normalize %s: %d units, %d with equal gap placement (%.1f %%)"
              % (scores_r, norm or "off", units, same, 100.0 * same / max(units, 1)), flush=True)
e.close()
