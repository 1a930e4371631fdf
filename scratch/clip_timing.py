"""The clip kernel against the verify kernel on config 2's pair list: one warm engine, one process, both
kernels over the same op bytes in the same CIGAR arenas; kernel times from awv_engine_clip_stats / awv_engine_verify_stats.
usage: python scratch/clip_timing.py [config, default c2] [pairs, default all] [match bonus, default 2]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allwave_amd import ffi, synth

cname = sys.argv[1] if len(sys.argv) > 1 else "c2"
cfg = synth.CONFIGS[cname]
kw = {"mixed_lengths": cfg["mixed_lengths"]} if "mixed_lengths" in cfg else {}
data, offs, ids = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"], **kw)
pairs = synth.all_pairs(cfg["nseq"])
if len(sys.argv) > 2 and int(sys.argv[2]) > 0:
    pairs = pairs[:int(sys.argv[2])]
pairs = np.ascontiguousarray(pairs)
bonus = int(sys.argv[3]) if len(sys.argv) > 3 else 2
scores = cfg["scores"]
print("%s: %d pairs, scores %s, match bonus %d" % (cname, len(pairs), scores, bonus), flush=True)
e = ffi.Engine(device=0, flags=ffi.AWV_F_KEEP_ON_DEVICE)
e.set_sequences((data, offs))
ref, _ = e.align_pairs(scores, pairs, want_cigars=False)  # (warm: the arenas are allocated here)
assert (ref["status"] == 0).all()
print("align_pairs: kernel %.1f ms, %d columns" % (e.stats().kernel_ms, int(ref["cigar_len"].sum())), flush=True)
for rep in range(3):
    res, _, vres = e.align_pairs(scores, pairs, want_cigars=False, verify=True)
    vs, a_ms = e.verify_stats(), e.stats().kernel_ms
    assert res.tobytes() == ref.tobytes() and (vres["code"] == 0).all()
    res, _, cres = e.align_pairs(scores, pairs, want_cigars=False, clip=bonus)
    cs, b_ms = e.clip_stats(), e.stats().kernel_ms
    assert res.tobytes() == ref.tobytes() and cs.columns == vs.columns and cs.pairs == vs.pairs
    print("run %d: verify kernel %8.3f ms  clip kernel %8.3f ms  clip / verify = %.3f  (%d columns; alignment kernels %.1f / %.1f ms)"
          % (rep, vs.kernel_ms, cs.kernel_ms, cs.kernel_ms / vs.kernel_ms, cs.columns, a_ms, b_ms), flush=True)
ok = cres["code"] == ffi.AWV_CL_OK
cols = (cres["col_end"] - cres["col_beg"]).astype(np.int64)
print("clips: %d ok, %d empty; columns kept %.4f of all; %d pairs lose a column" %
      (int(ok.sum()), int((cres["code"] == ffi.AWV_CL_EMPTY).sum()), cols[ok].sum() / max(int(ref["cigar_len"].sum()), 1), int((cols[ok] < ref["cigar_len"][ok]).sum())))
e.close()
