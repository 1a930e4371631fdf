"""Bounded full alignment on config 5's planned pair list: one warm engine, kernel time from awv_stats.
  (a) unbounded align_pairs
  (b) align_pairs with B = the median penalty of (a)
  (c) what (b) replaces: score_pairs under B, then align_pairs on its survivors -- kernel times summed
usage: python scratch/bounded_timing.py [config, default c5] [pairs, default all]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allwave_amd import ffi, synth, host as H

cname = sys.argv[1] if len(sys.argv) > 1 else "c5"
cfg = synth.CONFIGS[cname]
kw = {"mixed_lengths": cfg["mixed_lengths"]} if "mixed_lengths" in cfg else {}
data, offs, ids = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"], **kw)
if cfg.get("sparsify", "none") != "none":
    pairs = np.asarray(H.plan_pairs(ids, [bytes(data[offs[i]:offs[i + 1]]) for i in range(cfg["nseq"])], cfg["sparsify"]), dtype=np.int32).reshape(-1, 2)
else:
    pairs = synth.all_pairs(cfg["nseq"])
if len(sys.argv) > 2:
    pairs = pairs[:int(sys.argv[2])]
pairs = np.ascontiguousarray(pairs)
scores = cfg["scores"]
print("%s: %d pairs, scores %s" % (cname, len(pairs), scores), flush=True)
e = ffi.Engine(device=0, flags=ffi.AWV_F_KEEP_ON_DEVICE)
e.set_sequences((data, offs))


def line(what, st, extra=""):
    print("%-44s kernel %10.1f ms  cell-steps %16d  launches %d  completed %d%s" % (what, st.kernel_ms, st.cell_steps, st.launches, st.pairs_completed, extra),
          flush=True)
    return st.kernel_ms, st.cell_steps


ref, _ = e.align_pairs(scores, pairs, want_cigars=False)  # (the arenas are allocated here: kernel_ms is event time around the launches only)
a_ms, a_cells = line("(a) unbounded align_pairs", e.stats())
assert (ref["status"] == 0).all()
B = int(np.median(ref["penalty"]))
above = int((ref["penalty"] > B).sum())
print("B = median penalty = %d; %d of %d pairs above it" % (B, above, len(pairs)), flush=True)
res, _ = e.align_pairs(scores, pairs, want_cigars=False, max_penalty=B)
b_ms, b_cells = line("(b) align_pairs, max_penalty = B", e.stats(), "  above the bound %d" % int((res["status"] == ffi.AWV_ST_ABOVE_BOUND).sum()))
done = res["status"] == 0
assert (done == (ref["penalty"] <= B)).all() and res[done].tobytes() == ref[done].tobytes()
sc = e.score_pairs(scores, pairs, max_penalty=B)
c1_ms, c1_cells = line("(c1) score_pairs, max_penalty = B", e.stats())
assert (sc["status"] == res["status"]).all() and (sc["penalty"] == res["penalty"]).all()
surv = np.ascontiguousarray(pairs[sc["status"] == 0])
res2, _ = e.align_pairs(scores, surv, want_cigars=False)
c2_ms, c2_cells = line("(c2) align_pairs on the %d survivors" % len(surv), e.stats())
assert (res2["penalty"] == ref["penalty"][done]).all()
print("(c) = (c1) + (c2): kernel %.1f ms, cell-steps %d" % (c1_ms + c2_ms, c1_cells + c2_cells))
print("(b) / (a) = %.3f   (b) / (c) = %.3f   cell-steps (b) / (a) = %.3f, (b) / (c) = %.3f" % (b_ms / a_ms, b_ms / (c1_ms + c2_ms), b_cells / a_cells, b_cells / (c1_cells + c2_cells)))
e.close()
