"""A/B of the shared base case on config 2 inside one process per setting: default (a twin unit's base cases run once for
both orientations) and pinned (AWV_F_NO_TWIN_BASE: once per orientation, the path as it was).
usage: python scratch/twin_base_settings.py shared|pinned STEPS [config]   -> one JSON line"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: F401
import torch  # noqa: F401
from allwave_amd import ffi, synth
setting, steps = sys.argv[1], int(sys.argv[2])
cfg = synth.CONFIGS[sys.argv[3] if len(sys.argv) > 3 else "c2"]
data, offs, _ = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"])
pairs = synth.all_pairs(cfg["nseq"])
flags = ffi.AWV_F_KEEP_ON_DEVICE | {"shared": 0, "pinned": ffi.AWV_F_NO_TWIN_BASE}[setting]
e = ffi.Engine(flags=flags)
e.set_sequences((data, offs))
e.align_pairs(cfg["scores"], pairs, want_cigars=False)
ms = []
for _ in range(steps):
    t0 = time.perf_counter()
    res, _ = e.align_pairs(cfg["scores"], pairs, want_cigars=False)
    ms.append((time.perf_counter() - t0) * 1e3)
    st = e.stats()
assert (res["status"] == 0).all()
print(json.dumps({"setting": setting, "ms_per_step": ms, "kernel_ms": st.kernel_ms, "cell_steps": int(st.cell_steps), "n_breakpoints": int(st.n_breakpoints),
                  "n_base": int(st.n_base), "twin_stats": e.twin_stats(), "penalty_sum": int(res["penalty"].sum()), "cigar_len_sum": int(res["cigar_len"].sum())}))
e.close()
