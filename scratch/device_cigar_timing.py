"""Device-side CIGAR text measured: the end-to-end PAF path on config 2 with device_cigar off and on,
alternating in one process on warm engines (16 format threads, forward orientation), and the sizes and the kernel's time on a
sample of config 4's long low-divergence strings.
usage: python scratch/device_cigar_timing.py [runs of each kind, default 3] [sequences of config 4 to sample, default 16]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allwave_amd import ffi, synth, host as H

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cfg = synth.CONFIGS["c2"]
data, offs, _ = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"])
seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(cfg["nseq"])]
ids = ["s%05d" % i for i in range(cfg["nseq"])]
sc = ",".join(map(str, cfg["scores"]))


def one(flag):
    t0 = time.time()
    nb, nl, secs, st, _, ck = H.all_pairs_paf_count(ids, seqs, sc, orientation="forward", devices=[0], format_threads=16, checksum=True, device_cigar=flag)
    wall = time.time() - t0
    le = H.last_encode()
    dev_ms = st.kernel_ms + st.d2h_ms + st.h2d_ms + le["kernel_ms"]
    return dict(wall=wall, inside=secs, kernel_ms=st.kernel_ms, d2h_ms=st.d2h_ms, h2d_ms=st.h2d_ms, encode_ms=le["kernel_ms"], rest_ms=1000 * secs - dev_ms,
                bytes=nb, lines=nl, checksum=ck, enc=le)


print("c2: %d sequences, all pairs, scores %s, forward orientation, 16 format threads" % (cfg["nseq"], sc), flush=True)
for flag in (False, True):  # warm: engines, arenas, host buffers
    r = one(flag)
    print("warm-up, device_cigar %-5s: wall %.3f s" % (flag, r["wall"]), flush=True)
acc = {False: [], True: []}
for rep in range(runs):
    for flag in (False, True):
        r = one(flag)
        acc[flag].append(r)
        print("run %d, device_cigar %-5s: wall %.3f s, inside %.3f s, align kernels %.1f ms, d2h %.2f ms, h2d %.2f ms, encode kernels %.2f ms, "
              "rest of the call (formatting, hand-over) %.1f ms; %d lines, %d bytes, checksum %016x"
              % (rep, flag, r["wall"], r["inside"], r["kernel_ms"], r["d2h_ms"], r["h2d_ms"], r["encode_ms"], r["rest_ms"], r["lines"], r["bytes"], r["checksum"]), flush=True)
assert len({r["checksum"] for v in acc.values() for r in v}) == 1 and len({r["bytes"] for v in acc.values() for r in v}) == 1
enc = acc[True][-1]["enc"]
print("encoded: %d pairs, %d columns (op bytes), %d runs, %d text bytes: text / op bytes = %.4f, %.2f characters per run"
      % (enc["pairs"], enc["columns"], enc["runs"], enc["text_bytes"], enc["text_bytes"] / enc["columns"], enc["text_bytes"] / enc["runs"]), flush=True)
for key in ("wall", "inside", "d2h_ms", "rest_ms"):
    off, on = np.mean([r[key] for r in acc[False]]), np.mean([r[key] for r in acc[True]])
    print("mean %-8s off %.4f  on %.4f  on / off = %.4f" % (key, off, on, on / off), flush=True)
H.set_engine_config(release=True)

# ---- long low-divergence strings: a sample of config 4
nsub = int(sys.argv[2]) if len(sys.argv) > 2 else 16
cfg = synth.CONFIGS["c4"]
data, offs, _ = synth.generate(nsub, cfg["length"], cfg["d"], cfg["seed"])
pairs = np.ascontiguousarray(synth.all_pairs(nsub))
e = ffi.Engine(device=0, flags=ffi.AWV_F_NO_ARENA_PROBE)
e.set_sequences((data, offs))
for rep in range(2):
    res, cigs = e.align_pairs(cfg["scores"], pairs)
    d2h_plain, k_ms = e.stats().d2h_ms, e.stats().kernel_ms
    res2, texts, tout = e.align_pairs(cfg["scores"], pairs, encode=True)
    st, d2h_text = e.encode_stats(), e.stats().d2h_ms
    assert res2.tobytes() == res.tobytes() and sum(len(t) for t in texts) == st.text_bytes
    print("c4 sample (%d sequences of %d bp at %.0f %%, %d pairs), run %d: align kernels %.1f ms; op bytes %d, d2h %.2f ms; text bytes %d (%.4f of the op bytes), "
          "d2h %.2f ms, encode kernels %.3f ms, %d runs" % (nsub, cfg["length"], 100 * cfg["d"], len(pairs), rep, k_ms, st.columns, d2h_plain, st.text_bytes,
                                                            st.text_bytes / st.columns, d2h_text, st.kernel_ms, st.runs), flush=True)
e.close()
