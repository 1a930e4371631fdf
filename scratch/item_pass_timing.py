"""The five passes on caller-supplied records with slices measured: config 2's sequences, the 4,080 records of
every sequence against 16 targets (about 41 MB of op bytes), aligned once; then, in one process on the warm engine, N runs of
cs short and long, coverage `both`, variants into the engine's table, lift of a region table (150-base regions every 500 bases of
the targets, as queries on every record of their target) and msa over the 16 targets.  Per run the passes' own HIP-event times
from their stats, and a CRC of everything each call returns.
usage: python scratch/item_pass_timing.py [runs, default 3]"""
import os, sys, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allwave_amd import synth, ffi

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cfg = synth.CONFIGS["c2"]
data, offs, _ = synth.generate(cfg["nseq"], cfg["length"], cfg["d"], cfg["seed"])
seqs = [bytes(data[offs[i]:offs[i + 1]]) for i in range(cfg["nseq"])]
targets = list(range(0, cfg["nseq"], cfg["nseq"] // 16))[:16]
pairs = [(q, t) for t in targets for q in range(cfg["nseq"]) if q != t]

e = ffi.Engine()
e.set_sequences(seqs)
res, cigs = e.align_pairs(cfg["scores"], pairs)
assert (res["status"] == 0).all()
arena = np.frombuffer(b"".join(cigs), dtype=np.uint8)
res = res.copy()
res["cigar_off"] = np.concatenate([[0], np.cumsum([len(c) for c in cigs])[:-1]])
queries = [(k, "target", b, b + 150) for k, (q, t) in enumerate(pairs) for b in range(0, len(seqs[t]) - 150, 500)]
print("c2: %d records on %d targets, %d op bytes, %d lift queries" % (len(pairs), len(targets), arena.size, len(queries)), flush=True)


def crc(*parts):
    c = 0
    for p in parts:
        c = zlib.crc32(np.ascontiguousarray(p).tobytes(), c)
    return c


def one():
    out = {}
    for mode in ("short", "long"):
        text, csout, nbytes = e.cs_cigars(mode, pairs, res, arena)
        out["cs_" + mode] = (e.cs_stats().kernel_ms, crc(text, csout))
    e.coverage_begin("both")
    items = e.coverage_cigars(pairs, res, arena)
    ms = e.coverage_stats().kernel_ms
    _, aligned, matched = e.coverage_read()
    out["coverage"] = (ms, crc(items, aligned, matched))
    e.variants_begin()
    items, n_events = e.variants_cigars(pairs, res, arena, fold=ffi.AWV_VTAB_ACCUMULATE)
    ms = e.variants_stats().kernel_ms
    out["variants"] = (ms, crc(items, e.variants_read()) ^ n_events)
    before = e.lift_stats().kernel_ms
    lifted = e.lift_cigars(pairs, res, arena, queries)
    out["lift"] = (e.lift_stats().kernel_ms - before, crc(lifted))
    items, tgts, buf, size = e.msa_cigars(pairs, res, arena, targets)
    st = e.msa_stats()
    c = crc(items, tgts, buf)
    out["msa_width"], out["msa_scan"], out["msa_emit"] = (st.width_ms, c), (st.scan_ms, c), (st.emit_ms, c)
    return out


KEYS = ("cs_short", "cs_long", "coverage", "variants", "lift", "msa_width", "msa_scan", "msa_emit")
one()  # warm: buffers, tables
acc = []
for rep in range(runs):
    r = one()
    acc.append(r)
    print("run %d: " % rep + ", ".join("%s %.3f ms" % (k, r[k][0]) for k in KEYS), flush=True)
for k in KEYS:
    ms = [r[k][0] for r in acc]
    assert len({r[k][1] for r in acc}) == 1, k
    print("%-9s min %.3f  mean %.3f  max %.3f ms  (max + spread %.3f)  crc %08x" % (k, min(ms), np.mean(ms), max(ms), 2 * max(ms) - min(ms), acc[0][k][1]), flush=True)
e.close()
