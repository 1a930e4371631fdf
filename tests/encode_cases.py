"""What the tests of the run-length CIGAR text share (csrc/encode_device.hpp, csrc/encode.hip): the case list -- the smallest
op strings at which the encode kernels can go wrong -- and the random strings and slices, each built once."""
import random

import numpy as np

import clip_cases as K

RUN_LENGTHS = (1, 9, 10, 99, 100, 999, 1000, 1023, 1024, 1025, 2049, 9999, 10000, 99999, 100000, 1000000)  # the digit thresholds; one and several chunks
RUN_STARTS = tuple(range(0, 18)) + tuple(range(1008, 1041))  # across lane words (16 bytes) and across the chunk edge (1,024 bytes)
NOT_COMPLETED = 1  # awv_result.status of the case that has a string and no text (AWV_ST_CAPACITY)


def case_list():
    """[(name, ops, status)], in a fixed order."""
    out = [("empty", b"", 0)]
    out += [("one byte " + chr(op), bytes([op]), 0) for op in b"MXID"]
    for k, n in enumerate(RUN_LENGTHS):
        out.append(("single run of %d" % n, bytes([b"MXID"[k % 4]]) * n, 0))
    for start in RUN_STARTS:
        for n in range(1, 41):  # one run of n between two others, beginning at column `start`
            out.append(("run of %d at %d" % (n, start), b"M" * start + b"D" * n + b"M" * 3, 0))
    out.append(("4096 alternating bytes", b"MX" * 2048, 0))
    out.append(("17 one-byte runs inside long runs", b"M" * 500 + b"XIDXIDXIDXIDXIDXI" + b"M" * 700 + b"D" * 1500, 0))
    out.append(("17 one-byte runs across the chunk edge", b"I" * 1015 + b"XMXMXMXMXMXMXMXMX" + b"D" * 40, 0))
    out.append(("a stray byte", b"MMMNMM", 0))
    out.append(("stray zero bytes", b"MM\x00\x00M" + b"\x00" * 20 + b"X", 0))
    out.append(("not completed", b"MMXMMIIMM", NOT_COMPLETED))
    rng = random.Random(314)
    mixed = random_ops(rng, 3000)
    out += [("mixed string at residue %d" % sh, mixed, 0) for sh in range(16)]
    return out


def residues(cases):
    """The residue modulo 16 of every case's first byte in the packed arena: all sixteen for the mixed string, a cycle else."""
    return [int(name.rsplit(" ", 1)[1]) if name.startswith("mixed string at residue") else (7 * k + 3) % 16 for k, (name, _, _) in enumerate(cases)]


def random_ops(rng, n, alphabet=b"MMMMXID"):
    """n op bytes in runs of 1 .. 12 (now and then a long one)."""
    ops = bytearray()
    while len(ops) < n:
        ops += bytes([rng.choice(alphabet)]) * (rng.randint(1, 12) if rng.random() < 0.9 else rng.randint(13, 1500))
    return bytes(ops[:n])


def random_strings(seed=315, count=300):
    """300 strings over MXID plus a stray byte, 0 .. 2,600 bytes, from single bytes to long runs."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.choice([0, 1, 2, 15, 16, 17, 31, 1023, 1024, 1025]) if k % 3 == 0 else rng.randint(0, 2600)
        out.append(random_ops(rng, n, alphabet=b"MMMMXIDN" if k % 2 else b"MXID"))
    return out


def random_slices(strings, seed=316, count=200):
    """[(string index, col_beg, col_end)]: empty slices, whole strings, and slices cut inside a run."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        i = rng.randrange(len(strings))
        n = len(strings[i])
        b = rng.randint(0, n)
        e = b if k % 10 == 0 else n if k % 10 == 1 else rng.randint(b, n)
        out.append((i, b, e))
    return out


def pack(cases):
    """The cases as records and an arena (clip_cases.pack_arena: a junk byte between strings, the residues of residues())."""
    return K.pack_arena([c[1] for c in cases], residues(cases), [c[2] for c in cases])


def texts_of(text, tout):
    """The arena `text` (bytes or a uint8 array) cut by the records `tout`."""
    buf = bytes(bytearray(text))
    return [buf[int(t["off"]):int(t["off"]) + int(t["len"])] for t in tout]


def dense(tout, base=0):
    """The layout rule: off[0] = base, off[i + 1] = off[i] + len[i]."""
    off = np.concatenate(([base], base + np.cumsum(tout["len"].astype(np.uint64))))[:-1] if len(tout) else np.zeros(0, dtype=np.uint64)
    return bool((tout["off"] == off.astype(np.uint64)).all())
