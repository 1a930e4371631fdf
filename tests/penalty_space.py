"""The penalty space the kernels are run over, and a restatement of what the engine derives from a penalty set.

The kernels are compiled once; every penalty-dependent choice is made at run time by the host, in `plan_penalties`
(allwave_amd/csrc/batch_plan.hpp; engine.hip's `align_core` calls it first).  `derive` restates that derivation line by line so
that the tests can (o) compare it field for field with the header's own output (tests/test_batch_plan_cpu.py), (i) check that the named sets below reach every derived class -- ring depth, steps per multi-step pass, chained
sweeps, base-case history bound, 2-piece shape -- on both sides of every boundary, and (ii) check the restatement against
what the engine reports (awv_stats.multi_cell_steps, AWV_ERR_PENALTIES).

Scores are given the way the reference passes them: (match, x, o, e) for gap-affine, (match, x, o1, e1, o2, e2) for
2-piece.
"""
from collections import namedtuple

# allwave_amd/csrc/biwfa_device.hpp
MAX_SCOPE = 126            # plan_penalties: scope + 2 <= 128
MAX_RING = 256             # the deepest ring an accepted set can need (scope 126 plus a chained pass)
TMAX = 5                   # AWV_TMAX: steps per sweep
TMAX32 = 5                 # AWV_TMAX32: steps per sweep with 32-bit rows
CHAIN_MAX = 3              # AWV_CHAIN_MAX: sweeps a pass may chain
FALLBACK_MIN_SCORE = 250   # base case when score_remaining <= 250 ...
FALLBACK_MIN_LENGTH = 100  # ... or both lengths <= 100
MAX_SB = 4000              # plan_penalties: the base-case history is sized for scores up to 4000
NCOMP = 5                  # M, I1, I2, D1, D2 rows per direction

# flags of include/allwave_hip.h that change the derivation
AWV_F_SINGLE_STEP = 64
AWV_F_NO_CHAIN = 128

Derived = namedtuple("Derived", "accepted reason two_piece x o1 e1 o2 e2 scope multi_T multi_T32 chain_max ring sb")


def _pieces(scores):
    s = [int(v) for v in scores]
    if len(s) == 6:
        return s[0], s[1], s[2], s[3], s[4], s[5], True
    if len(s) == 4:
        return s[0], s[1], s[2], s[3], s[2], s[3], False   # gap-affine: piece 2 = piece 1 (batch_plan.hpp plan_penalties)
    raise ValueError("expected 4 or 6 scores, got %d" % len(s))


def gap(scores, n):
    """Cost of a gap of n > 0 bases: the cheaper piece."""
    _, _, o1, e1, o2, e2, _ = _pieces(scores)
    return min(o1 + n * e1, o2 + n * e2)


def derive(scores, flags=0):
    """What the engine derives from a penalty set (allwave_amd/csrc/batch_plan.hpp, plan_penalties)."""
    m, x, o1, e1, o2, e2, two_piece = _pieces(scores)

    def out(accepted, reason, scope=0, multi_T=0, multi_T32=0, chain_max=1, ring=0, sb=0):
        return Derived(accepted, reason, two_piece, x, o1, e1, o2, e2, scope, multi_T, multi_T32, chain_max, ring, sb)

    # check_signs, then the scope
    if m != 0:
        return out(False, "match != 0")
    if x <= 0 or o1 < 0 or e1 <= 0:
        return out(False, "need x > 0, o >= 0, e > 0")
    if two_piece and (o2 < 0 or e2 <= 0):
        return out(False, "need o2 >= 0, e2 > 0")
    scope = max(x, o1 + e1, o2 + e2) + 1
    if scope > MAX_SCOPE:
        return out(False, "scope", scope)
    # multi-step passes, T <= the nearest M source, only for the instantiated I/D depths
    multi_T = min(x, o1 + e1, TMAX)
    if two_piece:
        multi_T = min(multi_T, o2 + e2)
    if (e1 != 2 or e2 != 1) if two_piece else (e1 not in (1, 2)):
        multi_T = 0
    if multi_T < 2 or flags & AWV_F_SINGLE_STEP:
        multi_T = 0
    # chained sweeps: only with x = TMAX and o1 + e1 = 2 TMAX; the third source must come from earlier passes
    chain_max = 1
    if multi_T == TMAX and two_piece and x == TMAX and o1 + e1 == 2 * TMAX and not flags & AWV_F_NO_CHAIN:
        chain_max = max(1, min(CHAIN_MAX, (o2 + e2) // TMAX))
    ring = 4
    while ring < scope + 2 + (multi_T * chain_max - 1 if multi_T > 0 else 0):
        ring *= 2
    # base-case history: FALLBACK_MIN_SCORE plus an open, or the worst case of a FALLBACK_MIN_LENGTH square
    n = FALLBACK_MIN_LENGTH
    worst = min(2 * gap(scores, n), n * x + gap(scores, n))
    sb = max(FALLBACK_MIN_SCORE + max(o1, o2), worst)
    # 32-bit rows: sweeps of at most TMAX32 steps (engine.hip fill_kparams)
    multi_T32 = min(multi_T, TMAX32) if min(multi_T, TMAX32) >= 2 else 0
    if sb > MAX_SB:
        return out(False, "sb", scope, multi_T, multi_T32, chain_max, ring, sb)
    return out(True, "", scope, multi_T, multi_T32, chain_max, ring, sb)


def shapes(scores):
    """The 2-piece shapes a set has (several can hold at once); empty for gap-affine sets."""
    _, _, o1, e1, o2, e2, two_piece = _pieces(scores)
    if not two_piece:
        return set()
    out = set()
    if (o1, e1) == (o2, e2):
        out.add("equal")
    if o2 + e2 > o1 + e1 and e2 < e1:
        out.add("usual")        # piece 2 dearer to open, cheaper to extend: the presets
    if o2 + e2 < o1 + e1:
        out.add("inverted")     # piece 2 is the cheaper 1-base gap
    if e2 > e1:
        out.add("crossing")     # piece 2 extends at a higher rate
    if o2 == 0:
        out.add("o2_zero")
    if (o2, e2) != (o1, e1) and o2 <= o1 and e2 <= e1:
        out.add("piece1_never_cheapest")
    return out


# Named sets.  Comments give (scope, multi_T, chain_max, ring, sb) as derive() computes them.
PENALTY_SPACE = [
    ("edit_unit", (0, 1, 0, 1)),                    # 2, 0, 1, 4, 250: plain edit distance, the only ring-4 set
    ("edit_allwave", (0, 1, 1, 1)),                 # 3, 0, 1, 8, 251: allwave's "edit" mode
    ("affine_T2_x2", (0, 2, 1, 1)),                 # 3, 2, 1, 8, 251
    ("affine_T2_e2", (0, 3, 0, 2)),                 # 4, 2, 1, 8, 400
    ("affine_T3", (0, 3, 4, 1)),                    # 6, 3, 1, 16, 254
    ("affine_T4", (0, 4, 6, 2)),                    # 9, 4, 1, 16, 412: AffineWavefronts::default()
    ("affine_T5", (0, 6, 8, 2)),                    # 11, 5, 1, 32, 416
    ("affine_e3_gated", (0, 5, 8, 3)),              # 12, 0, 1, 16, 616: e = 3 has no multi-step instance
    ("affine_e3_o0", (0, 7, 0, 3)),                 # 8, 0, 1, 16, 600
    ("default_2p", (0, 5, 8, 2, 24, 1)),            # 26, 5, 3, 64, 274: the reference's default scores
    ("2p_T2", (0, 4, 0, 2, 10, 1)),                 # 12, 2, 1, 16, 260
    ("2p_chain2", (0, 5, 8, 2, 12, 1)),             # 14, 5, 2, 32, 262
    ("2p_T5_unchained", (0, 6, 8, 2, 24, 1)),       # 26, 5, 1, 32, 274: x != TMAX
    ("2p_e1_1_gated", (0, 3, 5, 1, 20, 1)),         # 22, 0, 1, 32, 270: e1 = 1 has no 2-piece instance
    ("2p_wide_gated", (0, 2, 12, 1, 40, 1)),        # 42, 0, 1, 64, 290
    ("2p_inverted", (0, 5, 8, 2, 4, 1)),            # 11, 5, 1, 32, 258: o2+e2 < o1+e1, passes on
    ("2p_crossing", (0, 5, 4, 1, 12, 2)),           # 15, 0, 1, 32, 262: e2 > e1 (piece 1 cheaper at every length)
    ("2p_crossing_at_5", (0, 5, 12, 1, 2, 3)),      # 14, 0, 1, 16, 262: the pieces cross at 5 bases
    ("2p_equal", (0, 5, 8, 2, 8, 2)),               # 11, 0, 1, 16, 416: T would be 5, e2 = 2 is not instantiated
    ("2p_o2_zero", (0, 4, 6, 2, 0, 1)),             # 9, 0, 1, 16, 256: o2+e2 = 1 leaves no room for a pass
    ("2p_piece1_never", (0, 6, 4, 2, 2, 1)),        # 7, 3, 1, 16, 254: piece 2 cheaper at every length
    ("ring128_T3", (0, 3, 90, 1)),                  # 92, 3, 1, 128, 380
    ("scope101_T5", (0, 100, 10, 1)),               # 101, 5, 1, 128, 260
    ("scope125", (0, 124, 0, 1)),                   # 125, 0, 1, 128, 250: the widest scope without passes
    ("ring256_scope123_e1", (0, 5, 121, 1)),        # 123, 5, 1, 256, 442
    ("ring256_scope123_e2", (0, 5, 120, 2)),        # 123, 5, 1, 256, 640
    ("ring256_scope126_e2", (0, 5, 123, 2)),        # 126, 5, 1, 256, 646: the accept limit with passes
    ("ring256_scope126_T4", (0, 125, 3, 1)),        # 126, 4, 1, 256, 253
    ("ring256_2p_chain3", (0, 5, 8, 2, 124, 1)),    # 126, 5, 3, 256, 416: the deepest ring of all
    ("sb2000", (0, 10, 0, 10)),                     # 11, 0, 1, 16, 2000
    ("sb4000", (0, 20, 0, 20)),                     # 21, 0, 1, 32, 4000: the accept limit of the history
    # rejected
    ("reject_scope127", (0, 126, 3, 1)),
    ("reject_scope127_e2", (0, 5, 124, 2)),
    ("reject_scope127_2p", (0, 5, 8, 2, 125, 1)),
    ("reject_sb4001", (0, 20, 1, 20)),
    ("reject_x0", (0, 0, 3, 1)),
    ("reject_e0", (0, 5, 8, 0)),
    ("reject_e2_0", (0, 5, 8, 2, 24, 0)),
    ("reject_o2_negative", (0, 5, 8, 2, -1, 1)),
    ("reject_o_negative", (0, 5, -1, 2)),
    ("reject_match", (1, 5, 8, 2)),
]

ACCEPTED = [(n, s) for n, s in PENALTY_SPACE if derive(s).accepted]
REJECTED = [(n, s) for n, s in PENALTY_SPACE if not derive(s).accepted]
BY_NAME = dict(PENALTY_SPACE)


# one representative per derived class: ring 4, T = 2, the usual 2-piece sets with and without chained sweeps, inverted,
# crossing, equal pieces, ring 128 at scope 125, ring 256 with one sweep and with three chained, and sb = 4000
FLAVOUR_SETS = ("edit_unit", "affine_T2_e2", "default_2p", "2p_chain2", "2p_inverted", "2p_crossing", "2p_equal",
                "scope125", "ring256_scope123_e1", "ring256_2p_chain3", "sb4000")


def scaled(scores, k):
    """Every score times k (match stays 0): every alignment's penalty is k times what it was."""
    return tuple(int(v) * k for v in scores)
