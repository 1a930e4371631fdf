/*
 * allwave_hip.h -- C ABI of the MI355X-native BiWFA engine (liballwave_hip.so).
 *
 * This is the drop-in boundary for allwave's per-pair hot path.  The reference reaches the
 * arithmetic through the lib_wfa2 crate (Rust FFI over WFA2-lib, not in /root/reference):
 *
 *   reference call (file:line, relative to /root/reference)            replaced by
 *   -----------------------------------------------------------------  --------------------------
 *   AffineWavefronts::with_penalties_and_memory_mode(m,x,o,e,Ultralow)  awv_penalties {two_piece=0}
 *     src/alignment.rs:265-278, src/wfa.rs:188-204
 *   AffineWavefronts::with_penalties_affine2p_and_memory_mode(...)      awv_penalties {two_piece=1}
 *     src/alignment.rs:279-287, src/wfa.rs:208-216
 *   set_alignment_scope(Alignment) / set_alignment_span(End2End) /      fixed behaviour of the engine
 *   set_heuristic(None)   src/alignment.rs:226-228, src/wfa.rs:221-223  (end-to-end, exact, with CIGAR)
 *   set_alignment_scope(ComputeScore) + wf.align + wf.score()            awv_score_pairs (exact penalty, no
 *                                                                        CIGAR; optional penalty bound)
 *   determine_orientation_wfa                  src/alignment.rs:157-175  awv_orient_pairs
 *   wf.align(query, target) -> AlignmentStatus   src/alignment.rs:231   awv_align_pairs / awv_align_one
 *   wf.score()                                   src/alignment.rs:235   awv_result.score (= -penalty)
 *   wf.cigar() -> &[u8]                          src/alignment.rs:236   CIGAR arena + awv_result.cigar_off/len
 *   per-thread aligner cache                     src/alignment.rs:11-22 awv_engine (owns all device state)
 *
 * A per-pair synchronous call cannot feed a GPU, so the primary entry point is batched:
 * the caller hands over the sequence set once and then lists of (query, target) index pairs
 * -- exactly the pair list AllPairIterator materialises (src/iterator.rs:38-50).
 *
 * Conventions kept from the reference boundary:
 *   - argument order: pattern = query, text = target (tests/debug/test_wfa_order.rs:1-31);
 *   - CIGAR op bytes, one per column, WFA2 alphabet: 'M' match, 'X' mismatch, 'I' consumes
 *     the text/target, 'D' consumes the pattern/query (src/alignment.rs:331-338,
 *     src/wfa.rs:128-149) -- so count_cigar_operations / parse_cigar_lengths /
 *     cigar_bytes_to_string (src/alignment.rs:292-376) apply unchanged;
 *   - bytes are compared verbatim (case-sensitive, 'N' == 'N');
 *   - only status 0 is success (AlignmentStatus::Completed, src/alignment.rs:233-258); the
 *     caller maps anything else to the "empty" result (src/alignment.rs:49-64).
 *
 * Plain C: pointers and sizes only, no C++ or torch types.  No global state; one engine per
 * GPU per process; calls on one engine must not overlap (single submitter).
 */
#ifndef ALLWAVE_HIP_H
#define ALLWAVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWV_ABI_VERSION 3

/* engine-level return codes (negative = failure; never aborts the process) */
#define AWV_OK 0
#define AWV_ERR_NO_DEVICE (-1)   /* no usable HIP device: the product path has no CPU fallback */
#define AWV_ERR_HIP (-2)         /* a HIP runtime call failed; see awv_last_error() */
#define AWV_ERR_ARG (-3)
#define AWV_ERR_PENALTIES (-4)   /* match != 0, x <= 0, e <= 0 ... (WFA2 would transform/reject) */
#define AWV_ERR_OOM (-5)
#define AWV_ERR_STATE (-6)       /* e.g. align before set_sequences */
#define AWV_ERR_SINK (-7)        /* the sink callback returned non-zero (first error wins) */

/* per-pair status (awv_result.status) */
#define AWV_ST_COMPLETED 0
#define AWV_ST_CAPACITY 1        /* an internal capacity bound was hit (wavefront width / history) */
/* One bound behind AWV_ST_CAPACITY is fixed: a workgroup's ring of wavefront rows (2 directions x 5 components x `ring` rows of
 * `wc` columns) is addressed with 32-bit offsets and must stay below 2 GiB, so rows hold at most
 * ((2^31 - 1) / (10 * ring * bytes per cell)) & ~255 columns -- with 32-bit cells (a sequence of 32,760 bases or more)
 * 838,656 at ring 64 (the default scores), 419,328 at ring 128 and 209,664 at ring 256 (ring: the power of two
 * >= max(x, o1+e1, o2+e2) + 3, plus up to 14 with multi-step passes).  A pair whose length difference alone cannot fit such
 * rows comes back AWV_ST_CAPACITY without being run; a pair whose wavefronts outgrow them (long, very divergent sequences)
 * comes back AWV_ST_CAPACITY after its last re-run. */
#define AWV_ST_INTERNAL 2        /* invariant violated (would be a bug) */
#define AWV_ST_MAX_STEPS 3       /* step guard tripped */
#define AWV_ST_ABOVE_BOUND 4     /* score-only and bounded calls: the penalty exceeds max_penalty */

typedef struct awv_engine awv_engine;

typedef struct {
  int32_t device;          /* HIP device ordinal */
  int32_t workgroups;      /* persistent workgroups = pairs in flight (0 = engine default: 16 per CU); the align kernels open
                              workgroups / (waves per workgroup) slots, at least one, and the record kernels (verify, clip,
                              split, normalize, encode, cs, coverage) launch min(records, workgroups) one-wave workgroups -- 0: min(records, 16 per CU) */
  int64_t max_batch_pairs; /* pairs per launch (0 = default) */
  int64_t max_arena_bytes; /* CIGAR arena budget per launch (0 = default 8 GiB) */
  int32_t flags;           /* AWV_F_* */
  int32_t first_row_cols;  /* 0 = default; > 0 caps the row width (columns, >= 2048) of a batch's first attempt: pairs whose
                              wavefronts outgrow it come back CAPACITY and are re-run wider (diagnostic / test hook) */
  int64_t max_scratch_bytes; /* cap on the per-workgroup wavefront arenas (0 = default 160 GiB) */
} awv_engine_config;

/* ---- flags a caller has a use for */
#define AWV_F_KEEP_ON_DEVICE 1 /* do not copy CIGARs back (kernel-only measurements) */
#define AWV_F_NO_ARENA_PROBE 32 /* take the first ring-arena allocation as it comes (default: allocate up to four candidates and keep the
                                   one a 1 ms traffic probe finds fastest -- worth up to 6 % of kernel time, costs 1-3 s once per engine:
                                   for short-lived processes with little work) */
#define AWV_F_NO_RERUN 1024    /* a pair whose wavefronts outgrow the first attempt's rows keeps status AWV_ST_CAPACITY instead of being re-run with
                                   wider rows (fail fast; with first_row_cols: the way to see a failed pair's record end to end) */
/* ---- variant pins: tests and A/B measurements only.  Results are identical under every one of them (tests/test_gpu_parity.py
 * runs the pairs of variants against each other and against the oracle); a product caller leaves them alone. */
#define AWV_F_FORCE_INT32 2    /* always use 32-bit wavefront rows, for every sub-problem (default: 16-bit when lengths < 32760,
                                  and -- in the four- and sixteen-wave flavours -- when only the shorter length is: rows of
                                  min(h, v); a launch with 32-bit rows searches the sub-problems that fit with 16-bit rows) */
#define AWV_F_NO_WIDE16 256    /* 32-bit rows whenever the longer sequence has 32760 bases or more (no min(h, v) rows) */
#define AWV_F_NO_PACKED_SEQ 4  /* never use the 2-bit packed sequences, staged in LDS or in place (raw-byte probes from HBM only) */
#define AWV_F_ONE_WAVE 8       /* always one wave per pair (default: four waves per pair for small batches, long sequences and unequal lengths, sixteen for a few very unequal pairs) */
#define AWV_F_FOUR_WAVES 16    /* always four waves per pair */
#define AWV_F_NO_CHAIN 128     /* multi-step passes of one sweep only (no chaining of sweeps through registers / LDS) */
#define AWV_F_NO_DEEP 512      /* the margin zone of a breakpoint search runs step by step (the round-2 path) instead of in passes that store every I/D row */
#define AWV_F_SINGLE_STEP 64   /* never use multi-step passes (every step stores all five rows; the round-1 kernel path) */
#define AWV_F_NO_TWIN 2048     /* align every entry of a pair list on its own (default: an entry (q, t) and its swapped entry (t, q) in the same launch
                                  are aligned as one unit that shares their breakpoint searches) */
#define AWV_F_TWIN_TOP_ONLY 4096 /* tests and A/B measurements only: such units share their top-level search only (default: every search whose sub-problem is still a mirror image) */
#define AWV_F_NO_TWIN_BASE 8192 /* tests and A/B measurements only: a base case under a shared search is run once per orientation (default: its wavefronts
                                   run once and are backtraced for both orientations) */
#define AWV_F_NO_ROW_REUSE 16384 /* tests and A/B measurements only: every breakpoint search computes all of its rows (default: in the one-wave kernels with
                                    16-bit rows the two searches below a pair's top-level search take the rows they share with it from an archive it keeps;
                                    awv_stats.prof[12] / prof[13] then count the cell-steps taken and the searches that took some) */
#define AWV_F_ROW_REUSE_LEVEL1 32768 /* tests and A/B measurements only: only the two searches right below a pair's top-level search take rows from its
                                        archive (default: every search below it that shares its origin or its end, however deep; awv_stats.prof[10] /
                                        prof[11] count the cell-steps and the searches of those further down, prof[12] / prof[13] stay the two's own) */

/* penalties as allwave passes them to lib_wfa2 (src/alignment.rs:263-289) */
typedef struct {
  int32_t match;     /* must be 0 */
  int32_t mismatch;  /* x  */
  int32_t gap_open1; /* o1 */
  int32_t gap_ext1;  /* e1 */
  int32_t gap_open2; /* o2, used when two_piece */
  int32_t gap_ext2;  /* e2, used when two_piece */
  int32_t two_piece; /* 0 = gap-affine (also allwave's "edit" mode x,x,x), 1 = 2-piece */
} awv_penalties;

typedef struct {
  int32_t q_idx;     /* query  = pattern */
  int32_t t_idx;     /* target = text */
  int32_t q_revcomp; /* align reverse_complement(query) (src/alignment.rs:178-190) */
} awv_pair;

typedef struct {
  int32_t status;         /* AWV_ST_* */
  int32_t penalty;        /* >= 0 */
  int32_t score;          /* = -penalty: what WFA2's cigar->score / wf.score() reports */
  uint32_t cigar_len;     /* op bytes */
  uint64_t cigar_off;     /* offset of the op bytes in the arena handed to the sink */
  int32_t num_matches;    /* #M */
  int32_t num_mismatches; /* #X */
  int32_t num_ins;        /* #I (text/target consumed) */
  int32_t num_del;        /* #D (pattern/query consumed) */
  int32_t q_end;          /* #M + #X + #D  (src/alignment.rs:320-344) */
  int32_t t_end;          /* #M + #X + #I */
} awv_result;

/* Sink: called once per launch batch with results[first..first+n) and the batch's CIGAR arena
 * (valid only during the call).  Calls never overlap and come in batch order; with several batches
 * in one awv_align_pairs call all but the last come from an engine-owned helper thread while the
 * next batch is being aligned (the reference's callback is invoked from worker threads too,
 * src/iterator.rs:208-252).  Return non-zero to stop: the call then fails with AWV_ERR_SINK before
 * any further sink call. */
typedef int (*awv_sink)(void* user, int64_t first, int64_t n, const awv_result* results,
                        const uint8_t* cigar_arena);

typedef struct {
  double kernel_ms;         /* HIP-event time of the alignment kernel launches, last call */
  double h2d_ms, d2h_ms;    /* copies, last call */
  uint64_t launches;        /* kernel launches, last call */
  uint64_t cell_steps;      /* wavefront cells computed (all components count as one cell) */
  uint64_t extend_steps;    /* 8-byte compare iterations of the extend loop, summed over lanes */
  uint64_t n_breakpoints;   /* BiWFA breakpoint searches */
  uint64_t n_base;          /* base-case alignments */
  uint64_t overlap_scans;   /* wavefront pairs scanned by the overlap search */
  uint64_t aligned_bp;      /* sum of query lengths of completed pairs */
  uint64_t pairs_completed;
  uint64_t scratch_bytes;   /* device scratch currently allocated */
  /* shader-clock cycles summed over workgroups; only filled by the -DAWV_PROF diagnostic build:
   * [0] total, [1] step compute, [2] step barrier wait, [3] step finalize, [4] overlap search,
   * [5] base-case steps, [6] backtrace, [7] CIGAR emission, [8] number of fused step passes,
   * [9..13] inside the step: row loads, DP arithmetic, extend, stores, reductions.
   * The product build stamps nothing; there [12] / [13] are the cell-steps taken from row archives by the two searches right below
   * a top-level search and those searches, [10] / [11] the same for the searches further down (AWV_F_ROW_REUSE_LEVEL1) */
  uint64_t prof[14];
  uint64_t restarts;          /* breakpoint searches run again step by step (multi-step passes met too early) */
  uint64_t multi_cell_steps;  /* cells computed by multi-step passes (I/D rows kept in registers) */
  uint64_t windows[4];        /* window iterations: [0] step-by-step (one step each), [1] multi-step passes (T steps each), [2] base case step-by-step, [3] base case multi-step passes */
  /* the shader clock the kernels actually ran at (ABI 3): every persistent workgroup stamps s_memtime (shader cycles) and
   * s_memrealtime (constant-rate ticks, `clock_tick_khz`) when it starts and when it has drained the work queue; summed over the
   * workgroups of the call's launches.  sustained clock = clock_cycles / clock_ticks * clock_tick_khz kHz */
  uint64_t clock_cycles, clock_ticks;
  uint64_t clock_tick_khz;    /* hipDeviceAttributeWallClockRate (100 000 on MI355X) */
  uint64_t deep_cell_steps;   /* of multi_cell_steps: cells of passes that also store every I/D row (the margin zone before the two searches meet) */
} awv_stats;

int awv_abi_version(void);
const char* awv_last_error(void); /* thread-local description of the last failure */

int awv_engine_create(const awv_engine_config* cfg, awv_engine** out);
void awv_engine_destroy(awv_engine* e);

/* Hands over the sequence set: n sequences, concatenated bytes, offsets[n+1].  The engine keeps
 * its own device copies (forward, reversed, and reverse-complement variants). */
int awv_engine_set_sequences(awv_engine* e, int32_t n, const uint8_t* concat_bytes,
                             const uint64_t* offsets);

/* Aligns pairs[0..npairs).  `out` (nullable) receives all results; `sink` (nullable) streams
 * them with their CIGARs.  out[i].cigar_off is relative to the batch arena passed to the sink. */
int awv_align_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                    awv_result* out, awv_sink sink, void* user);

/* Convenience mirror of AffineWavefronts::align + score + cigar for one pair
 * (src/alignment.rs:231-236).  cigar_buf needs plen + tlen bytes. */
int awv_align_one(awv_engine* e, const awv_penalties* pen, const uint8_t* pattern, int32_t plen,
                  const uint8_t* text, int32_t tlen, awv_result* result, uint8_t* cigar_buf,
                  size_t cigar_cap);

/* Score-only alignment (WFA2's AlignmentScope::ComputeScore): the optimal end-to-end penalty of pairs[0..npairs), no CIGAR.
 * Runs the top-level BiWFA breakpoint search only (its breakpoint score is the penalty); needs no CIGAR arena, so
 * max_arena_bytes never splits the call.  max_penalty >= 0 bounds the search: a pair whose penalty is proved above it stops
 * there and comes back AWV_ST_ABOVE_BOUND; max_penalty < 0 means no bound.  awv_engine_stats reports the call. */
typedef struct {
  int32_t status;  /* AWV_ST_* */
  int32_t penalty; /* exact when COMPLETED; max_penalty + 1 when ABOVE_BOUND; 0 on failure */
} awv_score_result;
int awv_score_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                    int32_t max_penalty /* < 0: no bound */, awv_score_result* out /* required */);

/* The same with a bound per pair: max_penalty[i] >= 0 bounds pair i (AWV_ST_ABOVE_BOUND with penalty max_penalty[i] + 1 when its
 * penalty is proved above it), max_penalty[i] < 0 leaves pair i unbounded.  awv_score_pairs is the one-bound case. */
int awv_score_pairs_bounded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                            const int32_t* max_penalty /* per pair, < 0: none */, awv_score_result* out /* required */);

/* ---- WFA orientation (determine_orientation_wfa, src/alignment.rs:157-175) ----------------------------------------------
 * The reference aligns a pair on both strands under the orientation penalties `pen` and takes forward iff
 * E_f <= E_r, E = #X + #I + #D of the strand's CIGAR.  With P a strand's optimal penalty, every edit column of ANY optimal
 * CIGAR adds at least cmin = min(x, e1[, e2]) and at most cmax = max(x, o1 + e1) (2-piece: max(x, min(o1 + e1, o2 + e2))), so
 *     ceil(P / cmax) <= E <= floor(P / cmin).
 * Hence forward is certain when floor(P_f / cmin) <= ceil(L_r / cmax) for any proved lower bound L_r <= P_r, and reverse is
 * certain when floor(P_r / cmin) < ceil(L_f / cmax).  awv_orient_pairs decides every pair it can from bounded score-only
 * searches (a race of a few rounds over a shrinking list of strands; the losing strand's search stops at the bound that
 * settles the pair) and runs the two full alignments only for the pairs the rule leaves open ("ambiguous").  The strands
 * are the reference's in either case.
 * The race is skipped -- every pair goes the full way -- when cmax >= 8 * cmin (AWV_ORIENT_SKIP_RATIO): the rule then
 * settles next to nothing, and the losing strand would be searched almost to its end anyway.  A single pair leaves the race
 * for the full alignments as soon as the bound that would settle it exceeds W = G + x * min(plen, tlen) / 2, G the cheapest
 * gap of |plen - tlen| columns: about what an unrelated strand costs, so that search would complete instead of settling
 * (very unequal lengths -- before round 0 --, very divergent pairs).  A cost estimate only: the answer is the same. */
#define AWV_ORIENT_FORWARD 0
#define AWV_ORIENT_REVERSE 1
#define AWV_ORIENT_UNDECIDED 2
#define AWV_ORIENT_SKIP_RATIO 8
#define AWV_ORIENT_BY_BOUND 0 /* awv_orient_result.how: from the proved penalty intervals */
#define AWV_ORIENT_BY_EDITS 1 /* from the edit counts of two full alignments */
#define AWV_ORIENT_FULL 1     /* flags: two full alignments for every pair (the reference's method; yardstick and opt-out) */
#define AWV_ORIENT_NO_EDITS UINT64_MAX /* edits of a strand that was not aligned in full, or whose alignment failed */

typedef struct {
  int32_t is_reverse;   /* 1: reverse-complement the query */
  int32_t how;          /* AWV_ORIENT_BY_BOUND / AWV_ORIENT_BY_EDITS */
  int32_t lo_f, hi_f;   /* proved interval of the forward strand's penalty; hi = INT32_MAX when only bounded below */
  int32_t lo_r, hi_r;   /* the reverse-complement strand's */
  uint64_t edits_f;     /* BY_EDITS: #X + #I + #D of the full alignments (AWV_ORIENT_NO_EDITS: failed); BY_BOUND: NO_EDITS */
  uint64_t edits_r;
  int32_t rounds;       /* score-only rounds the pair took part in (0: race skipped) */
  int32_t reserved;
} awv_orient_result;

/* Orients pairs[0..npairs) (q_revcomp is ignored).  flags: 0 or AWV_ORIENT_FULL.  awv_engine_stats afterwards reports the
 * whole call: launches, kernel time, cell-steps ... summed over the race's rounds and the full-alignment tail. */
int awv_orient_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, int32_t flags,
                     awv_orient_result* out /* required */);
/* The rule alone, on the host (needs no device): AWV_ORIENT_FORWARD / _REVERSE / _UNDECIDED from proved penalty intervals
 * [lo, hi] of the two strands (hi = INT32_MAX: unknown above); AWV_ERR_PENALTIES / AWV_ERR_ARG (< 0) on bad input.  The
 * race's device kernel applies this very function (csrc/orient_device.hpp). */
int awv_orient_decide(const awv_penalties* pen, int32_t lo_f, int32_t hi_f, int32_t lo_r, int32_t hi_r);
/* The bound the race gives the other strand's search once one strand's penalty is known: the smallest B >= 0 such that
 * "the other strand's penalty exceeds B" (a lower bound of B + 1) settles the pair; -1 when the known penalty settles
 * it alone (INT32_MAX: no bound; INT32_MIN: bad input).  known_is_reverse: which strand `penalty` belongs to. */
int32_t awv_orient_settling_bound(const awv_penalties* pen, int32_t known_is_reverse, int32_t penalty);

int awv_engine_stats(const awv_engine* e, awv_stats* out);
/* Twin units of the last awv_align_pairs[_verified] or unbounded awv_score_pairs call: out[0] units made of an entry and its swapped entry, out[1] breakpoint
 * searches run once for both, out[2] searches run per orientation inside such units, out[3] shared searches whose two
 * breakpoints were not mirror images of each other (a tie that the two orientations break differently). */
int awv_twin_stats(const awv_engine* e, uint64_t out[4]);

/* ---- verification on the device (csrc/verify.hip, csrc/verify_device.hpp) ---------------------------------------------
 * What the reference's validators check (validation.rs verify_cigar_alignment, validation_simple.rs, wfa.rs
 * validate_cigar_alignment), plus the penalty: an op string is verified against its pair when every column is what it
 * says, both sequences are consumed end to end, and the record's counts and penalty are the op string's.  The pattern is
 * the query, or its reverse complement when q_revcomp is set; bytes compare verbatim; 'I' consumes the text, 'D' the
 * pattern.  Re-scoring: each 'X' adds x; a maximal run of L equal gap ops adds o1 + L e1 (2-piece: min(o1 + L e1,
 * o2 + L e2)); an 'I' run followed directly by a 'D' run is two runs.
 * The code is the FIRST failure in this order: */
#define AWV_VF_OK 0        /* verified */
#define AWV_VF_SKIPPED 1   /* status is not AWV_ST_COMPLETED: nothing to check */
/* column-level, the smallest column wins; within one column in this order: */
#define AWV_VF_BAD_OP 2    /* the byte is not one of M, X, I, D */
#define AWV_VF_OVERRUN 3   /* the column needs a base beyond the end of either sequence */
#define AWV_VF_M_DIFFERS 4 /* an 'M' column whose bytes differ */
#define AWV_VF_X_EQUAL 5   /* an 'X' column whose bytes are equal */
/* on the whole string, after every column has passed: */
#define AWV_VF_SHORT 6     /* the ops end before both sequences are consumed */
#define AWV_VF_COUNTS 7    /* cigar_len, num_matches, num_mismatches, num_ins, num_del, q_end or t_end is not the op string's */
#define AWV_VF_PENALTY 8   /* the re-scored penalty differs from `penalty`, or score != -penalty */

typedef struct {
  int32_t code;     /* AWV_VF_* */
  int32_t reserved;
  int64_t column;   /* index of the offending op byte for column-level codes, else -1 */
  int64_t penalty;  /* the op string re-scored under pen when every column-level check passed, else -1 */
} awv_verify_result; /* 24 bytes */

typedef struct {
  double kernel_ms;  /* HIP-event time of the verify launches of the last verifying call */
  uint64_t pairs;    /* pairs handed to the check (skipped ones included) */
  uint64_t failed;   /* of them: code other than AWV_VF_OK / AWV_VF_SKIPPED */
  uint64_t columns;  /* op bytes looked at: min(cigar_len, pattern + text length + 1) of every pair not skipped, failed ones included */
} awv_verify_stats;

/* awv_align_pairs, and every batch's finished pairs checked on the device, on the engine's stream, before the batch's CIGARs
 * are copied back (pairs re-run after AWV_ST_CAPACITY included; also under AWV_F_KEEP_ON_DEVICE).  vout[i] belongs to
 * pairs[i].  Results and CIGARs are those of awv_align_pairs; a failed check is reported, never repaired. */
int awv_align_pairs_verified(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, awv_result* out,
                             awv_verify_result* vout /* required */, awv_sink sink, void* user);
/* The same check on records and op bytes the caller supplies, against the resident sequence set: results[i] claims that
 * cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i].  The arena goes up in pieces of at most max_arena_bytes.
 * A completed record whose op bytes lie outside the arena: AWV_ERR_ARG (nothing is read on the device). */
int awv_verify_cigars(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const awv_result* results,
                      const uint8_t* cigar_arena, uint64_t arena_bytes, awv_verify_result* vout /* required */);
/* The contract alone, on the host (needs no device): the yardstick the kernel is tested against, not a fallback -- no
 * product path calls it.  cigar: n op bytes; claimed: the record. */
int awv_verify_one_host(const awv_penalties* pen, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                        const uint8_t* cigar, int64_t n, const awv_result* claimed, awv_verify_result* out);
/* The last verifying call (awv_align_pairs_verified / awv_verify_cigars) of this engine. */
int awv_engine_verify_stats(const awv_engine* e, awv_verify_stats* out);

/* ---- ranges: sub-intervals of resident sequences ---------------------------------------------------------------------------
 * An awv_pair aligns two whole sequences; an awv_range_pair aligns query[q_beg, q_end) against target[t_beg, t_end), globally
 * (end to end over the two intervals), without the caller cutting and uploading substrings.  Coordinates follow PAF: the
 * query interval is given on the query's FORWARD strand whatever q_revcomp says; with q_revcomp the pattern is
 * reverse_complement(query[q_beg, q_end)), which the engine finds at [L - q_end, L - q_beg) of its resident
 * reverse-complement copy (L the query's length).  Empty intervals are legal: the result is one run of 'I' or 'D', or an
 * empty CIGAR with penalty 0.  The calls below follow the contracts of their whole-sequence counterparts in every other
 * respect (results, sinks, batches, statuses, stats -- aligned_bp sums the query intervals' lengths).
 * awv_result is unchanged: q_end / t_end stay the consumed lengths (#M + #X + #D, #M + #X + #I), so they are RELATIVE TO THE
 * RANGE -- the interval's length for a completed record -- not positions in the sequences.
 * AWV_ERR_ARG, before anything is launched, for an index out of range or an interval with beg < 0, beg > end or end > length.
 * The kernels take the packed (2-bit) path when the two SEQUENCES are pure upper-case ACGT, as for whole pairs: an 'N' outside
 * a range sends it down the raw-byte path, with equal results. */
typedef struct {
  int32_t q_idx, t_idx, q_revcomp;
  int32_t q_beg, q_end;   /* [q_beg, q_end) on the query's FORWARD strand (PAF convention) */
  int32_t t_beg, t_end;   /* [t_beg, t_end) on the target */
} awv_range_pair;         /* 28 bytes */

/* awv_align_pairs / awv_align_pairs_verified on ranges. */
int awv_align_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, awv_result* out,
                     awv_sink sink, void* user);
int awv_align_ranges_verified(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, awv_result* out,
                              awv_verify_result* vout /* required */, awv_sink sink, void* user);
/* awv_score_pairs_bounded on ranges; max_penalty == NULL: no bound for any range. */
int awv_score_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                     const int32_t* max_penalty /* per range, nullable; < 0: none */, awv_score_result* out /* required */);
/* awv_verify_cigars on ranges: results[i] claims that its op bytes align ranges[i] end to end over the two intervals. */
int awv_verify_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                      const uint8_t* cigar_arena, uint64_t arena_bytes, awv_verify_result* vout /* required */);

/* ---- full alignments under a penalty bound ------------------------------------------------------------------------------
 * awv_align_pairs with a bound per pair: max_penalty[i] >= 0 bounds pair i, max_penalty[i] < 0 leaves it unbounded.  A pair
 * whose penalty is proved above its bound is abandoned inside its top-level breakpoint search -- no sub-problem is searched,
 * no CIGAR is written -- and comes back AWV_ST_ABOVE_BOUND with penalty max_penalty[i] + 1, cigar_len 0, all four counts and
 * q_end / t_end 0.  The bound confines the top-level search only: every sub-problem runs as in awv_align_pairs.
 * The contract:
 *   - for every pair, status and penalty are what awv_score_pairs_bounded reports under the same bounds;
 *   - for every AWV_ST_COMPLETED pair, the whole record and the op bytes are awv_align_pairs's, byte for byte.
 * vout (nullable): non-null gives awv_align_pairs_verified's check; an AWV_ST_ABOVE_BOUND record verifies as AWV_VF_SKIPPED.
 * Arena slots, batching, sinks and stats are awv_align_pairs's. */
int awv_align_pairs_bounded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                            const int32_t* max_penalty /* per pair, required; < 0: none */, awv_result* out,
                            awv_verify_result* vout /* nullable */, awv_sink sink, void* user);
/* The same on ranges; max_penalty == NULL: no bound for any range (as in awv_score_ranges). */
int awv_align_ranges_bounded(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                             const int32_t* max_penalty /* per range, nullable; < 0: none */, awv_result* out,
                             awv_verify_result* vout /* nullable */, awv_sink sink, void* user);
/* The penalty bound that no alignment of divergence <= d can exceed, on the host (needs no device).  Divergence of an
 * alignment = E / columns, E = #X + #I + #D, columns = #M + #X + #I + #D.  From columns = plen + #I = tlen + #D follows
 * E <= d (plen + tlen) / (2 - d), and every edit column costs at most cmax (as above: max(x, o1 + e1), 2-piece:
 * max(x, min(o1 + e1, o2 + e2))), so
 *     B = cmax * (floor(d (plen + tlen) / (2 - d)) + 1)
 * (the + 1 absorbs floating-point rounding; an exact filter on the counts follows anyway).  A penalty above B proves that no
 * alignment of the pair, optimal or not, has divergence <= d.  Returns -1 ("no bound") when d >= 1 or B would pass
 * INT32_MAX; INT32_MIN for d < 0, NaN, negative lengths or bad penalties. */
int32_t awv_divergence_bound(const awv_penalties* pen, int32_t plen, int32_t tlen, double d);

/* ---- clipping to the best-scoring segment (csrc/clip.hip, csrc/clip_device.hpp) --------------------------------------------
 * Every alignment above is global: end to end over the sequences or the intervals, also through flanks that share nothing.
 * The clip of an op string is the part of it worth reporting.  It is a pure function of the op bytes c[0..n) over M X I D,
 * the penalties and a match bonus a >= 1; no sequence is read.
 * The score of a segment [i, j) of columns is a * #M - penalty(c[i..j)), the penalty being the segment re-scored as an op
 * string of its own by the rule of the verification above: each 'X' adds x, each maximal run of L equal gap ops adds
 * gap_cost(L) = o1 + L e1 (2-piece: min(o1 + L e1, o2 + L e2)), an 'I' run followed by a 'D' run is two runs.
 * The clip is the segment of maximal score; among those the one with the smallest end; among those the one with the largest
 * begin; empty when no segment scores above 0.  A maximal segment begins and ends with an 'M' column (dropping a leading
 * or trailing 'X' or gap column strictly raises the score), so no gap run is ever cut, and the contract equals this walk:
 *     S = 0; minS = 0; minI = 0; best = 0; b = e = 0
 *     for c in 0..n:
 *         S += a for 'M', -x for 'X', -(gap_cost(L) - gap_cost(L - 1)) for the L-th column of its gap run (gap_cost(0) = 0)
 *         if S <= minS: minS = S; minI = c + 1                        (a tie moves the minimum: the latest argmin)
 *         if S - minS > best: best = S - minS; b = minI; e = c + 1    (a tie keeps the best: the first argmax)
 * The clip is a slice description: records, op bytes and arenas are those of the unclipped call. */
#define AWV_CL_OK 0       /* the record holds a clip */
#define AWV_CL_SKIPPED 1  /* status is not AWV_ST_COMPLETED (AWV_ST_ABOVE_BOUND included): nothing to clip; all other fields 0 */
#define AWV_CL_EMPTY 2    /* no segment scores above 0; all other fields 0 */
#define AWV_CL_BAD_OP 3   /* a byte that is not M, X, I or D: col_beg = col_end = the smallest such column; all other fields 0 */
#define AWV_CLIP_MAX_BONUS 32767

typedef struct {
  int32_t code;            /* AWV_CL_* */
  int32_t reserved;
  int64_t score;           /* a * num_matches - penalty, > 0 */
  uint32_t col_beg, col_end; /* the segment, as a slice [col_beg, col_end) of the op string */
  int32_t q_skip, t_skip;  /* pattern bases (ops other than 'I') and text bases (ops other than 'D') consumed before col_beg */
  int32_t num_matches, num_mismatches, num_ins, num_del; /* of the segment */
  int32_t penalty;         /* the segment re-scored as an op string of its own */
  int32_t reserved2;
} awv_clip_result;         /* 56 bytes */

typedef struct {
  double kernel_ms;  /* HIP-event time of the clip launches of the last clipping call */
  uint64_t pairs;    /* records handed to the clip (skipped ones included) */
  uint64_t empty;    /* of them: AWV_CL_EMPTY */
  uint64_t columns;  /* op bytes of the records not skipped */
} awv_clip_stats;

/* The contract alone, on the host (needs no device): the yardstick the kernel is tested against, not a fallback -- no product
 * path calls it.  AWV_ERR_ARG unless 1 <= match_bonus <= AWV_CLIP_MAX_BONUS (every clipping call). */
int awv_clip_one_host(const awv_penalties* pen, int32_t match_bonus, const uint8_t* cigar, int64_t n, awv_clip_result* out);
/* Clips records and op bytes the caller supplies, on the device: cout[i] is the clip of
 * cigar_arena[results[i].cigar_off, + cigar_len) when results[i].status is AWV_ST_COMPLETED, else AWV_CL_SKIPPED.  The arena
 * goes up in pieces of at most max_arena_bytes.  Reads no sequence: the engine needs no sequence set.  A completed record
 * whose op bytes lie outside the arena: AWV_ERR_ARG (nothing is read on the device). */
int awv_clip_cigars(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, const awv_result* results, int64_t n,
                    const uint8_t* cigar_arena, uint64_t arena_bytes, awv_clip_result* cout /* required */);
/* awv_align_pairs_bounded / awv_align_ranges_bounded, and every batch's finished pairs clipped on the device, on the engine's
 * stream, after the optional check and before the batch's CIGARs are copied back (pairs re-run after AWV_ST_CAPACITY
 * included; also under AWV_F_KEEP_ON_DEVICE).  cout[first .. first + n) is filled before that batch's sink call, as vout is.
 * Records, op bytes, arena slots, batching and stats are those of the unclipped call, byte for byte: the full op string
 * still reaches the sink.  max_penalty == NULL: no bound for any pair. */
int awv_align_pairs_clipped(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                            const int32_t* max_penalty /* per pair, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                            awv_verify_result* vout /* nullable */, awv_clip_result* cout /* required */, awv_sink sink, void* user);
int awv_align_ranges_clipped(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                             const int32_t* max_penalty /* per range, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                             awv_verify_result* vout /* nullable */, awv_clip_result* cout /* required */, awv_sink sink, void* user);
/* The last clipping call (awv_align_*_clipped / awv_clip_cigars) of this engine. */
int awv_engine_clip_stats(const awv_engine* e, awv_clip_stats* out);

/* ---- splitting into all good segments (csrc/split.hip, csrc/split_device.hpp) ----------------------------------------------
 * The clip keeps one segment of an op string; the split keeps every maximal one that scores at least min_score (Ruzzo and
 * Tompa's "all maximal scoring subsequences", with the clip's tie rules inside every interval).  A pure function of the op
 * bytes c[0..n), the penalties, a match bonus 1 <= a <= AWV_CLIP_MAX_BONUS and a threshold min_score >= 1; no sequence is read:
 *     segments(lo, hi):
 *         if hi <= lo: return []
 *         r = clip(c[lo..hi))                  (the slice re-scored as an op string of its own, the contract above)
 *         if r is empty or r.score < min_score: return []
 *         b, e = lo + r.col_beg, lo + r.col_end
 *         return segments(lo, b) + [[b, e)] + segments(e, hi)
 *     split(c) = segments(0, n)
 * No part of an interval scores above that interval's clip, so the pruning at min_score is exact.  The segments are disjoint
 * and ascending, each begins and ends with an 'M' (no gap run is cut) and scores at least min_score, and what is left between
 * them holds nothing that does.  When the clip of the whole string scores at least min_score it is one of the segments, the
 * top-scoring one.  Each segment needs ceil(min_score / a) 'M' columns, so a string with m of them has at most
 * awv_split_slots(a, min_score, m) = floor(a * m / min_score) segments.
 * A segment is an awv_clip_result with code AWV_CL_OK: col_beg / col_end are columns of the WHOLE op string, q_skip / t_skip
 * the bases consumed before col_beg in the whole string; counts, penalty and score are the segment's.
 * Segment storage is the caller's and its layout is fixed before the call: seg_first holds n + 1 ascending entries, record i
 * owns sout[seg_first[i] .. seg_first[i + 1]) and its iout[i].count segments lie at the front of that region in ascending
 * col_beg; the slots behind them are left untouched.  A call is refused with AWV_ERR_ARG, before anything is launched, when a
 * record owns fewer slots than it may need: the aligning calls need awv_split_slots(a, min_score, min(plen, tlen)) over the
 * pattern and text lengths (the two interval lengths for ranges), awv_split_cigars needs awv_split_slots(a, min_score,
 * cigar_len) -- not num_matches, which a caller's record may misstate. */
typedef struct {
  int32_t code;    /* AWV_CL_OK: count >= 1 segments; AWV_CL_EMPTY: none reaches min_score; AWV_CL_SKIPPED: status is not
                      AWV_ST_COMPLETED (AWV_ST_ABOVE_BOUND included); AWV_CL_BAD_OP: as for the clip, count 0 */
  int32_t count;   /* segments of the record */
  int64_t column;  /* AWV_CL_BAD_OP: the smallest offending column; -1 for every other code */
} awv_split_index;   /* 16 bytes */

typedef struct {
  double kernel_ms;          /* HIP-event time of the split launches of the last splitting call */
  uint64_t pairs;            /* records handed to the split (skipped ones included) */
  uint64_t segments;         /* segments written */
  uint64_t empty;            /* records not skipped that have no segment (AWV_CL_EMPTY) */
  uint64_t columns;          /* op bytes of the records not skipped */
  uint64_t columns_scanned;  /* columns of every interval a wave scanned: / columns = the re-scan factor */
} awv_split_stats;

/* floor(match_bonus * m / min_score), on the host; -1 unless 1 <= match_bonus <= AWV_CLIP_MAX_BONUS, min_score >= 1, m >= 0. */
int64_t awv_split_slots(int32_t match_bonus, int64_t min_score, int64_t m);
/* seg_first[0] = 0, seg_first[i + 1] = seg_first[i] + what the aligning calls require for entry i: host arithmetic over the
 * resident set's lengths.  AWV_ERR_ARG for a bad index or interval, AWV_ERR_STATE without a sequence set. */
int awv_split_layout_pairs(awv_engine* e, const awv_pair* pairs, int64_t n, int32_t match_bonus, int64_t min_score,
                           uint64_t* seg_first /* n + 1 */);
int awv_split_layout_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, int32_t match_bonus, int64_t min_score,
                            uint64_t* seg_first /* n + 1 */);
/* The contract alone, on the host (needs no device), written as the recursion over the clip's host walk: the yardstick the
 * kernel is tested against, not a fallback -- no product path calls it.  sout: cap slots; *count: the segments found, of which
 * min(*count, cap) are written, in ascending col_beg.  index (nullable): the record's awv_split_index. */
int awv_split_one_host(const awv_penalties* pen, int32_t match_bonus, int64_t min_score, const uint8_t* cigar, int64_t n,
                       awv_clip_result* sout, int64_t cap, int64_t* count /* required */, awv_split_index* index);
/* Splits records and op bytes the caller supplies, on the device; staged and pieced as awv_clip_cigars does.  Reads no
 * sequence: the engine needs no sequence set.  A completed record whose op bytes lie outside the arena: AWV_ERR_ARG. */
int awv_split_cigars(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, int64_t min_score, const awv_result* results,
                     int64_t n, const uint8_t* cigar_arena, uint64_t arena_bytes, const uint64_t* seg_first /* n + 1 */,
                     awv_split_index* iout /* required */, awv_clip_result* sout /* required when any slot exists */);
/* awv_align_pairs_clipped / awv_align_ranges_clipped with the split in the clip's place: every batch's finished pairs are
 * split on the device, on the engine's stream, after the optional check and before the batch's CIGARs are copied back;
 * iout / sout of a batch are filled before that batch's sink call.  Records, op bytes, arena slots, batching and stats are
 * those of the unsplit call, byte for byte. */
int awv_align_pairs_split(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                          const int32_t* max_penalty /* per pair, nullable; < 0: none */, int32_t match_bonus, int64_t min_score,
                          awv_result* out, awv_verify_result* vout /* nullable */, const uint64_t* seg_first /* npairs + 1 */,
                          awv_split_index* iout /* required */, awv_clip_result* sout, awv_sink sink, void* user);
int awv_align_ranges_split(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                           const int32_t* max_penalty /* per range, nullable; < 0: none */, int32_t match_bonus, int64_t min_score,
                           awv_result* out, awv_verify_result* vout /* nullable */, const uint64_t* seg_first /* n + 1 */,
                           awv_split_index* iout /* required */, awv_clip_result* sout, awv_sink sink, void* user);
/* The last splitting call (awv_align_*_split / awv_split_cigars) of this engine. */
int awv_engine_split_stats(const awv_engine* e, awv_split_stats* out);

/* ---- gap runs moved to a canonical place (csrc/normalize.hip, csrc/normalize_device.hpp) ---------------------------------------
 * Where a gap sits among co-optimal alignments is a tie-break: in a repeat the same indel can lie anywhere along it at the
 * same penalty.  Normalization moves every gap run as far left as it goes without changing anything else.  It is a pure
 * function of an op string c[0..n) over M X I D and the two sequences it aligns; no penalties are involved.  'I' consumes the
 * text, 'D' the pattern; the pattern is the query, or its reverse complement under q_revcomp; bytes compare verbatim; a
 * range call's pattern and text are its intervals.
 * One left step: a maximal gap run of type g over columns [c, c + L) consumes bases [p, p + L) of its own sequence (the
 * pattern for 'D', the text for 'I').  It moves one column left when column c - 1 is 'M', seq[p - 1] == seq[p + L - 1], and
 * column c - 2 is not also g (a run never comes to rest directly next to a run of its own type): column c - 1 becomes g,
 * column c + L - 1 becomes 'M' -- still a true match, since seq[p + L - 1] == seq[p - 1] equals the other sequence's base.
 * The number, order, types and lengths of all runs, the counts and the penalty under any penalties are unchanged: the record
 * stays valid as it is, only op bytes move.  The left-normal form is the string in which no run can take a step; it is unique.
 * Closed form: number the gap runs left to right; m_i = the 'M' columns directly before run i in the input; a_i = the largest k
 * with seq[p_i - j] == seq[p_i + L_i - j] for j = 1..k; run i is linked to run i - 1 when only 'M' columns lie between them.
 *     s_i = min(a_i, b_i)      b_i = m_i                                              when not linked
 *                              b_i = m_i + s_(i-1) - (type_i == type_(i-1) ? 1 : 0)   when linked
 * and the output is the input with columns [c_i - s_i, c_i - s_i + L_i) set to g_i and [c_i - s_i + L_i, c_i + L_i) set to
 * 'M', for every i (disjoint zones).  The right-normal form is the mirror image:
 *     right(c, P, T) = reverse(left(reverse(c), reverse(P), reverse(T)))
 * (a '-' line's query is reverse-complemented: "left in the target's frame" is "right in the query's forward frame").
 * Checked up front, before any byte of the string is changed; on any code but AWV_NM_OK the string is left untouched.  M / X
 * truth is not checked: that is the verification's job. */
#define AWV_NORM_OFF 0
#define AWV_NORM_LEFT 1
#define AWV_NORM_RIGHT 2
#define AWV_NM_OK 0       /* normalized */
#define AWV_NM_SKIPPED 1  /* status is not AWV_ST_COMPLETED */
#define AWV_NM_BAD_OP 2   /* a byte outside MXID: columns_moved holds the smallest such column */
#define AWV_NM_LENGTHS 3  /* the ops do not consume exactly plen and tlen */

typedef struct {
  int32_t code;          /* AWV_NM_* */
  int32_t runs_moved;    /* gap runs with s_i > 0 */
  int64_t columns_moved; /* the sum of s_i (AWV_NM_BAD_OP: the smallest offending column) */
  int32_t max_shift;     /* the largest s_i */
  int32_t reserved;
} awv_norm_result;       /* 24 bytes */

typedef struct {
  double kernel_ms;        /* HIP-event time of the normalize launches of the last normalizing call */
  uint64_t pairs;          /* records handed to the step (skipped ones included) */
  uint64_t records_moved;  /* of them: at least one run moved */
  uint64_t runs;           /* gap runs of the records normalized */
  uint64_t runs_moved;
  uint64_t columns_moved;  /* the sum of all s_i */
  uint64_t columns;        /* op bytes of the records not skipped */
} awv_norm_stats;

/* The contract alone, on the host (needs no device): a serial walk, the yardstick the kernel is tested against, not a
 * fallback -- no product path calls it.  direction: AWV_NORM_LEFT / AWV_NORM_RIGHT.  out_cigar: n bytes, may be `cigar`. */
int awv_normalize_one_host(int32_t direction, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                           const uint8_t* cigar, int64_t n, uint8_t* out_cigar, awv_norm_result* out);
/* Normalizes records and op bytes the caller supplies, in place, against the resident sequence set: results[i] claims that
 * cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  The arena goes up and back in pieces of at most
 * max_arena_bytes; the op strings of two records must not overlap.  A completed record whose op bytes lie outside the arena:
 * AWV_ERR_ARG before anything is launched. */
int awv_normalize_cigars(awv_engine* e, int32_t direction, const awv_pair* pairs, int64_t n, const awv_result* results,
                         uint8_t* cigar_arena /* in/out */, uint64_t arena_bytes, awv_norm_result* nout /* required */);
int awv_normalize_ranges(awv_engine* e, int32_t direction, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                         uint8_t* cigar_arena /* in/out */, uint64_t arena_bytes, awv_norm_result* nout /* required */);
/* The engine's mode (AWV_NORM_OFF by default), read at the start of every aligning call: awv_align_pairs, awv_align_ranges,
 * their _verified, _bounded, _clipped, _split, _encoded and _cs forms, and awv_align_one.  When it is on, every batch's finished pairs are
 * normalized in the batch's arena on the device, on the engine's stream (pairs re-run after AWV_ST_CAPACITY included; also
 * under AWV_F_KEEP_ON_DEVICE), BEFORE the optional check, clip and split and before the copy back: vout, cout and the
 * segments describe the normalized string.  Records are byte-identical to the unnormalized call's.  When it is off there is
 * no launch, no allocation and no change.  Score-only and orientation calls ignore the mode. */
int awv_engine_set_normalize(awv_engine* e, int32_t mode);
/* The last normalizing call (an aligning call under a mode, awv_normalize_cigars / _ranges) of this engine. */
int awv_engine_normalize_stats(const awv_engine* e, awv_norm_stats* out);

/* ---- run-length CIGAR text made on the device (csrc/encode.hip, csrc/encode_device.hpp) ---------------------------------------
 * The engine keeps a CIGAR as one op byte per column; what a PAF line carries behind cg:Z: is its run-length text.  The text of
 * an op string c[0..n) is exactly what the reference's cigar_bytes_to_string (src/alignment.rs:347-376) returns: every maximal
 * run of equal bytes becomes its length in decimal followed by one character, 'M' -> '=', 'X' -> 'X', 'I' -> 'D', 'D' -> 'I'
 * (the gap letters swap), any other byte -> '?'.  An empty string has empty text.  A slice [col_beg, col_end) of a string is
 * encoded as an op string of its own, so a slice that begins or ends inside a run cuts that run.  A record whose status is not
 * AWV_ST_COMPLETED (AWV_ST_ABOVE_BOUND included) has empty text.  A pure function of the op bytes: no sequence, no penalties.
 * Layout: the texts of a call's (or a batch's) records lie in one text arena, dense and in record order -- off[0] = 0 and
 * off[i + 1] = off[i] + len[i] -- so one contiguous copy of exactly the text bytes brings them home, and the layout does not
 * depend on the order the device worked in.  A string or slice holds at most 2^31 - 1 columns (AWV_ERR_ARG beyond). */
typedef struct {
  uint64_t off;   /* of the record's text in the text arena */
  uint32_t len;   /* characters */
  uint32_t runs;  /* maximal runs = letters in the text */
} awv_cigar_text; /* 16 bytes */

typedef struct {
  double kernel_ms;     /* HIP-event time of the encode launches (measure, scan, emit) of the last encoding call */
  uint64_t pairs;       /* records handed to the step (the ones without text included) */
  uint64_t runs;        /* runs encoded */
  uint64_t text_bytes;  /* characters of all texts */
  uint64_t columns;     /* op bytes of the strings and slices encoded */
} awv_encode_stats;

/* The contract alone, on the host (needs no device): a serial walk, the yardstick the kernels are tested against, not a
 * fallback -- no product path calls it.  out->off is 0; the text is written to out_buf only when out->len <= cap. */
int awv_encode_one_host(const uint8_t* cigar, int64_t n, uint8_t* out_buf, uint64_t cap, awv_cigar_text* out /* required */);
/* Encodes records and op bytes the caller supplies, on the device; staged and pieced as awv_clip_cigars does, the offsets
 * running on from piece to piece.  slices (nullable): 2 n entries, record i is encoded over its columns [slices[2 i],
 * slices[2 i + 1]).  Reads no sequence: the engine needs no sequence set.  tout[0..n) and *text_bytes (the arena's size) are always
 * filled; the text is written to text_buf only when *text_bytes <= text_cap -- all of it or nothing -- so text_buf == NULL with
 * text_cap == 0 is the measuring call.  AWV_ERR_ARG, before anything is launched, for a completed record whose op bytes lie
 * outside the arena and for a slice with col_beg > col_end or col_end > cigar_len. */
int awv_encode_cigars(awv_engine* e, const awv_result* results, int64_t n, const uint8_t* cigar_arena, uint64_t arena_bytes,
                      const uint32_t* slices /* nullable */, awv_cigar_text* tout /* required */, uint8_t* text_buf, uint64_t text_cap,
                      uint64_t* text_bytes /* required */);
/* awv_align_pairs_clipped / awv_align_ranges_clipped with every batch's finished pairs encoded on the device, on the engine's
 * stream, last of the per-batch steps (after normalization, the optional check and the optional clip: the text is of the
 * normalized string under a mode).  match_bonus == 0: no clip, cout is not read and the text is the whole string's;
 * match_bonus >= 1: cout is required and the text is the clip's slice [col_beg, col_end), empty when the clip's code is not
 * AWV_CL_OK.  Records, vout and cout are the unencoded call's, byte for byte: cigar_off / cigar_len still describe the op
 * bytes, which stay on the device and are NOT copied back.  The sink is called as always, but its cigar_arena argument is the
 * batch's text arena, and tout[first .. first + n) is filled before the call, relative to that arena.  Under
 * AWV_F_KEEP_ON_DEVICE the step runs and tout is filled, but no text is copied (the sink's arena is NULL). */
int awv_align_pairs_encoded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                            const int32_t* max_penalty /* per pair, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                            awv_verify_result* vout /* nullable */, awv_clip_result* cout /* nullable when match_bonus == 0 */,
                            awv_cigar_text* tout /* required */, awv_sink sink, void* user);
int awv_align_ranges_encoded(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                             const int32_t* max_penalty /* per range, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                             awv_verify_result* vout /* nullable */, awv_clip_result* cout /* nullable when match_bonus == 0 */,
                             awv_cigar_text* tout /* required */, awv_sink sink, void* user);
/* The last encoding call (awv_align_*_encoded / awv_encode_cigars) of this engine. */
int awv_engine_encode_stats(const awv_engine* e, awv_encode_stats* out);

/* ---- minimap2's cs difference string made on the device (csrc/cs.hip, csrc/cs_device.hpp) --------------------------------------
 * The text behind a PAF line's cs:Z: tag says what the differing bases are.  The inputs are an op string c[0..n) over M X I D and
 * the two sequences it aligns: the pattern is the query, or its reverse complement when q_revcomp is set, the text is the target;
 * for a range call they are the two intervals, exactly as verification and normalization see them.  No penalties are involved.
 * Let p and t be the pattern and text positions consumed so far, lower(b) = b + 32 for 'A'..'Z' and b otherwise, upper its inverse
 * on 'a'..'z'.  The maximal runs of equal op bytes, left to right:
 *     a run of L 'M'    AWV_CS_SHORT: ':' + L in decimal    AWV_CS_LONG: '=' + upper(text[t .. t + L))    p and t advance by L
 *     each 'X' column   '*' + lower(text[t]) + lower(pattern[p])   (target base first)                    both by 1
 *     a run of L 'I'    '-' + lower(text[t .. t + L))       ('I' consumes the text)                       t by L
 *     a run of L 'D'    '+' + lower(pattern[p .. p + L))    ('D' consumes the pattern)                    p by L
 * An 'I' run directly followed by a 'D' run is two items.  Whether an 'M' column's bases are equal or an 'X' column's differ is
 * not checked (that is verification's job); the '=' bases are always the text's.  Known answer (minimap2's manual): the text
 * CGATCGATAAATAGAGTAGGAATAGCA, the pattern CGATCGAATAGAGTAGGTCGAATTGCA and the ops 6M 3I 10M 3D 4M 1X 3M give
 * ":6-ata:10+gtc:4*at:3" and "=CGATCG-ata=AATAGAGTAG+gtc=GAAT*at=GCA".
 * A slice is an op string of its own, columns [col_beg, col_end) of the record's, that starts at p = q_skip, t = t_skip (the
 * fields of an awv_clip_result): a slice that cuts a run cuts that item, and nothing before col_beg is read.
 * Layout: the texts of a call's (or a batch's) records lie in one cs arena, dense and in record order -- off[0] = 0 and
 * off[i + 1] = off[i] + len[i] -- like the run-length text arena.  A string or slice holds at most 2^30 columns (AWV_ERR_ARG beyond,
 * before anything is launched); a column gives at most 3 characters, so len fits 32 bits. */
#define AWV_CS_SHORT 1
#define AWV_CS_LONG 2
#define AWV_CST_OK 0       /* the record has a text (empty for an empty string) */
#define AWV_CST_SKIPPED 1  /* status is not AWV_ST_COMPLETED (AWV_ST_ABOVE_BOUND included), or, in a clipping call, the clip's code is not AWV_CL_OK */
#define AWV_CST_BAD_OP 2   /* a byte outside MXID */
#define AWV_CST_LENGTHS 3  /* q_skip + the pattern bases the string consumes > plen, or the same for the text */
typedef struct {
  uint64_t off;  /* of the record's text in the cs arena */
  uint32_t len;  /* characters; 0 for every code but AWV_CST_OK */
  int32_t code;  /* AWV_CST_* */
} awv_cs_text; /* 16 bytes */

typedef struct {
  uint32_t col_beg, col_end; /* the slice [col_beg, col_end) of the op string */
  int32_t q_skip, t_skip;    /* pattern and text bases consumed before col_beg */
} awv_cs_slice; /* 16 bytes */

typedef struct {
  double kernel_ms;     /* HIP-event time of the cs launches (measure, scan, emit) of the last cs call */
  uint64_t pairs;       /* records handed to the step (the ones without text included) */
  uint64_t failed;      /* of them: code other than AWV_CST_OK / AWV_CST_SKIPPED */
  uint64_t text_bytes;  /* characters of all texts */
  uint64_t columns;     /* op bytes of the strings and slices walked */
} awv_cs_stats; /* 40 bytes */

/* The sink of a cs call: awv_sink's arguments, and the batch's cs arena (valid only during the call, like cigar_arena). */
typedef int (*awv_cs_sink)(void* user, int64_t first, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                           const uint8_t* cs_arena);

/* The contract alone, on the host (needs no device): a serial walk, the yardstick the kernels are tested against, not a
 * fallback -- no product path calls it.  mode: AWV_CS_SHORT / AWV_CS_LONG.  slice (nullable): the whole string from p = t = 0.
 * out->off is 0; the text is written to out_buf only when out->code is AWV_CST_OK and out->len <= cap. */
int awv_cs_one_host(int32_t mode, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen, const uint8_t* cigar,
                    int64_t n, const awv_cs_slice* slice /* nullable */, uint8_t* out_buf, uint64_t cap,
                    awv_cs_text* out /* required */);
/* The cs texts of records and op bytes the caller supplies, on the device, against the resident sequence set (AWV_ERR_STATE
 * without one): results[i] claims that cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  Staged and
 * pieced as awv_encode_cigars does, the offsets running on from piece to piece.  slices (nullable): n entries.  csout[0..n) and
 * *text_bytes (the arena's size) are always filled; the text is written to text_buf only when *text_bytes <= text_cap -- all of
 * it or nothing -- so text_buf == NULL with text_cap == 0 is the measuring call.  AWV_ERR_ARG, before anything is launched, for a
 * mode other than the two, a completed record whose op bytes lie outside the arena, and a slice with col_beg > col_end,
 * col_end > cigar_len or a negative skip. */
int awv_cs_cigars(awv_engine* e, int32_t mode, const awv_pair* pairs, int64_t n, const awv_result* results,
                  const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */,
                  awv_cs_text* csout /* required */, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes /* required */);
int awv_cs_ranges(awv_engine* e, int32_t mode, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                  const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */,
                  awv_cs_text* csout /* required */, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes /* required */);
/* awv_align_pairs_encoded / awv_align_ranges_encoded (tout nullable here) with the cs text of every batch's finished pairs made
 * on the device, on the engine's stream, last of the per-batch steps: after normalization, the optional check, the optional clip
 * and the optional run-length text, so the cs text is of the normalized string under a mode.  match_bonus == 0: no clip;
 * match_bonus >= 1: cout is required and the slice is the clip's, with its q_skip / t_skip (AWV_CST_SKIPPED when the clip's code
 * is not AWV_CL_OK).  tout == NULL: the sink's cigar_arena is the op bytes, as in awv_align_pairs_clipped; non-null: it is the
 * batch's run-length text arena, as in awv_align_pairs_encoded.  Records, vout, cout and tout are those calls', byte for byte.
 * csout[first .. first + n) is filled before that batch's sink call, relative to the batch's cs arena, which is copied to a
 * host buffer of its own and is the sink's cs_arena.  Under AWV_F_KEEP_ON_DEVICE the step runs and csout is filled, but nothing
 * is copied (both of the sink's arenas are NULL). */
int awv_align_pairs_cs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                       const int32_t* max_penalty /* per pair, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                       awv_verify_result* vout /* nullable */, awv_clip_result* cout /* nullable when match_bonus == 0 */,
                       awv_cigar_text* tout /* nullable */, int32_t cs_mode, awv_cs_text* csout /* required */, awv_cs_sink sink,
                       void* user);
int awv_align_ranges_cs(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n,
                        const int32_t* max_penalty /* per range, nullable; < 0: none */, int32_t match_bonus, awv_result* out,
                        awv_verify_result* vout /* nullable */, awv_clip_result* cout /* nullable when match_bonus == 0 */,
                        awv_cigar_text* tout /* nullable */, int32_t cs_mode, awv_cs_text* csout /* required */, awv_cs_sink sink,
                        void* user);
/* The last cs call (awv_align_*_cs / awv_cs_cigars / awv_cs_ranges) of this engine. */
int awv_engine_cs_stats(const awv_engine* e, awv_cs_stats* out);

/* ---- per-base alignment depth accumulated on the device (csrc/coverage.hip, csrc/coverage_device.hpp) ---------------------------
 * For every base of every resident sequence: in how many alignments is it aligned, and in how many does it match?  Two tracks of
 * uint32 per forward-strand position: aligned[s][p] counts the contributing columns that are 'M' or 'X' and consume base p of
 * sequence s, matched[s][p] the 'M' columns among them.  A pure function of the items, exact and independent of their order.
 * An item is an op string c[0..n) over M X I D with its rectangle (pattern [pb, pe) against text [tb, te), the pattern's
 * coordinates those of the reverse-complement copy for a q_revcomp pair) and the skips q_skip, t_skip of a slice: exactly what
 * the cs text is made from.  Column k sits at pattern position x = pb + q_skip + #(ops other than 'I' before k) and at text
 * position y = tb + t_skip + #(ops other than 'D' before k).  The target's base is y; the query's forward-strand base is x for
 * a forward pair and len[q] - 1 - x for a q_revcomp pair.  roles says whose tracks a column is added to.
 * What contributes in an aligning call: without clip or split a record with status AWV_ST_COMPLETED, whole; in a clipping call
 * the clip's slice when its code is AWV_CL_OK and its score >= clip_min_score; in a splitting call every segment; nothing else
 * (failed records, records above the bound, empty clips, score-only and orientation calls).  The walk comes after normalization.
 * An item is all or nothing: one whose code is not AWV_CV_OK adds to no counter anywhere, and nothing is ever stored outside a
 * sequence's own slots, whatever the bytes say.  A string or slice holds at most 2^30 columns; an engine accumulates at most
 * 2^31 - 1 items between awv_engine_coverage_begin calls, so no depth can wrap (AWV_ERR_ARG beyond, before anything is launched). */
#define AWV_COV_TARGET 1
#define AWV_COV_QUERY 2
#define AWV_COV_BOTH 3
#define AWV_CV_OK 0       /* the item was added */
#define AWV_CV_SKIPPED 1  /* status is not AWV_ST_COMPLETED */
#define AWV_CV_BAD_OP 2   /* a byte outside MXID */
#define AWV_CV_LENGTHS 3  /* q_skip + the pattern bases the string consumes > the pattern interval, or the same for the text */
typedef struct {
  int32_t code;           /* AWV_CV_* */
  uint32_t aligned_cols;  /* 'M' and 'X' columns; the three counts are 0 for every code but AWV_CV_OK */
  uint32_t matched_cols;  /* 'M' columns */
  uint32_t boundaries;    /* 2 x (maximal runs of aligned columns + maximal runs of 'M'): the adds one role costs */
} awv_cov_item; /* 16 bytes */

typedef struct {
  double kernel_ms;     /* HIP-event time of the coverage launches (the read-out scans included) since awv_engine_coverage_begin */
  uint64_t items;       /* items handed to the pass since then (skipped ones included) */
  uint64_t failed;      /* of them: code other than AWV_CV_OK / AWV_CV_SKIPPED */
  uint64_t columns;     /* op bytes of the strings and slices walked */
  uint64_t boundaries;  /* adds made: the items' boundaries, once per role */
  uint64_t reads;       /* awv_engine_coverage_read calls */
} awv_cov_stats; /* 48 bytes */

/* The contract alone, on the host (needs no device): a per-column walk, the yardstick the kernel is tested against, not a
 * fallback -- no product path calls it.  qlen / tlen: the two sequences' lengths; the rectangle in pattern / text coordinates;
 * slice (nullable): the whole string, no skips.  q_aligned / q_matched: the query's tracks, qlen entries; t_aligned / t_matched:
 * the target's, tlen entries (for a self pair the same arrays may be passed twice); a null track is not kept.  Adds 1 per
 * contributing column, and nothing unless out->code is AWV_CV_OK. */
int awv_coverage_one_host(int32_t roles, int32_t q_revcomp, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb,
                          int32_t te, const uint8_t* cigar, int64_t n, const awv_cs_slice* slice /* nullable */,
                          uint32_t* q_aligned, uint32_t* q_matched, uint32_t* t_aligned, uint32_t* t_matched,
                          awv_cov_item* out /* required */);
/* Begins accumulation over the resident sequence set (AWV_ERR_STATE without one): allocates and zeroes the accumulators, two
 * difference tracks of len[s] + 1 slots per sequence.  From then on every aligning call of the engine -- awv_align_pairs and
 * awv_align_ranges in all their forms -- adds each batch's contributing items on the device, on the engine's stream, after the
 * clip / split step; records, op bytes, texts and stats of those calls are unchanged.  roles: AWV_COV_* (1..3); roles == 0 ends
 * coverage and frees the memory, and so does awv_engine_set_sequences.  clip_min_score: the threshold of clipping calls. */
int awv_engine_coverage_begin(awv_engine* e, int32_t roles, int64_t clip_min_score);
/* The depth so far: a segmented scan of the difference slots into separate buffers, copied back; the sequences concatenated in
 * set order.  The accumulators stay as they are: accumulation goes on after a read.  n_bases must be the sum of the lengths
 * (AWV_ERR_ARG); either pointer may be null.  AWV_ERR_STATE before begin.  A sequence whose scan does not end on 0 is a bug,
 * never an input error: AWV_ERR_HIP. */
int awv_engine_coverage_read(awv_engine* e, uint32_t* aligned, uint32_t* matched, uint64_t n_bases);
/* Accumulates records and op bytes the caller supplies into the engine's accumulators: results[i] claims that
 * cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  Staged and pieced as awv_cs_cigars does; slices
 * (nullable): n entries; items[0..n) is filled.  AWV_ERR_STATE before begin; AWV_ERR_ARG, before anything is launched, for what
 * awv_cs_cigars refuses. */
int awv_coverage_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                        uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, awv_cov_item* items /* required */);
int awv_coverage_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                        const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */,
                        awv_cov_item* items /* required */);
/* Since the last awv_engine_coverage_begin of this engine (all zero before one). */
int awv_engine_coverage_stats(const awv_engine* e, awv_cov_stats* out);

/* ---- the alleles of all alignments per target site (csrc/variants.hip, csrc/variants_device.hpp) --------------------------------
 * At this site of this sequence, which alleles do the other sequences carry, and how many carry each?  A keyed table: distinct
 * (site, allele) rows with a support count, deduplicated across records, batches and calls.  This section is the contract and
 * its host yardsticks; the device pass is declared behind them.  The hash, its combine and the key order are __host__ __device__
 * in variants_device.hpp.
 * A pure function of the contributing items, exact and independent of their order.
 * An item is exactly the coverage pass's item: an op string c[0..n) over M X I D with its rectangle (pattern [pb, pe) against
 * text [tb, te)), the skips of a slice, and the pair's q_idx, t_idx and q_revcomp; the pattern is the reverse-complement copy for
 * a q_revcomp pair, so allele bases are in target orientation.  Column k sits at pattern position x and text position y as above.
 * What contributes of an aligning call is the coverage rule, word for word (whole completed records, a clip's slice that reaches
 * clip_min_score, every split segment, after normalization); a slice that cuts a run cuts the event, as in cs.
 * The events of an item, left to right:
 *   each 'X' column               AWV_VAR_SNV  pos = y                        len 1  allele: the pattern base
 *   each maximal 'I' run of L     AWV_VAR_DEL  pos = y of its first column    len L  no allele ('I' consumes the text, cs's '-')
 *   each maximal 'D' run of L     AWV_VAR_INS  pos = y, the target base the   len L  allele: pattern[p, p + L)
 *                                              insertion precedes (tlen is allowed)  ('D' consumes the pattern, cs's '+')
 * An 'I' run directly followed by a 'D' run is two events.  Whether an 'X' column's bases really differ is not judged, as in cs.
 * Allele identity is (len, hash): hash runs over the upper-cased allele bytes modulo 2^61 - 1 with the base AWV_VAR_HASH_BASE:
 * h(empty) = 0, h(s.c) = (h(s) * B + upper(c)) mod (2^61 - 1), hence h(a.b) = (h(a) * B^|b| + h(b)) mod (2^61 - 1); a deletion has
 * hash 0.  The constant is part of the contract: tables of several devices are merged by key.  Two different insertions of equal
 * length at one site are told apart by this hash and nothing else.
 * Row key: (t_idx, pos, type, len, hash); the table is sorted ascending by it.  Row value: count, the number of contributing items
 * that carry the event, and rep, the smallest (uint64)q_idx << 32 | q_revcomp << 31 | p_beg over those items, p_beg the event's
 * first pattern position in the aligned copy's coordinates: the allele's bytes can be read from rep.  Sum and min: the table does
 * not depend on the order of items, batches, engines or devices.
 * An item is all or nothing: one whose code is not AWV_VR_OK adds no event.  A string or slice holds at most 2^30 columns, and
 * a table takes at most 2^31 - 1 items, so no count can wrap. */
#define AWV_VAR_SNV 0
#define AWV_VAR_DEL 1
#define AWV_VAR_INS 2
#define AWV_VAR_HASH_BASE 1983613069137408743ull /* B = 0x1b873593a5c1f2e7, below 2^61 - 1 */
#define AWV_VR_OK 0       /* the item's events were appended */
#define AWV_VR_SKIPPED 1  /* status is not AWV_ST_COMPLETED */
#define AWV_VR_BAD_OP 2   /* a byte outside MXID */
#define AWV_VR_LENGTHS 3  /* q_skip + the pattern bases the string consumes > the pattern interval, or the same for the text */
typedef struct {
  int32_t t_idx, pos, type, len; /* type: AWV_VAR_* */
  uint64_t hash, rep;
  uint32_t count, reserved;      /* reserved: 0 */
} awv_variant; /* 40 bytes */
typedef struct {
  int32_t code;           /* AWV_VR_* */
  uint32_t snv, ins, del; /* events of each type; 0 for every code but AWV_VR_OK */
} awv_var_item; /* 16 bytes */
/* The contract alone, on the host (needs no device): yardsticks for kernels to be tested against, not fallbacks -- no product
 * path of the engine calls them.  awv_variants_one_host is the serial per-column walk of one item into events with count 1, in column
 * order: pattern is the aligned copy of the query (qlen bytes), the rectangle and the slice as in awv_coverage_one_host; at most
 * cap events are written to `events` (nullable with cap 0), *n_events is their number whatever cap is, and nothing is written
 * unless out->code is AWV_VR_OK.  awv_variants_fold_host sorts rows[0..n) -- events or rows -- by key and reduces equal keys
 * (sum of count, min of rep) in place; *n_rows is the number of distinct rows left at the front. */
int awv_variants_one_host(int32_t q_idx, int32_t t_idx, int32_t q_revcomp, const uint8_t* pattern, int32_t qlen, int32_t tlen,
                          int32_t pb, int32_t pe, int32_t tb, int32_t te, const uint8_t* cigar, int64_t n,
                          const awv_cs_slice* slice /* nullable */, awv_variant* events, uint64_t cap, uint64_t* n_events,
                          awv_var_item* out /* required */);
int awv_variants_fold_host(awv_variant* rows, uint64_t n, uint64_t* n_rows);

/* The device pass (csrc/variants.hip: the events of every item, one wave per item; csrc/variants_fold.hip: the fold, a stable
 * radix sort by key and one reduction of equal keys).  Events and rows are awv_variants_one_host's and awv_variants_fold_host's,
 * byte for byte. */
#define AWV_VTAB_EVENTS 0     /* `fold` of awv_variants_cigars: the items' unfolded events, in record order, then column order */
#define AWV_VTAB_FOLDED 1     /* the folded table of the call */
#define AWV_VTAB_ACCUMULATE 2 /* the events go to the engine's table (AWV_ERR_STATE before awv_engine_variants_begin); no row comes back */
typedef struct {
  double kernel_ms;  /* HIP-event time of the event kernels (measure, scan, emit) since awv_engine_variants_begin */
  double fold_ms;    /* and of the folds */
  uint64_t items;    /* items handed to the pass since then (skipped ones included) */
  uint64_t failed;   /* of them: code other than AWV_VR_OK / AWV_VR_SKIPPED */
  uint64_t columns;  /* op bytes of the strings and slices walked */
  uint64_t snv, ins, del; /* events of each type */
  uint64_t rows;     /* rows of the engine's table after its last fold */
  uint64_t folds;    /* folds of the engine's table: those that made room, and one per read */
  uint64_t capacity_rows; /* the size of the engine's row buffer; it only grows between two begins, so this is its peak */
} awv_variants_stats; /* 88 bytes */
/* Begins a table over the resident sequence set (AWV_ERR_STATE without one): a device buffer of reserve_rows rows (0: a default).
 * From then on every aligning call of the engine -- awv_align_pairs and awv_align_ranges in all their forms -- appends each batch's
 * events on the device, on the engine's stream, after the clip / split step; records, op bytes, texts and stats of those calls are
 * unchanged.  When a batch's events would pass the buffer's end the table is folded in place, and doubled if it is then still
 * more than half full; a failed allocation is AWV_ERR_OOM and leaves the table as it was.  clip_min_score: the threshold of
 * clipping calls.  A begin ends the table before it, and so does awv_engine_set_sequences.  At most 2^31 - 1 items between two
 * begins (AWV_ERR_ARG beyond, before anything is launched). */
int awv_engine_variants_begin(awv_engine* e, int64_t clip_min_score, uint64_t reserve_rows);
/* Ends the table and frees its buffer (nothing to end: AWV_OK); the stats stay readable until the next begin. */
int awv_engine_variants_end(awv_engine* e);
/* The table so far: folds, then copies.  *n_rows is the number of rows whatever cap is; they are written to rows only when
 * *n_rows <= cap -- all of them or none -- so rows == NULL with cap == 0 is the measuring call.  Accumulation goes on after a
 * read.  AWV_ERR_STATE before begin. */
int awv_engine_variants_read(awv_engine* e, awv_variant* rows, uint64_t cap, uint64_t* n_rows /* required */);
/* Since the last awv_engine_variants_begin of this engine (since its creation before one); awv_variants_cigars / _ranges add
 * to items, failed, columns, the events and kernel_ms under every `fold`. */
int awv_engine_variants_stats(const awv_engine* e, awv_variants_stats* out);
/* The events of records and op bytes the caller supplies, on the device, against the resident sequence set: results[i] claims that
 * cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  Staged and pieced as awv_cs_cigars does; slices
 * (nullable): n entries; items[0..n) is filled.  fold: AWV_VTAB_*.  *n_rows is the number of rows (under AWV_VTAB_ACCUMULATE: of
 * events appended) whatever cap is; rows is written only when *n_rows <= cap, all or none.  AWV_ERR_ARG, before anything is
 * launched, for what awv_cs_cigars refuses. */
int awv_variants_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                        uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, int32_t fold,
                        awv_var_item* items /* required */, awv_variant* rows, uint64_t cap, uint64_t* n_rows /* required */);
int awv_variants_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                        const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, int32_t fold,
                        awv_var_item* items /* required */, awv_variant* rows, uint64_t cap, uint64_t* n_rows /* required */);
/* The device fold on the caller's rows: rows[0..n), n < 2^31, events or rows in any order and with any field values (the order is
 * awv_variants_fold_host's: the four 32-bit fields as signed numbers, the hash as an unsigned 64-bit word), become
 * awv_variants_fold_host's rows in place; *n_rows is their number.  Needs no sequence set. */
int awv_variants_fold(awv_engine* e, awv_variant* rows, uint64_t n, uint64_t* n_rows /* required */);

/* ---- regions lifted through alignments on the device (csrc/lift.hip, csrc/lift_device.hpp) --------------------------------------
 * This interval of sequence A: where is it on a sequence A was aligned with, and how well does it align there?  The one answer
 * that crosses sequences; the rule is __host__ __device__ in lift_device.hpp.  A pure function of the op bytes, the rectangle and
 * the interval: no penalties are involved and no sequence bytes are read.
 * An item is exactly the coverage pass's item: an op string c[0..n) over M X I D ('I' consumes the text only, 'D' the pattern
 * only, 'M' and 'X' both) with its rectangle (pattern [pb, pe) against text [tb, te), the pattern the reverse-complement copy for
 * a q_revcomp pair) and the skips of a slice.  Column k sits at pattern position x = pb + q_skip + #(ops other than 'I' before k)
 * and at text position y = tb + t_skip + #(ops other than 'D' before k).
 * A lift query names a side and a half-open interval [a, b) on the source sequence's forward strand.  AWV_LIFT_FROM_TARGET: the
 * source is the text, the destination the pattern; AWV_LIFT_FROM_QUERY: the reverse.  For a q_revcomp pair a query-side position
 * f is pattern position len[q] - 1 - f, so [a, b) becomes [len - b, len - a), and reported query intervals are turned back the
 * same way.  srcpos(k) is column k's source position, defined for the columns that consume the source; the item's source span is
 * [s0, s0 + S), s0 the source position of column 0 and S the source bases the string consumes.  The lift is the aligned core:
 *     col_beg = the smallest k with c[k] in {M, X} and srcpos(k) >= a     (n when there is none)
 *     col_end = 1 + the largest k with c[k] in {M, X} and srcpos(k) < b   (0 when there is none)
 * The interval does not meet the span: AWV_LF_OUTSIDE.  It does and col_beg >= col_end (it lies in a gap): AWV_LF_UNALIGNED.
 * Otherwise AWV_LF_OK, and the slice [col_beg, col_end) begins and ends on an 'M' / 'X' column: gap runs of either kind strictly
 * inside it belong to it, gap columns at its edges do not, and an interval reaching beyond the span is cut to it by the same rule.
 * AWV_LF_SKIPPED, AWV_LF_BAD_OP and AWV_LF_LENGTHS are coverage's codes and hold for the whole item: every query of such an item
 * carries the item's code, whatever its own columns look like.
 * Known answers (the ops of minimap2's cs example, 6M 3I 10M 3D 4M 1X 3M, whole sequences, a forward pair):
 *     from target [4, 12)   OK, slice [4, 12), target [4, 12), query [4, 9), 5 M and 3 I
 *     from target [6, 9)    AWV_LF_UNALIGNED
 *     from target [7, 10)   OK, slice [9, 10), target [9, 10), query [6, 7)
 *     from query [15, 20)   OK, slice [18, 23), query [15, 20), target [18, 20), 2 M and 3 D
 * A string or slice holds at most 2^30 columns, a call fewer than 2^30 queries (AWV_ERR_ARG otherwise, before anything is launched). */
#define AWV_LIFT_FROM_TARGET 1
#define AWV_LIFT_FROM_QUERY 2
#define AWV_LIFT_FROM_BOTH 3 /* a from_mask of awv_engine_lift_begin only */
#define AWV_LF_OK 0        /* the interval has an aligned core: the slice and the two intervals are filled */
#define AWV_LF_SKIPPED 1   /* status is not AWV_ST_COMPLETED */
#define AWV_LF_BAD_OP 2    /* a byte outside MXID anywhere in the string or slice */
#define AWV_LF_LENGTHS 3   /* the string consumes more than its rectangle */
#define AWV_LF_UNALIGNED 4 /* the interval meets the item's source span but holds no aligned column there */
#define AWV_LF_OUTSIDE 5   /* the interval does not meet the item's source span */
#define AWV_LIFT_ROW_REVCOMP 1    /* awv_lift_row.flags: the pair is q_revcomp */
#define AWV_LIFT_ROW_FROM_QUERY 2 /* the region lies on the query (src is the query, dst the target) */
typedef struct {
  int64_t record;   /* of the call's records */
  int32_t from;     /* AWV_LIFT_FROM_TARGET / AWV_LIFT_FROM_QUERY */
  int32_t beg, end; /* [beg, end) on the source sequence's forward strand */
  int32_t reserved; /* not read */
} awv_lift_query; /* 24 bytes */
typedef struct {
  int32_t code;              /* AWV_LF_*; every other field is 0 unless it is AWV_LF_OK */
  int32_t reserved;          /* 0 */
  uint32_t col_beg, col_end; /* with the skips exactly an awv_cs_slice of the record's op string: counted from the string's */
  int32_t q_skip, t_skip;    /* start, the item's own slice included */
  int32_t src_beg, src_end;  /* the source and destination intervals the slice covers, forward strand, sequence coordinates */
  int32_t dst_beg, dst_end;
  int32_t num_matches, num_mismatches, num_ins, num_del; /* the slice's 'M', 'X', 'I', 'D' bytes (as in awv_clip_result) */
} awv_lift_result; /* 56 bytes */
typedef struct {
  int32_t seq, beg, end; /* [beg, end) of resident sequence seq, forward strand */
} awv_region; /* 12 bytes */
typedef struct {
  int32_t region;             /* index into the begin's regions */
  int32_t q_idx, t_idx;       /* the alignment the row comes from */
  int32_t flags;              /* AWV_LIFT_ROW_* */
  int32_t src_beg, src_end;   /* on the region's sequence */
  int32_t dst_beg, dst_end;   /* on the other sequence of the pair */
  int32_t num_matches, num_mismatches, num_ins, num_del;
} awv_lift_row; /* 48 bytes */
typedef struct {
  double kernel_ms;   /* HIP-event time of the lift launches since awv_engine_lift_begin (since the engine's creation before one) */
  uint64_t records;   /* records walked: the ones with a query, each once per launch */
  uint64_t columns;   /* their op bytes, each once however many queries a record has */
  uint64_t queries;
  uint64_t ok, skipped, bad_op, lengths, unaligned, outside; /* queries that ended with each code */
} awv_lift_stats; /* 80 bytes */

/* The contract alone, on the host (needs no device): a serial per-column walk, the yardstick the kernel is tested against, not a
 * fallback -- no product path calls it.  The rectangle and the slice as in awv_coverage_one_host; [beg, end) on the source's
 * forward strand, 0 <= beg < end <= the source sequence's length (AWV_ERR_ARG otherwise). */
int awv_lift_one_host(int32_t from, int32_t q_revcomp, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb, int32_t te,
                      const uint8_t* cigar, int64_t n, const awv_cs_slice* slice /* nullable */, int32_t beg, int32_t end,
                      awv_lift_result* out /* required */);
/* Lifts intervals through records and op bytes the caller supplies, on the device: results[i] claims that
 * cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  The engine needs a sequence set for the lengths
 * only (AWV_ERR_STATE without one).  Queries come in any order and reach any number of records; lout[j] answers queries[j].  One
 * wave walks a record's op string once and answers all of its queries in that walk; a record without a query is not walked.
 * Staged and pieced as awv_coverage_cigars does; slices (nullable): n entries.  AWV_ERR_ARG, before anything is launched, for
 * what awv_cs_cigars refuses, a record index outside [0, n), a `from` other than the two sides, beg >= end, beg < 0 and an end
 * above the source sequence's length. */
int awv_lift_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                    uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, const awv_lift_query* queries, int64_t nq,
                    awv_lift_result* lout /* required when nq > 0 */);
int awv_lift_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                    uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, const awv_lift_query* queries, int64_t nq,
                    awv_lift_result* lout /* required when nq > 0 */);
/* Begins a table over the resident sequence set (AWV_ERR_STATE without one).  regions[0..n_regions): forward strand, in any
 * order; they may overlap, nest and repeat (AWV_ERR_ARG for a sequence index out of range or an interval that is empty or outside
 * its sequence).  From then on every aligning call of the engine -- awv_align_pairs and awv_align_ranges in all their forms --
 * lifts, per batch, on the device and on the engine's stream, after normalization and the clip / split step: every region through
 * every contributing item (the coverage rule, word for word) that overlaps it, regions on an item's target under
 * AWV_LIFT_FROM_TARGET, on its query under AWV_LIFT_FROM_QUERY.  The AWV_LF_OK results are appended to the table as rows, on the
 * host; records, op bytes, texts and stats of those calls are unchanged.  from_mask == 0 ends the table (the stats stay
 * readable), and so does awv_engine_set_sequences.  clip_min_score: the threshold of clipping calls. */
int awv_engine_lift_begin(awv_engine* e, const awv_region* regions, int64_t n_regions, int32_t from_mask, int64_t clip_min_score);
/* The table so far, sorted ascending by all fields in their order (region first; as signed numbers): it does not depend on the
 * order of batches, and tables of several engines merge by concatenating and sorting.  *n_rows is the number of rows whatever
 * cap is; they are written only when *n_rows <= cap, all or none, so rows == NULL with cap == 0 is the measuring call.
 * AWV_ERR_STATE before begin. */
int awv_engine_lift_read(awv_engine* e, awv_lift_row* rows, uint64_t cap, uint64_t* n_rows /* required */);
/* Since the last awv_engine_lift_begin of this engine (since its creation before one); awv_lift_cigars / _ranges add to it. */
int awv_engine_lift_stats(const awv_engine* e, awv_lift_stats* out);

/* ---- target-anchored multiple alignments on the device (csrc/msa.hip, csrc/msa_device.hpp) ------------------------------------
 * Every sequence laid out against one of them: a star multiple alignment anchored on a target, as a dense block of bytes.  The
 * rule is __host__ __device__ in msa_device.hpp.  A pure function of the items and the two sequences: no penalties are involved,
 * and nothing depends on the order of the items apart from the order of the rows.
 * An item is exactly the coverage pass's item: an op string c[0..n) over M X I D ('I' consumes the text only, 'D' the pattern
 * only, 'M' and 'X' both) with its rectangle (pattern [pb, pe) against text [tb, te), the pattern the reverse-complement copy for
 * a q_revcomp pair) and the skips of a slice.  Column k sits at pattern position x = pb + q_skip + #(ops other than 'I' before k)
 * and at text position y = tb + t_skip + #(ops other than 'D' before k).
 * The codes are coverage's, and AWV_MS_NOT_CHOSEN: the item's t_idx is not among the call's targets; such an item is not walked,
 * whatever its record says.  An item is all or nothing: one whose code is not AWV_MS_OK widens no slot and gets no row, whatever
 * bytes precede the bad one.
 * Widths.  A chosen target s of L bases has L + 1 slots: slot p is the gap before base p, slot L the one behind the last base.
 * ins[s][p] is the maximum, over the AWV_MS_OK items with t_idx == s, of the number of the item's 'D' columns at text position p.
 * In one string those columns are one run (any other op advances y); a slice that cuts a run counts only its own columns.
 * Columns.  col[s][p] = p + the sum of ins[s][r] for r <= p, in 64 bits.  Base p (p < L) sits in column col[p], slot p's insertion
 * columns are [col[p] - ins[p], col[p]), and the block is W = col[L] columns wide.
 * Rows.  A target's block is rows x W bytes, row-major, filled with '-'.  Row 0 is the target: upper(text[p]) at col[p].  Then one
 * row per AWV_MS_OK item of that target, in the call's item order: an 'M' or 'X' column at (x, y) puts upper(pattern[x]) at
 * col[y]; a 'D' column that is the j-th (from 0) of its run within the item, at slot y, puts upper(pattern[x]) at
 * col[y] - ins[y] + j (insertions are left-justified and not aligned among themselves); an 'I' column leaves the fill, and so does
 * everything outside the item's target span.
 * Known answer (minimap2's cs example): text CGATCGATAAATAGAGTAGGAATAGCA, pattern CGATCGAATAGAGTAGGTCGAATTGCA, ops
 * 6M 3I 10M 3D 4M 1X 3M, alone on its target: W = 30, row 0 CGATCGATAAATAGAGTAG---GAATAGCA, row 1 CGATCG---AATAGAGTAGGTCGAATTGCA.
 * A string or slice holds at most 2^30 columns (AWV_ERR_ARG otherwise, before anything is launched). */
#define AWV_MS_OK 0         /* the item widened its target's slots and has a row */
#define AWV_MS_SKIPPED 1    /* status is not AWV_ST_COMPLETED */
#define AWV_MS_BAD_OP 2     /* a byte outside MXID */
#define AWV_MS_LENGTHS 3    /* q_skip + the pattern bases the string consumes > the pattern interval, or the same for the text */
#define AWV_MS_NOT_CHOSEN 4 /* t_idx is not among the call's targets: the item was not walked */
typedef struct {
  int32_t code;             /* AWV_MS_*; every field below but `target` is 0 unless it is AWV_MS_OK */
  int32_t target;           /* index into the call's targets; -1 for AWV_MS_NOT_CHOSEN */
  int32_t row;              /* the item's row within its target's block (>= 1); 0 when it has none */
  uint32_t bases;           /* bases placed: the item's 'M', 'X' and 'D' columns */
  int64_t col_beg, col_end; /* the first and one past the last non-gap column of the row; 0, 0 for a row without a base */
} awv_msa_item; /* 32 bytes */
typedef struct {
  int32_t t_idx;  /* the target's sequence index */
  int32_t rows;   /* 1 + its AWV_MS_OK items */
  int64_t width;  /* W */
  uint64_t off;   /* the block begins at this byte of the arena and holds rows * width bytes */
} awv_msa_target; /* 24 bytes */
typedef struct {
  double width_ms;  /* HIP-event time of the width launches of the last awv_msa_* call */
  double scan_ms;   /* ... of the segmented scan and the items' column intervals */
  double emit_ms;   /* ... of the fill, the targets' rows and the emit launches (0 for a measuring call) */
  uint64_t items;   /* items of the call, the ones not chosen included */
  uint64_t failed;  /* of them: AWV_MS_BAD_OP and AWV_MS_LENGTHS */
  uint64_t columns; /* op bytes walked by the width launches, each once however often it is read */
  uint64_t runs;    /* 'D' runs of the AWV_MS_OK items: one atomic maximum each */
  uint64_t bases;   /* bases placed in the items' rows (counted by the width launches: also in a measuring call) */
  uint64_t bytes;   /* *msa_bytes */
} awv_msa_stats; /* 72 bytes */

/* The contract alone, on the host (needs no device): the serial per-column walk of ONE target's items, the yardstick the kernels
 * are tested against, not a fallback -- no product path calls it.  text[0..tlen): the target.  Item i: patterns[i][0..plens[i]) is
 * the aligned copy of its query (the reverse complement for a q_revcomp pair), rects[4 i .. 4 i + 4) = pb, pe, tb, te in pattern /
 * text coordinates, cigars[i][0..cigar_lens[i]) the op string (cigar_lens[i] < 0: a record that is not completed,
 * AWV_MS_SKIPPED), slices (nullable) n entries.  Writes ins[0..tlen], *width, codes[0..n) and *block_bytes = rows * width always;
 * block[0..*block_bytes) only when *block_bytes <= cap. */
int awv_msa_host(const uint8_t* text, int32_t tlen, int64_t n, const uint8_t* const* patterns, const int32_t* plens, const int32_t* rects,
                 const uint8_t* const* cigars, const int64_t* cigar_lens, const awv_cs_slice* slices /* nullable */, uint32_t* ins,
                 int64_t* width, int32_t* codes, uint8_t* block /* nullable when cap == 0 */, uint64_t cap, uint64_t* block_bytes);
/* Builds the blocks of targets[0..nt) (distinct sequence indices) from records and op bytes the caller supplies, on the device:
 * results[i] claims that cigar_arena[results[i].cigar_off, + cigar_len) aligns pairs[i] (ranges[i]).  Needs a sequence set
 * (AWV_ERR_STATE without one).  items[i] answers item i; tgts[j] describes targets[j]; the blocks lie in one arena in `targets`
 * order, tgts[0].off = 0 and tgts[j + 1].off = tgts[j].off + rows[j] * width[j].  *msa_bytes is the arena's size, always filled;
 * buf[0..*msa_bytes) is written only when *msa_bytes <= cap, all of it or nothing, so buf == NULL with cap == 0 is the measuring
 * call (items and tgts are filled all the same).  A target without items gets a block of one row and width L.
 * Three steps on the engine's stream: a width kernel (a record pass: every item walked twice in one launch, the second walk one
 * no-return atomic maximum per 'D' run), a segmented scan of the slots into 64-bit columns, and -- when the arena fits -- a fill
 * with '-', the targets' rows and an emit kernel (the same walk, one byte store per base).  Staged and pieced as
 * awv_coverage_cigars does under awv_engine_config.max_arena_bytes; the pieces go up once for the widths and once for the rows.
 * slices (nullable): n entries.  AWV_ERR_ARG, before anything is launched, for what awv_cs_cigars refuses, a target index
 * outside the set and a repeated target. */
int awv_msa_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                   uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, const int32_t* targets, int64_t nt,
                   awv_msa_item* items, awv_msa_target* tgts, uint8_t* buf, uint64_t cap, uint64_t* msa_bytes /* required */);
int awv_msa_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                   uint64_t arena_bytes, const awv_cs_slice* slices /* nullable */, const int32_t* targets, int64_t nt,
                   awv_msa_item* items, awv_msa_target* tgts, uint8_t* buf, uint64_t cap, uint64_t* msa_bytes /* required */);
/* Of the engine's last awv_msa_cigars / awv_msa_ranges call (zeros before one). */
int awv_engine_msa_stats(const awv_engine* e, awv_msa_stats* out);
/* ---- device pair planning (csrc/planner.hip) -------------------------------------------------------------------------
 * Integer work over the engine's resident sequence set, on its device and stream; results equal the host planner's
 * (csrc/host/planner.cpp) bit for bit.  Every call but awv_keep_pairs needs a sequence set (else AWV_ERR_STATE); a new set
 * drops the sketches of the old one.  A null engine: AWV_ERR_NO_DEVICE without a GPU, else AWV_ERR_ARG. */
#define AWV_SK_CANONICAL 0 /* min(hash(k-mer), hash(upper-cased reverse complement)) of the forward copy (mash.rs) */
#define AWV_SK_FORWARD 1   /* stranded, forward copy (alignment.rs:96-122) */
#define AWV_SK_REVCOMP 2   /* stranded, reverse-complement copy */
#define AWV_PLAN_MAX_K 64
#define AWV_PLAN_MAX_S 4096
#define AWV_PLAN_MAX_KNN 64

/* Builds and keeps the sketch set of `kind`: per sequence the distinct hashes among the s smallest k-mer hashes (duplicates
 * counted; k-mers with a non-ACGT byte skipped), 1 <= k <= 64, 1 <= s <= 4096.  sizes (nullable): n entries. */
int awv_sketch(awv_engine* e, int32_t kind, int32_t k, int32_t s, uint32_t* sizes);
/* Copies the kept sketch set of `kind` out: offsets[n + 1] (nullable) and the ascending hashes, offsets[n] of them (nullable). */
int awv_sketch_copy(awv_engine* e, int32_t kind, uint64_t* offsets, uint64_t* hashes);
/* inter[p] = |sketch_a(a[p]) n sketch_b(b[p])| for p < npairs (sketches of kinds kind_a, kind_b). */
int awv_sketch_pair_counts(awv_engine* e, int32_t kind_a, int32_t kind_b, const int32_t* a, const int32_t* b, int64_t npairs,
                           uint16_t* inter);
/* inter[r * n + j] = |S(row0 + r) n S(j)| for r < nrows, j < n (one kind against itself). */
int awv_sketch_rows(awv_engine* e, int32_t kind, int32_t row0, int32_t nrows, uint16_t* inter);
/* Per row i: the k_nearest columns j != i of largest Jaccard and the k_farthest of smallest, ties to the smaller j, in that
 * order (nearest[i * k_nearest + t], farthest[i * k_farthest + t]; -1 past n - 1 columns).  Jaccards are compared exactly
 * (inter_a * uni_b against inter_b * uni_a; uni = 0 counts as 0).  0 <= k_nearest, k_farthest <= 64. */
int awv_sketch_knn(awv_engine* e, int32_t kind, int32_t k_nearest, int32_t k_farthest, int32_t* nearest, int32_t* farthest);
/* The hashed keep test of the sparsifiers (iterator.rs:261-281): bit j & 31 of bitmap[i * ((n + 31) / 32) + j / 32] is set
 * when keep_all or DefaultHasher("id_i:id_j") < threshold, for i != j (and i == j with include_diag).  The ids: n strings,
 * id_bytes[id_offsets[i], id_offsets[i + 1]).  Reads no sequence: the engine needs no sequence set for it. */
int awv_keep_pairs(awv_engine* e, int32_t n, const uint8_t* id_bytes, const uint64_t* id_offsets, uint64_t threshold,
                   int32_t keep_all, int32_t include_diag, uint32_t* bitmap);

#ifdef __cplusplus
}
#endif
#endif
