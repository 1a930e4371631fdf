// allwave.hpp -- C++ host-side mirror of allwave's API surface for the per-pair hot path,
// implemented over the C ABI of include/allwave_hip.h (the reference's own host language, Rust,
// is not available in this environment; INTEGRATION.md shows the Rust-side binding instead).
//
// Same names, argument meaning and error behaviour as the reference so the tests read like the
// reference's own (file:line relative to /root/reference):
//   Sequence, AlignmentResult, AlignmentParams, AlignmentMode, AlignmentError   src/types.rs:7-131
//   parse_scores, alignment_to_paf                                               src/lib.rs:71-153
//   cigar_bytes_to_string, reverse_complement, align_pair's result mapping       src/alignment.rs:25-66,178-190,347-376
//   AllPairIterator (-p none enumeration, WFA orientation, callback streaming)   src/iterator.rs:12-253
//   wfa::align_sequences / validate_cigar_alignment                              src/wfa.rs:105-258
// This build's own: on-device verification of the alignments a run produces (with_verify) and of a PAF file (check_paf);
// alignments clipped to their best-scoring segment on the device (with_clip).
// Pair planning (mash orientation, sparsifiers, kNN/tree pairs) lives in planner.hpp; the CLI in main.cpp.
#pragma once

#include <cstdint>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "allwave_hip.h"
#include "delivery.hpp"  // BoundStats, ClipStats, SplitStats; the delivery rule of a filtering run

namespace allwave {

struct Sequence {  // types.rs:7-10
  std::string id;
  std::vector<uint8_t> seq;
};

struct AlignmentResult {  // types.rs:14-33
  size_t query_idx = 0, target_idx = 0;
  size_t query_start = 0, query_end = 0, target_start = 0, target_end = 0;
  bool is_reverse = false;
  std::vector<uint8_t> cigar_bytes;  // raw WFA2-alphabet op bytes
  int32_t score = 0;                 // WFA2 score (= -penalty); i32::MAX on failure
  size_t num_matches = 0;
  size_t alignment_length = 0;       // #M + #X
};

struct AlignmentParams {  // types.rs:37-74
  int32_t match_score = 0, mismatch_penalty = 5, gap_open = 8, gap_extend = 2;
  std::optional<int32_t> gap2_open = 24, gap2_extend = 1;
  std::optional<double> max_divergence;
  static AlignmentParams edit_distance();
  bool operator==(const AlignmentParams& o) const;
};

enum class AlignmentMode { EditDistance, SinglePieceAffine, TwoPieceAffine };  // types.rs:99-117
AlignmentMode alignment_mode_from_params(const AlignmentParams& p);
awv_penalties to_penalties(const AlignmentParams& p);  // create_wfa_aligner, alignment.rs:263-289

struct AlignmentError : std::runtime_error {  // types.rs:121-131
  using std::runtime_error::runtime_error;
};

struct SparsificationStrategy {  // types.rs:78-95
  enum Kind { None, Random, Auto, Connectivity, TreeSampling } kind = None;
  double value = 0.0;                     // Random(frac) / Connectivity(prob)
  size_t k_nearest = 0, k_farthest = 0;   // TreeSampling(k_nearest, k_farthest, random_fraction, kmer_size)
  double random_fraction = 0.0;
  std::optional<size_t> kmer_size;
  // the CLI's -p syntax (main.rs:136-203): none | auto | random:<f> | giant:<p> | connectivity:<p> | tree:<n>:<f>:<r>[:<k>]
  static SparsificationStrategy parse(const std::string& s);  // throws std::invalid_argument with main.rs's messages
};

// lib.rs:116-153 -- throws std::invalid_argument with the reference's messages
AlignmentParams parse_scores(const std::string& scores_str);
// alignment.rs:347-376
std::string cigar_bytes_to_string(const uint8_t* ops, size_t n);
inline std::string cigar_bytes_to_string(const std::vector<uint8_t>& v) { return cigar_bytes_to_string(v.data(), v.size()); }
// alignment.rs:178-190
std::vector<uint8_t> reverse_complement(const std::vector<uint8_t>& seq);
// lib.rs:71-112
std::string alignment_to_paf(const AlignmentResult& r, const std::vector<Sequence>& sequences);
void append_paf(std::string& out, const AlignmentResult& r, const uint8_t* ops, size_t nops,
                const std::vector<Sequence>& sequences);
// the same line from the CIGAR's ready run-length text (awv_cigar_text: made on the device) instead of its op bytes
void append_paf_text(std::string& out, const AlignmentResult& r, const uint8_t* text, size_t ntext,
                     const std::vector<Sequence>& sequences);

// Orientation of the query before the final alignment (alignment.rs:35-39).
enum class Orientation {
  Wfa,          // determine_orientation_wfa (alignment.rs:157-175): what AllPairIterator::new uses
  ForwardOnly,  // extension: skip orientation (all '+'); used when strands are known
  Mash          // determine_orientation_mash (alignment.rs:69-154), hoisted to per-sequence sketches
};

// One pair's score-only result (AllPairIterator::scores): the optimal penalty without a CIGAR, WFA2's
// AlignmentScope::ComputeScore.  status: AWV_ST_*; penalty: exact when AWV_ST_COMPLETED, max_penalty + 1 when
// AWV_ST_ABOVE_BOUND, 0 on failure.
struct PairScore {
  size_t query_idx = 0, target_idx = 0;
  bool is_reverse = false;
  int32_t penalty = 0;
  int32_t status = AWV_ST_COMPLETED;
};

using Callback = std::function<void(AlignmentResult&&)>;  // may throw: first error aborts the run

// One interval pair to align globally (awv_range_pair): query[query_start, query_end) -- on the query's FORWARD strand, as PAF
// writes it, also when is_reverse -- against target[target_start, target_end).  Its AlignmentResult carries these coordinates
// (a failed range: query_start twice and target_start twice, an empty CIGAR), so alignment_to_paf prints columns 3-4 and 8-9
// as the interval and columns 2 and 7 as the full lengths.
struct AlignmentRange {
  size_t query_idx = 0, target_idx = 0;
  bool is_reverse = false;
  size_t query_start = 0, query_end = 0, target_start = 0, target_end = 0;
};

// One pair whose alignment did not pass the on-device check (AllPairIterator::with_verify): code = AWV_VF_*, column and
// penalty as in awv_verify_result.
struct VerifyFailure {
  size_t index = 0;  // in the pair list
  size_t query_idx = 0, target_idx = 0;
  bool is_reverse = false;
  int32_t code = 0;
  int64_t column = -1, penalty = -1;
};
// What run() does with one engine call's verify results vr[0, m): entry i of the call is entry k = idx ? idx[i] : i of the
// run's range plist (pair-list index first + k), on strand rev[i]; every code other than OK / SKIPPED is appended.
void append_verify_failures(std::vector<VerifyFailure>& out, const awv_verify_result* vr, int64_t m, size_t first, const size_t* idx,
                            const std::pair<size_t, size_t>* plist, const uint8_t* rev);
void sort_verify_failures(std::vector<VerifyFailure>& f);  // by pair-list index (the slots' lists, merged)
// `--verify`'s report: up to `limit` lines `verify: pair <index> <qname> <tname> <strand> <class> column <c> penalty <p>`
// appended to `out`; returns the exit status, 4 when there is a failure, else 0
int report_verify_failures(const std::vector<VerifyFailure>& vf, const std::vector<Sequence>& sequences, std::string& out, size_t limit = 20);
const char* verify_code_name(int32_t code);  // "ok", "skipped", "bad_op", "overrun", "m_differs", "x_equal", "short", "counts", "penalty"

// awv_engine_config.flags (AWV_F_*) for the per-device engines this library creates from now on
// (an engine lives for the rest of the process once created).
void set_engine_flags(int flags);
void set_engine_first_row_cols(int cols);  // awv_engine_config.first_row_cols, likewise (diagnostic / test hook)
// destroys the engines this library holds, one per (device, slot) (their HBM arenas are freed; the next run creates fresh
// ones with the flags then in force) and forgets the scratch split of devices that ran several slots
void release_engines();
// number of HIP devices visible to this process, asked of the HIP runtime liballwave_hip has loaded; throws AlignmentError
// when there is none
int visible_device_count();

class AllPairParallelIterator;
class AllPairIterator;

// The options of one run that filter or rewrite what it delivers, in one place: AllPairIterator::with_max_penalty,
// with_max_divergence (std::nullopt: no bound), with_clip and with_split (match bonus 0: off), with_normalize (AWV_NORM_OFF: off),
// with_device_cigar, with_cs (0: off), with_coverage (0: off), with_variants, with_liftover (liftover_from 0: off),
// with_msa (msa false: off).
struct RunOptions {
  std::optional<int> max_penalty;
  std::optional<double> max_divergence;
  int clip_match_bonus = 0;
  int64_t clip_min_score = 1;
  int split_match_bonus = 0;
  int64_t split_min_score = 1;
  int normalize = AWV_NORM_OFF;
  bool device_cigar = false;
  int cs = 0;
  int coverage = 0;
  bool variants = false;
  std::vector<awv_region> liftover;  // with liftover_from: the regions lifted through the run's alignments
  int liftover_from = 0;             // AWV_LIFT_FROM_TARGET, AWV_LIFT_FROM_QUERY or AWV_LIFT_FROM_BOTH; 0: off
  bool msa = false;                  // with msa_targets (empty: every sequence) and msa_max_bytes: the multiple alignments built from the run's alignments
  std::vector<int> msa_targets;
  uint64_t msa_max_bytes = (uint64_t)1 << 30;
  void apply(AllPairIterator& it) const;  // the with_* calls of what is set; they throw std::invalid_argument as documented there
  bool any() const { return max_penalty || max_divergence || clip_match_bonus != 0 || split_match_bonus != 0 || normalize != AWV_NORM_OFF || device_cigar || cs != 0 || coverage != 0 || variants || liftover_from != 0 || msa; }
};

// What a run leaves behind besides its results (AllPairIterator::last_report): the failed checks sorted by pair-list index,
// and every counter summed over the slots (kernel_ms: summed kernel time).
struct RunReport {
  std::vector<VerifyFailure> verify_failures;
  awv_verify_stats verify_stats{};
  BoundStats bound_stats{};
  ClipStats clip_stats{};
  SplitStats split_stats{};
  awv_norm_stats normalize_stats{};
  awv_encode_stats encode_stats{};
  awv_cs_stats cs_stats{};
  awv_cov_stats coverage_stats{};
  awv_variants_stats variants_stats{};  // rows: of the merged table; folds: the engines' folds
  awv_lift_stats lift_stats{};
  awv_msa_stats msa_stats{};  // of the run's one awv_msa_ranges call
};

// One target's multiple alignment of a run with with_msa (AllPairIterator::last_msa): rows x width bytes, row-major; names[0] is the
// target's name, names[r] of an item's row `qname/qbeg-qend` and the strand sign, the query interval on the forward strand.
struct MsaBlock {
  int t_idx = 0;
  int64_t rows = 0, width = 0;
  std::vector<std::string> names;
  std::vector<uint8_t> bytes;
};

// The per-base depth a run with with_coverage leaves behind (AllPairIterator::last_coverage): sequence s owns entries
// [offsets[s], offsets[s + 1]) of both tracks, one per forward-strand base.  Empty without the setting.
struct Coverage {
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> aligned, matched;
};

class AllPairIterator {  // iterator.rs:12-171
 public:
  AllPairIterator(const std::vector<Sequence>& sequences, AlignmentParams params);  // ::new
  static AllPairIterator with_options(const std::vector<Sequence>& sequences, AlignmentParams params,
                                      bool exclude_self, bool use_mash_orientation, SparsificationStrategy s);
  // the same, the pair list planned on the HIP device `plan_device` (planner.hpp's device variants: the same list, byte for byte;
  // AlignmentError without that device); plan_device < 0: on the host, as above.  The plan device also runs mash orientation.
  static AllPairIterator with_options(const std::vector<Sequence>& sequences, AlignmentParams params, bool exclude_self,
                                      bool use_mash_orientation, SparsificationStrategy s, int plan_device);
  // An iterator over a list of interval pairs instead of a planned pair list: entry k aligns ranges[k] (awv_align_ranges; the
  // strand is the range's own, no orientation pass runs).  Every consumer, with_devices, with_verify, with_min_batch_pairs and
  // scores() work as on a pair list -- the same slots and batches; with_shard and with_sparsification do not apply.
  // std::invalid_argument for an index or an interval out of range.
  static AllPairIterator for_ranges(const std::vector<Sequence>& sequences, std::vector<AlignmentRange> ranges, AlignmentParams params);
  // the device mash orientation and with_sparsification plan on from now on (< 0: the host, the default); the current list stays
  AllPairIterator& with_plan_device(int plan_device);
  int plan_device() const { return plan_device_; }
  AllPairIterator& with_orientation_params(AlignmentParams p);
  // iterator.rs:101-110: a NEW iterator over the same sequences / params / exclude_self / orientation choice with the pair
  // list planned again under `strategy` -- through with_options, exactly like the reference, so the orientation params go
  // back to their default (edit_distance) there too; the device and thread settings (this build's extensions) carry over
  AllPairIterator with_sparsification(SparsificationStrategy strategy) const;
  // iterator.rs:113-125: the batch-parallel consumer (rayon's par_iter in the reference)
  AllPairParallelIterator into_par_iter() const;
  // iterator.rs:151-171 (`impl Iterator`): the next pair's alignment, in pair-list order; std::nullopt at the end.  A per-pair
  // call cannot feed a GPU, so the results are buffered: an empty buffer aligns the next `next_chunk` pairs in one engine call.
  std::optional<AlignmentResult> next();
  AllPairIterator& with_next_chunk(size_t pairs_per_engine_call);
  // host threads for sketching / orientation / formatting of THIS iterator's runs (the reference's `-t`; 0 = the
  // process-wide planner::host_threads())
  AllPairIterator& with_threads(int host_threads);
  AllPairIterator& with_orientation(Orientation o);
  // WFA orientation (awv_orient_pairs) decides a pair from bounded strand scores wherever those prove which strand has
  // fewer edits, and aligns both strands in full only where they do not; true: both strands in full for every pair, the
  // reference's method (AWV_ORIENT_FULL).  The strands chosen are the same.
  AllPairIterator& with_full_wfa_orientation(bool full);
  // Every alignment consumer (for_each_with_callback, for_each_paf_batch, next, into_par_iter, collect) goes through
  // awv_align_pairs_verified: each batch's records and op bytes are checked on the device before they are copied back.  The
  // results handed out are the same; what failed is listed by verify_failures().  scores() ignores the setting, and the
  // strand alignments inside WFA orientation are not checked: only the final ones are.
  AllPairIterator& with_verify(bool on);
  bool verify() const { return verify_; }
  // Bounds on the final alignments (awv_align_pairs_bounded / awv_align_ranges_bounded).  A pair above a bound reaches no
  // alignment consumer -- no callback, no next() item, no PAF line (unlike a failed pair, which still gives the reference's
  // "empty" result); last_bound_stats() counts what was left out.  Orientation runs first, under its own penalties, untouched;
  // scores() ignores both.
  //   with_max_penalty(B), B >= 0: a pair whose optimal penalty exceeds B is abandoned inside its top-level search.
  //   with_max_divergence(d), 0 <= d < 1: keeps the pairs whose alignment has (#X + #I + #D) <= d * columns.  Each pair is
  //   searched under awv_divergence_bound(pen, plen, tlen, d) (a range: its rectangle's lengths), and a completed pair is
  //   kept iff (double)E <= d * (double)columns on its record's counts.  AlignmentParams::max_divergence of the alignment
  //   params means the same; the setter wins.  With both bounds the smaller penalty bound applies.
  // Every alignment consumer receives each alignment clipped to its best-scoring segment (awv_align_pairs_clipped /
  // awv_align_ranges_clipped; include/allwave_hip.h has the contract): cigar_bytes is the slice, num_matches,
  // alignment_length and score (= -penalty, the segment re-scored) are the segment's.  A pair whose clip is empty or scores
  // below min_score reaches no consumer, like a pair above a bound; a failed pair still gives the "empty" result.
  // Coordinates follow PAF.  With [qb, qe) the query's range (the whole sequence on a pair list), tb the target range's
  // start, q_skip / t_skip the bases before the segment and q_len / t_len the bases it consumes:
  //   forward:  query_start = qb + q_skip, query_end = query_start + q_len
  //   reverse:  query_end = qe - q_skip, query_start = query_end - q_len     (on the query's FORWARD strand)
  //   target_start = tb + t_skip, target_end = target_start + t_len
  // so a clipped '-' line of a whole-sequence pair carries forward-strand query coordinates -- the convention check_paf's
  // `partial` and parse_paf_ranges read.  The full alignment is what with_verify checks and what the bounds filter on, as
  // without clipping; scores() ignores the setting.  1 <= match_bonus <= 32767, min_score >= 1.
  AllPairIterator& with_clip(int match_bonus, int64_t min_score = 1);
  bool clip() const { return clip_bonus_ > 0; }
  // Every alignment consumer receives one AlignmentResult per segment of each alignment's split (awv_align_pairs_split /
  // awv_align_ranges_split: every maximal segment that scores at least min_score), in column order within a pair and pair
  // order across the pairs of a batch; each is what with_clip would give for that segment, coordinates included.  A pair
  // without a segment reaches no consumer.  Segment storage is allocated per engine call from awv_split_layout_*.  Not
  // together with with_clip (std::invalid_argument); scores() ignores the setting.
  AllPairIterator& with_split(int match_bonus, int64_t min_score);
  bool split() const { return split_bonus_ > 0; }
  SplitStats last_split_stats() const { return report_.split_stats; }
  // of the last run (next(): of the chunks since the list's start), summed over the slots
  ClipStats last_clip_stats() const { return report_.clip_stats; }
  // Every alignment consumer receives each alignment with its gap runs at their left- (AWV_NORM_LEFT) or right-normal
  // (AWV_NORM_RIGHT) place (awv_engine_set_normalize; include/allwave_hip.h has the contract): every slot's engine gets the
  // mode for its engine calls, under its device's mutex, and is switched off again afterwards.  Normalization comes before the
  // check, the clip and the split, which then describe the normalized string; records and coordinates are unchanged.
  // scores() and orientation ignore the setting.  AWV_NORM_OFF: off (the default).
  AllPairIterator& with_normalize(int direction);
  int normalize() const { return normalize_; }
  // of the last run (next(): of the chunks since the list's start), summed over the slots (kernel_ms: summed kernel time)
  awv_norm_stats last_normalize_stats() const { return report_.normalize_stats; }
  // for_each_paf_batch takes every CIGAR's run-length text from the device (awv_align_pairs_encoded / awv_align_ranges_encoded;
  // include/allwave_hip.h has the contract): each batch's op strings -- normalized, and clipped, when those are set -- are
  // encoded on the device, the text comes back in the op bytes' place and goes into the PAF lines as it is.  The lines are
  // byte-identical to those of a run without the setting.  The consumers that hand out cigar_bytes (for_each_with_callback,
  // next, into_par_iter, collect) and scores() ignore it.  Not together with with_split (std::invalid_argument).
  AllPairIterator& with_device_cigar(bool on);
  bool device_cigar() const { return device_cigar_; }
  // of the last run, summed over the slots (kernel_ms: summed kernel time)
  awv_encode_stats last_encode_stats() const { return report_.encode_stats; }
  // for_each_paf_batch appends minimap2's cs difference string to every line, "\tcs:Z:<text>" after the cg:Z: field
  // (AWV_CS_SHORT / AWV_CS_LONG; 0: off; awv_align_pairs_cs / awv_align_ranges_cs, include/allwave_hip.h has the contract): the
  // text is made on the device from each batch's op strings -- normalized, and clipped, when those are set -- and the resident
  // sequences, and copied back next to the CIGARs.  The line up to the tag is the line without the setting.  The consumers that
  // hand out AlignmentResults (for_each_with_callback, next, into_par_iter, collect) and scores() ignore it.  Not together with
  // with_split (std::invalid_argument).
  AllPairIterator& with_cs(int mode);
  int cs() const { return cs_; }
  // of the last run, summed over the slots (kernel_ms: summed kernel time)
  awv_cs_stats last_cs_stats() const { return report_.cs_stats; }
  // Every alignment consumer also accumulates the per-base depth of what the engine aligned (awv_engine_coverage_begin;
  // include/allwave_hip.h has the contract): roles is AWV_COV_TARGET, AWV_COV_QUERY or AWV_COV_BOTH, 0: off.  Every slot's engine
  // begins at a run's start -- with with_clip's min_score as its clip_min_score -- and is read at the run's end; the slots' arrays
  // are summed on the host, so several devices, and one ordinal given twice, give the one-engine result exactly.  What counts is
  // what the contract says: with_clip's slices that reach min_score, with_split's segments, else every completed record, after
  // with_normalize; the strand alignments of WFA orientation do not count, nor does scores().  (A completed pair that only
  // with_max_divergence's host-side test drops has been aligned under its bound, and counts.)  Results, lines and the other
  // counters are those of the run without the setting.  next() accumulates since the list's start, like the report.
  AllPairIterator& with_coverage(int roles);
  int coverage() const { return coverage_; }
  const Coverage& last_coverage() const { return cov_; }
  // Every alignment consumer also tallies the per-site allele table of what the engine aligned (awv_engine_variants_begin;
  // include/allwave_hip.h has the contract).  Every slot's engine keeps a table of its own; the slots' tables are concatenated and
  // folded on the host (awv_variants_fold_host: sum and min), so several devices, or one ordinal given twice, give the
  // one-engine table exactly.  Clipping runs count the clips that reach clip_min_score.  last_variants(): the table of the last
  // run, in key order (next(): since the list's start); empty without the setting.
  AllPairIterator& with_variants(bool on) {
    variants_ = on;
    return *this;
  }
  bool variants() const { return variants_; }
  const std::vector<awv_variant>& last_variants() const { return var_; }
  // Every alignment consumer also lifts `regions` (forward strand, any order; they may overlap, nest and repeat) through what the
  // engine aligned (awv_engine_lift_begin; include/allwave_hip.h has the contract): regions on an alignment's target under
  // AWV_LIFT_FROM_TARGET, on its query under AWV_LIFT_FROM_QUERY, both under AWV_LIFT_FROM_BOTH; from 0: off.  Every slot's
  // engine keeps a table of its own; the slots' rows are concatenated and sorted on the host, so several devices, or one ordinal
  // given twice, give the one-engine table exactly.  What an alignment contributes is the coverage rule.  last_liftover(): the
  // table of the last run, in the rows' order (next(): since the list's start); empty without the setting.
  // std::invalid_argument for a mask other than these and for a region outside its sequence.
  AllPairIterator& with_liftover(std::vector<awv_region> regions, int from);
  int liftover_from() const { return lift_from_; }
  const std::vector<awv_region>& liftover_regions() const { return lift_regions_; }
  const std::vector<awv_lift_row>& last_liftover() const { return lift_; }
  // Every alignment consumer also lays every sequence out against each of `targets` (distinct sequence indices; empty: every
  // sequence) as a target-anchored multiple alignment, on the device (awv_msa_ranges; include/allwave_hip.h has the contract).  The
  // batch sink keeps, on the host, what the run delivered for the chosen targets -- whole completed records, a clip's slice that
  // reaches clip_min_score, every split segment, after normalization: pair, span, slice and op bytes -- and after the run makes one
  // call on the run's first device, so several devices, or one ordinal given twice, give the one-engine blocks exactly.  The rows
  // of a target are ordered by (q_idx, q_revcomp, pattern begin, column begin).  The kept op bytes and the arena of blocks are each
  // bounded by max_bytes: beyond it the run's alignments are delivered as always, and then the run fails with an AlignmentError
  // that names the bound and the size needed.  Not together with with_device_cigar (the sink then carries text, not op bytes).
  // std::invalid_argument for a target out of range or named twice, and for max_bytes == 0.
  AllPairIterator& with_msa(std::vector<int> targets, uint64_t max_bytes = (uint64_t)1 << 30);
  AllPairIterator& without_msa() { msa_ = false; msa_targets_.clear(); return *this; }
  bool msa() const { return msa_; }
  const std::vector<MsaBlock>& last_msa() const { return msa_blocks_; }
  AllPairIterator& with_max_penalty(int max_penalty);
  AllPairIterator& with_max_divergence(double max_divergence);
  // of the last run (next(): of the chunks since the list's start), summed over the slots
  BoundStats last_bound_stats() const { return report_.bound_stats; }
  // of the last run (next(): of the chunks since the list's start): the failed pairs sorted by pair-list index, and the
  // verify counters summed over the slots (kernel_ms: summed kernel time)
  const std::vector<VerifyFailure>& verify_failures() const { return report_.verify_failures; }
  awv_verify_stats last_verify_stats() const { return report_.verify_stats; }
  const RunReport& last_report() const { return report_; }  // all of the last_*_stats() and verify_failures() in one
  AllPairIterator& with_device(int device);  // = with_devices({device})
  // Aligns the pair list on several engines at once, one "slot" per entry: an ordinal may appear more than once, and each
  // occurrence is an engine of its own (stream, arenas; the slots of one device split its default scratch budget).  With
  // two or more slots the list is cut into planner::device_batches, handed out from one cursor to one submitter thread per
  // slot; one slot aligns the list in one batch on the calling thread.
  AllPairIterator& with_devices(std::vector<int> devices);
  // pairs per batch at the least when several slots share the list (default 16,384: 4 x the engine's pairs in flight)
  AllPairIterator& with_min_batch_pairs(size_t pairs);
  const std::vector<int>& devices() const { return devices_; }
  // keep this process's part of a cost-balanced partition of the planned list into `world` shards
  // (planner::assign_shards_lpt: every process derives the same partition, each keeps its pairs in list
  // order; one process per GPU, or per group of GPUs with with_devices)
  AllPairIterator& with_shard(size_t rank, size_t world);
  size_t pair_count() const { return pairs_.size(); }
  const std::vector<std::pair<size_t, size_t>>& get_pairs() const { return pairs_; }
  // iterator.rs:127-137,206-253: streams results (order unspecified in the reference for T>1; here
  // batches arrive in pair order on one slot, in no fixed order on several).  Calls never overlap.
  void for_each_with_callback(const Callback& cb);
  // formats every record with alignment_to_paf on a small thread pool and hands whole batches to
  // `sink` (replaces the single unbuffered writer thread of src/main.rs:347-367); sink calls never overlap
  void for_each_paf_batch(const std::function<void(const std::string&)>& sink, int format_threads = 8);
  // Score-only consumer (awv_score_pairs): one PairScore per planned pair, in pair-list order, through the same orientation,
  // sparsification, shard and device settings as the alignment consumers (the final alignment is scored only; WFA orientation
  // is awv_orient_pairs: bounded strand scores, full alignments only for the pairs those leave open).  max_penalty: a bound -- pairs proved above it come back
  // AWV_ST_ABOVE_BOUND, and their search stops there.
  std::vector<PairScore> scores(std::optional<int> max_penalty = std::nullopt);
  // counters of the last run, summed over its slots (kernel_ms: summed kernel time, not wall time)
  awv_stats last_stats() const { return stats_; }
  // the same, one entry per slot, in with_devices order
  const std::vector<awv_stats>& last_slot_stats() const { return slot_stats_; }

 private:
  friend class AllPairParallelIterator;
  // One engine call's results, handed to a run's batch callback: results res[0, n) belong to entries first .. first + n - 1
  // of the call's pair array, whose pair-list index is pair(i) (relative to the run's range) and orientation is_rev(i).
  struct Batch {
    int64_t first, n;
    const awv_result* res;
    const uint8_t* arena;
    const uint8_t* rev;  // per entry of the call's pair array
    const size_t* idx;   // pair-list index per entry; nullptr: the entry's own position
    const awv_clip_result* clip = nullptr;  // a clipping run: per entry its clip; res[] then describes the segment
    const awv_cigar_text* text = nullptr;   // an encoding run: per entry its text; `arena` is then the call's text arena
    const awv_cigar_text* text_at(int64_t i) const { return text ? text + first + i : nullptr; }
    const awv_cs_text* cs = nullptr;        // a cs run: per entry its cs text, in the call's cs arena
    const uint8_t* cs_arena = nullptr;
    const awv_cs_text* cs_at(int64_t i) const { return cs ? cs + first + i : nullptr; }
    size_t pair(int64_t i) const { return idx ? idx[first + i] : (size_t)(first + i); }
    const awv_clip_result* clip_at(int64_t i) const { return clip ? clip + first + i : nullptr; }
    bool is_rev(int64_t i) const { return rev[first + i] != 0; }
  };
  using BatchCb = std::function<void(const Batch&)>;
  // The engine call a run makes per batch: an alignment call, or awv_score_pairs under max_penalty (< 0: no bound; one sink
  // call per batch, results carry status and penalty, no arena); encode: the alignment call's _encoded form (with_device_cigar);
  // cs: its _cs form under that mode (with_cs), which takes the encoding too.
  struct EngineCall {
    bool score_only;
    int32_t max_penalty;
    bool encode;
    int cs;
  };
  // pairs_[first, first + count) on the with_devices slots; batch indices are relative to `first`.  Per batch: orientation,
  // one engine call, the batch callback, the counters.  One slot: one batch, the whole range in list order, on the calling
  // thread.  With several slots, batch callbacks of different slots run concurrently: consumers that call user code
  // serialise it.
  void run(size_t first, size_t count, const BatchCb& batch_cb, EngineCall call = {false, -1, false, 0});
  void run(const BatchCb& batch_cb, EngineCall call = {false, -1, false, 0}) { run(0, pairs_.size(), batch_cb, call); }
  // run()'s steps (allwave.cpp): what the slots of one run share and what each of them counts; one batch made ready for its
  // engine call; the engine's sink, which hands a call's results to the batch callback; the counters taken after a call
  struct RunState;
  struct SlotTotals;
  struct PreparedBatch;
  struct SinkCtx;
  PreparedBatch prepare_batch(const RunState& rs, awv_engine* e, size_t b, SlotTotals& totals) const;
  static int batch_sink(void* user, int64_t first, int64_t cnt, const awv_result* res, const uint8_t* arena);
  static int batch_cs_sink(void* user, int64_t first, int64_t cnt, const awv_result* res, const uint8_t* arena, const uint8_t* cs_arena);
  static void take_call_totals(const RunState& rs, const PreparedBatch& pb, awv_engine* e, bool ok, SlotTotals& totals);
  // run(first, count) into one result per delivered entry, in pair-list order: a pair's segments in column order (with_split),
  // the pairs a run drops left out
  std::vector<AlignmentResult> collect_ordered(size_t first, size_t count);
  // align_pair's result mapping for entry k of the pair list (a range list: in the range's coordinates)
  // cl (nullable): the entry's clip, r the segment's record -- the coordinates are shifted by the skips (with_clip)
  AlignmentResult result_at(size_t k, bool is_rev, const awv_result& r, const uint8_t* arena, bool copy_cigar,
                            const awv_clip_result* cl = nullptr) const;
  std::shared_ptr<const std::vector<AlignmentRange>> ranges_;  // for_ranges: entry k of pairs_ is this interval pair
  AllPairIterator(const std::vector<Sequence>& sequences, AlignmentParams params, bool enumerate);  // enumerate = false: no pairs
  const std::vector<Sequence>& sequences_;
  AlignmentParams params_, orientation_params_;
  int plan_device_ = -1;
  bool exclude_self_ = true;
  Orientation orientation_ = Orientation::Wfa;
  bool full_wfa_orientation_ = false;
  bool verify_ = false;
  std::optional<int> max_penalty_;
  std::optional<double> max_divergence_;
  std::optional<double> divergence_bound() const { return max_divergence_ ? max_divergence_ : params_.max_divergence; }
  bool bounded() const { return max_penalty_.has_value() || divergence_bound().has_value(); }
  int clip_bonus_ = 0;  // with_clip (0: off)
  int64_t clip_min_score_ = 1;
  int normalize_ = AWV_NORM_OFF;  // with_normalize
  bool device_cigar_ = false;     // with_device_cigar
  int cs_ = 0;                    // with_cs (0: off)
  int coverage_ = 0;              // with_coverage (0: off)
  Coverage cov_;                  // of the last run (next(): since the list's start)
  bool variants_ = false;         // with_variants
  std::vector<awv_variant> var_;  // the allele table of the last run (next(): since the list's start)
  int lift_from_ = 0;                     // with_liftover (0: off)
  std::vector<awv_region> lift_regions_;  // its regions
  std::vector<awv_lift_row> lift_;        // the lifted rows of the last run (next(): since the list's start)
  // with_msa: what the sink keeps of an item, the kept op bytes, what they would take without the bound, and the last run's blocks
  struct MsaKept {
    awv_range_pair range;
    int32_t q_skip, t_skip, pattern_beg;
    uint32_t col_beg, len;
    uint64_t off;  // of the item's op bytes
  };
  struct MsaStore {
    std::vector<MsaKept> kept;
    std::vector<uint8_t> ops;
    uint64_t need = 0;
  };
  bool msa_ = false;
  std::vector<int> msa_targets_;
  uint64_t msa_max_bytes_ = (uint64_t)1 << 30;
  MsaStore msa_store_;                 // of the last run (next(): since the list's start)
  std::vector<MsaBlock> msa_blocks_;
  void keep_msa(const RunState& rs, const Batch& b, MsaStore& st) const;
  awv_msa_stats build_msa(awv_engine* e);
  int split_bonus_ = 0;  // with_split (0: off)
  int64_t split_min_score_ = 1;
  bool drops_pairs() const { return bounded() || clip() || split(); }  // consumers that keep a slot per pair compact what was delivered
  RunReport report_;
  std::vector<int> devices_{0};
  size_t min_batch_pairs_ = 16384;
  int threads_ = 0;
  std::vector<std::pair<size_t, size_t>> pairs_;
  awv_stats stats_{};
  std::vector<awv_stats> slot_stats_;
  // sequential iteration (next): position in the pair list and the buffered results of the running chunk
  size_t next_pos_ = 0, next_chunk_ = 16384;
  std::vector<AlignmentResult> next_buf_;
  size_t next_buf_pos_ = 0;
};

// iterator.rs:174-253.  The reference's parallel iterator maps align_pair over the pairs on rayon's workers and hands every
// result to a consumer that runs on those workers concurrently; here the pairs go through the engine in batches and every
// batch's results are handed to `callback` from `threads` host threads at once (same contract: the callback must be
// thread-safe; the first error it throws wins, stops the run and is rethrown -- iterator.rs:220-251).
class AllPairParallelIterator {
 public:
  size_t pair_count() const { return it_.pair_count(); }
  AllPairParallelIterator& with_threads(int threads) { threads_ = threads; return *this; }
  void for_each_with_callback(const Callback& cb);   // iterator.rs:206-253
  std::vector<AlignmentResult> collect();           // rayon's collect() on the parallel iterator: results in pair-list order
  awv_stats last_stats() const { return it_.last_stats(); }
  const std::vector<awv_stats>& last_slot_stats() const { return it_.last_slot_stats(); }
  const std::vector<VerifyFailure>& verify_failures() const { return it_.verify_failures(); }
  awv_verify_stats last_verify_stats() const { return it_.last_verify_stats(); }
  BoundStats last_bound_stats() const { return it_.last_bound_stats(); }
  ClipStats last_clip_stats() const { return it_.last_clip_stats(); }
  SplitStats last_split_stats() const { return it_.last_split_stats(); }
  awv_norm_stats last_normalize_stats() const { return it_.last_normalize_stats(); }
  awv_encode_stats last_encode_stats() const { return it_.last_encode_stats(); }
  awv_cs_stats last_cs_stats() const { return it_.last_cs_stats(); }
  const Coverage& last_coverage() const { return it_.last_coverage(); }
  const std::vector<awv_variant>& last_variants() const { return it_.last_variants(); }
  const std::vector<awv_lift_row>& last_liftover() const { return it_.last_liftover(); }
  const std::vector<MsaBlock>& last_msa() const { return it_.last_msa(); }
  const RunReport& last_report() const { return it_.last_report(); }
 private:
  friend class AllPairIterator;
  explicit AllPairParallelIterator(const AllPairIterator& it) : it_(it) {}
  AllPairIterator it_;
  int threads_ = 0;  // 0 = planner::host_threads()
};

// lib.rs:57-68: AllPairIterator::with_options(sequences, params, exclude_self = true, mash orientation = true, sparsification)
// .for_each_with_callback(callback) on device 0 (the overload below with devices {0}); the callback may throw (first error
// aborts and is rethrown)
void process_alignments_with_callback(const std::vector<Sequence>& sequences, AlignmentParams params,
                                      SparsificationStrategy sparsification, const Callback& callback);
// the same on the engines `devices` names (AllPairIterator::with_devices; the callback's calls never overlap)
void process_alignments_with_callback(const std::vector<Sequence>& sequences, AlignmentParams params,
                                      SparsificationStrategy sparsification, const Callback& callback,
                                      const std::vector<int>& devices);

// A range's engine record as an AlignmentResult in the sequences' coordinates: the record's q_end / t_end are consumed
// lengths, so the interval's starts are added (a failed record: the starts twice, score i32::MAX, no CIGAR).
AlignmentResult range_alignment_result(const AlignmentRange& range, const awv_result& r, const uint8_t* arena, bool copy_cigar);

// The interval pairs `ranges` aligned globally under `params` on the engines `devices` names (AllPairIterator::for_ranges +
// for_each_with_callback: the callback's calls never overlap; on one slot they come in list order).  verify: every finished
// range is checked on the device (awv_align_ranges_verified); failures (nullable) receives what failed, index = list index.
void align_ranges(const std::vector<Sequence>& sequences, const std::vector<AlignmentRange>& ranges, AlignmentParams params,
                  const Callback& callback, const std::vector<int>& devices = {0}, bool verify = false,
                  std::vector<VerifyFailure>* failures = nullptr, awv_verify_stats* verify_stats = nullptr);
// the same under `options` (a range above a bound, or without a clip or a segment worth reporting, gives no callback; a split
// range gives one per segment); report (nullable) receives what the run left behind
void align_ranges(const std::vector<Sequence>& sequences, const std::vector<AlignmentRange>& ranges, AlignmentParams params,
                  const Callback& callback, const std::vector<int>& devices, bool verify, const RunOptions& options,
                  RunReport* report = nullptr);

// ---- mappings in, alignments out: the interval pairs a PAF file names (columns 1-9 of each line) ----
struct PafRangeLine {
  size_t line = 0;   // 1-based line of the text
  std::string cls;   // empty: ranges[index] is this line's interval pair; else "bad_line", "unknown_name", "length_mismatch"
  size_t index = 0;
};
struct PafRanges {
  std::vector<AlignmentRange> ranges;  // of the good lines, in line order
  std::vector<PafRangeLine> lines;     // every non-empty line
};
// Names are resolved as check_paf resolves them (the first of equal names).  "bad_line": fewer than 9 columns, a strand other
// than + / -, a number that does not parse, or an interval that is not 0 <= start <= end <= length.
PafRanges parse_paf_ranges(const std::vector<Sequence>& sequences, const std::string& paf_text);

// ---- checking a PAF file against the sequences, on the device (nothing is aligned) ----
// the op bytes of a PAF cg string, cigar_bytes_to_string undone ('=' -> M, X -> X, D -> I, I -> D); false when the string
// is not <count><op>... over those four letters with counts >= 1
bool cigar_string_to_bytes(const std::string& cg, std::vector<uint8_t>& ops);

struct PafCheckFailure {
  size_t line = 0;  // 1-based line of the PAF text
  std::string qname, tname;
  char strand = '?';
  // host-side: "bad_line", "unknown_name", "length_mismatch", "not_end_to_end", "bad_cigar"; from the device check:
  // "bad_op", "overrun", "m_differs", "x_equal", "short", "counts"; with `optimal`: "not_optimal", "below_optimum"
  std::string cls;
  int64_t column = -1, penalty = -1;  // as in awv_verify_result
  int64_t optimum = -1;               // with `optimal`, for lines whose op string is valid: the optimal penalty (-1: none)
};
struct PafCheckReport {
  size_t lines = 0, checked = 0, skipped = 0;  // non-empty lines; lines that went through the device check; empty records
  std::vector<PafCheckFailure> failures;       // in line order
  awv_verify_stats stats{};
};
// Every line of `paf_text` (12 columns and a cg:Z: tag, as alignment_to_paf writes them) against `sequences` under `params`:
// names, lengths and end-to-end coordinates on the host, the op string and the counts (column 10 = #M, column 11 = the
// longer span) through awv_verify_cigars on `device`.  A line carries no penalty: the re-scored one is reported and never
// compared.  optimal: awv_score_pairs on the same (pair, strand) list as well; an op string that costs more than the
// optimum is "not_optimal", one that costs less "below_optimum" (a finding against the engine, not the PAF).
// partial: a line whose coordinates are a proper interval (0 <= start <= end <= length on both sequences) is checked as the
// global alignment of that interval pair (awv_verify_ranges; `optimal`: awv_score_ranges) instead of being "not_end_to_end".
PafCheckReport check_paf(const std::vector<Sequence>& sequences, const std::string& paf_text, const AlignmentParams& params,
                         bool optimal, int device = 0, bool partial = false);
// one tab-separated line per failure: line qname tname strand class column penalty [optimum]
std::string format_paf_check(const PafCheckReport& r);

namespace wfa {  // src/wfa.rs
struct Penalties { int32_t mismatch, gap_opening1, gap_extension1, gap_opening2, gap_extension2; };
struct AlignmentResult {
  int32_t score;
  std::string cigar;
  size_t matches, mismatches, insertions, deletions, alignment_length;
};
// wfa.rs:105-176 -- returns "" when valid, else the reference's message
std::string validate_cigar_alignment(const uint8_t* cigar, size_t n, size_t query_len, size_t reference_len);
// wfa.rs:178-258 (fresh aligner per call in the reference; here one engine call)
AlignmentResult align_sequences(const std::vector<uint8_t>& pattern, const std::vector<uint8_t>& text,
                                const Penalties& p, AlignmentMode mode, int device = 0);
}  // namespace wfa

}  // namespace allwave
