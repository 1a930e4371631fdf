// capi.cpp -- extern "C" hooks over the C++ host mirror so the Python tests and bench.py can drive
// it through ctypes (plain pointers and sizes only).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "allwave.hpp"
#include "planner.hpp"

using namespace allwave;

namespace {
void set_err(char* err, size_t cap, const std::string& m) {
  if (err && cap) snprintf(err, cap, "%s", m.c_str());
}
// What the calling thread's last alignment hook left behind, its iterator's last_report(): the verify counters and failures
// for awh_last_verify, the other counters for awh_last_bounds, awh_last_clip, awh_last_split, awh_last_normalize, awh_last_encode and awh_last_cs.
thread_local RunReport g_report;
thread_local Coverage g_coverage;  // and its last_coverage(), for awh_last_coverage
thread_local std::vector<awv_variant> g_variants;  // and its last_variants(), for awh_last_variants
thread_local std::vector<awv_lift_row> g_liftover;  // and its last_liftover(), for awh_last_liftover
thread_local std::vector<MsaBlock> g_msa;           // and its last_msa(), for awh_last_msa_block
template <typename It>
void keep(const It& it) {
  g_report = it.last_report();
  g_coverage = it.last_coverage();
  g_variants = it.last_variants();
  g_liftover = it.last_liftover();
  g_msa = it.last_msa();
}
// The options of the calling thread's NEXT alignment hook: awh_set_bounds, awh_set_clip, awh_set_split, awh_set_normalize and
// awh_set_device_cigar, awh_set_cs, awh_set_coverage, awh_set_variants, awh_set_liftover, awh_set_msa
// leave them here; the hook takes them (they hold for that one call) and starts the counters they go with afresh.
thread_local RunOptions g_next;
RunOptions take_run_options() {
  const RunOptions o = g_next;
  g_next = RunOptions{};
  g_report.bound_stats = BoundStats{};
  g_report.clip_stats = ClipStats{};
  g_report.split_stats = SplitStats{};
  g_report.normalize_stats = awv_norm_stats{};
  g_report.encode_stats = awv_encode_stats{};
  g_report.cs_stats = awv_cs_stats{};
  g_report.coverage_stats = awv_cov_stats{};
  g_coverage = Coverage{};
  g_report.variants_stats = awv_variants_stats{};
  g_variants.clear();
  g_report.lift_stats = awv_lift_stats{};
  g_liftover.clear();
  g_report.msa_stats = awv_msa_stats{};
  g_msa.clear();
  return o;
}
// the hooks' orientation code on an iterator: 0 forward, 1 WFA, 2 mash, 3 WFA by two full alignments per pair
void set_orientation(AllPairIterator& it, int orientation) {
  it.with_orientation(orientation == 0 ? Orientation::ForwardOnly : (orientation == 1 || orientation == 3) ? Orientation::Wfa : Orientation::Mash);
  it.with_full_wfa_orientation(orientation == 3);
}

std::vector<Sequence> make_seqs(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs) {
  std::vector<Sequence> s((size_t)n);
  for (int i = 0; i < n; ++i) {
    s[i].id = ids[i];
    s[i].seq.assign(bytes + offs[i], bytes + offs[i + 1]);
  }
  return s;
}

}  // namespace

extern "C" {

int awh_parse_scores(const char* s, int32_t out[6], int* n, char* err, size_t cap) {
  try {
    const AlignmentParams p = parse_scores(s);
    out[0] = p.match_score; out[1] = p.mismatch_penalty; out[2] = p.gap_open; out[3] = p.gap_extend;
    *n = 4;
    if (p.gap2_open && p.gap2_extend) { out[4] = *p.gap2_open; out[5] = *p.gap2_extend; *n = 6; }
    const awv_penalties q = to_penalties(p);
    (void)q;
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// mode of AlignmentMode::from_params: 0 edit, 1 single-piece, 2 two-piece; pen = penalties handed to the engine
int awh_mode_from_scores(const char* s, int* mode, int32_t pen[7], char* err, size_t cap) {
  try {
    const AlignmentParams p = parse_scores(s);
    *mode = (int)alignment_mode_from_params(p);
    const awv_penalties q = to_penalties(p);
    pen[0] = q.match; pen[1] = q.mismatch; pen[2] = q.gap_open1; pen[3] = q.gap_ext1; pen[4] = q.gap_open2; pen[5] = q.gap_ext2; pen[6] = q.two_piece;
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

int awh_cigar_to_string(const uint8_t* ops, size_t n, char* out, size_t cap) {
  const std::string s = cigar_bytes_to_string(ops, n);
  if (s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

int awh_reverse_complement(const uint8_t* in, size_t n, uint8_t* out) {
  const std::vector<uint8_t> r = reverse_complement(std::vector<uint8_t>(in, in + n));
  if (n) memcpy(out, r.data(), n);
  return 0;
}

// Formats one record from explicit fields (unit-tests alignment_to_paf without a GPU).
int awh_format_paf(const char* qid, size_t qlen, const char* tid, size_t tlen, size_t qs, size_t qe, size_t ts, size_t te,
                   int is_reverse, size_t num_matches, size_t alignment_length, const uint8_t* ops, size_t nops, char* out,
                   size_t cap) {
  std::vector<Sequence> seqs(2);
  seqs[0].id = qid; seqs[0].seq.assign(qlen, 'A');
  seqs[1].id = tid; seqs[1].seq.assign(tlen, 'A');
  AlignmentResult r;
  r.query_idx = 0; r.target_idx = 1; r.query_start = qs; r.query_end = qe; r.target_start = ts; r.target_end = te;
  r.is_reverse = is_reverse != 0; r.num_matches = num_matches; r.alignment_length = alignment_length;
  r.cigar_bytes.assign(ops, ops + nops);
  const std::string s = alignment_to_paf(r, seqs);
  if (s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// AllPairIterator + alignment_to_paf per record on the engines `devices[0, n_devices)` names (min_batch_pairs <= 0: the
// default; slot_stats: nullable, n_devices entries); out = the PAF lines
int awh_all_pairs_paf_devices(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores,
                              const char* sparsification, int orientation, int exclude_self, const int32_t* devices, int n_devices,
                              int64_t min_batch_pairs, int verify, awv_stats* slot_stats, char** out, size_t* out_len, char* err,
                              size_t cap) {
  const RunOptions opts = take_run_options();
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    AllPairIterator it = AllPairIterator::with_options(seqs, parse_scores(scores), exclude_self != 0, orientation == 2,
                                                      SparsificationStrategy::parse(sparsification ? sparsification : "none"));
    set_orientation(it, orientation);
    if (!devices || n_devices < 1) throw std::invalid_argument("awh_all_pairs_paf: empty device list");
    it.with_devices(std::vector<int>(devices, devices + n_devices));
    if (min_batch_pairs > 0) it.with_min_batch_pairs((size_t)min_batch_pairs);
    it.with_verify(verify != 0);
    opts.apply(it);
    std::string all;
    if (opts.device_cigar || opts.cs != 0) {  // the consumer that takes the device's text: whole formatted batches
      it.for_each_paf_batch([&](const std::string& chunk) { all += chunk; });
    } else {
      it.for_each_with_callback([&](AlignmentResult&& r) {  // the reference's own per-record path
        all += alignment_to_paf(r, seqs);
        all.push_back('\n');
      });
    }
    keep(it);
    if (slot_stats) for (int k = 0; k < n_devices; ++k) slot_stats[k] = it.last_slot_stats()[(size_t)k];
    *out = (char*)malloc(all.size() + 1);
    memcpy(*out, all.c_str(), all.size() + 1);
    *out_len = all.size();
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// Every consumer of the pair list the reference offers, one per `mode` (tests/test_host_api.py), on the engines
// `devices[0, n_devices)` names (AllPairIterator::with_devices; an ordinal may repeat):
//   0  AllPairIterator::for_each_with_callback                 iterator.rs:127-137
//   1  the sequential `impl Iterator` (next() until the end)    iterator.rs:151-171
//   2  into_par_iter().for_each_with_callback on `threads`      iterator.rs:113-125,206-253
//   3  into_par_iter().collect()                                iterator.rs:182-203 (rayon collect)
//   4  process_alignments_with_callback                         lib.rs:57-68 (mash orientation, exclude_self)
// `resparsify`: plan with -p none first, then call with_sparsification(strategy) (iterator.rs:101-110).  Batches of at
// least `min_batch_pairs` pairs (<= 0: the default), on shard `shard_rank` of `shard_world` (world <= 1: the whole list; not
// in mode 4).  out = PAF lines in the order the records arrived.  slot_stats (nullable, n_devices entries) receives
// last_slot_stats() -- zeros in mode 4 without min_batch_pairs, where process_alignments_with_callback owns the iterator.
// `fail_at` >= 0: the callback throws at its fail_at-th record; the call must fail with that message (first error wins),
// "callback failed at record <fail_at>", and callback calls after it say "failed again".  On failure n_records still
// receives the number of records that arrived and late_calls (nullable) how many callback calls followed the first failure.
int awh_iterate_devices(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores,
                        const char* sparsification, int orientation, int mode, int threads, int chunk, int resparsify, long fail_at,
                        const int32_t* devices, int n_devices, int64_t min_batch_pairs, int64_t shard_rank, int64_t shard_world,
                        int verify_on, awv_stats* slot_stats, char** out, size_t* out_len, size_t* n_records, size_t* late_calls,
                        char* err, size_t cap) {
  const RunOptions opts = take_run_options();
  if (!devices || n_devices < 1) { set_err(err, cap, "awh_iterate_devices: empty device list"); return -1; }
  size_t seen = 0, late = 0;
  bool thrown = false;
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    const SparsificationStrategy strat = SparsificationStrategy::parse(sparsification ? sparsification : "none");
    std::mutex mu;
    std::string all;
    auto record = [&](AlignmentResult&& r) {
      std::string line = alignment_to_paf(r, seqs);
      std::lock_guard<std::mutex> g(mu);
      if (fail_at >= 0 && (long)seen == fail_at) {
        // (a later failure is told from the first one, and the calls that follow the first are counted)
        if (thrown) throw std::runtime_error("callback failed again, call " + std::to_string(++late) + " after the first failure");
        thrown = true;
        throw std::runtime_error("callback failed at record " + std::to_string(seen));
      }
      ++seen;
      all += line;
      all.push_back('\n');
    };
    const std::vector<int> devs(devices, devices + n_devices);
    std::vector<awv_stats> st;
    const bool verify = verify_on != 0;
    if (mode == 4 && min_batch_pairs <= 0 && !verify && !opts.any()) {
      process_alignments_with_callback(seqs, parse_scores(scores), strat, record, devs);
    } else if (mode == 4) {  // what that overload does, with the batch size of the call and the check
      AllPairIterator it = AllPairIterator::with_options(seqs, parse_scores(scores), true, true, strat);
      it.with_devices(devs).with_verify(verify);
      opts.apply(it);
      if (min_batch_pairs > 0) it.with_min_batch_pairs((size_t)min_batch_pairs);
      it.for_each_with_callback(record);
      st = it.last_slot_stats();
      keep(it);
    } else {
      AllPairIterator it0 = AllPairIterator::with_options(seqs, parse_scores(scores), true, orientation == 2,
                                                         resparsify ? SparsificationStrategy{} : strat);
      set_orientation(it0, orientation);
      it0.with_devices(devs);
      if (shard_world > 1) it0.with_shard((size_t)shard_rank, (size_t)shard_world);
      if (min_batch_pairs > 0) it0.with_min_batch_pairs((size_t)min_batch_pairs);
      if (chunk > 0) it0.with_next_chunk((size_t)chunk);
      it0.with_verify(verify);
      opts.apply(it0);
      AllPairIterator it = resparsify ? it0.with_sparsification(strat).with_shard((size_t)shard_rank, (size_t)shard_world) : it0;
      if (mode == 0) { it.for_each_with_callback(record); st = it.last_slot_stats(); keep(it); }
      else if (mode == 1) { while (auto r = it.next()) record(std::move(*r)); st = it.last_slot_stats(); keep(it); }
      else if (mode == 2) { auto par = it.into_par_iter(); par.with_threads(threads).for_each_with_callback(record); st = par.last_slot_stats(); keep(par); }
      else if (mode == 3) { auto par = it.into_par_iter(); for (auto& r : par.collect()) record(std::move(r)); st = par.last_slot_stats(); keep(par); }
      else throw std::invalid_argument("awh_iterate_devices: unknown mode");
    }
    if (slot_stats)
      for (int k = 0; k < n_devices; ++k) slot_stats[k] = (size_t)k < st.size() ? st[(size_t)k] : awv_stats{};
    *out = (char*)malloc(all.size() + 1);
    memcpy(*out, all.c_str(), all.size() + 1);
    *out_len = all.size();
    *n_records = seen;
    return 0;
  } catch (const std::exception& e) {
    set_err(err, cap, e.what());
    *n_records = seen;
    if (late_calls) *late_calls = late;
    return -1;
  }
}
// AllPairIterator::scores over the pair list AllPairIterator::with_options(..., exclude_self = true, mash orientation when
// orientation == 2, sparsification) plans, oriented by `orientation` (0 forward, 1 WFA, 2 mash, 3 WFA by two full alignments per pair: with_full_wfa_orientation -- in every hook here), on the engines
// `devices[0, n_devices)` names, on shard `shard_rank` of `shard_world` (world <= 1: the whole list).  max_penalty < 0: no
// bound.  out = malloc'ed int64 records of five (query_idx, target_idx, is_reverse, penalty, status), one per planned pair in
// pair-list order; st (nullable) receives last_stats().
int awh_all_pairs_scores(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores,
                         const char* sparsification, int orientation, const int32_t* devices, int n_devices, int64_t shard_rank,
                         int64_t shard_world, int64_t max_penalty, int64_t** out, size_t* npairs, awv_stats* st, char* err, size_t cap) {
  try {
    if (!devices || n_devices < 1) throw std::invalid_argument("awh_all_pairs_scores: empty device list");
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    AllPairIterator it = AllPairIterator::with_options(seqs, parse_scores(scores), true, orientation == 2,
                                                      SparsificationStrategy::parse(sparsification ? sparsification : "none"));
    set_orientation(it, orientation);
    it.with_devices(std::vector<int>(devices, devices + n_devices));
    if (shard_world > 1) it.with_shard((size_t)shard_rank, (size_t)shard_world);
    if (max_penalty > INT32_MAX) max_penalty = -1;  // (no pair can score that much: no bound)
    const std::vector<PairScore> r = it.scores(max_penalty >= 0 ? std::optional<int>((int)max_penalty) : std::nullopt);
    *out = (int64_t*)malloc(sizeof(int64_t) * 5 * (r.size() + 1));
    if (!*out) throw std::bad_alloc();
    for (size_t i = 0; i < r.size(); ++i) {
      int64_t* o = *out + 5 * i;
      o[0] = (int64_t)r[i].query_idx; o[1] = (int64_t)r[i].target_idx; o[2] = r[i].is_reverse ? 1 : 0;
      o[3] = r[i].penalty; o[4] = r[i].status;
    }
    *npairs = r.size();
    if (st) *st = it.last_stats();
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// End-to-end measurement: sequences -> GPU alignment -> D2H -> PAF text into a counting sink, on the engines
// `devices[0, n_devices)` names (min_batch_pairs <= 0: the default), over the pair list `sparsification` plans (nullable:
// every pair, AllPairIterator::new); slot_stats (nullable, n_devices entries) receives last_slot_stats(), st (nullable)
// their sum, out_checksum (nullable) the sum of the lines' FNV-1a hashes (the same for the same lines in any order)
int awh_all_pairs_paf_count_devices(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores,
                                    int orientation, const char* sparsification, const int32_t* devices, int n_devices,
                                    int64_t min_batch_pairs, int format_threads, int verify, uint64_t* out_bytes, uint64_t* out_lines,
                                    uint64_t* out_checksum, double* secs, awv_stats* st, awv_stats* slot_stats, char* err, size_t cap) {
  const RunOptions opts = take_run_options();
  if (!devices || n_devices < 1) { set_err(err, cap, "awh_all_pairs_paf_count_devices: empty device list"); return -1; }
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    AllPairIterator it = sparsification ? AllPairIterator::with_options(seqs, parse_scores(scores), true, false,
                                                                       SparsificationStrategy::parse(sparsification))
                                        : AllPairIterator(seqs, parse_scores(scores));
    set_orientation(it, orientation);
    it.with_devices(std::vector<int>(devices, devices + n_devices));
    if (min_batch_pairs > 0) it.with_min_batch_pairs((size_t)min_batch_pairs);
    it.with_threads(format_threads);  // this call's sketching / orientation threads: carried by the iterator, not a process-wide setting
    it.with_verify(verify != 0);
    opts.apply(it);
    uint64_t nb = 0, nl = 0, sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    it.for_each_paf_batch([&](const std::string& s) {
      nb += s.size();
      for (char c : s) nl += c == '\n';
      if (out_checksum) {  // order-independent: the sum of every line's FNV-1a 64-bit hash
        uint64_t h = 14695981039346656037ull;
        for (char c : s) {
          if (c == '\n') { sum += h; h = 14695981039346656037ull; }
          else { h ^= (uint8_t)c; h *= 1099511628211ull; }
        }
      }
    }, format_threads);
    *secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out_bytes = nb;
    *out_lines = nl;
    if (out_checksum) *out_checksum = sum;
    keep(it);
    if (st) *st = it.last_stats();
    if (slot_stats) for (int k = 0; k < n_devices; ++k) slot_stats[k] = it.last_slot_stats()[(size_t)k];
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}
int awh_align_sequences(const uint8_t* pattern, size_t plen, const uint8_t* text, size_t tlen, const int32_t pen[5], int mode,
                        int device, int32_t* score, char* cigar, size_t ccap, uint64_t counts[5], char* err, size_t cap) {
  try {
    const wfa::Penalties p{pen[0], pen[1], pen[2], pen[3], pen[4]};
    const wfa::AlignmentResult r = wfa::align_sequences(std::vector<uint8_t>(pattern, pattern + plen),
                                                        std::vector<uint8_t>(text, text + tlen), p, (AlignmentMode)mode, device);
    *score = r.score;
    if (r.cigar.size() + 1 > ccap) { set_err(err, cap, "cigar buffer too small"); return -2; }
    memcpy(cigar, r.cigar.c_str(), r.cigar.size() + 1);
    counts[0] = r.matches; counts[1] = r.mismatches; counts[2] = r.insertions; counts[3] = r.deletions; counts[4] = r.alignment_length;
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

int awh_validate_cigar(const uint8_t* cigar, size_t n, size_t qlen, size_t rlen, char* err, size_t cap) {
  const std::string m = wfa::validate_cigar_alignment(cigar, n, qlen, rlen);
  if (m.empty()) return 0;
  set_err(err, cap, m);
  return -1;
}

// ---- planner hooks (no GPU needed) ----
uint64_t awh_siphash(const uint8_t* p, size_t n, uint64_t k0, uint64_t k1, int c, int d) { return planner::siphash(p, n, k0, k1, c, d); }
uint64_t awh_hash_bytes(const uint8_t* p, size_t n) { return planner::default_hash_bytes(p, n); }
uint64_t awh_hash_str(const char* s) { return planner::default_hash_str(s); }
double awh_connectivity_probability(size_t n, double x) { return planner::compute_connectivity_probability(n, x); }

// pair list of AllPairIterator::with_options(..., strategy) without aligning: out = malloc'ed (i, j) int64 pairs
int awh_plan_pairs(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* sparsification,
                   int exclude_self, int64_t** out, size_t* npairs, char* err, size_t cap) {
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    // exclude_self & 2: plan with -p none first, then with_sparsification(strategy) (iterator.rs:101-110)
    const bool resparsify = (exclude_self & 2) != 0;
    AllPairIterator it0 = AllPairIterator::with_options(seqs, AlignmentParams{}, (exclude_self & 1) != 0, false,
                                                       resparsify ? SparsificationStrategy{} : SparsificationStrategy::parse(sparsification));
    AllPairIterator it = resparsify ? it0.with_sparsification(SparsificationStrategy::parse(sparsification)) : it0;
    const auto& p = it.get_pairs();
    *out = (int64_t*)malloc(sizeof(int64_t) * 2 * (p.size() + 1));
    for (size_t i = 0; i < p.size(); ++i) { (*out)[2 * i] = (int64_t)p[i].first; (*out)[2 * i + 1] = (int64_t)p[i].second; }
    *npairs = p.size();
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

int awh_knn_graph(const double* dist, int n, int k, int farthest, int64_t** out, size_t* npairs) {
  std::vector<std::vector<double>> d((size_t)n, std::vector<double>((size_t)n));
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) d[i][j] = dist[i * n + j];
  const auto p = planner::build_knn_graph(d, (size_t)k, farthest != 0);
  *out = (int64_t*)malloc(sizeof(int64_t) * 2 * (p.size() + 1));
  for (size_t i = 0; i < p.size(); ++i) { (*out)[2 * i] = (int64_t)p[i].first; (*out)[2 * i + 1] = (int64_t)p[i].second; }
  *npairs = p.size();
  return 0;
}

int awh_mash_matrix(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, int k, double* out) {
  const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
  const auto m = planner::compute_distance_matrix(seqs, (size_t)k, 1000);
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) out[i * n + j] = m[i][j];
  return 0;
}

int awh_orient_mash(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const int64_t* pairs,
                    size_t npairs, uint8_t* is_rev) {
  const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
  std::vector<std::pair<size_t, size_t>> p(npairs);
  for (size_t i = 0; i < npairs; ++i) p[i] = {(size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]};
  const auto r = planner::orient_pairs_mash(seqs, p.data(), p.size(), 8);
  memcpy(is_rev, r.data(), npairs);
  return 0;
}

// ---- device planning (planner.hpp's device variants; they fail without a GPU: -1 and the message in err) ----
// awh_mash_matrix on `device`
int awh_mash_matrix_gpu(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, int k, int device, double* out,
                        char* err, size_t cap) {
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    const auto m = planner::compute_distance_matrix(seqs, (size_t)k, 1000, device);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) out[i * n + j] = m[i][j];
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// awh_plan_pairs with the list planned on `device` (AllPairIterator::with_options(..., plan_device))
int awh_plan_pairs_gpu(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* sparsification,
                       int exclude_self, int device, int64_t** out, size_t* npairs, char* err, size_t cap) {
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    const bool resparsify = (exclude_self & 2) != 0;
    AllPairIterator it0 = AllPairIterator::with_options(seqs, AlignmentParams{}, (exclude_self & 1) != 0, false,
                                                       resparsify ? SparsificationStrategy{} : SparsificationStrategy::parse(sparsification),
                                                       device);
    AllPairIterator it = resparsify ? it0.with_sparsification(SparsificationStrategy::parse(sparsification)) : it0;
    const auto& p = it.get_pairs();
    *out = (int64_t*)malloc(sizeof(int64_t) * 2 * (p.size() + 1));
    for (size_t i = 0; i < p.size(); ++i) { (*out)[2 * i] = (int64_t)p[i].first; (*out)[2 * i + 1] = (int64_t)p[i].second; }
    *npairs = p.size();
    return 0;
  } catch (const std::invalid_argument& e) { set_err(err, cap, e.what()); return -1;  // (a bad -p string)
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -2; }     // (the device)
}

// awh_orient_mash on `device`
int awh_orient_mash_gpu(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const int64_t* pairs, size_t npairs,
                        int device, uint8_t* is_rev, char* err, size_t cap) {
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    std::vector<std::pair<size_t, size_t>> p(npairs);
    for (size_t i = 0; i < npairs; ++i) p[i] = {(size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]};
    const auto r = planner::orient_pairs_mash(seqs, p.data(), p.size(), 8, device);
    if (npairs) memcpy(is_rev, r.data(), npairs);
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// sketches of every sequence (planner::sketch_all; kind 0 canonical, 1 forward, 2 reverse complement; device < 0: the host
// code): offsets_out = malloc'ed n + 1 offsets, hashes_out = malloc'ed hashes
int awh_sketch(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, int k, int s, int kind, int device,
               uint64_t** offsets_out, uint64_t** hashes_out, char* err, size_t cap) {
  try {
    if (kind < 0 || kind > 2) throw std::invalid_argument("sketch: kind must be 0, 1 or 2");
    if (k < 0 || s < 0) throw std::invalid_argument("sketch: k and s must be >= 0");
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    const auto sk = planner::sketch_all(seqs, (planner::SketchKind)kind, (size_t)k, (size_t)s, device);
    *offsets_out = (uint64_t*)malloc(sizeof(uint64_t) * ((size_t)n + 1));
    (*offsets_out)[0] = 0;
    for (int i = 0; i < n; ++i) (*offsets_out)[i + 1] = (*offsets_out)[i] + sk[i].size();
    *hashes_out = (uint64_t*)malloc(sizeof(uint64_t) * ((*offsets_out)[n] + 1));
    for (int i = 0; i < n; ++i)
      if (!sk[i].empty()) memcpy(*hashes_out + (*offsets_out)[i], sk[i].data(), sk[i].size() * sizeof(uint64_t));
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// planner::keep_threshold: keep iff keep_all or h < the returned threshold
uint64_t awh_keep_threshold(double fraction, int* keep_all) {
  bool all = false;
  const uint64_t t = planner::keep_threshold(fraction, &all);
  *keep_all = all ? 1 : 0;
  return t;
}

// shard of every pair under the cost-balanced (LPT) partition AllPairIterator::with_shard uses; cost_out (nullable)
// receives the predicted costs
int awh_shard_pairs(const int64_t* pairs, size_t npairs, const int64_t* lens, size_t nseq, const char* scores, size_t world, uint32_t* shard_out,
                    double* cost_out, char* err, size_t cap) {
  try {
    const AlignmentParams p = parse_scores(scores);
    if (world == 0) throw std::invalid_argument("shard_pairs: world must be at least 1");
    std::vector<double> cost(npairs);
    for (size_t i = 0; i < npairs; ++i) {
      const int64_t a = pairs[2 * i], b = pairs[2 * i + 1];
      if (a < 0 || b < 0 || (uint64_t)a >= nseq || (uint64_t)b >= nseq)
        throw std::invalid_argument("shard_pairs: pair " + std::to_string(i) + " names a sequence outside [0, " + std::to_string(nseq) + ")");
      cost[i] = planner::predicted_pair_cost((size_t)lens[a], (size_t)lens[b], p);
    }
    const std::vector<uint32_t> sh = planner::assign_shards_lpt(cost, world);
    for (size_t i = 0; i < npairs; ++i) shard_out[i] = sh[i];
    if (cost_out) for (size_t i = 0; i < npairs; ++i) cost_out[i] = cost[i];
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// batch of every pair under planner::device_batches(cost, slots, min_batch_pairs) (the batches of a multi-device run);
// n_batches receives their number
int awh_device_batches(const double* cost, size_t n, size_t slots, size_t min_batch_pairs, uint32_t* batch_out, size_t* n_batches,
                       char* err, size_t cap) {
  try {
    const auto b = planner::device_batches(std::vector<double>(cost, cost + n), slots, min_batch_pairs);
    for (size_t k = 0; k < b.size(); ++k)
      for (size_t i : b[k]) batch_out[i] = (uint32_t)k;
    *n_batches = b.size();
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// engine configuration of the engines the host library creates from now on; release = destroy the cached ones first
void awh_set_engine_config(int flags, int first_row_cols, int release) {
  if (release) release_engines();
  set_engine_flags(flags);
  set_engine_first_row_cols(first_row_cols);
}

// ---- on-device verification ----
// The path a failed check takes above the engine, without an engine: verify results (code, column, penalty per entry) of
// `calls` engine calls -- call c covers entries [cuts[c], cuts[c + 1]) of the arrays, each entry naming its place idx[i] in
// the run's range of `npairs` pairs (q, t) that starts at pair-list index `first` -- go through append_verify_failures one
// call at a time, in the order given (as slots finish in any order), then sort_verify_failures; the result is left for
// awh_last_verify, and report (cap bytes) receives report_verify_failures' lines.  Returns its exit status.
int awh_verify_failure_path(int n, const char* const* ids, const int64_t* pairs, size_t npairs, size_t first, const int64_t* idx,
                            const uint8_t* rev, const int32_t* code, const int64_t* column, const int64_t* penalty,
                            const size_t* cuts, size_t calls, char* report, size_t cap) {
  std::vector<Sequence> seqs((size_t)n);
  for (int i = 0; i < n; ++i) seqs[(size_t)i].id = ids[i];
  std::vector<std::pair<size_t, size_t>> plist(npairs);
  for (size_t i = 0; i < npairs; ++i) plist[i] = {(size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]};
  std::vector<VerifyFailure> all;
  awv_verify_stats st{};
  for (size_t c = 0; c < calls; ++c) {
    const size_t lo = cuts[c], hi = cuts[c + 1];
    std::vector<awv_verify_result> vr(hi - lo);
    std::vector<size_t> ix(hi - lo);
    for (size_t i = lo; i < hi; ++i) {
      vr[i - lo] = awv_verify_result{code[i], 0, column[i], penalty[i]};
      ix[i - lo] = (size_t)idx[i];
      st.failed += code[i] != AWV_VF_OK && code[i] != AWV_VF_SKIPPED;
    }
    st.pairs += hi - lo;
    append_verify_failures(all, vr.data(), (int64_t)(hi - lo), first, ix.data(), plist.data(), rev + lo);
  }
  sort_verify_failures(all);
  g_report.verify_stats = st;
  g_report.verify_failures = all;
  std::string text;
  const int status = report_verify_failures(all, seqs, text);
  snprintf(report, cap, "%s", text.c_str());
  return status;
}

// what the calling thread's last alignment hook left: last_verify_stats() and verify_failures() as malloc'ed int64 records of seven (pair-list
// index, query_idx, target_idx, is_reverse, code, column, penalty)
int awh_last_verify(awv_verify_stats* st, int64_t** out, size_t* n) {
  *st = g_report.verify_stats;
  *out = (int64_t*)malloc(sizeof(int64_t) * 7 * (g_report.verify_failures.size() + 1));
  if (!*out) return -1;
  for (size_t i = 0; i < g_report.verify_failures.size(); ++i) {
    const VerifyFailure& f = g_report.verify_failures[i];
    int64_t* o = *out + 7 * i;
    o[0] = (int64_t)f.index; o[1] = (int64_t)f.query_idx; o[2] = (int64_t)f.target_idx; o[3] = f.is_reverse ? 1 : 0;
    o[4] = f.code; o[5] = f.column; o[6] = f.penalty;
  }
  *n = g_report.verify_failures.size();
  return 0;
}

// cigar_string_to_bytes: the op bytes of a cg string into out[0, cap); returns their number, -1 for a malformed string, -2
// when cap is too small
long awh_cigar_string_to_bytes(const char* cg, uint8_t* out, size_t cap) {
  std::vector<uint8_t> ops;
  if (!cigar_string_to_bytes(cg, ops)) return -1;
  if (ops.size() > cap) return -2;
  if (!ops.empty()) memcpy(out, ops.data(), ops.size());
  return (long)ops.size();
}

// check_paf on `device`: out = format_paf_check's lines (malloc'ed), counts = {lines, checked, skipped, failures}
int awh_check_paf(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores, const char* paf,
                  size_t paf_len, int optimal, int partial, int device, char** out, size_t* out_len, uint64_t counts[4], awv_verify_stats* st,
                  char* err, size_t cap) {
  try {
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    const PafCheckReport r = check_paf(seqs, std::string(paf, paf_len), parse_scores(scores), optimal != 0, device, partial != 0);
    const std::string txt = format_paf_check(r);
    *out = (char*)malloc(txt.size() + 1);
    if (!*out) throw std::bad_alloc();
    memcpy(*out, txt.c_str(), txt.size() + 1);
    *out_len = txt.size();
    counts[0] = r.lines; counts[1] = r.checked; counts[2] = r.skipped; counts[3] = r.failures.size();
    if (st) *st = r.stats;
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// ---- ranges ----
// allwave::align_ranges + alignment_to_paf per record: ranges = nr records of seven int64 (query_idx, target_idx, is_reverse,
// query_start, query_end, target_start, target_end), on the engines `devices[0, n_devices)` names; out = the PAF lines in
// list order (malloc'ed).  The verify counters and failures are left for awh_last_verify.
int awh_align_ranges_paf(int n, const char* const* ids, const uint8_t* bytes, const uint64_t* offs, const char* scores, const int64_t* ranges,
                         size_t nr, const int32_t* devices, int n_devices, int verify, char** out, size_t* out_len, char* err, size_t cap) {
  const RunOptions opts = take_run_options();
  try {
    if (!devices || n_devices < 1) throw std::invalid_argument("awh_align_ranges_paf: empty device list");
    const std::vector<Sequence> seqs = make_seqs(n, ids, bytes, offs);
    std::vector<AlignmentRange> rg(nr);
    for (size_t i = 0; i < nr; ++i) {
      const int64_t* r = ranges + 7 * i;
      for (int k = 0; k < 7; ++k)
        if (r[k] < 0) throw std::invalid_argument("awh_align_ranges_paf: negative field in range " + std::to_string(i));
      rg[i] = AlignmentRange{(size_t)r[0], (size_t)r[1], r[2] != 0, (size_t)r[3], (size_t)r[4], (size_t)r[5], (size_t)r[6]};
    }
    AllPairIterator it = AllPairIterator::for_ranges(seqs, rg, parse_scores(scores));
    it.with_devices(std::vector<int>(devices, devices + n_devices)).with_verify(verify != 0);
    opts.apply(it);
    std::string all;
    if (opts.device_cigar || opts.cs != 0) {  // the consumer that takes the device's text (in list order on one slot, in batch order on several)
      it.for_each_paf_batch([&](const std::string& chunk) { all += chunk; });
      keep(it);
    } else {
      AllPairParallelIterator par = it.into_par_iter();
      const std::vector<AlignmentResult> res = par.collect();  // (in list order, on any number of slots)
      keep(par);
      for (const AlignmentResult& r : res) {
        all += alignment_to_paf(r, seqs);
        all.push_back('\n');
      }
    }
    *out = (char*)malloc(all.size() + 1);
    if (!*out) throw std::bad_alloc();
    memcpy(*out, all.c_str(), all.size() + 1);
    *out_len = all.size();
    return 0;
  } catch (const std::exception& e) { set_err(err, cap, e.what()); return -1; }
}

// The PAF line of one range's engine record (range_alignment_result + alignment_to_paf; needs no device): range = the seven
// fields of awh_align_ranges_paf, rec = one awv_result whose cigar_off / cigar_len point into `arena`
int awh_range_record_paf(const char* qid, size_t qlen, const char* tid, size_t tlen, const int64_t range[7], const awv_result* rec,
                         const uint8_t* arena, char* out, size_t cap) {
  std::vector<Sequence> seqs(2);
  seqs[0].id = qid; seqs[0].seq.assign(qlen, 'A');
  seqs[1].id = tid; seqs[1].seq.assign(tlen, 'A');
  const AlignmentRange g{(size_t)range[0], (size_t)range[1], range[2] != 0, (size_t)range[3], (size_t)range[4], (size_t)range[5], (size_t)range[6]};
  const std::string s = alignment_to_paf(range_alignment_result(g, *rec, arena, true), seqs);
  if (s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// parse_paf_ranges: out = malloc'ed int64 records of nine per non-empty line (line, class index into "", bad_line, unknown_name,
// length_mismatch; then the range's seven fields, zeros for a bad line)
int awh_parse_paf_ranges(int n, const char* const* ids, const int64_t* lens, const char* paf, size_t paf_len, int64_t** out, size_t* nlines) {
  std::vector<Sequence> seqs((size_t)n);
  for (int i = 0; i < n; ++i) {
    seqs[(size_t)i].id = ids[i];
    seqs[(size_t)i].seq.assign((size_t)lens[i], 'A');
  }
  const PafRanges pr = parse_paf_ranges(seqs, std::string(paf, paf_len));
  static const char* const classes[] = {"", "bad_line", "unknown_name", "length_mismatch"};
  *out = (int64_t*)malloc(sizeof(int64_t) * 9 * (pr.lines.size() + 1));
  if (!*out) return -1;
  for (size_t i = 0; i < pr.lines.size(); ++i) {
    int64_t* o = *out + 9 * i;
    memset(o, 0, 9 * sizeof(int64_t));
    o[0] = (int64_t)pr.lines[i].line;
    for (int c = 0; c < 4; ++c)
      if (pr.lines[i].cls == classes[c]) o[1] = c;
    if (pr.lines[i].cls.empty()) {
      const AlignmentRange& g = pr.ranges[pr.lines[i].index];
      o[2] = (int64_t)g.query_idx; o[3] = (int64_t)g.target_idx; o[4] = g.is_reverse ? 1 : 0;
      o[5] = (int64_t)g.query_start; o[6] = (int64_t)g.query_end; o[7] = (int64_t)g.target_start; o[8] = (int64_t)g.target_end;
    }
  }
  *nlines = pr.lines.size();
  return 0;
}

// ---- bounds on the final alignments ----
// The calling thread's NEXT alignment hook (awh_all_pairs_paf_devices, awh_iterate_devices, awh_all_pairs_paf_count_devices,
// awh_align_ranges_paf) runs under AllPairIterator::with_max_penalty(max_penalty) (< 0: none) and
// with_max_divergence(max_divergence) (< 0: none); the hooks after it run unbounded again.
void awh_set_bounds(int64_t max_penalty, double max_divergence) {
  g_next.max_penalty = max_penalty >= 0 ? std::optional<int>((int)std::min<int64_t>(max_penalty, INT32_MAX)) : std::nullopt;
  g_next.max_divergence = max_divergence >= 0.0 ? std::optional<double>(max_divergence) : std::nullopt;
}
// ---- clipping to the best-scoring segment ----
// The calling thread's NEXT alignment hook runs with_clip(match_bonus, min_score) (match_bonus 0: off); the hooks after it
// run unclipped again.
void awh_set_clip(int match_bonus, int64_t min_score) {
  g_next.clip_match_bonus = match_bonus;
  g_next.clip_min_score = min_score;
}
// ---- splitting into all good segments ----
// The calling thread's NEXT alignment hook runs with_split(match_bonus, min_score) (match_bonus 0: off); the hooks after it
// run unsplit again.
void awh_set_split(int match_bonus, int64_t min_score) {
  g_next.split_match_bonus = match_bonus;
  g_next.split_min_score = min_score;
}
// ---- gap runs at their normal place ----
// The calling thread's NEXT alignment hook runs with_normalize(direction) (AWV_NORM_LEFT / AWV_NORM_RIGHT; AWV_NORM_OFF: off); the
// hooks after it run without again.
void awh_set_normalize(int direction) { g_next.normalize = direction; }
// The calling thread's NEXT alignment hook runs with_device_cigar(on).  The hooks that format PAF (awh_all_pairs_paf_devices,
// awh_all_pairs_paf_count_devices, awh_align_ranges_paf) then go through for_each_paf_batch; awh_iterate_devices' consumers hand
// out op bytes and ignore it.
void awh_set_device_cigar(int on) { g_next.device_cigar = on != 0; }
// The calling thread's NEXT alignment hook runs with_cs(mode) (AWV_CS_SHORT / AWV_CS_LONG; 0: off).  The hooks that format PAF then
// go through for_each_paf_batch, as under awh_set_device_cigar; awh_iterate_devices' consumers ignore it.
void awh_set_cs(int mode) { g_next.cs = mode; }
// last_cs_stats() of the calling thread's last alignment hook: {pairs, failed, text_bytes, columns} and the summed kernel time
void awh_last_cs(uint64_t out[4], double* kernel_ms) {
  out[0] = g_report.cs_stats.pairs;
  out[1] = g_report.cs_stats.failed;
  out[2] = g_report.cs_stats.text_bytes;
  out[3] = g_report.cs_stats.columns;
  *kernel_ms = g_report.cs_stats.kernel_ms;
}
// ---- per-base depth ----
// The calling thread's NEXT alignment hook runs with_coverage(roles) (AWV_COV_*; 0: off); the hooks after it run without again.
void awh_set_coverage(int roles) { g_next.coverage = roles; }
// last_coverage() of the calling thread's last alignment hook.  *n_offsets is the number of sequences + 1, or 0 for a call without
// coverage; the three arrays are malloc'd copies (awh_free each), offsets[*n_offsets - 1] entries per track.  stats:
// {items, failed, columns, boundaries, reads} and the summed kernel time.  Returns -1 when memory runs out.
int awh_last_coverage(uint64_t** offsets, size_t* n_offsets, uint32_t** aligned, uint32_t** matched, uint64_t stats[5], double* kernel_ms) {
  const awv_cov_stats& cs = g_report.coverage_stats;
  stats[0] = cs.items; stats[1] = cs.failed; stats[2] = cs.columns; stats[3] = cs.boundaries; stats[4] = cs.reads;
  *kernel_ms = cs.kernel_ms;
  *n_offsets = g_coverage.offsets.size();
  const size_t nb = g_coverage.aligned.size();
  *offsets = (uint64_t*)malloc(std::max<size_t>(*n_offsets, 1) * sizeof(uint64_t));
  *aligned = (uint32_t*)malloc(std::max<size_t>(nb, 1) * sizeof(uint32_t));
  *matched = (uint32_t*)malloc(std::max<size_t>(nb, 1) * sizeof(uint32_t));
  if (!*offsets || !*aligned || !*matched) {
    free(*offsets); free(*aligned); free(*matched);
    *offsets = nullptr; *aligned = *matched = nullptr; *n_offsets = 0;
    return -1;
  }
  if (*n_offsets) memcpy(*offsets, g_coverage.offsets.data(), *n_offsets * sizeof(uint64_t));
  if (nb) memcpy(*aligned, g_coverage.aligned.data(), nb * sizeof(uint32_t));
  if (nb) memcpy(*matched, g_coverage.matched.data(), nb * sizeof(uint32_t));
  return 0;
}
// ---- the per-site allele table ----
// The calling thread's NEXT alignment hook runs with_variants(on != 0); the hooks after it run without again.
void awh_set_variants(int on) { g_next.variants = on != 0; }
// last_variants() of the calling thread's last alignment hook: *rows is a malloc'd copy of the *n_rows rows (awh_free), stats the
// run's awv_variants_stats summed over the slots.  Returns -1 when memory runs out.
int awh_last_variants(awv_variant** rows, size_t* n_rows, awv_variants_stats* stats) {
  *stats = g_report.variants_stats;
  *n_rows = g_variants.size();
  *rows = (awv_variant*)malloc(std::max<size_t>(*n_rows, 1) * sizeof(awv_variant));
  if (!*rows) {
    *n_rows = 0;
    return -1;
  }
  if (*n_rows) memcpy(*rows, g_variants.data(), *n_rows * sizeof(awv_variant));
  return 0;
}
// ---- regions lifted through the alignments ----
// The calling thread's NEXT alignment hook runs with_liftover(regions[0 .. n), from) (AWV_LIFT_FROM_*; 0: off); the hooks after it
// run without again.
void awh_set_liftover(const awv_region* regions, size_t n, int from) {
  g_next.liftover.assign(regions, regions + (regions ? n : 0));
  g_next.liftover_from = from;
}
// last_liftover() of the calling thread's last alignment hook: *rows is a malloc'd copy of the *n_rows rows (awh_free), stats the
// run's awv_lift_stats summed over the slots.  Returns -1 when memory runs out.
int awh_last_liftover(awv_lift_row** rows, size_t* n_rows, awv_lift_stats* stats) {
  *stats = g_report.lift_stats;
  *n_rows = g_liftover.size();
  *rows = (awv_lift_row*)malloc(std::max<size_t>(*n_rows, 1) * sizeof(awv_lift_row));
  if (!*rows) {
    *n_rows = 0;
    return -1;
  }
  if (*n_rows) memcpy(*rows, g_liftover.data(), *n_rows * sizeof(awv_lift_row));
  return 0;
}
// ---- target-anchored multiple alignments ----
// The calling thread's NEXT alignment hook runs with_msa(targets[0 .. n), max_bytes) (n == 0: every sequence; max_bytes == 0: the
// default bound) when on != 0; the hooks after it run without again.
void awh_set_msa(int on, const int* targets, size_t n, uint64_t max_bytes) {
  g_next.msa = on != 0;
  g_next.msa_targets.assign(targets, targets + (targets && on ? n : 0));
  g_next.msa_max_bytes = max_bytes ? max_bytes : (uint64_t)1 << 30;
}
// last_msa() of the calling thread's last alignment hook: the number of blocks and the call's awv_msa_stats
size_t awh_last_msa(awv_msa_stats* stats) {
  *stats = g_report.msa_stats;
  return g_msa.size();
}
// Block j of it: *names is a malloc'd copy of the rows' names, one per line, *bytes one of the rows * width bytes (awh_free both).
// Returns -1 when j is out of range or memory runs out.
int awh_last_msa_block(size_t j, int* t_idx, int64_t* rows, int64_t* width, char** names, size_t* names_len, uint8_t** bytes) {
  if (j >= g_msa.size()) return -1;
  const MsaBlock& b = g_msa[j];
  std::string all;
  for (const std::string& nm : b.names) all += nm + "\n";
  *t_idx = b.t_idx;
  *rows = b.rows;
  *width = b.width;
  *names_len = all.size();
  *names = (char*)malloc(std::max<size_t>(all.size(), 1));
  *bytes = (uint8_t*)malloc(std::max<size_t>(b.bytes.size(), 1));
  if (!*names || !*bytes) {
    free(*names);
    free(*bytes);
    *names = nullptr;
    *bytes = nullptr;
    return -1;
  }
  memcpy(*names, all.data(), all.size());
  if (!b.bytes.empty()) memcpy(*bytes, b.bytes.data(), b.bytes.size());
  return 0;
}
// last_encode_stats() of the calling thread's last alignment hook: {pairs, runs, text_bytes, columns} and the summed kernel time
void awh_last_encode(uint64_t out[4], double* kernel_ms) {
  out[0] = g_report.encode_stats.pairs;
  out[1] = g_report.encode_stats.runs;
  out[2] = g_report.encode_stats.text_bytes;
  out[3] = g_report.encode_stats.columns;
  *kernel_ms = g_report.encode_stats.kernel_ms;
}
// last_normalize_stats() of the calling thread's last alignment hook: {pairs, records_moved, runs, runs_moved, columns_moved,
// columns} and the kernel time
void awh_last_normalize(uint64_t out[6], double* kernel_ms) {
  out[0] = g_report.normalize_stats.pairs;
  out[1] = g_report.normalize_stats.records_moved;
  out[2] = g_report.normalize_stats.runs;
  out[3] = g_report.normalize_stats.runs_moved;
  out[4] = g_report.normalize_stats.columns_moved;
  out[5] = g_report.normalize_stats.columns;
  *kernel_ms = g_report.normalize_stats.kernel_ms;
}
// last_split_stats() of the calling thread's last alignment hook: {pairs, segments, empty} and the kernel time
void awh_last_split(uint64_t out[3], double* kernel_ms) {
  out[0] = g_report.split_stats.pairs;
  out[1] = g_report.split_stats.segments;
  out[2] = g_report.split_stats.empty;
  *kernel_ms = g_report.split_stats.kernel_ms;
}
// last_clip_stats() of the calling thread's last alignment hook: {pairs, empty, below_min_score} and the kernel time
void awh_last_clip(uint64_t out[3], double* kernel_ms) {
  out[0] = g_report.clip_stats.pairs;
  out[1] = g_report.clip_stats.empty;
  out[2] = g_report.clip_stats.below_min_score;
  *kernel_ms = g_report.clip_stats.kernel_ms;
}

// last_bound_stats() of the calling thread's last alignment hook: {pairs, above_penalty, above_divergence}
void awh_last_bounds(uint64_t out[3]) {
  out[0] = g_report.bound_stats.pairs;
  out[1] = g_report.bound_stats.above_penalty;
  out[2] = g_report.bound_stats.above_divergence;
}

void awh_free(void* p) { free(p); }

}  // extern "C"
