// allwave.cpp -- host-side mirror of allwave's API over the C ABI (see allwave.hpp).
#include "allwave.hpp"
#include "planner.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <tuple>
#include <chrono>
#include <condition_variable>
#include <dlfcn.h>
#include <link.h>
#include <thread>

namespace allwave {

// ---- types.rs -------------------------------------------------------------------------------
AlignmentParams AlignmentParams::edit_distance() {  // types.rs:62-73
  AlignmentParams p;
  p.match_score = 0;
  p.mismatch_penalty = 1;
  p.gap_open = 1;
  p.gap_extend = 1;
  p.gap2_open.reset();
  p.gap2_extend.reset();
  p.max_divergence.reset();
  return p;
}

bool AlignmentParams::operator==(const AlignmentParams& o) const {
  return match_score == o.match_score && mismatch_penalty == o.mismatch_penalty && gap_open == o.gap_open &&
         gap_extend == o.gap_extend && gap2_open == o.gap2_open && gap2_extend == o.gap2_extend &&
         max_divergence == o.max_divergence;
}

AlignmentMode alignment_mode_from_params(const AlignmentParams& p) {  // types.rs:107-116
  if (p.gap2_open.has_value() && p.gap2_extend.has_value()) return AlignmentMode::TwoPieceAffine;
  if (p.gap_open == p.gap_extend && p.gap_open == p.mismatch_penalty) return AlignmentMode::EditDistance;
  return AlignmentMode::SinglePieceAffine;
}

awv_penalties to_penalties(const AlignmentParams& p) {  // alignment.rs:263-289
  awv_penalties q{};
  q.match = p.match_score;
  q.mismatch = p.mismatch_penalty;
  switch (alignment_mode_from_params(p)) {
    case AlignmentMode::EditDistance:  // "edit" is gap-affine (x, x, x)
      q.gap_open1 = p.mismatch_penalty;
      q.gap_ext1 = p.mismatch_penalty;
      break;
    case AlignmentMode::SinglePieceAffine:
      q.gap_open1 = p.gap_open;
      q.gap_ext1 = p.gap_extend;
      break;
    case AlignmentMode::TwoPieceAffine:
      q.gap_open1 = p.gap_open;
      q.gap_ext1 = p.gap_extend;
      q.gap_open2 = p.gap2_open.value_or(p.gap_open);
      q.gap_ext2 = p.gap2_extend.value_or(p.gap_extend);
      q.two_piece = 1;
      break;
  }
  return q;
}

// ---- lib.rs ---------------------------------------------------------------------------------
AlignmentParams parse_scores(const std::string& scores_str) {  // lib.rs:116-153
  std::vector<int32_t> scores;
  size_t pos = 0;
  while (true) {
    size_t comma = scores_str.find(',', pos);
    std::string tok = scores_str.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
    size_t b = tok.find_first_not_of(" \t\n\r"), e = tok.find_last_not_of(" \t\n\r");
    tok = b == std::string::npos ? "" : tok.substr(b, e - b + 1);
    size_t used = 0;
    long v = 0;
    bool ok = !tok.empty();
    if (ok) {
      try { v = std::stol(tok, &used, 10); } catch (...) { ok = false; }
      ok = ok && used == tok.size() && v >= INT32_MIN && v <= INT32_MAX;
    }
    if (!ok) throw std::invalid_argument("Failed to parse scores: invalid digit found in string");
    scores.push_back((int32_t)v);
    if (comma == std::string::npos) break;
    pos = comma + 1;
  }
  AlignmentParams p;
  p.max_divergence.reset();
  if (scores.size() == 4 || scores.size() == 6) {
    p.match_score = scores[0];
    p.mismatch_penalty = scores[1];
    p.gap_open = scores[2];
    p.gap_extend = scores[3];
    if (scores.size() == 6) { p.gap2_open = scores[4]; p.gap2_extend = scores[5]; }
    else { p.gap2_open.reset(); p.gap2_extend.reset(); }
    return p;
  }
  throw std::invalid_argument("Invalid number of scores: " + std::to_string(scores.size()) + ". Expected 4 or 6 values.");
}

static inline void append_uint(std::string& out, size_t v) {
  char buf[24];
  int n = 0;
  do { buf[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) out.push_back(buf[--n]);
}

static void append_cigar(std::string& out, const uint8_t* ops, size_t n) {  // alignment.rs:347-376
  // Run-length encoding straight into the string's storage (a run costs at most two characters per op byte), runs
  // found eight op bytes at a time: formatting 65,280 CIGARs of 10 kbp alignments was 0.27 s of the 2.1 s end-to-end
  // call when it went byte by byte through push_back.
  const size_t base = out.size();
  out.resize(base + 2 * n + 24);
  char* const w0 = &out[0] + base;
  char* w = w0;
  size_t i = 0;
  while (i < n) {
    const uint8_t op = ops[i];
    const uint64_t pat = 0x0101010101010101ull * op;
    size_t j = i + 1;
    bool ended = false;
    while (j + 8 <= n) {
      uint64_t x;
      memcpy(&x, ops + j, 8);
      x ^= pat;
      if (x) { j += (size_t)(__builtin_ctzll(x) >> 3); ended = true; break; }
      j += 8;
    }
    if (!ended) while (j < n && ops[j] == op) ++j;
    size_t len = j - i;
    char buf[24];
    int k = 0;
    do { buf[k++] = (char)('0' + len % 10); len /= 10; } while (len);
    while (k) *w++ = buf[--k];
    *w++ = op == 'M' ? '=' : op == 'X' ? 'X' : op == 'I' ? 'D' : op == 'D' ? 'I' : '?';
    i = j;
  }
  out.resize(base + (size_t)(w - w0));
}

std::string cigar_bytes_to_string(const uint8_t* ops, size_t n) {
  std::string s;
  append_cigar(s, ops, n);
  return s;
}

std::vector<uint8_t> reverse_complement(const std::vector<uint8_t>& seq) {  // alignment.rs:178-190
  std::vector<uint8_t> out(seq.size());
  for (size_t i = 0; i < seq.size(); ++i) {
    uint8_t b = seq[seq.size() - 1 - i], c;
    switch (b) {
      case 'A': case 'a': c = 'T'; break;
      case 'T': case 't': c = 'A'; break;
      case 'C': case 'c': c = 'G'; break;
      case 'G': case 'g': c = 'C'; break;
      default: c = 'N'; break;
    }
    out[i] = c;
  }
  return out;
}

// the line up to and including "cg:Z:"
static void append_paf_head(std::string& out, const AlignmentResult& r, const std::vector<Sequence>& sequences) {  // lib.rs:71-112
  const Sequence& q = sequences[r.query_idx];
  const Sequence& t = sequences[r.target_idx];
  const size_t qa = r.query_end - r.query_start, ta = r.target_end - r.target_start;
  const size_t block_len = std::max(ta, qa);
  const double identity = r.alignment_length > 0 ? (double)r.num_matches / (double)r.alignment_length : 0.0;
  out += q.id; out.push_back('\t');
  append_uint(out, q.seq.size()); out.push_back('\t');
  append_uint(out, r.query_start); out.push_back('\t');
  append_uint(out, r.query_end); out.push_back('\t');
  out.push_back(r.is_reverse ? '-' : '+'); out.push_back('\t');
  out += t.id; out.push_back('\t');
  append_uint(out, t.seq.size()); out.push_back('\t');
  append_uint(out, r.target_start); out.push_back('\t');
  append_uint(out, r.target_end); out.push_back('\t');
  append_uint(out, r.num_matches); out.push_back('\t');
  append_uint(out, block_len); out.push_back('\t');
  out += "60\tgi:f:";
  char buf[32];
  snprintf(buf, sizeof(buf), "%.6f", identity);
  out += buf;
  out += "\tcg:Z:";
}

void append_paf(std::string& out, const AlignmentResult& r, const uint8_t* ops, size_t nops, const std::vector<Sequence>& sequences) {
  append_paf_head(out, r, sequences);
  append_cigar(out, ops, nops);
}

void append_paf_text(std::string& out, const AlignmentResult& r, const uint8_t* text, size_t ntext, const std::vector<Sequence>& sequences) {
  append_paf_head(out, r, sequences);
  out.append((const char*)text, ntext);
}

std::string alignment_to_paf(const AlignmentResult& r, const std::vector<Sequence>& sequences) {
  std::string s;
  append_paf(s, r, r.cigar_bytes.data(), r.cigar_bytes.size(), sequences);
  return s;
}

// ---- iterator.rs ----------------------------------------------------------------------------
namespace {
// One engine per (device, slot) and process, created on first use and kept (like the reference's cached
// per-thread aligners, alignment.rs:11-22): its HBM arenas are tens of GB, and allocating them right
// after a free can take the driver seconds.  A run takes slots 0, 1, ... of each device it names (one slot:
// slot 0) and owns their engines under their mutexes.  Lock order: a slot's mutex, then the table's (never
// the other way round).
std::atomic<int> g_engine_flags{0};  // awv_engine_config.flags of engines created from now on (set_engine_flags)
std::atomic<int> g_engine_first_row_cols{0};  // awv_engine_config.first_row_cols, likewise (diagnostic / test hook)
constexpr int64_t kDefaultScratch = (int64_t)160 << 30;  // the engine's default max_scratch_bytes
struct EngineSlot {
  awv_engine* e = nullptr;
  std::unique_ptr<std::mutex> mu{new std::mutex()};  // one run at a time per slot
};
struct EngineTable {
  std::mutex mu;  // guards the table (entries are never erased: slot mutexes stay put)
  std::map<std::pair<int, int>, EngineSlot> engines;  // (device, slot)
  // slots per device of the widest run that created engines there: those engines get max_scratch_bytes = 160 GiB / k
  // (kept until release_engines)
  std::map<int, int> scratch_split;
};
EngineTable& engine_table() {
  static EngineTable t;
  return t;
}
std::mutex* slot_mutex(int device, int slot) {
  EngineTable& tb = engine_table();
  std::lock_guard<std::mutex> g(tb.mu);
  return tb.engines[{device, slot}].mu.get();
}
// the slot's engine, created if need be; the caller holds the slot's mutex, so nobody else creates or destroys this slot's
// engine meanwhile, and the creation itself runs outside the table's lock (slots of different devices start in parallel).
// `slots_on_device`: how many slots of this device the calling run uses
awv_engine* slot_engine(int device, int slot, int slots_on_device) {
  EngineTable& tb = engine_table();
  EngineSlot* es;
  awv_engine_config cfg{};
  {
    std::lock_guard<std::mutex> g(tb.mu);
    es = &tb.engines[{device, slot}];
    if (es->e) return es->e;
    cfg.device = device;
    cfg.flags = g_engine_flags.load();
    cfg.first_row_cols = g_engine_first_row_cols.load();
    auto sp = tb.scratch_split.find(device);
    const int k = std::max(slots_on_device, sp == tb.scratch_split.end() ? 1 : sp->second);
    if (k > 1) {
      tb.scratch_split[device] = k;
      cfg.max_scratch_bytes = kDefaultScratch / k;
    }
  }
  awv_engine* e = nullptr;
  if (awv_engine_create(&cfg, &e) != AWV_OK) throw AlignmentError(std::string("engine: ") + awv_last_error());
  std::lock_guard<std::mutex> g(tb.mu);
  es->e = e;
  return e;
}
void upload(awv_engine* e, const std::vector<Sequence>& seqs) {
  std::vector<uint64_t> offs(seqs.size() + 1, 0);
  for (size_t i = 0; i < seqs.size(); ++i) offs[i + 1] = offs[i] + seqs[i].seq.size();
  std::vector<uint8_t> cat(offs.back() + 1);
  for (size_t i = 0; i < seqs.size(); ++i)
    if (!seqs[i].seq.empty()) memcpy(cat.data() + offs[i], seqs[i].seq.data(), seqs[i].seq.size());
  if (awv_engine_set_sequences(e, (int32_t)seqs.size(), cat.data(), offs.data()) != AWV_OK)
    throw AlignmentError(std::string("set_sequences: ") + awv_last_error());
}

// planner::predicted_pair_cost of pairs[0, n) (ranges, nullable: entry i is that interval pair -- its lengths count)
std::vector<double> pair_costs(const std::vector<Sequence>& seqs, const std::pair<size_t, size_t>* pairs, size_t n,
                               const AlignmentParams& params, const AlignmentRange* ranges = nullptr) {
  std::vector<double> cost(n);
  for (size_t i = 0; i < n; ++i)
    cost[i] = ranges ? planner::predicted_pair_cost(ranges[i].query_end - ranges[i].query_start, ranges[i].target_end - ranges[i].target_start, params)
                     : planner::predicted_pair_cost(seqs[pairs[i].first].seq.size(), seqs[pairs[i].second].seq.size(), params);
  return cost;
}

// align_pair's result mapping (alignment.rs:42-65, 239-253)
AlignmentResult make_result(size_t qi, size_t ti, bool is_rev, const awv_result& r, const uint8_t* arena, bool copy_cigar) {
  AlignmentResult a;
  a.query_idx = qi;
  a.target_idx = ti;
  a.is_reverse = is_rev;
  if (r.status != AWV_ST_COMPLETED) {  // "empty" alignment on failure, still emitted
    a.score = INT32_MAX;
    return a;
  }
  a.query_end = (size_t)r.q_end;
  a.target_end = (size_t)r.t_end;
  a.score = r.score;
  a.num_matches = (size_t)r.num_matches;
  a.alignment_length = (size_t)r.num_matches + (size_t)r.num_mismatches;
  if (copy_cigar && arena) a.cigar_bytes.assign(arena + r.cigar_off, arena + r.cigar_off + r.cigar_len);
  return a;
}
}  // namespace

AlignmentResult range_alignment_result(const AlignmentRange& g, const awv_result& r, const uint8_t* arena, bool copy_cigar) {
  AlignmentResult a = make_result(g.query_idx, g.target_idx, g.is_reverse, r, arena, copy_cigar);
  a.query_start = g.query_start;
  a.query_end += g.query_start;
  a.target_start = g.target_start;
  a.target_end += g.target_start;
  return a;
}

AlignmentResult AllPairIterator::result_at(size_t k, bool is_rev, const awv_result& r, const uint8_t* arena, bool copy_cigar,
                                           const awv_clip_result* cl) const {
  if (cl && cl->code == AWV_CL_OK && r.status == AWV_ST_COMPLETED) {  // r describes the segment: q_end / t_end are the bases it consumes
    const size_t qi = pairs_[k].first, ti = pairs_[k].second;
    const size_t qb = ranges_ ? (*ranges_)[k].query_start : 0, qe = ranges_ ? (*ranges_)[k].query_end : sequences_[qi].seq.size();
    const size_t tb = ranges_ ? (*ranges_)[k].target_start : 0;
    AlignmentResult a = make_result(qi, ti, ranges_ ? (*ranges_)[k].is_reverse : is_rev, r, arena, copy_cigar);
    const size_t q_len = a.query_end, t_len = a.target_end;
    if (a.is_reverse) {
      a.query_end = qe - (size_t)cl->q_skip;
      a.query_start = a.query_end - q_len;
    } else {
      a.query_start = qb + (size_t)cl->q_skip;
      a.query_end = a.query_start + q_len;
    }
    a.target_start = tb + (size_t)cl->t_skip;
    a.target_end = a.target_start + t_len;
    return a;
  }
  if (ranges_) return range_alignment_result((*ranges_)[k], r, arena, copy_cigar);
  return make_result(pairs_[k].first, pairs_[k].second, is_rev, r, arena, copy_cigar);
}

AllPairIterator AllPairIterator::for_ranges(const std::vector<Sequence>& sequences, std::vector<AlignmentRange> ranges, AlignmentParams params) {
  AllPairIterator it(sequences, std::move(params), false);
  it.pairs_.reserve(ranges.size());
  for (size_t k = 0; k < ranges.size(); ++k) {
    const AlignmentRange& g = ranges[k];
    if (g.query_idx >= sequences.size() || g.target_idx >= sequences.size() || g.query_start > g.query_end ||
        g.query_end > sequences[g.query_idx].seq.size() || g.target_start > g.target_end || g.target_end > sequences[g.target_idx].seq.size())
      throw std::invalid_argument("for_ranges: range " + std::to_string(k) + " names a sequence index or an interval out of range");
    it.pairs_.emplace_back(g.query_idx, g.target_idx);
  }
  it.orientation_ = Orientation::ForwardOnly;  // (the strand is each range's own)
  it.ranges_ = std::make_shared<const std::vector<AlignmentRange>>(std::move(ranges));
  return it;
}

void align_ranges(const std::vector<Sequence>& sequences, const std::vector<AlignmentRange>& ranges, AlignmentParams params,
                  const Callback& callback, const std::vector<int>& devices, bool verify, std::vector<VerifyFailure>* failures,
                  awv_verify_stats* verify_stats) {
  AllPairIterator it = AllPairIterator::for_ranges(sequences, ranges, std::move(params));
  it.with_devices(devices).with_verify(verify);
  it.for_each_with_callback(callback);
  if (failures) *failures = it.verify_failures();
  if (verify_stats) *verify_stats = it.last_verify_stats();
}

void RunOptions::apply(AllPairIterator& it) const {
  if (normalize != AWV_NORM_OFF) it.with_normalize(normalize);
  if (device_cigar) it.with_device_cigar(true);
  if (cs != 0) it.with_cs(cs);
  if (coverage != 0) it.with_coverage(coverage);
  if (variants) it.with_variants(true);
  if (liftover_from != 0) it.with_liftover(liftover, liftover_from);
  if (msa) it.with_msa(msa_targets, msa_max_bytes);
  if (max_penalty) it.with_max_penalty(*max_penalty);
  if (max_divergence) it.with_max_divergence(*max_divergence);
  if (clip_match_bonus != 0) it.with_clip(clip_match_bonus, clip_min_score);
  if (split_match_bonus != 0) it.with_split(split_match_bonus, split_min_score);
}

void align_ranges(const std::vector<Sequence>& sequences, const std::vector<AlignmentRange>& ranges, AlignmentParams params,
                  const Callback& callback, const std::vector<int>& devices, bool verify, const RunOptions& options, RunReport* report) {
  AllPairIterator it = AllPairIterator::for_ranges(sequences, ranges, std::move(params));
  it.with_devices(devices).with_verify(verify);
  options.apply(it);
  it.for_each_with_callback(callback);
  if (report) *report = it.last_report();
}

AllPairIterator::AllPairIterator(const std::vector<Sequence>& sequences, AlignmentParams params)
    : AllPairIterator(sequences, std::move(params), true) {}

AllPairIterator::AllPairIterator(const std::vector<Sequence>& sequences, AlignmentParams params, bool enumerate)
    : sequences_(sequences), params_(std::move(params)), orientation_params_(AlignmentParams::edit_distance()) {
  if (!enumerate) return;
  const size_t n = sequences.size();
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if (i != j) pairs_.emplace_back(i, j);  // iterator.rs:38-43 row-major, i != j
}

AllPairIterator AllPairIterator::with_options(const std::vector<Sequence>& sequences, AlignmentParams params, bool exclude_self,
                                              bool use_mash_orientation, SparsificationStrategy s, int plan_device) {
  if (plan_device < 0 || s.kind == SparsificationStrategy::None) {
    AllPairIterator it = with_options(sequences, std::move(params), exclude_self, use_mash_orientation, std::move(s));
    return it.with_plan_device(plan_device);
  }
  // the same lists as below, planned on the device without enumerating all N^2 pairs on the host first
  AllPairIterator it(sequences, std::move(params), false);
  it.exclude_self_ = exclude_self;
  it.plan_device_ = plan_device;
  const size_t n = sequences.size();
  switch (s.kind) {
    case SparsificationStrategy::None: break;
    case SparsificationStrategy::Random:
      it.pairs_ = planner::apply_random_sparsification(sequences, s.value, exclude_self, plan_device);
      break;
    case SparsificationStrategy::Auto:
      it.pairs_ = planner::apply_random_sparsification(sequences, planner::compute_connectivity_probability(n, 0.95), exclude_self, plan_device);
      break;
    case SparsificationStrategy::Connectivity:
      it.pairs_ = planner::apply_random_sparsification(sequences, planner::compute_connectivity_probability(n, s.value), exclude_self, plan_device);
      break;
    case SparsificationStrategy::TreeSampling:
      it.pairs_ = planner::extract_tree_pairs(sequences, s.k_nearest, s.k_farthest, s.random_fraction, s.kmer_size.value_or(15), plan_device);
      break;
  }
  it.orientation_ = use_mash_orientation ? Orientation::Mash : Orientation::Wfa;
  return it;
}

AllPairIterator AllPairIterator::with_options(const std::vector<Sequence>& sequences, AlignmentParams params,
                                              bool exclude_self, bool use_mash_orientation, SparsificationStrategy s) {
  AllPairIterator it(sequences, std::move(params));
  it.exclude_self_ = exclude_self;
  if (!exclude_self) {  // iterator.rs:44-46
    it.pairs_.clear();
    for (size_t i = 0; i < sequences.size(); ++i)
      for (size_t j = 0; j < sequences.size(); ++j) it.pairs_.emplace_back(i, j);
  }
  switch (s.kind) {  // iterator.rs:49-79
    case SparsificationStrategy::None: break;
    case SparsificationStrategy::Random:
      it.pairs_ = planner::apply_random_sparsification(std::move(it.pairs_), s.value, sequences);
      break;
    case SparsificationStrategy::Auto:
      it.pairs_ = planner::apply_random_sparsification(std::move(it.pairs_),
                                                      planner::compute_connectivity_probability(sequences.size(), 0.95), sequences);
      break;
    case SparsificationStrategy::Connectivity:
      it.pairs_ = planner::apply_random_sparsification(std::move(it.pairs_),
                                                      planner::compute_connectivity_probability(sequences.size(), s.value), sequences);
      break;
    case SparsificationStrategy::TreeSampling:
      it.pairs_ = planner::extract_tree_pairs(sequences, s.k_nearest, s.k_farthest, s.random_fraction, s.kmer_size.value_or(15));
      break;
  }
  it.orientation_ = use_mash_orientation ? Orientation::Mash : Orientation::Wfa;
  return it;
}

AllPairIterator& AllPairIterator::with_plan_device(int plan_device) { plan_device_ = plan_device < 0 ? -1 : plan_device; return *this; }
AllPairIterator& AllPairIterator::with_orientation_params(AlignmentParams p) { orientation_params_ = std::move(p); return *this; }
AllPairIterator& AllPairIterator::with_orientation(Orientation o) { orientation_ = o; return *this; }
AllPairIterator& AllPairIterator::with_full_wfa_orientation(bool full) { full_wfa_orientation_ = full; return *this; }
AllPairIterator& AllPairIterator::with_device(int device) { devices_.assign(1, device); return *this; }
AllPairIterator& AllPairIterator::with_devices(std::vector<int> devices) {
  if (devices.empty()) throw std::invalid_argument("with_devices: the device list is empty");
  devices_ = std::move(devices);
  return *this;
}
AllPairIterator& AllPairIterator::with_min_batch_pairs(size_t n) { min_batch_pairs_ = std::max<size_t>(1, n); return *this; }
void set_engine_flags(int flags) { g_engine_flags.store(flags); }
void set_engine_first_row_cols(int cols) { g_engine_first_row_cols.store(cols); }
void release_engines() {
  EngineTable& tb = engine_table();
  std::vector<std::pair<EngineSlot*, std::mutex*>> slots;
  {
    std::lock_guard<std::mutex> g(tb.mu);
    for (auto& kv : tb.engines) slots.emplace_back(&kv.second, kv.second.mu.get());
  }
  for (auto& sm : slots) {
    std::lock_guard<std::mutex> busy(*sm.second);  // (waits for a run in flight on that slot)
    awv_engine* e;
    {
      std::lock_guard<std::mutex> g(tb.mu);
      e = sm.first->e;
      sm.first->e = nullptr;
    }
    if (e) awv_engine_destroy(e);
  }
  std::lock_guard<std::mutex> g(tb.mu);
  tb.scratch_split.clear();
}
int visible_device_count() {
  // the HIP runtime is found among the objects already loaded (liballwave_hip links it): no path or version of it is assumed
  std::string path;
  dl_iterate_phdr([](dl_phdr_info* info, size_t, void* p) -> int {
    if (info->dlpi_name && strstr(info->dlpi_name, "libamdhip64")) {
      *(std::string*)p = info->dlpi_name;
      return 1;
    }
    return 0;
  }, &path);
  void* h = path.empty() ? nullptr : dlopen(path.c_str(), RTLD_NOW | RTLD_NOLOAD);
  if (!h) throw AlignmentError("no HIP device available (the HIP runtime is not loaded)");
  typedef int (*CountFn)(int*);           // hipGetDeviceCount; hipError_t: hipSuccess = 0
  typedef const char* (*ErrFn)(int);      // hipGetErrorString
  CountFn count = (CountFn)dlsym(h, "hipGetDeviceCount");
  ErrFn err_str = (ErrFn)dlsym(h, "hipGetErrorString");
  int n = 0;
  const int rc = count ? count(&n) : -1;
  const std::string why = rc == 0 ? "no device" : (err_str && rc > 0 ? err_str(rc) : "hipGetDeviceCount failed");
  dlclose(h);
  if (rc != 0 || n <= 0) throw AlignmentError("no HIP device available (" + why + ")");
  return n;
}

AllPairIterator& AllPairIterator::with_shard(size_t rank, size_t world) {
  // cost-balanced shards (planner::assign_shards_lpt): every process derives the same partition and
  // keeps its own part, in list order; equal-cost lists (config 2 / 3) come out strided
  if (world <= 1) return *this;
  if (ranges_) throw std::invalid_argument("with_shard: not for a range list");
  const std::vector<uint32_t> shard = planner::assign_shards_lpt(pair_costs(sequences_, pairs_.data(), pairs_.size(), params_), world);
  std::vector<std::pair<size_t, size_t>> mine;
  mine.reserve(pairs_.size() / world + 1);
  for (size_t i = 0; i < pairs_.size(); ++i)
    if (shard[i] == (uint32_t)rank) mine.push_back(pairs_[i]);
  pairs_.swap(mine);
  return *this;
}

AllPairIterator AllPairIterator::with_sparsification(SparsificationStrategy strategy) const {  // iterator.rs:101-110
  if (ranges_) throw std::invalid_argument("with_sparsification: not for a range list");
  AllPairIterator it = with_options(sequences_, params_, exclude_self_, orientation_ == Orientation::Mash, std::move(strategy), plan_device_);
  if (orientation_ == Orientation::ForwardOnly) it.orientation_ = Orientation::ForwardOnly;  // (this build's extension survives)
  it.devices_ = devices_;
  it.min_batch_pairs_ = min_batch_pairs_;
  it.threads_ = threads_;
  it.next_chunk_ = next_chunk_;
  it.full_wfa_orientation_ = full_wfa_orientation_;
  it.verify_ = verify_;
  it.max_penalty_ = max_penalty_;
  it.max_divergence_ = max_divergence_;
  it.clip_bonus_ = clip_bonus_;
  it.clip_min_score_ = clip_min_score_;
  it.split_bonus_ = split_bonus_;
  it.split_min_score_ = split_min_score_;
  it.normalize_ = normalize_;
  it.device_cigar_ = device_cigar_;
  it.cs_ = cs_;
  it.coverage_ = coverage_;
  it.variants_ = variants_;
  it.lift_from_ = lift_from_;
  it.lift_regions_ = lift_regions_;
  it.msa_ = msa_;
  it.msa_targets_ = msa_targets_;
  it.msa_max_bytes_ = msa_max_bytes_;
  return it;
}
AllPairIterator& AllPairIterator::with_device_cigar(bool on) {
  if (on && split()) throw std::invalid_argument("with_device_cigar: not together with with_split");
  device_cigar_ = on;
  return *this;
}
AllPairIterator& AllPairIterator::with_cs(int mode) {
  if (mode != 0 && mode != AWV_CS_SHORT && mode != AWV_CS_LONG) throw std::invalid_argument("with_cs: 0, AWV_CS_SHORT or AWV_CS_LONG");
  if (mode != 0 && split()) throw std::invalid_argument("with_cs: not together with with_split");
  cs_ = mode;
  return *this;
}
AllPairIterator& AllPairIterator::with_coverage(int roles) {
  if (roles < 0 || roles > AWV_COV_BOTH) throw std::invalid_argument("with_coverage: 0, AWV_COV_TARGET, AWV_COV_QUERY or AWV_COV_BOTH");
  coverage_ = roles;
  return *this;
}
AllPairIterator& AllPairIterator::with_liftover(std::vector<awv_region> regions, int from) {
  if (from < 0 || from > AWV_LIFT_FROM_BOTH) throw std::invalid_argument("with_liftover: 0, AWV_LIFT_FROM_TARGET, AWV_LIFT_FROM_QUERY or AWV_LIFT_FROM_BOTH");
  for (const awv_region& g : regions)
    if (g.seq < 0 || (size_t)g.seq >= sequences_.size() || g.beg < 0 || g.beg >= g.end || (size_t)g.end > sequences_[(size_t)g.seq].seq.size())
      throw std::invalid_argument("with_liftover: a region names a sequence out of range, or an interval that is empty or outside its sequence");
  lift_from_ = from;
  lift_regions_ = from != 0 ? std::move(regions) : std::vector<awv_region>{};
  return *this;
}
AllPairIterator& AllPairIterator::with_msa(std::vector<int> targets, uint64_t max_bytes) {
  if (max_bytes == 0) throw std::invalid_argument("with_msa: max_bytes must be positive");
  std::vector<uint8_t> seen(sequences_.size(), 0);
  for (int t : targets) {
    if (t < 0 || (size_t)t >= sequences_.size()) throw std::invalid_argument("with_msa: a target names a sequence out of range");
    if (seen[(size_t)t]++) throw std::invalid_argument("with_msa: a target is named twice");
  }
  if (targets.empty())
    for (size_t t = 0; t < sequences_.size(); ++t) targets.push_back((int)t);
  msa_ = true;
  msa_targets_ = std::move(targets);
  msa_max_bytes_ = max_bytes;
  return *this;
}
AllPairIterator& AllPairIterator::with_normalize(int direction) {
  if (direction != AWV_NORM_OFF && direction != AWV_NORM_LEFT && direction != AWV_NORM_RIGHT)
    throw std::invalid_argument("with_normalize: AWV_NORM_OFF, AWV_NORM_LEFT or AWV_NORM_RIGHT");
  normalize_ = direction;
  return *this;
}
AllPairIterator& AllPairIterator::with_verify(bool on) { verify_ = on; return *this; }
AllPairIterator& AllPairIterator::with_clip(int match_bonus, int64_t min_score) {
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS) throw std::invalid_argument("with_clip: match_bonus must be in [1, 32767]");
  if (min_score < 1) throw std::invalid_argument("with_clip: min_score must be >= 1");
  if (split()) throw std::invalid_argument("with_clip: not together with with_split");
  clip_bonus_ = match_bonus;
  clip_min_score_ = min_score;
  return *this;
}
AllPairIterator& AllPairIterator::with_split(int match_bonus, int64_t min_score) {
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS) throw std::invalid_argument("with_split: match_bonus must be in [1, 32767]");
  if (min_score < 1) throw std::invalid_argument("with_split: min_score must be >= 1");
  if (clip()) throw std::invalid_argument("with_split: not together with with_clip");
  if (device_cigar_) throw std::invalid_argument("with_split: not together with with_device_cigar");
  if (cs_ != 0) throw std::invalid_argument("with_split: not together with with_cs");
  split_bonus_ = match_bonus;
  split_min_score_ = min_score;
  return *this;
}
AllPairIterator& AllPairIterator::with_max_penalty(int max_penalty) {
  if (max_penalty < 0) throw std::invalid_argument("with_max_penalty: max_penalty must be >= 0");
  max_penalty_ = max_penalty;
  return *this;
}
AllPairIterator& AllPairIterator::with_max_divergence(double max_divergence) {
  if (!(max_divergence >= 0.0 && max_divergence < 1.0)) throw std::invalid_argument("with_max_divergence: need 0 <= max_divergence < 1");
  max_divergence_ = max_divergence;
  return *this;
}
AllPairIterator& AllPairIterator::with_next_chunk(size_t n) { next_chunk_ = std::max<size_t>(1, n); return *this; }
AllPairIterator& AllPairIterator::with_threads(int t) { threads_ = t; return *this; }
AllPairParallelIterator AllPairIterator::into_par_iter() const { return AllPairParallelIterator(*this); }

std::vector<AlignmentResult> AllPairIterator::collect_ordered(size_t first, size_t cnt) {
  std::vector<AlignmentResult> buf(cnt);
  std::vector<uint8_t> have(cnt, 0);  // (a pair the run drops is not delivered: its slot stays empty and is skipped)
  std::vector<std::vector<AlignmentResult>> more(split() ? cnt : 0);  // a splitting run: a pair's segments after its first
  run(first, cnt, [&](const Batch& b) {  // (every pair has its own slot of buf: no lock)
    for (int64_t i = 0; i < b.n; ++i) {
      const size_t k = b.pair(i);
      AlignmentResult a = result_at(first + k, b.is_rev(i), b.res[i], b.arena, true, b.clip_at(i));
      if (have[k]) more[k].push_back(std::move(a));
      else buf[k] = std::move(a);
      have[k] = 1;
    }
  });
  if (!drops_pairs()) return buf;
  std::vector<AlignmentResult> kept;  // the delivered pairs in pair-list order, each pair's segments in column order
  for (size_t k = 0; k < cnt; ++k) {
    if (!have[k]) continue;
    kept.push_back(std::move(buf[k]));
    if (split())
      for (auto& a : more[k]) kept.push_back(std::move(a));
  }
  return kept;
}

std::optional<AlignmentResult> AllPairIterator::next() {  // iterator.rs:151-171
  if (next_buf_pos_ >= next_buf_.size()) {
    if (next_pos_ >= pairs_.size()) return std::nullopt;
    const size_t cnt = std::min(next_chunk_, pairs_.size() - next_pos_);
    // (only a run that returned moves the position on: after an error the next call runs the same chunk again)
    next_buf_ = collect_ordered(next_pos_, cnt);
    next_buf_pos_ = 0;
    next_pos_ += cnt;
    if (next_buf_.empty()) return next();  // (a chunk of dropped pairs only: on to the next one)
  }
  return std::move(next_buf_[next_buf_pos_++]);
}

void AllPairParallelIterator::for_each_with_callback(const Callback& cb) {
  // the threads are shared out among the slots, whose batches are consumed at the same time
  const int want = std::max<int>(1, (threads_ > 0 ? threads_ : (it_.threads_ > 0 ? it_.threads_ : planner::host_threads())) /
                                        (int)it_.devices_.size());
  // the first error wins (iterator.rs:236-242); the other workers, on every slot, stop at their next pair
  std::mutex mu;
  std::exception_ptr err;
  std::atomic<bool> stop{false};
  it_.run([&](const AllPairIterator::Batch& b) {
    const int64_t cnt = b.n;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(want, cnt));
    std::atomic<int64_t> cursor{0};
    auto work = [&]() {
      for (;;) {
        const int64_t i = cursor.fetch_add(1);
        if (i >= cnt || stop.load()) return;
        try {
          cb(it_.result_at(b.pair(i), b.is_rev(i), b.res[i], b.arena, true, b.clip_at(i)));
        } catch (...) {
          std::lock_guard<std::mutex> g(mu);
          if (!err) err = std::current_exception();
          stop.store(true);
          return;
        }
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    std::lock_guard<std::mutex> g(mu);
    if (err) std::rethrow_exception(err);
  });
}

std::vector<AlignmentResult> AllPairParallelIterator::collect() { return it_.collect_ordered(0, it_.pairs_.size()); }

void process_alignments_with_callback(const std::vector<Sequence>& sequences, AlignmentParams params,
                                      SparsificationStrategy sparsification, const Callback& callback) {  // lib.rs:57-68
  process_alignments_with_callback(sequences, std::move(params), std::move(sparsification), callback, {0});
}

void process_alignments_with_callback(const std::vector<Sequence>& sequences, AlignmentParams params,
                                      SparsificationStrategy sparsification, const Callback& callback,
                                      const std::vector<int>& devices) {
  AllPairIterator aligner = AllPairIterator::with_options(sequences, std::move(params), true, true, std::move(sparsification));
  aligner.with_devices(devices);
  aligner.for_each_with_callback(callback);
}

namespace {
// determine_orientation_wfa (alignment.rs:157-175) for the pairs (q, t) of ap[0, n): forward unless the reverse-complement
// alignment under the orientation params has fewer #X+#I+#D; forward wins ties; a failed alignment counts as usize::MAX.
// awv_orient_pairs decides from bounded strand scores wherever those prove the comparison and aligns both strands in full
// only where they do not; `full`: both strands in full for every pair (AWV_ORIENT_FULL)
void orient_wfa(awv_engine* e, const awv_penalties& open, const awv_pair* ap, int64_t n, bool full, uint8_t* is_rev) {
  std::vector<awv_orient_result> orr((size_t)n);
  if (awv_orient_pairs(e, &open, ap, n, full ? AWV_ORIENT_FULL : 0, orr.data()) != AWV_OK)
    throw AlignmentError(std::string("orientation pass: ") + awv_last_error());
  for (int64_t i = 0; i < n; ++i) is_rev[i] = orr[(size_t)i].is_reverse ? 1 : 0;
}

// counters of several engine calls: summed, except the clock rate (a property of the device) and scratch_bytes (what is
// allocated now: summed over slots, the last call's within one)
void add_stats(awv_stats& acc, const awv_stats& x, bool same_engine) {
  acc.kernel_ms += x.kernel_ms;
  acc.h2d_ms += x.h2d_ms;
  acc.d2h_ms += x.d2h_ms;
  acc.launches += x.launches;
  acc.cell_steps += x.cell_steps;
  acc.extend_steps += x.extend_steps;
  acc.n_breakpoints += x.n_breakpoints;
  acc.n_base += x.n_base;
  acc.overlap_scans += x.overlap_scans;
  acc.aligned_bp += x.aligned_bp;
  acc.pairs_completed += x.pairs_completed;
  acc.scratch_bytes = same_engine ? x.scratch_bytes : acc.scratch_bytes + x.scratch_bytes;
  for (int i = 0; i < 14; ++i) acc.prof[i] += x.prof[i];
  acc.restarts += x.restarts;
  acc.multi_cell_steps += x.multi_cell_steps;
  for (int i = 0; i < 4; ++i) acc.windows[i] += x.windows[i];
  acc.clock_cycles += x.clock_cycles;
  acc.clock_ticks += x.clock_ticks;
  if (!acc.clock_tick_khz) acc.clock_tick_khz = x.clock_tick_khz;
  acc.deep_cell_steps += x.deep_cell_steps;
}

// the other counters of a run, one sum per kind
void add(awv_verify_stats& acc, const awv_verify_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.pairs += x.pairs;
  acc.failed += x.failed;
  acc.columns += x.columns;
}
void add(BoundStats& acc, const BoundStats& x) {
  acc.pairs += x.pairs;
  acc.above_penalty += x.above_penalty;
  acc.above_divergence += x.above_divergence;
}
void add(ClipStats& acc, const ClipStats& x) {
  acc.pairs += x.pairs;
  acc.empty += x.empty;
  acc.below_min_score += x.below_min_score;
  acc.kernel_ms += x.kernel_ms;
}
void add(SplitStats& acc, const SplitStats& x) {
  acc.pairs += x.pairs;
  acc.segments += x.segments;
  acc.empty += x.empty;
  acc.kernel_ms += x.kernel_ms;
}
void add(awv_norm_stats& acc, const awv_norm_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.pairs += x.pairs;
  acc.records_moved += x.records_moved;
  acc.runs += x.runs;
  acc.runs_moved += x.runs_moved;
  acc.columns_moved += x.columns_moved;
  acc.columns += x.columns;
}
void add(awv_encode_stats& acc, const awv_encode_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.pairs += x.pairs;
  acc.runs += x.runs;
  acc.text_bytes += x.text_bytes;
  acc.columns += x.columns;
}
void add(awv_cs_stats& acc, const awv_cs_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.pairs += x.pairs;
  acc.failed += x.failed;
  acc.text_bytes += x.text_bytes;
  acc.columns += x.columns;
}
void add(awv_cov_stats& acc, const awv_cov_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.items += x.items;
  acc.failed += x.failed;
  acc.columns += x.columns;
  acc.boundaries += x.boundaries;
  acc.reads += x.reads;
}
void add(awv_variants_stats& acc, const awv_variants_stats& x) {  // (rows: set behind the merge)
  acc.kernel_ms += x.kernel_ms;
  acc.fold_ms += x.fold_ms;
  acc.items += x.items;
  acc.failed += x.failed;
  acc.columns += x.columns;
  acc.snv += x.snv;
  acc.ins += x.ins;
  acc.del += x.del;
  acc.folds += x.folds;
  acc.capacity_rows += x.capacity_rows;
}
void add(awv_lift_stats& acc, const awv_lift_stats& x) {
  acc.kernel_ms += x.kernel_ms;
  acc.records += x.records;
  acc.columns += x.columns;
  acc.queries += x.queries;
  acc.ok += x.ok;
  acc.skipped += x.skipped;
  acc.bad_op += x.bad_op;
  acc.lengths += x.lengths;
  acc.unaligned += x.unaligned;
  acc.outside += x.outside;
}
// the table's order: all twelve fields of a row in their order, region first
bool lift_row_less(const awv_lift_row& a, const awv_lift_row& b) {
  static_assert(sizeof(awv_lift_row) == 12 * sizeof(int32_t), "awv_lift_row is twelve 32-bit fields");
  const int32_t* const u = &a.region;
  const int32_t* const w = &b.region;
  return std::lexicographical_compare(u, u + 12, w, w + 12);
}
void add(RunReport& acc, const RunReport& x) {
  acc.verify_failures.insert(acc.verify_failures.end(), x.verify_failures.begin(), x.verify_failures.end());
  add(acc.verify_stats, x.verify_stats);
  add(acc.bound_stats, x.bound_stats);
  add(acc.clip_stats, x.clip_stats);
  add(acc.split_stats, x.split_stats);
  add(acc.normalize_stats, x.normalize_stats);
  add(acc.encode_stats, x.encode_stats);
  add(acc.cs_stats, x.cs_stats);
  add(acc.coverage_stats, x.coverage_stats);
  add(acc.variants_stats, x.variants_stats);
  add(acc.lift_stats, x.lift_stats);
}

// One batch's engine call, by name.  ranges (nullable): the batch is these n interval pairs, `pairs` is not read.  Alignment
// calls only: verify (nullable), bounds (nullable: one penalty bound per entry, < 0: none), clip (nullable: the clips, under
// clip_bonus), seg_first (nullable: the split under split_bonus / split_min_score, into index and seg), text (nullable: the
// texts of the call's _encoded form -- not with a split), cs (nullable: the cs texts of the call's _cs form under cs_mode, which
// takes the text too -- not with a split).
struct EngineRequest {
  bool score_only = false;
  int32_t max_penalty = -1;  // the score call's bound (< 0: none)
  const awv_penalties* pen = nullptr;
  const awv_pair* pairs = nullptr;
  const awv_range_pair* ranges = nullptr;
  int64_t n = 0;
  awv_verify_result* verify = nullptr;
  const int32_t* bounds = nullptr;
  int clip_bonus = 0;
  awv_clip_result* clip = nullptr;
  int split_bonus = 0;
  int64_t split_min_score = 1;
  const uint64_t* seg_first = nullptr;
  awv_split_index* index = nullptr;
  awv_clip_result* seg = nullptr;
  awv_cigar_text* text = nullptr;
  int cs_mode = 0;
  awv_cs_text* cs = nullptr;
};

// The entry point a request names: the cs call (which takes all the encoded call does, and cs_sink as its sink), else the encoded call (which takes the bounds, the check and the clip), else the split, else the clip, else the bounded call, else the verified or the plain one, each
// on pairs or on ranges (all follow one rule: a call resets the counters of the steps it asks for and of no other);
// or awv_score_pairs / awv_score_ranges with the
// results handed to the sink in one call (status and penalty, no arena).
int engine_call(awv_engine* e, const EngineRequest& q, awv_sink sink, awv_cs_sink cs_sink, void* user) {
  const awv_penalties* pen = q.pen;
  const int64_t n = q.n;
  if (q.cs && !q.score_only)
    return q.ranges ? awv_align_ranges_cs(e, pen, q.ranges, n, q.bounds, q.clip ? q.clip_bonus : 0, nullptr, q.verify, q.clip, q.text, q.cs_mode, q.cs, cs_sink, user)
                    : awv_align_pairs_cs(e, pen, q.pairs, n, q.bounds, q.clip ? q.clip_bonus : 0, nullptr, q.verify, q.clip, q.text, q.cs_mode, q.cs, cs_sink, user);
  if (q.text && !q.score_only)
    return q.ranges ? awv_align_ranges_encoded(e, pen, q.ranges, n, q.bounds, q.clip ? q.clip_bonus : 0, nullptr, q.verify, q.clip, q.text, sink, user)
                    : awv_align_pairs_encoded(e, pen, q.pairs, n, q.bounds, q.clip ? q.clip_bonus : 0, nullptr, q.verify, q.clip, q.text, sink, user);
  if (q.seg_first && !q.score_only)
    return q.ranges ? awv_align_ranges_split(e, pen, q.ranges, n, q.bounds, q.split_bonus, q.split_min_score, nullptr, q.verify, q.seg_first, q.index, q.seg, sink, user)
                    : awv_align_pairs_split(e, pen, q.pairs, n, q.bounds, q.split_bonus, q.split_min_score, nullptr, q.verify, q.seg_first, q.index, q.seg, sink, user);
  if (q.clip && !q.score_only)
    return q.ranges ? awv_align_ranges_clipped(e, pen, q.ranges, n, q.bounds, q.clip_bonus, nullptr, q.verify, q.clip, sink, user)
                    : awv_align_pairs_clipped(e, pen, q.pairs, n, q.bounds, q.clip_bonus, nullptr, q.verify, q.clip, sink, user);
  if (q.bounds && !q.score_only)
    return q.ranges ? awv_align_ranges_bounded(e, pen, q.ranges, n, q.bounds, nullptr, q.verify, sink, user)
                    : awv_align_pairs_bounded(e, pen, q.pairs, n, q.bounds, nullptr, q.verify, sink, user);
  if (q.ranges && !q.score_only) return q.verify ? awv_align_ranges_verified(e, pen, q.ranges, n, nullptr, q.verify, sink, user) : awv_align_ranges(e, pen, q.ranges, n, nullptr, sink, user);
  if (!q.score_only && q.verify) return awv_align_pairs_verified(e, pen, q.pairs, n, nullptr, q.verify, sink, user);
  if (!q.score_only) return awv_align_pairs(e, pen, q.pairs, n, nullptr, sink, user);
  std::vector<awv_score_result> sr((size_t)n);
  std::vector<int32_t> bounds(q.ranges && q.max_penalty >= 0 ? (size_t)n : 0, q.max_penalty);
  const int rc = q.ranges ? awv_score_ranges(e, pen, q.ranges, n, bounds.empty() ? nullptr : bounds.data(), sr.data())
                          : awv_score_pairs(e, pen, q.pairs, n, q.max_penalty, sr.data());
  if (rc != AWV_OK || n == 0) return rc;
  std::vector<awv_result> res((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    res[(size_t)i].status = sr[(size_t)i].status;
    res[(size_t)i].penalty = sr[(size_t)i].penalty;
    res[(size_t)i].score = -sr[(size_t)i].penalty;
  }
  return sink(user, 0, n, res.data(), nullptr) == 0 ? AWV_OK : AWV_ERR_SINK;
}
}  // namespace

// What one slot of a run counts: written by its submitter thread and its sink calls (which never overlap) only.
struct AllPairIterator::SlotTotals {
  awv_stats engine{};
  RunReport report;
  std::vector<uint32_t> cov_aligned, cov_matched;  // a coverage run: the slot's tracks, read when its batches are done
  std::vector<awv_variant> var_rows;                // a variants run: the slot's folded table, likewise
  std::vector<awv_lift_row> lift_rows;              // a liftover run: the slot's rows, likewise
  MsaStore msa;                                     // an msa run: what the slot's sink calls kept
};

// What the slots of one run share.  The settings hold for alignment calls only: a score-only run has none of them.
struct AllPairIterator::RunState {
  size_t first = 0, count = 0;
  const std::pair<size_t, size_t>* plist = nullptr;  // pairs_.data() + first
  const BatchCb* batch_cb = nullptr;
  EngineCall call{false, -1, false, 0};
  std::vector<std::vector<size_t>> batches;  // pair indices (relative to `first`) of each batch; one slot's single batch: empty, the whole range
  std::vector<uint8_t> mash_rev;             // mash orientation of the whole range, computed up front
  bool verify = false, bounded = false, clipping = false, splitting = false, encoding = false;
  int cs = 0;  // the cs mode of the run's alignment calls (0: none)
  int coverage = 0;  // the roles of a run that accumulates the per-base depth (0: none)
  bool variants = false;  // a run that tallies the allele table
  int liftover = 0;  // the side mask of a run that lifts regions (0: none)
  const AllPairIterator* msa = nullptr;  // a run that keeps items for the multiple alignments (nullptr: none)
  std::vector<uint8_t> msa_chosen;        // per sequence: it is one of the targets
  uint64_t n_bases = 0;  // the sum of the sequences' lengths
  int normalizing = AWV_NORM_OFF;
  std::optional<double> div;  // the divergence bound of a bounded run
  awv_penalties pen{}, open{};
  std::vector<SlotTotals> totals;
  // the first error -- an engine's or a batch callback's -- wins: every slot takes no new batch and stops at its next sink call
  std::mutex mu;  // guards err (and run()'s start barrier)
  std::exception_ptr err;
  std::atomic<bool> stop{false};
  void fail(std::exception_ptr e) {
    std::lock_guard<std::mutex> g(mu);
    if (!err) err = e;
    stop.store(true);
  }
  bool timing = false;  // diagnostic (AWH_TIMING): a one-slot run's stage times on stderr
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(const char* what) const {
    if (timing) fprintf(stderr, "[awh] %-18s %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
};

// One batch made ready for its engine call: the arrays the call reads and writes, which this object owns, the request that
// names them and the delivery rule over them (delivery.hpp).
struct AllPairIterator::PreparedBatch {
  const size_t* idx = nullptr;  // pair-list index (relative to the run's range) per entry; nullptr: the entry's own position
  int64_t m = 0;
  std::vector<awv_pair> ap;
  std::vector<uint8_t> rev;
  std::vector<awv_range_pair> rp;
  std::vector<int32_t> bounds;  // one penalty bound per entry: the smaller of with_max_penalty's and the one the divergence bound implies
  std::vector<uint8_t> by_div;
  std::vector<awv_verify_result> vr;
  std::vector<awv_clip_result> cr;
  std::vector<awv_cigar_text> tx;
  std::vector<awv_cs_text> cx;
  // a splitting run: this call's segment storage, laid out by the engine's own arithmetic over the resident lengths
  std::vector<uint64_t> seg_first;
  std::vector<awv_split_index> six;
  std::vector<awv_clip_result> sseg;
  EngineRequest request;
  Delivery delivery;
};

AllPairIterator::PreparedBatch AllPairIterator::prepare_batch(const RunState& rs, awv_engine* e, size_t b, SlotTotals& totals) const {
  PreparedBatch pb;
  const bool whole = devices_.size() == 1;  // one slot: one batch, the whole range in list order
  const size_t* idx = pb.idx = whole ? nullptr : rs.batches[b].data();
  const int64_t m = pb.m = (int64_t)(whole ? rs.count : rs.batches[b].size());
  auto at = [&](int64_t i) { return idx ? idx[i] : (size_t)i; };
  pb.ap.resize((size_t)m);
  pb.rev.assign((size_t)m, 0);
  for (int64_t i = 0; i < m; ++i) pb.ap[i] = awv_pair{(int32_t)rs.plist[at(i)].first, (int32_t)rs.plist[at(i)].second, 0};
  if (ranges_) {
    pb.rp.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
      const AlignmentRange& g = (*ranges_)[rs.first + at(i)];
      pb.rev[i] = g.is_reverse ? 1 : 0;
      pb.rp[i] = awv_range_pair{pb.ap[i].q_idx, pb.ap[i].t_idx, pb.rev[i], (int32_t)g.query_start, (int32_t)g.query_end, (int32_t)g.target_start, (int32_t)g.target_end};
    }
  } else if (orientation_ == Orientation::Mash) {
    for (int64_t i = 0; i < m; ++i) pb.rev[i] = rs.mash_rev[at(i)];
  } else if (orientation_ == Orientation::Wfa) {
    orient_wfa(e, rs.open, pb.ap.data(), m, full_wfa_orientation_, pb.rev.data());
  }
  for (int64_t i = 0; i < m; ++i) pb.ap[i].q_revcomp = pb.rev[i];
  rs.lap("pairs oriented");
  EngineRequest& q = pb.request;
  Delivery& d = pb.delivery;
  q.score_only = rs.call.score_only;
  q.max_penalty = rs.call.max_penalty;
  q.pen = &rs.pen;
  q.pairs = pb.ap.data();
  q.ranges = ranges_ ? pb.rp.data() : nullptr;
  q.n = m;
  d.rev = pb.rev.data();
  d.idx = idx;
  if (rs.bounded) {
    pb.bounds.assign((size_t)m, max_penalty_ ? (int32_t)*max_penalty_ : -1);
    pb.by_div.assign((size_t)m, 0);
    for (int64_t i = 0; rs.div && i < m; ++i) {
      const int32_t ql = ranges_ ? pb.rp[i].q_end - pb.rp[i].q_beg : (int32_t)sequences_[rs.plist[at(i)].first].seq.size();
      const int32_t tl = ranges_ ? pb.rp[i].t_end - pb.rp[i].t_beg : (int32_t)sequences_[rs.plist[at(i)].second].seq.size();
      const int32_t db = awv_divergence_bound(&rs.pen, ql, tl, *rs.div);
      if (db == INT32_MIN) throw AlignmentError(std::string("max_divergence: ") + awv_last_error());
      if (db >= 0 && (pb.bounds[(size_t)i] < 0 || db < pb.bounds[(size_t)i])) {
        pb.bounds[(size_t)i] = db;
        pb.by_div[(size_t)i] = 1;
      }
    }
    q.bounds = pb.bounds.data();
    d.by_div = pb.by_div.data();
    d.div = rs.div ? *rs.div : -1.0;
    d.bounds = &totals.report.bound_stats;
    d.bounds->pairs += (uint64_t)m;
  }
  if (rs.verify) {
    pb.vr.resize((size_t)m);
    q.verify = pb.vr.data();
  }
  if (rs.clipping) {
    pb.cr.resize((size_t)std::max<int64_t>(m, 1));
    q.clip_bonus = clip_bonus_;
    q.clip = pb.cr.data();
    d.clip = pb.cr.data();
    d.min_score = clip_min_score_;
    d.clips = &totals.report.clip_stats;
  }
  if (rs.splitting) {
    pb.seg_first.resize((size_t)m + 1);
    pb.six.resize((size_t)std::max<int64_t>(m, 1));
    const int lrc = ranges_ ? awv_split_layout_ranges(e, pb.rp.data(), m, split_bonus_, split_min_score_, pb.seg_first.data())
                            : awv_split_layout_pairs(e, pb.ap.data(), m, split_bonus_, split_min_score_, pb.seg_first.data());
    if (lrc != AWV_OK) throw AlignmentError(std::string("split layout: ") + awv_last_error());
    pb.sseg.resize((size_t)std::max<uint64_t>(pb.seg_first[(size_t)m], 1));
    q.split_bonus = split_bonus_;
    q.split_min_score = split_min_score_;
    q.seg_first = d.seg_first = pb.seg_first.data();
    q.index = pb.six.data();
    d.index = pb.six.data();
    q.seg = pb.sseg.data();
    d.seg = pb.sseg.data();
    d.splits = &totals.report.split_stats;
  }
  if (rs.encoding) {
    pb.tx.resize((size_t)std::max<int64_t>(m, 1));
    q.text = pb.tx.data();
    d.text = pb.tx.data();
  }
  if (rs.cs != 0) {
    pb.cx.resize((size_t)std::max<int64_t>(m, 1));
    q.cs_mode = rs.cs;
    q.cs = pb.cx.data();
    d.cs = pb.cx.data();
  }
  return pb;
}

// The engine's sink of every alignment and score call of a run: the batch callback sees the call's entries as they are --
// no copy, no per-entry vector -- or, in a run that filters, the ones delivery.hpp's rule keeps.
struct AllPairIterator::SinkCtx {
  RunState* rs;
  const Delivery* d;
  bool failed;
  SlotTotals* totals;
};
int AllPairIterator::batch_sink(void* user, int64_t first, int64_t cnt, const awv_result* res, const uint8_t* arena) {
  return batch_cs_sink(user, first, cnt, res, arena, nullptr);
}
// (the sink of a cs call: the same, with the call's cs arena)
int AllPairIterator::batch_cs_sink(void* user, int64_t first, int64_t cnt, const awv_result* res, const uint8_t* arena, const uint8_t* cs_arena) {
  SinkCtx* c = (SinkCtx*)user;
  if (c->rs->stop.load()) return 1;  // another slot failed: stop here, report nothing
  try {
    if (c->d->filters()) {
      const Delivered k = deliver(*c->d, first, cnt, res);
      const Batch b{0, (int64_t)k.res.size(), k.res.data(), arena, k.rev.data(), k.idx.data(), k.clip.empty() ? nullptr : k.clip.data(),
                    k.text.empty() ? nullptr : k.text.data(), k.cs.empty() ? nullptr : k.cs.data(), cs_arena};
      if (c->rs->msa) c->rs->msa->keep_msa(*c->rs, b, c->totals->msa);
      (*c->rs->batch_cb)(b);
    } else {
      const Batch b{first, cnt, res, arena, c->d->rev, c->d->idx, nullptr, c->d->text, c->d->cs, cs_arena};
      if (c->rs->msa) c->rs->msa->keep_msa(*c->rs, b, c->totals->msa);
      (*c->rs->batch_cb)(b);
    }
  } catch (...) {
    c->rs->fail(std::current_exception());  // recorded now, and every slot stops at its next sink call
    c->failed = true;
    return 1;
  }
  return 0;
}

// What the sink keeps of a delivered batch for the multiple alignments: batch_items.hpp's rule on what the batch delivered -- a
// completed record as it reaches the consumer is a whole record, a clip's slice that scored enough or one split segment -- for the
// chosen targets only: pair, span, slice and op bytes.  Beyond the bound only the size is counted.
void AllPairIterator::keep_msa(const RunState& rs, const Batch& b, MsaStore& st) const {
  for (int64_t i = 0; i < b.n; ++i) {
    const awv_result& r = b.res[i];
    if (r.status != AWV_ST_COMPLETED) continue;
    const size_t pi = b.pair(i);
    const size_t q = rs.plist[pi].first, t = rs.plist[pi].second;
    if (!rs.msa_chosen[t]) continue;
    const int32_t qlen = (int32_t)sequences_[q].seq.size(), tlen = (int32_t)sequences_[t].seq.size();
    const int32_t rev = b.is_rev(i) ? 1 : 0;
    MsaKept k{};
    if (ranges_) {
      const AlignmentRange& g = (*ranges_)[rs.first + pi];
      k.range = awv_range_pair{(int32_t)q, (int32_t)t, rev, (int32_t)g.query_start, (int32_t)g.query_end, (int32_t)g.target_start, (int32_t)g.target_end};
    } else {
      k.range = awv_range_pair{(int32_t)q, (int32_t)t, rev, 0, qlen, 0, tlen};
    }
    const awv_clip_result* cl = b.clip_at(i);
    k.q_skip = cl ? cl->q_skip : 0;
    k.t_skip = cl ? cl->t_skip : 0;
    k.col_beg = cl ? cl->col_beg : 0u;
    k.pattern_beg = (rev ? qlen - k.range.q_end : k.range.q_beg) + k.q_skip;
    k.len = r.cigar_len;
    k.off = st.ops.size();
    st.need += r.cigar_len;
    if (st.need > msa_max_bytes_) continue;
    st.ops.insert(st.ops.end(), b.arena + r.cigar_off, b.arena + r.cigar_off + r.cigar_len);
    st.kept.push_back(k);
  }
}

// The run's one awv_msa_ranges call, on engine e (which holds the run's sequences): the kept items in the rows' order, measured
// first; the blocks and their row names are left in msa_blocks_.
awv_msa_stats AllPairIterator::build_msa(awv_engine* e) {
  const auto bound = [&](const char* what, uint64_t need) {
    return AlignmentError(std::string("msa: ") + what + " need " + std::to_string(need) + " bytes, more than msa_max_bytes = " + std::to_string(msa_max_bytes_));
  };
  msa_blocks_.clear();
  const MsaStore& st = msa_store_;
  if (st.need > msa_max_bytes_) throw bound("the kept op bytes", st.need);
  std::vector<size_t> order(st.kept.size());
  std::iota(order.begin(), order.end(), (size_t)0);
  const auto key = [&](size_t i) {
    const MsaKept& k = st.kept[i];
    return std::make_tuple(k.range.q_idx, k.range.q_revcomp, k.pattern_beg, k.col_beg, k.range.t_idx, k.range.t_beg + k.t_skip, k.len);
  };
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key(a) < key(b); });
  const int64_t n = (int64_t)order.size(), nt = (int64_t)msa_targets_.size();
  std::vector<awv_range_pair> ranges((size_t)n);
  std::vector<awv_result> recs((size_t)n);
  std::vector<awv_cs_slice> slices((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const MsaKept& k = st.kept[order[(size_t)i]];
    ranges[(size_t)i] = k.range;
    recs[(size_t)i] = awv_result{};
    recs[(size_t)i].status = AWV_ST_COMPLETED;
    recs[(size_t)i].cigar_off = k.off;
    recs[(size_t)i].cigar_len = k.len;
    slices[(size_t)i] = awv_cs_slice{0u, k.len, k.q_skip, k.t_skip};
  }
  std::vector<int32_t> targets(msa_targets_.begin(), msa_targets_.end());
  std::vector<awv_msa_item> items((size_t)std::max<int64_t>(n, 1));
  std::vector<awv_msa_target> tgts((size_t)std::max<int64_t>(nt, 1));
  uint64_t bytes = 0;
  const uint8_t none = 0;
  const uint8_t* const ops = st.ops.empty() ? &none : st.ops.data();
  if (awv_msa_ranges(e, ranges.data(), n, recs.data(), ops, st.ops.size(), slices.data(), targets.data(), nt, items.data(), tgts.data(), nullptr, 0, &bytes) != AWV_OK)
    throw AlignmentError(std::string("msa: ") + awv_last_error());
  if (bytes > msa_max_bytes_) throw bound("the blocks", bytes);
  std::vector<uint8_t> buf((size_t)std::max<uint64_t>(bytes, 1));
  if (awv_msa_ranges(e, ranges.data(), n, recs.data(), ops, st.ops.size(), slices.data(), targets.data(), nt, items.data(), tgts.data(), buf.data(), bytes, &bytes) != AWV_OK)
    throw AlignmentError(std::string("msa: ") + awv_last_error());
  msa_blocks_.resize((size_t)nt);
  for (int64_t j = 0; j < nt; ++j) {
    MsaBlock& blk = msa_blocks_[(size_t)j];
    blk.t_idx = tgts[(size_t)j].t_idx;
    blk.rows = tgts[(size_t)j].rows;
    blk.width = tgts[(size_t)j].width;
    blk.names.assign((size_t)blk.rows, std::string());
    blk.names[0] = sequences_[(size_t)blk.t_idx].id;
    blk.bytes.assign(buf.begin() + (ptrdiff_t)tgts[(size_t)j].off, buf.begin() + (ptrdiff_t)(tgts[(size_t)j].off + (uint64_t)blk.rows * (uint64_t)blk.width));
  }
  for (int64_t i = 0; i < n; ++i) {
    const awv_msa_item& it = items[(size_t)i];
    if (it.code != AWV_MS_OK || it.row <= 0) continue;
    const MsaKept& k = st.kept[order[(size_t)i]];
    const int64_t qlen = (int64_t)sequences_[(size_t)k.range.q_idx].seq.size(), x0 = k.pattern_beg, x1 = x0 + (int64_t)it.bases;
    const int64_t fb = k.range.q_revcomp ? qlen - x1 : x0, fe = k.range.q_revcomp ? qlen - x0 : x1;
    msa_blocks_[(size_t)it.target].names[(size_t)it.row] =
        sequences_[(size_t)k.range.q_idx].id + "/" + std::to_string(fb) + "-" + std::to_string(fe) + (k.range.q_revcomp ? "-" : "+");
  }
  awv_msa_stats ms{};
  awv_engine_msa_stats(e, &ms);
  return ms;
}

// What a slot's totals take from its engine after one call: awv_engine_stats always, the kernel times and the verify
// failures only from a call that returned AWV_OK.
void AllPairIterator::take_call_totals(const RunState& rs, const PreparedBatch& pb, awv_engine* e, bool ok, SlotTotals& t) {
  if (rs.normalizing != AWV_NORM_OFF && ok) {
    awv_norm_stats nx{};
    awv_engine_normalize_stats(e, &nx);
    add(t.report.normalize_stats, nx);
  }
  if (rs.encoding && ok) {
    awv_encode_stats ex{};
    awv_engine_encode_stats(e, &ex);
    add(t.report.encode_stats, ex);
  }
  if (rs.cs != 0 && ok) {
    awv_cs_stats cx{};
    awv_engine_cs_stats(e, &cx);
    add(t.report.cs_stats, cx);
  }
  awv_stats x{};
  awv_engine_stats(e, &x);
  add_stats(t.engine, x, true);
  if (rs.verify && ok) {
    awv_verify_stats vx{};
    awv_engine_verify_stats(e, &vx);
    add(t.report.verify_stats, vx);
    append_verify_failures(t.report.verify_failures, pb.vr.data(), pb.m, rs.first, pb.idx, rs.plist, pb.rev.data());
  }
  if (rs.clipping && ok) {
    awv_clip_stats cx{};
    awv_engine_clip_stats(e, &cx);
    t.report.clip_stats.kernel_ms += cx.kernel_ms;
  }
  if (rs.splitting && ok) {
    awv_split_stats sx{};
    awv_engine_split_stats(e, &sx);
    t.report.split_stats.kernel_ms += sx.kernel_ms;
  }
}

// The run's pairs go to its slots in batches.  One slot: one batch, the whole range in list order, on the calling thread.
// Several slots: planner::device_batches over the predicted costs, one submitter thread per slot.  Every slot creates its
// engine and uploads the sequences; only when all have done so (a failure there ends the run before any launch) does slot
// s take batch s, and then the next batch from one cursor each time its previous call returns.  Per batch: WFA orientation
// on the slot's own engine (mash orientation is computed once for the whole range, up front), then one engine call.  The
// first error -- an engine's or a batch callback's -- wins: the other slots take no new batch and stop at their next sink
// call; it is rethrown here once every thread has ended.
void AllPairIterator::run(size_t first, size_t count, const BatchCb& batch_cb, EngineCall call) {
  if (first > pairs_.size() || count > pairs_.size() - first) throw AlignmentError("pair range out of bounds");
  const size_t S = devices_.size();
  RunState rs;
  rs.first = first;
  rs.count = count;
  rs.plist = pairs_.data() + first;
  rs.batch_cb = &batch_cb;
  rs.call = call;
#ifdef AWV_DEBUG_KNOBS
  rs.timing = S == 1 && getenv("AWH_TIMING") != nullptr;
#endif
  rs.batches = S > 1 ? planner::device_batches(pair_costs(sequences_, rs.plist, count, params_, ranges_ ? ranges_->data() + first : nullptr), S, min_batch_pairs_)
                     : std::vector<std::vector<size_t>>(1);
  if (orientation_ == Orientation::Mash && !ranges_)  // alignment.rs:69-94 (host threads: the CLI's -t)
    rs.mash_rev = planner::orient_pairs_mash(sequences_, rs.plist, count, threads_ > 0 ? threads_ : planner::host_threads(), plan_device_);
  // slot number of every entry on its device, and how many slots each device has in this run
  std::map<int, int> per_device;
  std::vector<int> slot_no(S);
  for (size_t s = 0; s < S; ++s) slot_no[s] = per_device[devices_[s]]++;
  // the slots' mutexes, taken here in (device, slot) order: two runs over the same slots cannot deadlock
  std::vector<std::pair<std::pair<int, int>, size_t>> order;
  for (size_t s = 0; s < S; ++s) order.push_back({{devices_[s], slot_no[s]}, s});
  std::sort(order.begin(), order.end());
  std::vector<std::unique_lock<std::mutex>> locks;
  for (const auto& o : order) locks.emplace_back(*slot_mutex(o.first.first, o.first.second));

  rs.verify = verify_ && !call.score_only;
  rs.bounded = bounded() && !call.score_only;
  rs.clipping = clip() && !call.score_only;
  rs.splitting = split() && !call.score_only;
  rs.encoding = call.encode && !call.score_only;
  rs.cs = call.score_only ? 0 : call.cs;
  rs.normalizing = call.score_only ? AWV_NORM_OFF : normalize_;
  rs.coverage = call.score_only ? 0 : coverage_;
  rs.variants = variants_ && !call.score_only;
  rs.liftover = call.score_only ? 0 : lift_from_;
  if (msa_ && !call.score_only) {
    if (call.encode) throw std::invalid_argument("with_msa: not together with with_device_cigar (the sink then carries text, not op bytes)");
    rs.msa = this;
    rs.msa_chosen.assign(sequences_.size(), 0);
    for (int t : msa_targets_) rs.msa_chosen[(size_t)t] = 1;
  }
  for (const Sequence& q : sequences_) rs.n_bases += q.seq.size();
  rs.div = divergence_bound();
  rs.pen = to_penalties(params_);
  rs.open = to_penalties(orientation_params_);
  if (rs.bounded && rs.div && !(*rs.div >= 0.0 && *rs.div < 1.0)) throw std::invalid_argument("max_divergence: need 0 <= max_divergence < 1");
  rs.totals.resize(S);
  std::condition_variable cv;  // the start barrier, under rs.mu
  size_t ready = 0;
  bool aborted = false;  // a submitter thread could not be started: nobody waits for the whole set at the barrier
  std::atomic<size_t> cursor{S};
  auto worker = [&](size_t s) {
    awv_engine* e = nullptr;
    try {
      e = slot_engine(devices_[s], slot_no[s], per_device.at(devices_[s]));
      rs.lap("engine created");
      upload(e, sequences_);
      rs.lap("sequences uploaded");
      // (a new set ended whatever coverage the engine had: the slot's depth starts from zero with every run)
      if (rs.coverage != 0 && awv_engine_coverage_begin(e, rs.coverage, clip_min_score_) != AWV_OK) throw AlignmentError(std::string("coverage: ") + awv_last_error());
      if (rs.variants && awv_engine_variants_begin(e, clip_min_score_, 0) != AWV_OK) throw AlignmentError(std::string("variants: ") + awv_last_error());
      if (rs.liftover != 0 && awv_engine_lift_begin(e, lift_regions_.data(), (int64_t)lift_regions_.size(), rs.liftover, clip_min_score_) != AWV_OK)
        throw AlignmentError(std::string("liftover: ") + awv_last_error());
    } catch (...) {
      rs.fail(std::current_exception());
    }
    {
      std::unique_lock<std::mutex> g(rs.mu);
      if (++ready == S) cv.notify_all();
      else cv.wait(g, [&] { return ready == S || aborted; });
    }
    if (rs.stop.load()) return;
    try {
      for (size_t b = s; b < rs.batches.size() && !rs.stop.load(); b = cursor.fetch_add(1)) {
        const PreparedBatch pb = prepare_batch(rs, e, b, rs.totals[s]);
        SinkCtx ctx{&rs, &pb.delivery, false, &rs.totals[s]};
        // the slot's engine is this thread's until its device lock goes: the mode holds for this call and is off again after it
        if (rs.normalizing != AWV_NORM_OFF && awv_engine_set_normalize(e, rs.normalizing) != AWV_OK) throw AlignmentError(std::string("normalize: ") + awv_last_error());
        const int rc = engine_call(e, pb.request, batch_sink, batch_cs_sink, &ctx);
        if (rs.normalizing != AWV_NORM_OFF) awv_engine_set_normalize(e, AWV_NORM_OFF);
        rs.lap("aligned + sunk");
        take_call_totals(rs, pb, e, rc == AWV_OK, rs.totals[s]);
        if (ctx.failed) return;  // (the error is already recorded)
        if (rc != AWV_OK) {
          if (rc == AWV_ERR_SINK && rs.stop.load()) return;  // stopped by another slot's error, which is the one reported
          throw AlignmentError(std::string("align_pairs: ") + awv_last_error());
        }
      }
      if (rs.coverage != 0 && !rs.stop.load()) {  // the slot's depth, and what it cost
        SlotTotals& t = rs.totals[s];
        t.cov_aligned.assign((size_t)rs.n_bases, 0);
        t.cov_matched.assign((size_t)rs.n_bases, 0);
        if (awv_engine_coverage_read(e, t.cov_aligned.data(), t.cov_matched.data(), rs.n_bases) != AWV_OK) throw AlignmentError(std::string("coverage: ") + awv_last_error());
        awv_cov_stats cx{};
        awv_engine_coverage_stats(e, &cx);
        add(t.report.coverage_stats, cx);
      }
      if (rs.variants && !rs.stop.load()) {  // the slot's table, and what it cost
        SlotTotals& t = rs.totals[s];
        uint64_t n_rows = 0;
        if (awv_engine_variants_read(e, nullptr, 0, &n_rows) != AWV_OK) throw AlignmentError(std::string("variants: ") + awv_last_error());
        t.var_rows.resize((size_t)n_rows);
        if (n_rows && awv_engine_variants_read(e, t.var_rows.data(), n_rows, &n_rows) != AWV_OK) throw AlignmentError(std::string("variants: ") + awv_last_error());
        awv_variants_stats vx{};
        awv_engine_variants_stats(e, &vx);
        add(t.report.variants_stats, vx);
      }
      if (rs.liftover != 0 && !rs.stop.load()) {  // the slot's rows, and what they cost
        SlotTotals& t = rs.totals[s];
        uint64_t n_rows = 0;
        if (awv_engine_lift_read(e, nullptr, 0, &n_rows) != AWV_OK) throw AlignmentError(std::string("liftover: ") + awv_last_error());
        t.lift_rows.resize((size_t)n_rows);
        if (n_rows && awv_engine_lift_read(e, t.lift_rows.data(), n_rows, &n_rows) != AWV_OK) throw AlignmentError(std::string("liftover: ") + awv_last_error());
        awv_lift_stats lx{};
        awv_engine_lift_stats(e, &lx);
        add(t.report.lift_stats, lx);
      }
    } catch (...) {
      rs.fail(std::current_exception());
    }
    if (e && rs.liftover != 0) awv_engine_lift_begin(e, nullptr, 0, 0, 0);  // the table goes with the run
    if (e && rs.coverage != 0) awv_engine_coverage_begin(e, 0, 0);  // the accumulators go with the run
    if (e && rs.variants) awv_engine_variants_end(e);               // and so does the table
  };
  std::vector<std::thread> th;
  try {
    for (size_t s = 1; s < S; ++s) th.emplace_back(worker, s);
  } catch (...) {
    rs.fail(std::current_exception());
    std::lock_guard<std::mutex> g(rs.mu);
    aborted = true;
    cv.notify_all();
  }
  if (th.size() == S - 1) worker(0);
  for (auto& t : th) t.join();
  awv_msa_stats msa_stats{};
  if (rs.msa) {  // the slots' items (and, for next()'s chunks, the items so far) in one call on the run's first device, still under its lock
    if (first == 0) msa_store_ = MsaStore{};
    for (SlotTotals& t : rs.totals) {
      for (MsaKept k : t.msa.kept) {
        k.off += msa_store_.ops.size();
        msa_store_.kept.push_back(k);
      }
      msa_store_.need += t.msa.need;
      if (msa_store_.need <= msa_max_bytes_) msa_store_.ops.insert(msa_store_.ops.end(), t.msa.ops.begin(), t.msa.ops.end());
      t.msa = MsaStore{};
    }
    if (!rs.err) {
      try {
        msa_stats = build_msa(slot_engine(devices_[0], slot_no[0], per_device.at(devices_[0])));
      } catch (...) {
        rs.fail(std::current_exception());
      }
    }
  }
  locks.clear();
  slot_stats_.clear();
  stats_ = awv_stats{};
  if (first == 0) report_ = RunReport{};  // a run from the list's start begins anew; a later range (next()'s chunks) adds to it
  if (first == 0 && !call.score_only) cov_ = Coverage{};
  if (first == 0 && !call.score_only) var_.clear();
  if (first == 0 && !call.score_only) lift_.clear();
  if (!call.score_only && !rs.msa) msa_blocks_.clear();
  if (rs.coverage != 0 && cov_.offsets.empty()) {
    cov_.offsets.assign(sequences_.size() + 1, 0);
    for (size_t i = 0; i < sequences_.size(); ++i) cov_.offsets[i + 1] = cov_.offsets[i] + sequences_[i].seq.size();
    cov_.aligned.assign((size_t)rs.n_bases, 0);
    cov_.matched.assign((size_t)rs.n_bases, 0);
  }
  for (const SlotTotals& t : rs.totals) {
    slot_stats_.push_back(t.engine);
    add_stats(stats_, t.engine, false);
    add(report_, t.report);
    for (size_t i = 0; i < t.cov_aligned.size(); ++i) {  // the slots' depths add up to the one-engine result
      cov_.aligned[i] += t.cov_aligned[i];
      cov_.matched[i] += t.cov_matched[i];
    }
  }
  if (rs.variants) {  // the slots' tables (and, for next()'s chunks, the table so far) merge by key: sum and min
    for (const SlotTotals& t : rs.totals) var_.insert(var_.end(), t.var_rows.begin(), t.var_rows.end());
    uint64_t left = var_.size();
    if (awv_variants_fold_host(var_.data(), var_.size(), &left) != AWV_OK) throw AlignmentError(std::string("variants: ") + awv_last_error());
    var_.resize((size_t)left);
    report_.variants_stats.rows = left;
  }
  if (rs.liftover != 0) {  // the slots' rows (and, for next()'s chunks, the rows so far) merge by concatenating and sorting
    for (const SlotTotals& t : rs.totals) lift_.insert(lift_.end(), t.lift_rows.begin(), t.lift_rows.end());
    std::sort(lift_.begin(), lift_.end(), lift_row_less);
  }
  if (rs.msa) report_.msa_stats = msa_stats;
  sort_verify_failures(report_.verify_failures);
  if (rs.err) std::rethrow_exception(rs.err);
}

void AllPairIterator::for_each_with_callback(const Callback& cb) {
  // the callback's calls never overlap (several slots deliver batches at once), and none follows its first error: a
  // batch that gets the lock after it rethrows that same error (so whichever slot reports first, the error is the same)
  std::mutex mu;
  std::exception_ptr first;
  run([&](const Batch& b) {
    std::lock_guard<std::mutex> g(mu);
    if (first) std::rethrow_exception(first);
    try {
      for (int64_t i = 0; i < b.n; ++i) cb(result_at(b.pair(i), b.is_rev(i), b.res[i], b.arena, true, b.clip_at(i)));
    } catch (...) {
      first = std::current_exception();
      throw;
    }
  });
}

void AllPairIterator::for_each_paf_batch(const std::function<void(const std::string&)>& sink, int format_threads) {
  // sink calls never overlap (several slots deliver batches at once) and none follows its first error; formatting runs
  // outside the lock, on the format threads shared out among the slots
  std::mutex mu;
  std::exception_ptr first;
  const int per_slot = std::max(1, format_threads / (int)devices_.size());
  run([&](const Batch& b) {
    const int64_t cnt = b.n;
    const awv_result* res = b.res;
    const uint8_t* arena = b.arena;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(per_slot, cnt / 64 + 1));
    std::vector<std::string> parts((size_t)T);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) {
      th.emplace_back([&, t]() {
        const int64_t lo = cnt * t / T, hi = cnt * (t + 1) / T;
        std::string& out = parts[(size_t)t];
        out.reserve((size_t)(hi - lo) * 4096);
        for (int64_t i = lo; i < hi; ++i) {
          const AlignmentResult a = result_at(b.pair(i), b.is_rev(i), res[i], arena, false, b.clip_at(i));
          const bool ok = res[i].status == AWV_ST_COMPLETED;
          if (const awv_cigar_text* tx = b.text_at(i)) append_paf_text(out, a, tx->len ? arena + tx->off : nullptr, tx->len, sequences_);
          else append_paf(out, a, ok ? arena + res[i].cigar_off : nullptr, ok ? res[i].cigar_len : 0, sequences_);
          if (const awv_cs_text* cx = b.cs_at(i)) {
            out += "\tcs:Z:";
            if (cx->len) out.append((const char*)b.cs_arena + cx->off, cx->len);
          }
          out.push_back('\n');
        }
      });
    }
    for (auto& x : th) x.join();
#ifdef AWV_DEBUG_KNOBS
    if (getenv("AWH_TIMING")) fprintf(stderr, "[awh] formatted %lld pairs on %d threads\n", (long long)cnt, T);
#endif
    std::lock_guard<std::mutex> g(mu);
    if (first) std::rethrow_exception(first);
    try {
      for (const auto& p : parts) sink(p);
    } catch (...) {
      first = std::current_exception();
      throw;
    }
  }, EngineCall{false, -1, device_cigar_, cs_});
}

std::vector<PairScore> AllPairIterator::scores(std::optional<int> max_penalty) {
  if (max_penalty && *max_penalty < 0) throw std::invalid_argument("scores: max_penalty must be >= 0");
  std::vector<PairScore> out(pairs_.size());
  run([&](const Batch& b) {  // (every entry has its own slot of `out`: no lock)
    for (int64_t i = 0; i < b.n; ++i) {
      const size_t k = b.pair(i);
      PairScore& p = out[k];
      p.query_idx = pairs_[k].first;
      p.target_idx = pairs_[k].second;
      p.is_reverse = b.is_rev(i);
      p.status = b.res[i].status;
      p.penalty = b.res[i].penalty;
    }
  }, EngineCall{true, max_penalty ? *max_penalty : -1, false, 0});
  return out;
}

// ---- verification ---------------------------------------------------------------------------
const char* verify_code_name(int32_t code) {
  static const char* const names[] = {"ok", "skipped", "bad_op", "overrun", "m_differs", "x_equal", "short", "counts", "penalty"};
  return code >= 0 && code <= AWV_VF_PENALTY ? names[code] : "unknown";
}

void append_verify_failures(std::vector<VerifyFailure>& out, const awv_verify_result* vr, int64_t m, size_t first, const size_t* idx,
                            const std::pair<size_t, size_t>* plist, const uint8_t* rev) {
  for (int64_t i = 0; i < m; ++i) {
    if (vr[i].code == AWV_VF_OK || vr[i].code == AWV_VF_SKIPPED) continue;
    const size_t k = idx ? idx[i] : (size_t)i;
    out.push_back(VerifyFailure{first + k, plist[k].first, plist[k].second, rev[i] != 0, vr[i].code, vr[i].column, vr[i].penalty});
  }
}

void sort_verify_failures(std::vector<VerifyFailure>& f) {
  std::sort(f.begin(), f.end(), [](const VerifyFailure& a, const VerifyFailure& b) { return a.index < b.index; });
}

int report_verify_failures(const std::vector<VerifyFailure>& vf, const std::vector<Sequence>& sequences, std::string& out, size_t limit) {
  for (size_t i = 0; i < vf.size() && i < limit; ++i)
    out += "verify: pair " + std::to_string(vf[i].index) + " " + sequences[vf[i].query_idx].id + " " + sequences[vf[i].target_idx].id + " " +
           (vf[i].is_reverse ? '-' : '+') + " " + verify_code_name(vf[i].code) + " column " + std::to_string(vf[i].column) + " penalty " +
           std::to_string(vf[i].penalty) + "\n";
  if (vf.size() > limit) out += "verify: ... and " + std::to_string(vf.size() - limit) + " more\n";
  return vf.empty() ? 0 : 4;
}

bool cigar_string_to_bytes(const std::string& cg, std::vector<uint8_t>& ops) {
  ops.clear();
  size_t i = 0;
  while (i < cg.size()) {
    uint64_t len = 0;
    size_t d = 0;
    while (i < cg.size() && cg[i] >= '0' && cg[i] <= '9' && d < 10) {
      len = len * 10 + (uint64_t)(cg[i] - '0');
      ++i;
      ++d;
    }
    if (d == 0 || len == 0 || i >= cg.size() || ops.size() + len > (uint64_t)INT32_MAX) return false;
    uint8_t op;
    switch (cg[i++]) {  // append_cigar's mapping undone
      case '=': op = 'M'; break;
      case 'X': op = 'X'; break;
      case 'D': op = 'I'; break;
      case 'I': op = 'D'; break;
      default: return false;
    }
    ops.insert(ops.end(), (size_t)len, op);
  }
  return true;
}

namespace {
bool parse_size(const std::string& s, size_t& v) {
  if (s.empty() || s.size() > 18 || s.find_first_not_of("0123456789") != std::string::npos) return false;
  v = (size_t)strtoull(s.c_str(), nullptr, 10);
  return true;
}
}  // namespace

namespace {
std::vector<std::string> split_tabs(const std::string& line) {
  std::vector<std::string> f;
  for (size_t b = 0;;) {
    const size_t e = line.find('\t', b);
    f.push_back(line.substr(b, e == std::string::npos ? std::string::npos : e - b));
    if (e == std::string::npos) break;
    b = e + 1;
  }
  return f;
}
}  // namespace

PafRanges parse_paf_ranges(const std::vector<Sequence>& sequences, const std::string& paf_text) {
  PafRanges out;
  std::map<std::string, size_t> by_name;
  for (size_t i = 0; i < sequences.size(); ++i) by_name.emplace(sequences[i].id, i);  // (the first of equal names)
  size_t pos = 0, line_no = 0;
  while (pos < paf_text.size()) {
    size_t nl = paf_text.find('\n', pos);
    if (nl == std::string::npos) nl = paf_text.size();
    std::string line = paf_text.substr(pos, nl - pos);
    pos = nl + 1;
    ++line_no;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const std::vector<std::string> f = split_tabs(line);
    PafRangeLine pl;
    pl.line = line_no;
    size_t qlen, qs, qe, tlen, ts, te;
    if (f.size() < 9 || f[4].size() != 1 || (f[4][0] != '+' && f[4][0] != '-') || !parse_size(f[1], qlen) || !parse_size(f[2], qs) ||
        !parse_size(f[3], qe) || !parse_size(f[6], tlen) || !parse_size(f[7], ts) || !parse_size(f[8], te)) {
      pl.cls = "bad_line";
    } else {
      const auto qi = by_name.find(f[0]), ti = by_name.find(f[5]);
      if (qi == by_name.end() || ti == by_name.end()) pl.cls = "unknown_name";
      else if (qlen != sequences[qi->second].seq.size() || tlen != sequences[ti->second].seq.size()) pl.cls = "length_mismatch";
      else if (qs > qe || qe > qlen || ts > te || te > tlen) pl.cls = "bad_line";  // (numbers that cannot be an interval of the sequence)
      else {
        pl.index = out.ranges.size();
        out.ranges.push_back(AlignmentRange{qi->second, ti->second, f[4][0] == '-', qs, qe, ts, te});
      }
    }
    out.lines.push_back(std::move(pl));
  }
  return out;
}

PafCheckReport check_paf(const std::vector<Sequence>& sequences, const std::string& paf_text, const AlignmentParams& params,
                         bool optimal, int device, bool partial) {
  PafCheckReport rep;
  std::map<std::string, size_t> by_name;
  for (size_t i = 0; i < sequences.size(); ++i) by_name.emplace(sequences[i].id, i);  // (the first of equal names)
  struct Entry {
    size_t failure;  // index into `pending`
    size_t col10, col11, qspan, tspan;
  };
  // every non-empty line gets a slot of `pending` (cls empty: nothing found so far); the device-checked ones also an Entry
  std::vector<PafCheckFailure> pending;
  std::vector<Entry> entries;
  std::vector<awv_pair> ap;
  std::vector<awv_range_pair> rp;  // `partial`: the same entries as interval pairs
  std::vector<awv_result> recs;
  std::vector<uint8_t> arena, ops;
  size_t pos = 0, line_no = 0;
  while (pos < paf_text.size()) {
    size_t nl = paf_text.find('\n', pos);
    if (nl == std::string::npos) nl = paf_text.size();
    std::string line = paf_text.substr(pos, nl - pos);
    pos = nl + 1;
    ++line_no;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    ++rep.lines;
    const std::vector<std::string> f = split_tabs(line);
    PafCheckFailure pf;
    pf.line = line_no;
    if (f.size() > 0) pf.qname = f[0];
    if (f.size() > 5) pf.tname = f[5];
    if (f.size() > 4 && f[4].size() == 1) pf.strand = f[4][0];
    const std::string* cg = nullptr;
    for (size_t k = 12; k < f.size(); ++k)
      if (f[k].compare(0, 5, "cg:Z:") == 0) cg = &f[k];
    size_t qlen, qs, qe, tlen, ts, te, c10, c11;
    if (f.size() < 12 || !cg || (pf.strand != '+' && pf.strand != '-') || !parse_size(f[1], qlen) || !parse_size(f[2], qs) ||
        !parse_size(f[3], qe) || !parse_size(f[6], tlen) || !parse_size(f[7], ts) || !parse_size(f[8], te) || !parse_size(f[9], c10) ||
        !parse_size(f[10], c11)) {
      pf.cls = "bad_line";
      pending.push_back(pf);
      continue;
    }
    const auto qi = by_name.find(pf.qname), ti = by_name.find(pf.tname);
    if (qi == by_name.end() || ti == by_name.end()) {
      pf.cls = "unknown_name";
    } else if (qlen != sequences[qi->second].seq.size() || tlen != sequences[ti->second].seq.size()) {
      pf.cls = "length_mismatch";
    } else if (cg->size() == 5 && qs == 0 && qe == 0 && ts == 0 && te == 0) {
      ++rep.skipped;  // the empty record a failed pair leaves
      continue;
    } else if ((qs != 0 || ts != 0 || qe != qlen || te != tlen) && !(partial && qs <= qe && qe <= qlen && ts <= te && te <= tlen)) {
      pf.cls = "not_end_to_end";
    } else if (!cigar_string_to_bytes(cg->substr(5), ops)) {
      pf.cls = "bad_cigar";
    }
    if (!pf.cls.empty()) {
      pending.push_back(pf);
      continue;
    }
    awv_result r{};
    r.status = AWV_ST_COMPLETED;
    r.cigar_off = arena.size();
    r.cigar_len = (uint32_t)ops.size();
    int64_t nx = 0, ni = 0, nd = 0;
    for (uint8_t op : ops) {
      nx += op == 'X';
      ni += op == 'I';
      nd += op == 'D';
    }
    r.num_matches = (int32_t)std::min<size_t>(c10, INT32_MAX);  // the line's claim; the other counts are the string's own
    r.num_mismatches = (int32_t)nx;
    r.num_ins = (int32_t)ni;
    r.num_del = (int32_t)nd;
    r.q_end = (int32_t)(qe - qs);  // (consumed lengths: the whole sequences' for an end-to-end line)
    r.t_end = (int32_t)(te - ts);
    arena.insert(arena.end(), ops.begin(), ops.end());
    ap.push_back(awv_pair{(int32_t)qi->second, (int32_t)ti->second, pf.strand == '-' ? 1 : 0});
    if (partial) rp.push_back(awv_range_pair{ap.back().q_idx, ap.back().t_idx, ap.back().q_revcomp, (int32_t)qs, (int32_t)qe, (int32_t)ts, (int32_t)te});
    recs.push_back(r);
    entries.push_back(Entry{pending.size(), c10, c11, qe - qs, te - ts});
    pending.push_back(pf);
  }
  rep.checked = entries.size();
  if (!entries.empty()) {
    const awv_penalties pen = to_penalties(params);
    std::unique_lock<std::mutex> lock(*slot_mutex(device, 0));
    awv_engine* e = slot_engine(device, 0, 1);
    upload(e, sequences);
    std::vector<awv_verify_result> vr(entries.size());
    arena.resize(arena.size() + 16);  // (never an empty arena)
    if ((partial ? awv_verify_ranges(e, &pen, rp.data(), (int64_t)rp.size(), recs.data(), arena.data(), arena.size(), vr.data())
                 : awv_verify_cigars(e, &pen, ap.data(), (int64_t)ap.size(), recs.data(), arena.data(), arena.size(), vr.data())) != AWV_OK)
      throw AlignmentError(std::string("verify_cigars: ") + awv_last_error());
    awv_engine_verify_stats(e, &rep.stats);
    std::vector<awv_score_result> sr;
    if (optimal) {
      sr.resize(entries.size());
      if ((partial ? awv_score_ranges(e, &pen, rp.data(), (int64_t)rp.size(), nullptr, sr.data())
                   : awv_score_pairs(e, &pen, ap.data(), (int64_t)ap.size(), -1, sr.data())) != AWV_OK)
        throw AlignmentError(std::string("score_pairs: ") + awv_last_error());
    }
    for (size_t k = 0; k < entries.size(); ++k) {
      PafCheckFailure& pf = pending[entries[k].failure];
      const awv_verify_result& v = vr[k];
      pf.column = v.column;
      pf.penalty = v.penalty;
      // (the record carries no penalty: AWV_VF_PENALTY, the last check in order, means every other one passed)
      const bool valid = v.code == AWV_VF_OK || v.code == AWV_VF_PENALTY;
      if (!valid) pf.cls = verify_code_name(v.code);
      else if (entries[k].col11 != std::max(entries[k].qspan, entries[k].tspan)) pf.cls = "counts";
      if (optimal && valid && sr[k].status == AWV_ST_COMPLETED) {
        pf.optimum = sr[k].penalty;
        if (pf.cls.empty() && v.penalty > pf.optimum) pf.cls = "not_optimal";
        if (pf.cls.empty() && v.penalty < pf.optimum) pf.cls = "below_optimum";
      }
    }
  }
  for (auto& pf : pending)
    if (!pf.cls.empty()) rep.failures.push_back(std::move(pf));
  return rep;
}

std::string format_paf_check(const PafCheckReport& r) {
  std::string out;
  for (const PafCheckFailure& f : r.failures) {
    out += std::to_string(f.line) + '\t' + f.qname + '\t' + f.tname + '\t' + f.strand + '\t' + f.cls + '\t' + std::to_string(f.column) +
           '\t' + std::to_string(f.penalty);
    if (f.optimum >= 0) out += '\t' + std::to_string(f.optimum);
    out.push_back('\n');
  }
  return out;
}

// ---- wfa.rs ---------------------------------------------------------------------------------
namespace wfa {

std::string validate_cigar_alignment(const uint8_t* cigar, size_t n, size_t query_len, size_t reference_len) {
  size_t q = 0, r = 0;
  char buf[160];
  for (size_t i = 0; i < n; ++i) {
    const uint8_t op = cigar[i];
    if (op == 'M' || op == '=' || op == 'X') {
      if (q >= query_len || r >= reference_len) {
        snprintf(buf, sizeof(buf), "CIGAR extends beyond sequences at M/=/X op: q_pos=%zu, r_pos=%zu, query_len=%zu, ref_len=%zu",
                 q, r, query_len, reference_len);
        return buf;
      }
      ++q; ++r;
    } else if (op == 'I') {  // WFA2: I consumes the reference
      if (r >= reference_len) {
        snprintf(buf, sizeof(buf), "CIGAR extends beyond reference at I op: r_pos=%zu, ref_len=%zu", r, reference_len);
        return buf;
      }
      ++r;
    } else if (op == 'D') {  // WFA2: D consumes the query
      if (q >= query_len) {
        snprintf(buf, sizeof(buf), "CIGAR extends beyond query at D op: q_pos=%zu, query_len=%zu", q, query_len);
        return buf;
      }
      ++q;
    } else {
      snprintf(buf, sizeof(buf), "Invalid CIGAR operation: %c (0x%02x)", (char)op, op);
      return buf;
    }
  }
  if (q != query_len) { snprintf(buf, sizeof(buf), "CIGAR doesn't cover full query: %zu vs %zu", q, query_len); return buf; }
  if (r != reference_len) { snprintf(buf, sizeof(buf), "CIGAR doesn't cover full reference: %zu vs %zu", r, reference_len); return buf; }
  return "";
}

AlignmentResult align_sequences(const std::vector<uint8_t>& pattern, const std::vector<uint8_t>& text,
                                const Penalties& p, AlignmentMode mode, int device) {
  awv_penalties q{};
  q.match = 0;
  q.mismatch = p.mismatch;
  switch (mode) {  // wfa.rs:185-218
    case AlignmentMode::EditDistance: q.gap_open1 = p.mismatch; q.gap_ext1 = p.mismatch; break;
    case AlignmentMode::SinglePieceAffine: q.gap_open1 = p.gap_opening1; q.gap_ext1 = p.gap_extension1; break;
    case AlignmentMode::TwoPieceAffine:
      q.gap_open1 = p.gap_opening1; q.gap_ext1 = p.gap_extension1;
      q.gap_open2 = p.gap_opening2; q.gap_ext2 = p.gap_extension2; q.two_piece = 1;
      break;
  }
  std::lock_guard<std::mutex> slot(*slot_mutex(device, 0));
  awv_engine* e = slot_engine(device, 0, 1);
  std::vector<uint8_t> cig(pattern.size() + text.size() + 1);
  awv_result r{};
  if (awv_align_one(e, &q, pattern.data(), (int32_t)pattern.size(), text.data(), (int32_t)text.size(), &r,
                    cig.data(), cig.size()) != AWV_OK)
    throw AlignmentError(std::string("Alignment failed: ") + awv_last_error());
  if (r.status != AWV_ST_COMPLETED) throw AlignmentError("Alignment failed with status: " + std::to_string(r.status));
  const std::string bad = validate_cigar_alignment(cig.data(), r.cigar_len, pattern.size(), text.size());
  if (!bad.empty()) throw AlignmentError("CIGAR validation failed: " + bad);
  AlignmentResult out;
  out.score = r.score;
  out.cigar = cigar_bytes_to_string(cig.data(), r.cigar_len);
  out.matches = (size_t)r.num_matches;
  out.mismatches = (size_t)r.num_mismatches;
  out.deletions = (size_t)r.num_ins;   // WFA2 'I' means standard 'D' (wfa.rs:94-96)
  out.insertions = (size_t)r.num_del;  // WFA2 'D' means standard 'I'
  out.alignment_length = out.matches + out.mismatches;
  return out;
}

}  // namespace wfa
}  // namespace allwave

namespace allwave {
SparsificationStrategy SparsificationStrategy::parse(const std::string& s) {  // main.rs:136-203
  SparsificationStrategy r;
  auto to_double = [](const std::string& t, const char* msg) {
    size_t used = 0;
    double v = 0;
    try { v = std::stod(t, &used); } catch (...) { throw std::invalid_argument(msg); }
    if (used != t.size() || t.empty()) throw std::invalid_argument(msg);
    return v;
  };
  auto to_usize = [](const std::string& t, const char* msg) {
    if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos) throw std::invalid_argument(msg);
    return (size_t)std::stoull(t);
  };
  if (s == "none") return r;
  if (s == "auto") { r.kind = Auto; return r; }
  if (s.rfind("random:", 0) == 0) {
    r.kind = Random;
    r.value = to_double(s.substr(7), "Invalid random fraction");
    if (r.value <= 0.0 || r.value > 1.0) throw std::invalid_argument("Random fraction must be between 0 and 1");
    return r;
  }
  if (s.rfind("giant:", 0) == 0 || s.rfind("connectivity:", 0) == 0) {
    const bool giant = s[0] == 'g';
    r.kind = Connectivity;
    r.value = to_double(s.substr(giant ? 6 : 13), giant ? "Invalid giant component probability" : "Invalid connectivity probability");
    if (r.value <= 0.0 || r.value >= 1.0)
      throw std::invalid_argument(giant ? "Giant component probability must be between 0 and 1" : "Connectivity probability must be between 0 and 1");
    return r;
  }
  if (s.rfind("tree:", 0) == 0) {
    std::vector<std::string> parts;
    size_t pos = 5;
    while (true) {
      const size_t c = s.find(':', pos);
      parts.push_back(s.substr(pos, c == std::string::npos ? std::string::npos : c - pos));
      if (c == std::string::npos) break;
      pos = c + 1;
    }
    if (parts.size() < 3 || parts.size() > 4)
      throw std::invalid_argument("Invalid tree format. Use: tree:<k_nearest>:<k_farthest>:<random_fraction>[:<kmer_size>]");
    r.kind = TreeSampling;
    r.k_nearest = to_usize(parts[0], "Invalid k nearest count");
    r.k_farthest = to_usize(parts[1], "Invalid k farthest count");
    r.random_fraction = to_double(parts[2], "Invalid random fraction");
    if (r.k_nearest == 0 && r.k_farthest == 0)
      throw std::invalid_argument("At least one of k_nearest or k_farthest must be greater than 0");
    if (!(r.random_fraction >= 0.0 && r.random_fraction <= 1.0)) throw std::invalid_argument("Random fraction must be between 0 and 1");
    if (parts.size() == 4) {
      const size_t k = to_usize(parts[3], "Invalid k-mer size");
      if (k < 3 || k > 31) throw std::invalid_argument("K-mer size must be between 3 and 31");
      r.kmer_size = k;
    }
    return r;
  }
  throw std::invalid_argument("Invalid sparsification strategy. Use: none, auto, giant:<probability>, random:<fraction>, or tree:<near>:<far>:<random>[:<kmer>]");
}
}  // namespace allwave
