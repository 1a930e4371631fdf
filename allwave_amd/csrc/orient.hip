// orient.hip -- WFA orientation from bounded strand scores (awv_orient_pairs, awv_orient_decide; include/allwave_hip.h).
//
// The reference aligns every pair on both strands in full and compares edit counts.  Here a pair's strands race: rounds of
// score-only launches (awv_score_pairs_bounded) over a shrinking list of (pair, strand, bound) entries, and between two
// rounds one small kernel that reads the round's (status, penalty) records, narrows each strand's proved penalty interval,
// applies the rule of orient_device.hpp, writes the pair's decision and compacts the next round's entries:
//   * round 0 scores both strands under awo::first_bound; while neither penalty is known both bounds grow by awo::GROWTH
//     per round (cells at most GROWTH^2 times the round before: the earlier rounds together cost less than a third of the last);
//   * once one strand's penalty is known the other strand is searched once more, under awo::settling_bound -- the smallest
//     bound whose "above" settles the pair -- and never beyond it;
//   * both penalties known and the rule still silent, or a strand that ended neither COMPLETED nor ABOVE_BOUND: ambiguous;
//     so is a pair whose next search would run under a bound above what an unrelated strand is expected to cost
//     (awo::worth_racing: that search would complete instead of settling, and cost what the full alignment costs).
// Ambiguous pairs, and only they, get the reference's two full alignments in one awv_align_pairs call at the end.
// The engine plans every launch on the host (batches, kernel flavours, row widths, re-runs), so a round's entry list comes
// back to the host: per round 8 bytes per entry go up (the score records) and 8 bytes per surviving entry plus two counts
// come down; the per-pair state stays on the device until the race is over.
#include "orient_device.hpp"

#include <algorithm>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "coverage_device.hpp"   // (awv_internal_coverage_paused)
#include "normalize_device.hpp"  // (awv_internal_normalize_mode)
#include "planner_device.hpp"  // (EngineView, awv_internal_view, awv_internal_fail)

namespace awo {

constexpr int DEC_AMBIGUOUS = 3;  // beside AWV_ORIENT_FORWARD / _REVERSE / _UNDECIDED
constexpr int ROUND_WG = 256;

struct RoundParams {
  Rule rule;
  int n_act;
  // this round: active pair k is pair act_pair[k]; its records are res[act_ent[k]...], one per strand in act_mask[k]
  // (bit 0 forward, bit 1 reverse-complement), forward first
  const int32_t* act_pair;
  const int32_t* act_ent;
  const int32_t* act_mask;
  const awv_score_result* res;
  // per-pair state: proved interval [lo, hi] of strand s at [2 i + s], the bound both strands were last searched under,
  // the decision and the rounds taken part in
  int32_t* lo;
  int32_t* hi;
  int32_t* bound;
  const int32_t* base;  // the forced gap's cost: what the bound's slack grows above (awo::grown_bound)
  const int32_t* west;  // awo::wrong_estimate of the pair
  int32_t* decision;
  int32_t* rounds;
  // next round: the same three lists, and per entry its id (2 * pair + strand) and bound; counts[0] pairs, counts[1] entries
  int32_t* nxt_pair;
  int32_t* nxt_ent;
  int32_t* nxt_mask;
  int32_t* ent_id;
  int32_t* ent_bound;
  unsigned int* counts;
};

// what one pair does with its round's records: returns the strands to search next (mask) and their bounds
struct Step {
  int decision;
  int mask;
  int bound[2];
};

__host__ __device__ inline Step step_pair(const Rule& r, int mask, const awv_score_result* rec, int32_t* lo, int32_t* hi, int32_t* bound,
                                          int base, int west) {
  Step st;
  st.mask = 0;
  st.bound[0] = st.bound[1] = 0;
  bool failed = false;
  for (int s = 0, k = 0; s < 2; ++s) {
    if (!((mask >> s) & 1)) continue;
    const awv_score_result x = rec[k++];
    if (x.status == AWV_ST_COMPLETED) lo[s] = hi[s] = x.penalty;
    else if (x.status == AWV_ST_ABOVE_BOUND) lo[s] = x.penalty > lo[s] ? x.penalty : lo[s];  // (penalty: the bound + 1)
    else failed = true;
  }
  if (failed) {
    st.decision = DEC_AMBIGUOUS;
    return st;
  }
  st.decision = decide(r, lo[0], hi[0], lo[1], hi[1]);
  if (st.decision != AWV_ORIENT_UNDECIDED) return st;
  const bool kf = hi[0] != HI_NONE, kr = hi[1] != HI_NONE;
  if (kf && kr) {
    st.decision = DEC_AMBIGUOUS;
  } else if (kf || kr) {  // the other strand once more, to the bound that settles the pair
    const int other = kf ? 1 : 0;
    const int B = settling_bound(r, kr ? 1 : 0, kf ? hi[0] : hi[1]);
    if (B < 0 || B + 1LL <= (long long)lo[other] || B > west) {  // (B > west: that search is expected to complete, not to settle)
      st.decision = DEC_AMBIGUOUS;
    } else {
      st.mask = 1 << other;
      st.bound[other] = B;
    }
  } else if (!worth_racing(r, lo[0] < lo[1] ? lo[0] : lo[1], west)) {
    st.decision = DEC_AMBIGUOUS;
  } else {
    *bound = grown_bound(*bound, base);
    st.mask = 3;
    st.bound[0] = st.bound[1] = *bound;
  }
  return st;
}

__global__ __launch_bounds__(ROUND_WG) void orient_round_kernel(RoundParams p) {
  const int k = blockIdx.x * ROUND_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int pair = 0, nent = 0;
  Step st;
  st.mask = 0;
  if (k < p.n_act) {
    pair = p.act_pair[k];
    int32_t lo[2] = {p.lo[2 * (size_t)pair], p.lo[2 * (size_t)pair + 1]};
    int32_t hi[2] = {p.hi[2 * (size_t)pair], p.hi[2 * (size_t)pair + 1]};
    int32_t b = p.bound[pair];
    st = step_pair(p.rule, p.act_mask[k], p.res + p.act_ent[k], lo, hi, &b, p.base[pair], p.west[pair]);
    p.lo[2 * (size_t)pair] = lo[0];
    p.lo[2 * (size_t)pair + 1] = lo[1];
    p.hi[2 * (size_t)pair] = hi[0];
    p.hi[2 * (size_t)pair + 1] = hi[1];
    p.bound[pair] = b;
    p.decision[pair] = st.decision;
    p.rounds[pair] += 1;
    nent = (st.mask & 1) + (st.mask >> 1);
  }
  // compaction: a wave counts its survivors by ballot, its first lane reserves the wave's share of both lists
  const unsigned long long one = __ballot(nent == 1), two = __ballot(nent == 2);
  const unsigned long long below = lane ? (~0ULL >> (64 - lane)) : 0ULL;
  const int pairs_before = __popcll((one | two) & below);
  const int ents_before = __popcll(one & below) + 2 * __popcll(two & below);
  unsigned int base_pair = 0, base_ent = 0;
  if (lane == 0 && (one | two)) {
    base_pair = atomicAdd(&p.counts[0], (unsigned)__popcll(one | two));
    base_ent = atomicAdd(&p.counts[1], (unsigned)(__popcll(one) + 2 * __popcll(two)));
  }
  base_pair = __shfl(base_pair, 0);
  base_ent = __shfl(base_ent, 0);
  if (nent > 0) {
    const unsigned at = base_pair + pairs_before;
    unsigned en = base_ent + ents_before;
    p.nxt_pair[at] = pair;
    p.nxt_ent[at] = (int32_t)en;
    p.nxt_mask[at] = st.mask;
    for (int s = 0; s < 2; ++s) {
      if (!((st.mask >> s) & 1)) continue;
      p.ent_id[en] = 2 * pair + s;
      p.ent_bound[en] = st.bound[s];
      ++en;
    }
  }
}

}  // namespace awo

namespace {

// device allocations of one call, freed whichever way it ends
struct Scratch {
  std::vector<void*> blocks;
  ~Scratch() {
    for (void* b : blocks) (void)hipFree(b);
  }
  template <typename T>
  hipError_t get(T** out, size_t n) {
    void* q = nullptr;
    const hipError_t err = hipMalloc(&q, (n ? n : 1) * sizeof(T));
    if (err == hipSuccess) blocks.push_back(q);
    *out = (T*)q;
    return err;
  }
};

void add_stats(awv_stats& acc, const awv_stats& x) {
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
  if (x.scratch_bytes) acc.scratch_bytes = x.scratch_bytes;
  for (int i = 0; i < 14; ++i) acc.prof[i] += x.prof[i];
  acc.restarts += x.restarts;
  acc.multi_cell_steps += x.multi_cell_steps;
  for (int i = 0; i < 4; ++i) acc.windows[i] += x.windows[i];
  acc.clock_cycles += x.clock_cycles;
  acc.clock_ticks += x.clock_ticks;
  if (x.clock_tick_khz) acc.clock_tick_khz = x.clock_tick_khz;
  acc.deep_cell_steps += x.deep_cell_steps;
}

int rule_of(const awv_penalties* pen, awo::Rule& r) {
  if (!pen) return awv_internal_fail(AWV_ERR_ARG, "penalties: null");
  if (pen->match != 0) return awv_internal_fail(AWV_ERR_PENALTIES, "match score must be 0 (WFA2 penalty transformation is out of scope)");
  if (pen->mismatch <= 0 || pen->gap_open1 < 0 || pen->gap_ext1 <= 0) return awv_internal_fail(AWV_ERR_PENALTIES, "need x > 0, o >= 0, e > 0");
  if (pen->two_piece && (pen->gap_open2 < 0 || pen->gap_ext2 <= 0)) return awv_internal_fail(AWV_ERR_PENALTIES, "need o2 >= 0, e2 > 0");
  r = awo::make_rule(pen->mismatch, pen->gap_open1, pen->gap_ext1, pen->two_piece ? 1 : 0, pen->gap_open2, pen->gap_ext2);
  return AWV_OK;
}

// the race over pairs[0, n): decision (AWV_ORIENT_* or DEC_AMBIGUOUS), intervals and rounds of every pair
int race(awv_engine* e, const awp::EngineView& v, const awv_penalties* pen, const awo::Rule& rule, const awv_pair* pairs, int64_t n,
         std::vector<int32_t>& decision, std::vector<int32_t>& lo, std::vector<int32_t>& hi, std::vector<int32_t>& rounds, awv_stats& total) {
  using namespace awo;
  Scratch sc;
  int32_t *d_act[2][3], *d_lo, *d_hi, *d_bound, *d_base, *d_west, *d_dec, *d_rounds, *d_ent_id, *d_ent_bound;
  awv_score_result* d_res;
  unsigned int* d_counts;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 3; ++b) AWV_TRY(sc.get(&d_act[a][b], (size_t)n));
  AWV_TRY(sc.get(&d_lo, (size_t)2 * n));
  AWV_TRY(sc.get(&d_hi, (size_t)2 * n));
  AWV_TRY(sc.get(&d_bound, (size_t)n));
  AWV_TRY(sc.get(&d_base, (size_t)n));
  AWV_TRY(sc.get(&d_west, (size_t)n));
  AWV_TRY(sc.get(&d_dec, (size_t)n));
  AWV_TRY(sc.get(&d_rounds, (size_t)n));
  AWV_TRY(sc.get(&d_ent_id, (size_t)2 * n));
  AWV_TRY(sc.get(&d_ent_bound, (size_t)2 * n));
  AWV_TRY(sc.get(&d_res, (size_t)2 * n));
  AWV_TRY(sc.get(&d_counts, 2));
  // round 0: both strands under the first bound, of every pair worth racing (the others stay undecided: the caller aligns
  // them in full)
  std::vector<int32_t> h_pair, h_ent, h_mask, h_bound((size_t)n, 0), h_base((size_t)n, 0), h_west((size_t)n, 0);
  std::vector<int32_t> ent_id((size_t)2 * n), ent_bound((size_t)2 * n);
  int64_t n_act = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int plen = v.len_host[pairs[i].q_idx], tlen = v.len_host[pairs[i].t_idx];
    const int G = (int32_t)std::min<long long>(gap_cost(*pen, plen > tlen ? plen - tlen : tlen - plen), INT32_MAX);
    const int W = wrong_estimate(*pen, plen, tlen);
    if (!worth_racing(rule, G, W)) continue;
    const int B = first_bound(rule, *pen, plen, tlen);
    h_bound[(size_t)i] = B;
    h_base[(size_t)i] = G;
    h_west[(size_t)i] = W;
    h_pair.push_back((int32_t)i);
    h_ent.push_back((int32_t)(2 * n_act));
    h_mask.push_back(3);
    ent_id[(size_t)2 * n_act] = (int32_t)(2 * i);
    ent_id[(size_t)2 * n_act + 1] = (int32_t)(2 * i + 1);
    ent_bound[(size_t)2 * n_act] = ent_bound[(size_t)2 * n_act + 1] = B;
    ++n_act;
  }
  if (n_act > 0) {
    AWV_TRY(hipMemcpyAsync(d_act[0][0], h_pair.data(), (size_t)n_act * 4, hipMemcpyHostToDevice, v.stream));
    AWV_TRY(hipMemcpyAsync(d_act[0][1], h_ent.data(), (size_t)n_act * 4, hipMemcpyHostToDevice, v.stream));
    AWV_TRY(hipMemcpyAsync(d_act[0][2], h_mask.data(), (size_t)n_act * 4, hipMemcpyHostToDevice, v.stream));
  }
  AWV_TRY(hipMemcpyAsync(d_bound, h_bound.data(), (size_t)n * 4, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(d_base, h_base.data(), (size_t)n * 4, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(d_west, h_west.data(), (size_t)n * 4, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemsetAsync(d_lo, 0, (size_t)2 * n * 4, v.stream));
  AWV_TRY(hipMemsetD32Async((hipDeviceptr_t)d_hi, HI_NONE, (size_t)2 * n, v.stream));
  AWV_TRY(hipMemsetD32Async((hipDeviceptr_t)d_dec, AWV_ORIENT_UNDECIDED, (size_t)n, v.stream));
  AWV_TRY(hipMemsetAsync(d_rounds, 0, (size_t)n * 4, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  int64_t n_ent = 2 * n_act;
  std::vector<awv_pair> ep;
  std::vector<awv_score_result> res;
  for (int cur = 0; n_ent > 0; cur ^= 1) {
    ep.resize((size_t)n_ent);
    res.resize((size_t)n_ent);
    for (int64_t k = 0; k < n_ent; ++k) {
      const awv_pair& src = pairs[ent_id[(size_t)k] >> 1];
      ep[(size_t)k] = awv_pair{src.q_idx, src.t_idx, ent_id[(size_t)k] & 1};
    }
    if (int rc = awv_score_pairs_bounded(e, pen, ep.data(), n_ent, ent_bound.data(), res.data())) return rc;
    awv_stats st{};
    awv_engine_stats(e, &st);
    add_stats(total, st);
    AWV_TRY(hipMemcpyAsync(d_res, res.data(), (size_t)n_ent * sizeof(awv_score_result), hipMemcpyHostToDevice, v.stream));
    AWV_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned int), v.stream));
    RoundParams rp{};
    rp.rule = rule;
    rp.n_act = (int)n_act;
    rp.act_pair = d_act[cur][0];
    rp.act_ent = d_act[cur][1];
    rp.act_mask = d_act[cur][2];
    rp.res = d_res;
    rp.lo = d_lo;
    rp.hi = d_hi;
    rp.bound = d_bound;
    rp.base = d_base;
    rp.west = d_west;
    rp.decision = d_dec;
    rp.rounds = d_rounds;
    rp.nxt_pair = d_act[cur ^ 1][0];
    rp.nxt_ent = d_act[cur ^ 1][1];
    rp.nxt_mask = d_act[cur ^ 1][2];
    rp.ent_id = d_ent_id;
    rp.ent_bound = d_ent_bound;
    rp.counts = d_counts;
    hipLaunchKernelGGL(orient_round_kernel, dim3((unsigned)((n_act + ROUND_WG - 1) / ROUND_WG)), dim3(ROUND_WG), 0, v.stream, rp);
    AWV_TRY(hipGetLastError());
    unsigned int counts[2] = {0, 0};
    AWV_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
    if ((int64_t)counts[0] > n_act || (int64_t)counts[1] > 2 * (int64_t)counts[0])
      return awv_internal_fail(AWV_ERR_HIP, "orient_pairs: inconsistent round counts");
    n_act = counts[0];
    n_ent = counts[1];
    if (n_ent > 0) {
      AWV_TRY(hipMemcpyAsync(ent_id.data(), d_ent_id, (size_t)n_ent * 4, hipMemcpyDeviceToHost, v.stream));
      AWV_TRY(hipMemcpyAsync(ent_bound.data(), d_ent_bound, (size_t)n_ent * 4, hipMemcpyDeviceToHost, v.stream));
      AWV_TRY(hipStreamSynchronize(v.stream));
    }
  }
  decision.resize((size_t)n);
  rounds.resize((size_t)n);
  lo.resize((size_t)2 * n);
  hi.resize((size_t)2 * n);
  AWV_TRY(hipMemcpyAsync(decision.data(), d_dec, (size_t)n * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipMemcpyAsync(rounds.data(), d_rounds, (size_t)n * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipMemcpyAsync(lo.data(), d_lo, (size_t)2 * n * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipMemcpyAsync(hi.data(), d_hi, (size_t)2 * n * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

int orient_core(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t n, int32_t flags, awv_orient_result* out) {
  awo::Rule rule;
  if (int rc = rule_of(pen, rule)) return rc;
  awp::EngineView v;
  if (int rc = awv_internal_view(e, &v)) return n == 0 && rc == AWV_ERR_STATE ? AWV_OK : rc;
  if (n >= (int64_t)1 << 29) return awv_internal_fail(AWV_ERR_ARG, "orient_pairs: too many pairs for one call");
  for (int64_t i = 0; i < n; ++i)
    if (pairs[i].q_idx < 0 || pairs[i].q_idx >= v.n || pairs[i].t_idx < 0 || pairs[i].t_idx >= v.n)
      return awv_internal_fail(AWV_ERR_ARG, "orient_pairs: sequence index out of range");
  AWV_TRY(hipSetDevice(v.device));
  awv_stats total{};
  std::vector<int32_t> decision, lo, hi, rounds;
  const bool raced = n > 0 && !(flags & AWV_ORIENT_FULL) && awo::race_pays(rule);
  if (raced) {
    if (int rc = race(e, v, pen, rule, pairs, n, decision, lo, hi, rounds, total)) return rc;
  }
  std::vector<int64_t> tail;
  for (int64_t i = 0; i < n; ++i) {
    awv_orient_result& o = out[i];
    o = awv_orient_result{};
    o.how = AWV_ORIENT_BY_BOUND;
    o.lo_f = raced ? lo[(size_t)2 * i] : 0;
    o.hi_f = raced ? hi[(size_t)2 * i] : awo::HI_NONE;
    o.lo_r = raced ? lo[(size_t)2 * i + 1] : 0;
    o.hi_r = raced ? hi[(size_t)2 * i + 1] : awo::HI_NONE;
    o.edits_f = o.edits_r = AWV_ORIENT_NO_EDITS;
    o.rounds = raced ? rounds[(size_t)i] : 0;
    const int d = raced ? decision[(size_t)i] : awo::DEC_AMBIGUOUS;  // (undecided: a pair the race left out)
    if (d == AWV_ORIENT_FORWARD || d == AWV_ORIENT_REVERSE) o.is_reverse = d == AWV_ORIENT_REVERSE;
    else tail.push_back(i);
  }
  if (!tail.empty()) {  // determine_orientation_wfa as it stands: both strands in full, fewer edits win, forward wins ties
    const int64_t m = (int64_t)tail.size();
    std::vector<awv_pair> op((size_t)2 * m);
    for (int64_t j = 0; j < m; ++j) {
      op[(size_t)2 * j] = awv_pair{pairs[tail[(size_t)j]].q_idx, pairs[tail[(size_t)j]].t_idx, 0};
      op[(size_t)2 * j + 1] = awv_pair{pairs[tail[(size_t)j]].q_idx, pairs[tail[(size_t)j]].t_idx, 1};
    }
    std::vector<awv_result> orr((size_t)2 * m);
    int32_t& norm_mode = awv_internal_normalize_mode(e);  // orientation ignores the engine's normalize mode: edit counts do not move
    const int32_t saved_mode = norm_mode;
    norm_mode = AWV_NORM_OFF;
    bool& cov_paused = awv_internal_coverage_paused(e);  // nor do these strand alignments count towards the depth: only final ones do
    const bool saved_paused = cov_paused;
    cov_paused = true;
    const int arc = awv_align_pairs(e, pen, op.data(), 2 * m, orr.data(), nullptr, nullptr);
    cov_paused = saved_paused;
    norm_mode = saved_mode;
    if (arc) return arc;
    awv_stats st{};
    awv_engine_stats(e, &st);
    add_stats(total, st);
    for (int64_t j = 0; j < m; ++j) {
      awv_orient_result& o = out[tail[(size_t)j]];
      const awv_result& f = orr[(size_t)2 * j];
      const awv_result& r = orr[(size_t)2 * j + 1];
      auto dist = [](const awv_result& x) -> uint64_t {
        return x.status == AWV_ST_COMPLETED ? (uint64_t)x.num_mismatches + (uint64_t)x.num_ins + (uint64_t)x.num_del : AWV_ORIENT_NO_EDITS;
      };
      o.how = AWV_ORIENT_BY_EDITS;
      o.edits_f = dist(f);
      o.edits_r = dist(r);
      o.is_reverse = o.edits_f <= o.edits_r ? 0 : 1;
      if (f.status == AWV_ST_COMPLETED) o.lo_f = o.hi_f = f.penalty;
      if (r.status == AWV_ST_COMPLETED) o.lo_r = o.hi_r = r.penalty;
    }
  }
  awv_internal_set_stats(e, &total);
  return AWV_OK;
}

}  // namespace

extern "C" {

int awv_orient_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, int32_t flags,
                     awv_orient_result* out) {
  if (!e) return awv_internal_null_engine();
  if (npairs < 0 || (npairs > 0 && (!pairs || !out))) return awv_internal_fail(AWV_ERR_ARG, "orient_pairs: null pairs or out");
  if (flags & ~AWV_ORIENT_FULL) return awv_internal_fail(AWV_ERR_ARG, "orient_pairs: unknown flag");
  AWV_GUARDED(return orient_core(e, pen, pairs, npairs, flags, out);)
}

int awv_orient_decide(const awv_penalties* pen, int32_t lo_f, int32_t hi_f, int32_t lo_r, int32_t hi_r) {
  awo::Rule rule;
  if (int rc = rule_of(pen, rule)) return rc;
  if (lo_f < 0 || lo_r < 0 || hi_f < lo_f || hi_r < lo_r) return awv_internal_fail(AWV_ERR_ARG, "orient_decide: need 0 <= lo <= hi");
  return awo::decide(rule, lo_f, hi_f, lo_r, hi_r);
}

int32_t awv_orient_settling_bound(const awv_penalties* pen, int32_t known_is_reverse, int32_t penalty) {
  awo::Rule rule;
  if (rule_of(pen, rule) != AWV_OK) return INT32_MIN;
  if (penalty < 0) {
    (void)awv_internal_fail(AWV_ERR_ARG, "orient_settling_bound: penalty < 0");
    return INT32_MIN;
  }
  return awo::settling_bound(rule, known_is_reverse ? 1 : 0, penalty);
}

}  // extern "C"
