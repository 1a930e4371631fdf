// batch_plan.hpp -- the routing rules of an aligning call: what a penalty set lets the kernels do, how a
// pair list is carved into batches, in which order a batch is dispatched, which kernel flavour and row width each pair
// gets, and how wide a group's rows, arenas and LDS regions are.
//
// Plain C++ with no HIP types and no engine state, so that it can be built and tested on its own (tests/batch_plan_driver.cpp):
// everything here depends on lengths, flags and numbers alone.  The device's constants come in through `Limits`, which
// engine.hip fills once from biwfa_device.hpp; engine.hip consumes the plans stage by stage and owns every device call.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "allwave_hip.h"

namespace awvb {

struct Limits {  // biwfa_device.hpp
  int tmax, tmax32, chain_max, max_ring, max_scope, ncomp, col_pad, fallback_min_score, fallback_min_length, waves_per_simd,
      static_lds_reserve;
  size_t ev_stack_words, ev_twin_words;            // uint32 words behind a workgroup's events: the DFS stack; a twin search's last-hit table
  size_t row_meta, row_meta16, breakpoint;         // sizeof(RowMeta), sizeof(RowMeta16), sizeof(Breakpoint)
};

struct Config {  // what the plans read of an engine
  int32_t flags = 0;  // AWV_F_*
  int num_cus = 0;
  int workgroups = 0;             // awv_engine_config: 0 = fill the machine
  int64_t max_scratch_bytes = 0;  // 0 = 160 GiB
  int first_row_cols = 0;         // 0 = the rules below
};

// ---- penalties ----------------------------------------------------------------------------------------------------------
struct PenaltyPlan {
  int code = AWV_OK;  // or the rejection, with its message
  std::string message;
  bool late = false;  // a rejection the engine reports only after the call's pairs have been checked (ring, base-case history)
  int x = 0, o1 = 0, e1 = 0, o2 = 0, e2 = 0, two_piece = 0, scope = 0;  // DevPenalties; scope = max(x, o1+e1, o2+e2) + 1
  int multi_T = 0, chain_max = 1, ring = 4, sb_cap = 0, wb_cap = 0;
  PenaltyPlan& reject(int c, const std::string& m, bool is_late) {
    code = c;
    message = m;
    late = is_late;
    return *this;
  }
};

// what makes a penalty set meaningful at all (the verify check re-scores under any such set)
inline int check_signs(const awv_penalties* p, std::string& msg) {
  if (!p) return msg = "penalties: null", AWV_ERR_ARG;
  if (p->match != 0) return msg = "match score must be 0 (WFA2 penalty transformation is out of scope)", AWV_ERR_PENALTIES;
  if (p->mismatch <= 0 || p->gap_open1 < 0 || p->gap_ext1 <= 0) return msg = "need x > 0, o >= 0, e > 0", AWV_ERR_PENALTIES;
  if (p->two_piece && (p->gap_open2 < 0 || p->gap_ext2 <= 0)) return msg = "need o2 >= 0, e2 > 0", AWV_ERR_PENALTIES;
  return AWV_OK;
}

// worst-case penalty of an end-to-end alignment of two sequences of length <= n
inline long long worst_case_penalty(const PenaltyPlan& d, long long n) {
  auto gap = [&](long long l) {
    long long g = d.o1 + l * d.e1;
    if (d.two_piece) g = std::min(g, (long long)d.o2 + l * d.e2);
    return g;
  };
  return std::min(2 * gap(n), n * (long long)d.x + gap(n));
}

// and what the alignment kernels can run under it: the score ring holds max(x, o1 + e1, o2 + e2) + 1 rows
inline PenaltyPlan plan_penalties(const Limits& L, const awv_penalties* p, int32_t flags) {
  PenaltyPlan d;
  std::string msg;
  if (int rc = check_signs(p, msg)) return d.reject(rc, msg, false);
  d.x = p->mismatch;
  d.o1 = p->gap_open1;
  d.e1 = p->gap_ext1;
  d.two_piece = p->two_piece ? 1 : 0;
  d.o2 = d.two_piece ? p->gap_open2 : p->gap_open1;
  d.e2 = d.two_piece ? p->gap_ext2 : p->gap_ext1;
  int scope = std::max(d.x, d.o1 + d.e1);
  if (d.two_piece) scope = std::max(scope, d.o2 + d.e2);
  d.scope = scope + 1;
  if (d.scope > L.max_scope) return d.reject(AWV_ERR_PENALTIES, "penalties too large: max(x, o1+e1, o2+e2) must be < 126", false);
  // multi-step passes (biwfa_device.hpp, compute_rows_multi): T steps per pass, T <= the nearest M source
  // (so that every M row a pass reads was written by an earlier pass); instantiated for the I/D depths
  // of the reference's presets (2-piece: e1 = 2 / e2 = 1; gap-affine: e = 1 or 2)
  d.multi_T = std::min(std::min(d.x, d.o1 + d.e1), L.tmax);
  if (d.two_piece) d.multi_T = std::min(d.multi_T, d.o2 + d.e2);
  if (d.two_piece ? (d.e1 != 2 || d.e2 != 1) : (d.e1 != 1 && d.e1 != 2)) d.multi_T = 0;
  if (d.multi_T < 2 || (flags & AWV_F_SINGLE_STEP)) d.multi_T = 0;
  // chained sweeps (compute_rows_multi, CHAIN): the previous one / two sweeps' M rows are this sweep's sources 5 and 10
  // scores back -- only with x = TMAX and o1 + e1 = 2 TMAX (the default scores); the third source must still come from
  // earlier passes: TMAX * chain_max <= o2 + e2
  if (d.multi_T == L.tmax && d.two_piece && d.x == L.tmax && d.o1 + d.e1 == 2 * L.tmax && !(flags & AWV_F_NO_CHAIN))
    d.chain_max = std::max(1, std::min(L.chain_max, (d.o2 + d.e2) / L.tmax));
  while (d.ring < d.scope + 2 + (d.multi_T > 0 ? d.multi_T * d.chain_max - 1 : 0)) d.ring *= 2;
  if (d.ring > L.max_ring) return d.reject(AWV_ERR_PENALTIES, "ring of " + std::to_string(d.ring) + " rows exceeds MAX_RING", true);  // (unreachable: MAX_SCOPE)
  // base-case capacities: score_remaining <= 250 or both lengths <= 100
  // A sub-problem that ends in an indel component pays that gap's open on top of the
  // score_remaining its parent hands down (the reverse aligner starts with the open pre-paid).
  const long long sb = std::max<long long>(L.fallback_min_score + std::max(d.o1, d.o2), worst_case_penalty(d, L.fallback_min_length));
  d.sb_cap = (int)std::min<long long>(sb, INT_MAX);
  if (sb > 4000) return d.reject(AWV_ERR_PENALTIES, "penalties too large for the base-case history", true);
  d.wb_cap = ((2 * d.sb_cap + 9 + 2 * L.col_pad) + 63) & ~63;
  return d;
}

// ---- entries, carving, dispatch order -----------------------------------------------------------------------------------
// One pair of a batch.  batch_index is its slot in the batch's caller-order results; the entries are permuted, filtered and
// grouped as whole structs and split into the device's arrays only at upload.
struct Entry {
  int32_t q, t, rc;
  int32_t ql, tl;  // the (pattern, text) lengths it is aligned over: a range call's are its rectangle's
  uint64_t off;    // of its CIGAR in the batch's arena
  int64_t batch_index;
};

// What orders and routes pairs: the work of a pair grows with the square of its score, estimated from the lengths and the gap
// a length difference forces.
inline uint64_t pair_cost(int ql, int tl) { return (uint64_t)((int64_t)ql + tl + 4 * std::llabs((int64_t)ql - tl)); }

struct Carve {
  int64_t n = 0;
  uint64_t arena = 0;  // bytes of CIGAR arena: every pair owns ql + tl bytes rounded up to 8 (none in a score-only call)
};
// The batch that starts at pair `first` of the call: pairs in order while they are at most max_batch and their arena stays
// within max_arena (a batch of one pair may exceed it).  lens(i, ql, tl) gives pair i's lengths; `out` gets the entries'
// ql, tl, off and batch_index.
template <typename Lens>
Carve carve_batch(Lens&& lens, int64_t first, int64_t npairs, int64_t max_batch, uint64_t max_arena, bool score_only, std::vector<Entry>& out) {
  Carve c;
  out.clear();
  while (first + c.n < npairs && c.n < max_batch) {
    Entry en{};
    lens(first + c.n, en.ql, en.tl);
    const uint64_t need = score_only ? 0 : ((uint64_t)en.ql + (uint64_t)en.tl + 7) & ~(uint64_t)7;
    if (c.n > 0 && c.arena + need > max_arena) break;
    en.off = c.arena;
    en.batch_index = c.n;
    out.push_back(en);
    c.arena += need;
    ++c.n;
  }
  return c;
}

// Dispatch order: workgroups take pairs from a shared cursor, so the most expensive pairs go first
// (longest-processing-time-first).  Stable, so equal costs keep caller order and a uniform batch is left as it is.
// Returns `skewed`: the most expensive pair costs at least three times the median one.
inline bool order_by_cost(std::vector<Entry>& en) {
  const size_t n = en.size();
  std::vector<uint64_t> cost(n);
  bool uniform = true;
  for (size_t i = 0; i < n; ++i) {
    cost[i] = pair_cost(en[i].ql, en[i].tl);
    uniform = uniform && cost[i] == cost[0];
  }
  if (uniform) return false;
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
  std::vector<Entry> sorted(n);
  for (size_t i = 0; i < n; ++i) sorted[i] = en[order[i]];
  en.swap(sorted);
  return cost[order[0]] >= 3 * cost[order[n / 2]];
}

// ---- groups -------------------------------------------------------------------------------------------------------------
// One group = one kernel flavour x one row width: group = flavour (0 one wave per pair, 1 four, 2 sixteen) * 3 + row width
// (0: 16-bit rows, 1: 32-bit rows, 2: 16-bit rows holding min(h, v) with 32-bit row metadata).
constexpr int NG = 9;
inline int waves_of(int g) { return g / 3 == 0 ? 1 : g / 3 == 1 ? 4 : 16; }
inline int width_of(int g) { return g % 3; }

struct GroupPlan {
  std::vector<uint8_t> group;  // per entry, in dispatch order
  size_t count[NG] = {0};
  int maxsum[NG] = {0};  // the widest ql + tl of a group
  int demand_order[NG];  // all groups, the one with the largest estimated ring demand first
};
// Flavour: all of a small batch goes four waves per pair (latency), and so do pairs of long sequences (rows tens of windows
// wide; measured +17 % on 100 kbp pairs) and pairs a length difference makes expensive -- pair by pair, so that the short
// pairs of a mixed set keep the throughput flavour.  Row width: 16-bit rows when both lengths fit.
// `en` is in dispatch (descending cost) order.  force_sixteen_len (AWV_DEBUG_KNOBS builds): sixteen waves for sequences at least
// that long, INT_MAX otherwise.
inline GroupPlan assign_groups(const Limits& L, const Config& cfg, const std::vector<Entry>& en, bool skewed, int force_sixteen_len) {
  GroupPlan gp;
  const int64_t n = (int64_t)en.size();
  const bool never_wide = (cfg.flags & AWV_F_ONE_WAVE) != 0;
  // (a batch of uneven pairs that fits the machine about once is bound by its longest pairs, not by throughput)
  const bool all_wide = !never_wide && ((cfg.flags & AWV_F_FOUR_WAVES) || n <= (int64_t)(L.waves_per_simd * cfg.num_cus) ||
                                        (skewed && n <= (int64_t)(4 * L.waves_per_simd * cfg.num_cus)));
  // sixteen waves per pair only pay while such pairs are too few to fill the machine four waves at a time
  int64_t n_huge = 0;
  for (const Entry& p : en) n_huge += std::abs(p.ql - p.tl) >= 16384;
  const bool use_sixteen = !never_wide && !(cfg.flags & AWV_F_FOUR_WAVES) && n_huge > 0 && n_huge <= (int64_t)cfg.num_cus;
  const bool force32 = (cfg.flags & AWV_F_FORCE_INT32) != 0;
  const bool no_wide16 = (cfg.flags & AWV_F_NO_WIDE16) != 0;
  std::vector<uint8_t> fl((size_t)n);
  int64_t n_one = 0, n_four = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int ql = en[(size_t)i].ql, tl = en[(size_t)i].tl, dl = std::abs(ql - tl);
    int f = (all_wide || (!never_wide && (dl >= 4096 || std::max(ql, tl) >= 32760))) ? 1 : 0;
    if (use_sixteen && dl >= 16384) f = 2;  // a forced gap that long: rows hundreds of windows wide
    if (std::max(ql, tl) >= force_sixteen_len) f = 2;
    fl[(size_t)i] = (uint8_t)f;
    n_one += f == 0;
    n_four += f == 1;
  }
  // One-wave pairs that cannot fill the machine even once, next to pairs that go four waves anyway, are bound by their
  // most expensive pair on a single wave while most of the machine idles: when their costs are uneven they go four
  // waves too (config 5: 3,315 such pairs, 2.9 s at 61 % of the CUs busy).  (Pairs come in descending cost order.)
  if (!never_wide && n_one > 0 && n_four > 0 && n_one <= (int64_t)(L.waves_per_simd * 256 / 64) * cfg.num_cus) {
    int64_t first_one = -1, seen = 0, median_one = -1;
    for (int64_t i = 0; i < n && median_one < 0; ++i) {
      if (fl[(size_t)i] != 0) continue;
      if (first_one < 0) first_one = i;
      if (seen++ == n_one / 2) median_one = i;
    }
    const Entry &a = en[(size_t)first_one], &b = en[(size_t)median_one];
    if (2 * pair_cost(a.ql, a.tl) >= 3 * pair_cost(b.ql, b.tl))  // (work grows with the square of this length measure: 1.5 x = more than twice the work)
      for (int64_t i = 0; i < n; ++i)
        if (fl[(size_t)i] == 0) fl[(size_t)i] = 1;
  }
  gp.group.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int ql = en[(size_t)i].ql, tl = en[(size_t)i].tl, f = fl[(size_t)i];
    // row width: every stored value must fit 16 bits -- text offsets (both lengths short), or min(h, v) when only
    // the shorter sequence is (the kernels for that exist in the four- and sixteen-wave flavours)
    int w = force32 || std::max(ql, tl) >= 32760 ? 1 : 0;
    if (w == 1 && !force32 && !no_wide16 && f >= 1 && std::min(ql, tl) < 32760) w = 2;
    const int g = f * 3 + w;
    gp.group[(size_t)i] = (uint8_t)g;
    ++gp.count[g];
    gp.maxsum[g] = std::max(gp.maxsum[g], ql + tl);
  }
  // the arenas are sized for the most demanding group first: growing them between two groups would
  // mean a free followed by a large allocation, which the driver can take seconds over
  std::pair<size_t, int> demand[NG];
  for (int g = 0; g < NG; ++g) {
    demand[g] = {0, g};
    if (gp.count[g] == 0) continue;
    const int64_t slots = std::min<int64_t>((L.waves_per_simd * 256 / (64 * waves_of(g))) * cfg.num_cus, (int64_t)gp.count[g]);
    demand[g].first = (size_t)slots * (size_t)gp.maxsum[g] * (width_of(g) == 1 ? 4 : 2);
  }
  std::sort(demand, demand + NG, [](const std::pair<size_t, int>& a, const std::pair<size_t, int>& b) { return a.first > b.first; });
  for (int k = 0; k < NG; ++k) gp.demand_order[k] = demand[k].second;
  return gp;
}

// ---- rows of a group ----------------------------------------------------------------------------------------------------
inline size_t row_elem_bytes(int width) { return width != 1 ? 2 : 4; }
// Row offsets inside a workgroup's ring arena are 32-bit and its buffer descriptor holds at most 2^31 - 1 bytes
// (row_off, make_rsrc in biwfa_device.hpp): a row past 2 GiB would read 0 and lose its writes.  So no attempt, the first
// or a re-run, uses rows wider than wc_2g columns: with 32-bit rows 838,656 at ring 64, 419,328 at ring 128 and 209,664
// at ring 256; with 16-bit rows 1,677,568 at ring 64 and 838,656 at ring 128.
inline int wc_2g(const Limits& L, int ring, int width) {
  return (int)(((size_t)INT32_MAX / ((size_t)2 * L.ncomp * ring * row_elem_bytes(width))) & ~(size_t)255);
}
// A pair whose length difference alone cannot fit such rows ends CAPACITY before any launch (the kernel would find out only
// after a long search).  The two searches meet on one diagonal, and a row of wc columns reaches at most half + COL_PAD - 2
// diagonals beyond its search's origin on either side: find_breakpoint clips its diagonal range to
// half = (wc - 2 COL_PAD - 9 - 256) / 2 on each side, and the capacity test of compute_row keeps 257 / 262 columns at the
// row's ends.  So the searches span at most 2 half + 2 COL_PAD diagonals between them.
inline long long capacity_span(const Limits& L, int wc2g) { return 2 * (((long long)wc2g - 2 * L.col_pad - 9 - 256) / 2) + 2 * L.col_pad; }
inline bool beyond_span(int ql, int tl, long long span) { return ql > 0 && tl > 0 && std::llabs((long long)ql - tl) > span; }

struct RowPlan {
  int waves = 1, width = 0, wg = 64;
  size_t esz = 2;     // bytes per row element
  int ring = 4, ncomp = 5;
  int wc_2g = 0;      // the 2 GiB limit, in columns
  int nslots_g = 0;   // workgroups the group may use
  int wcap_full = 0;  // rows that hold any alignment of the group's widest pair
  int wcap = 0;       // the first attempt's row capacity (columns)
  int wc_last = 0;    // the widest rows a re-run may use
  bool twin_here = false;
  size_t ev_extra = 0;  // uint32 words behind a workgroup's events
  size_t lds_meta = 0, lds_seq = 0, dyn_lds = 0, lds_budget = 0;
  size_t hist_rows = 0, hist_stride = 0;
  size_t budget = 0;  // bytes of scratch all slots may take together
  size_t ring_stride(int wc) const { return (size_t)2 * ncomp * ring * wc * esz; }
  size_t ev_stride(int wc) const { return (size_t)wc + ev_extra; }  // run-length events + the DFS stack
  // per-workgroup arenas as a function of the row capacity
  size_t per_slot(int wc) const { return ring_stride(wc) + hist_stride + ev_stride(wc) * sizeof(uint32_t); }
  // workgroups of an attempt on m pairs: keep the per-workgroup arenas inside the scratch budget
  int slots(int wc, int64_t m) const {
    const int want = (int)std::min<int64_t>(nslots_g, m);
    const size_t fit = std::max<size_t>(1, budget / per_slot(wc));
    return (size_t)want > fit ? (int)fit : want;
  }
  int next_wc(int wc) const { return (int)std::min<long long>(wc_last, 4LL * wc); }  // a re-run's rows
};

// The rows of one group whose pairs (already without those beyond the span) are `en`.  twin_ok: the call allows twin units.
inline RowPlan plan_rows(const Limits& L, const Config& cfg, const PenaltyPlan& pp, const std::vector<Entry>& en, int waves, int width, bool twin_ok) {
  RowPlan r;
  int maxsum = 0, maxlen = 0, maxdelta = 0;
  for (const Entry& p : en) {
    maxsum = std::max(maxsum, p.ql + p.tl);
    maxlen = std::max(maxlen, std::max(p.ql, p.tl));
    maxdelta = std::max(maxdelta, std::abs(p.ql - p.tl));  // (a length difference forces a gap that long: the rows must span it in both directions)
  }
  r.waves = waves;
  r.width = width;
  r.wg = 64 * waves;
  // 16-bit wavefront rows whenever every offset fits (halves the HBM/L2 traffic of the rings): pairs are grouped by row
  // width, so one long sequence does not drag a whole batch to 32-bit rows
  r.esz = row_elem_bytes(width);
  r.ring = pp.ring;
  r.ncomp = L.ncomp;
  r.wc_2g = wc_2g(L, pp.ring, width);
  r.nslots_g = cfg.workgroups > 0 ? std::max(1, cfg.workgroups / waves) : (L.waves_per_simd * 256 / r.wg) * cfg.num_cus;
  r.wcap_full = ((maxsum + 9 + 256 + 2 * L.col_pad) + 255) & ~255;
  const int nslots_want = (int)std::min<int64_t>(r.nslots_g, (int64_t)en.size());
  // twin units only in a group that runs the kernel built with them: one wave per pair, 16-bit rows.  Only
  // there do the LDS metadata (32 B: the twin record) and the event arena (the last-hit table) grow.
  r.twin_here = twin_ok && waves == 1 && width == 0;
  r.ev_extra = L.ev_stack_words + (r.twin_here ? L.ev_twin_words : 0);
  // dynamic LDS = ring metadata (16-bit entries with 16-bit rows; aliased with the base-case table; the last 32 bytes: the
  // swapped pair's breakpoint of a twin search) + staging of the 2-bit packed sequences: what the largest pair needs, within
  // 160 KB / (16 waves per CU) per workgroup; sub-problems that do not fit read global memory instead
  const size_t meta_elem = width == 0 ? L.row_meta16 : L.row_meta;
  r.lds_meta = ((size_t)2 * L.ncomp * pp.ring * meta_elem + (size_t)4 * pp.ring * sizeof(int) + (size_t)pp.scope * L.ncomp * sizeof(int) +
                (r.twin_here ? L.breakpoint : 0) + 15) & ~(size_t)15;
  const size_t seq_need = ((((size_t)maxlen + 15) / 16 + 2) * 2 + 10) * 4;
  r.lds_budget = (size_t)(160 * 1024 / (L.waves_per_simd * 256 / r.wg)) - L.static_lds_reserve;
  r.lds_seq = (cfg.flags & AWV_F_NO_PACKED_SEQ) ? 0 : (r.lds_meta < r.lds_budget ? std::min(seq_need, r.lds_budget - r.lds_meta) : 0);
  r.lds_seq &= ~(size_t)15;
  r.dyn_lds = r.lds_meta + r.lds_seq;
  r.hist_rows = ((size_t)(pp.sb_cap + 1) * L.ncomp * pp.wb_cap * r.esz + 63) & ~(size_t)63;
  r.hist_stride = r.hist_rows + (((size_t)(pp.sb_cap + 1) * L.ncomp * L.row_meta + 63) & ~(size_t)63);
  r.budget = cfg.max_scratch_bytes > 0 ? (size_t)cfg.max_scratch_bytes : (size_t)160 << 30;
  // Row capacity of the first attempt.  A wavefront at score s spans at most ~2 s / min(e) diagonals,
  // far fewer than plen + tlen for similar sequences; when full-width rows would not leave room for
  // every workgroup's arenas (long sequences), start with the widest rows that do and re-run only
  // the pairs whose wavefronts outgrow them (status CAPACITY) with wider rows.
  // Half-width rows (at least 8192 columns) already hold every pair whose optimal score is below
  // about a quarter of plen + tlen; they halve the arenas (allocating -- and the driver clearing --
  // tens of GB is the largest fixed cost of a call) and only unusually divergent pairs are re-run.
  r.wcap = std::min(r.wcap_full, std::max(std::max(8192, (r.wcap_full / 2 + 255) & ~255), (2 * maxdelta + 4096 + 255) & ~255));
  if (r.per_slot(r.wcap) * (size_t)nslots_want > r.budget) {
    const size_t fixed = r.hist_stride + r.ev_extra * sizeof(uint32_t);
    const size_t per_col = (size_t)2 * L.ncomp * pp.ring * r.esz + sizeof(uint32_t);
    const size_t share = r.budget / (size_t)nslots_want;
    long long wc = share > fixed ? (long long)((share - fixed) / per_col) : 0;
    wc = std::max<long long>(wc & ~255LL, 8192);
    r.wcap = (int)std::min<long long>(r.wcap, wc);
  }
  // (diagnostic / test hook: a narrower first attempt, so that the CAPACITY re-run path can be exercised on short sequences)
  if (cfg.first_row_cols > 0) r.wcap = std::min(r.wcap, std::max(2048, (cfg.first_row_cols + 255) & ~255));
  r.wcap = std::min(r.wcap, r.wc_2g);
  r.wc_last = std::min(r.wcap_full, r.wc_2g);
  return r;
}

}  // namespace awvb
