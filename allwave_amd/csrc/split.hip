// split.hip -- alignments split into all their good segments on the device: the per-batch step of awv_align_pairs_split /
// awv_align_ranges_split, awv_split_cigars, awv_split_one_host, the layout helpers and awv_engine_split_stats
// (include/allwave_hip.h).  What "split" means is split_device.hpp; this file walks the same intervals with a wave.
//
// clip.hip's shape: one wave per record, persistent waves taking records (longest op string first) from a cursor.  A record's
// intervals are scanned one after the other by clip_scan.hpp's scan_ops, the clip kernel's chunk loop (64 lanes x 16 op
// bytes), each interval as an op string of its own at cigar_off + lo.  After an interval's clip [b, e) the right remainder
// goes onto the record's stack in device memory and the left one is scanned next; a remainder too short to reach min_score
// with matches alone (a * columns < min_score) is dropped unscanned, which leaves the result as it is.  The stack and every
// decision are uniform across the wave: all lanes store and load the same stack entry, so each lane reads what it wrote
// itself, and the values pass through readfirstlane before they steer a branch.
// Segments are written by lane 0 in the order they are found (an interval's clip before the clips of its remainders); the
// host puts each record's segments into ascending col_beg after the copy-back, before the call hands them on.
// No atomics but the work cursor and the end-of-kernel stats.  All sums are 64-bit, as in clip.hip.
#include "clip_scan.hpp"
#include "split_device.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "range_span.hpp"
#include "record_pass.hpp"  // the host skeleton of a record pass: RecordPass, pack_piece, AWV_TRY

namespace awvs {

struct KParams {
  const awv_result* results;    // cigar_off relative to `arena`
  const int32_t* order;         // dispatch slot -> record
  const uint8_t* arena;         // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  const uint64_t* seg_first;    // npairs + 1, from 0: record i owns seg[seg_first[i] .. seg_first[i + 1]) and
  awv_clip_result* seg;         //   stack[seg_first[i] + i .. seg_first[i + 1] + i + 1)
  Interval* stack;
  awv_split_index* index;
  unsigned long long* counters;  // [0] cursor, [1] records without a segment, [2] columns, [3] segments, [4] columns scanned, [5] records that ran out of slots
  long long npairs;
  long long min_score;
  awv_penalties pen;
  int32_t match_bonus;
};

__device__ __forceinline__ unsigned uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ awv_split_index make_index(int code, int count, long long column) {
  awv_split_index ix;
  ix.code = code;
  ix.count = count;
  ix.column = column;
  return ix;
}

__global__ __launch_bounds__(64) void awv_split_kernel(KParams kp) {
  const int lane = threadIdx.x;
  const long long a = kp.match_bonus;
  unsigned long long n_empty = 0, n_columns = 0, n_segments = 0, n_scanned = 0, n_overflow = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.index[pair] = make_index(AWV_CL_SKIPPED, 0, -1);
      continue;
    }
    const unsigned long long s0 = kp.seg_first[pair], s1 = kp.seg_first[pair + 1];
    const unsigned long long cap = (unsigned long long)uniform((unsigned)(s1 - s0)) | ((unsigned long long)uniform((unsigned)((s1 - s0) >> 32)) << 32);
    awv_clip_result* seg = kp.seg + s0;
    Interval* stack = kp.stack + s0 + (unsigned long long)pair;  // cap + 1 entries
    n_columns += (unsigned long long)rec.cigar_len;

    unsigned long long count = 0, sp = 0;
    Interval cur{0, rec.cigar_len, 0, 0};
    bool have = rec.cigar_len > 0, first = true, bad = false, overflow = false;
    for (;;) {
      if (!have) {
        if (sp == 0) break;
        const Interval top = stack[--sp];  // (every lane wrote this entry itself)
        cur = Interval{uniform(top.lo), uniform(top.hi), uniform(top.q_before), uniform(top.t_before)};
      }
      have = false;
      const long long len = (long long)cur.hi - (long long)cur.lo;
      n_scanned += (unsigned long long)len;
      const awvc::Scan sc = awvc::scan_ops(kp.pen, a, kp.arena, rec.cigar_off + cur.lo, len, lane);
      if (first && sc.bad_col >= 0) {  // the first scan covers the whole string
        if (lane == 0) kp.index[pair] = make_index(AWV_CL_BAD_OP, 0, sc.bad_col);
        bad = true;
        break;
      }
      first = false;
      if (sc.bad_col >= 0 || sc.best <= 0 || sc.best < kp.min_score) continue;
      if (count >= cap) {  // (cannot happen under the slot rule: never write past the record's region)
        overflow = true;
        break;
      }
      if (lane == 0) seg[count] = lift(awvc::make_clip(a, sc.best, sc.beg, sc.end, sc.at_beg, sc.at_end), cur);
      ++count;
      const Interval right{cur.lo + sc.end, cur.hi, cur.q_before + sc.at_end.q, cur.t_before + sc.at_end.t};
      if (worth(a, kp.min_score, right.lo, right.hi)) {
        if (sp > cap) {  // (likewise: the stack holds cap + 1 entries)
          overflow = true;
          break;
        }
        stack[sp++] = right;
      }
      if (worth(a, kp.min_score, cur.lo, cur.lo + sc.beg)) {
        cur.hi = cur.lo + sc.beg;
        have = true;
      }
    }
    if (bad) continue;
    if (lane == 0) kp.index[pair] = make_index(count > 0 ? AWV_CL_OK : AWV_CL_EMPTY, (int)count, -1);
    n_segments += count;
    n_empty += count == 0;
    n_overflow += overflow;
  }
  if (lane == 0) {
    if (n_empty) atomicAdd(&kp.counters[1], n_empty);
    if (n_columns) atomicAdd(&kp.counters[2], n_columns);
    if (n_segments) atomicAdd(&kp.counters[3], n_segments);
    if (n_scanned) atomicAdd(&kp.counters[4], n_scanned);
    if (n_overflow) atomicAdd(&kp.counters[5], n_overflow);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State : awvw::RecordPass {
  Buf<uint64_t> d_seg_first;
  Buf<awv_clip_result> d_seg;
  Buf<Interval> d_stack;
  Buf<awv_split_index> d_index;
  awv_split_stats stats{};
  void release() {
    RecordPass::release();
    d_seg_first.release();
    d_seg.release();
    d_stack.release();
    d_index.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
void stats_reset(State* s) { awvw::reset_stats(s); }

namespace {

// the clip's rules for penalties and bonus, and the threshold
int check_args(const awv_penalties* p, int32_t match_bonus, int64_t min_score, awv_penalties& out) {
  if (int rc = awv_internal_check_penalties(p)) return rc;
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS)
    return awv_internal_fail(AWV_ERR_ARG, "split: match_bonus must be in [1, " + std::to_string(AWV_CLIP_MAX_BONUS) + "]");
  if (min_score < 1) return awv_internal_fail(AWV_ERR_ARG, "split: min_score must be >= 1");
  out = *p;
  out.two_piece = p->two_piece ? 1 : 0;
  if (!out.two_piece) out.gap_open2 = out.gap_ext2 = 0;
  return AWV_OK;
}

// (the split reads no sequence: an engine without a set will do)
int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_split(e), e, v, st, false); }

bool ascending(const uint64_t* seg_first, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (seg_first[i + 1] < seg_first[i]) return false;
  return true;
}

// One launch over n records whose op bytes are on the device already.  The slot regions are the caller's layout, whatever
// rule it was checked by -- the kernel stays inside them.  Record i's segments go to sout[seg_first[i] ..), sorted; slots
// behind them are not written.
int launch(const awp::EngineView& v, State* st, const awv_penalties& pen, int32_t match_bonus, int64_t min_score, int64_t n, const awv_result* results,
           const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* seg_first, awv_split_index* iout, awv_clip_result* sout) {
  if (n == 0) return AWV_OK;
  if (!ascending(seg_first, n)) return awv_internal_fail(AWV_ERR_ARG, "split: seg_first must ascend");
  if (int rc = st->begin(v, "split", n, results, arena_bytes)) return rc;
  std::vector<uint64_t> rel((size_t)n + 1);
  for (int64_t i = 0; i <= n; ++i) rel[(size_t)i] = seg_first[i] - seg_first[0];
  const uint64_t total = rel[(size_t)n];
  AWV_TRY(st->d_seg_first.reserve((size_t)n + 1));
  AWV_TRY(st->d_index.reserve((size_t)n));
  AWV_TRY(st->d_seg.reserve((size_t)total + 1));
  AWV_TRY(st->d_stack.reserve((size_t)total + (size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_seg_first.p, rel.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, v.stream));
  if (int rc = st->clear_counters(v, 8)) return rc;
  KParams kp{};
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.seg_first = st->d_seg_first.p;
  kp.seg = st->d_seg.p;
  kp.stack = st->d_stack.p;
  kp.index = st->d_index.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.min_score = min_score;
  kp.pen = pen;
  kp.match_bonus = match_bonus;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_split_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  unsigned long long hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<awv_split_index> hix((size_t)n);
  float ms = 0;
  AWV_TRY(hipMemcpyAsync(hix.data(), st->d_index.p, (size_t)n * sizeof(awv_split_index), hipMemcpyDeviceToHost, v.stream));
  if (int rc = st->finish(v, hc, 8, ms)) return rc;
  if (hc[5] != 0) return awv_internal_fail(AWV_ERR_HIP, "split: internal error: a record found more segments than its slots hold");
  // the slot region as far as it is used: the index says where the last segment lies
  uint64_t used = 0;
  for (int64_t i = 0; i < n; ++i)
    if (hix[(size_t)i].count > 0) used = std::max(used, rel[(size_t)i] + (uint64_t)hix[(size_t)i].count);
  std::vector<awv_clip_result> hseg((size_t)used);
  if (used) {
    AWV_TRY(hipMemcpyAsync(hseg.data(), st->d_seg.p, (size_t)used * sizeof(awv_clip_result), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = hix[(size_t)i].count;
    if (c > 0) {
      awv_clip_result* s = hseg.data() + rel[(size_t)i];
      std::sort(s, s + c, [](const awv_clip_result& x, const awv_clip_result& y) { return x.col_beg < y.col_beg; });
      std::memcpy(sout + seg_first[i], s, (size_t)c * sizeof(awv_clip_result));
    }
    iout[i] = hix[(size_t)i];
  }
  st->stats.kernel_ms += ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.empty += hc[1];
  st->stats.columns += hc[2];
  st->stats.segments += hc[3];
  st->stats.columns_scanned += hc[4];
  return AWV_OK;
}

int split_cigars_core(awv_engine* e, const awv_penalties* pen_in, int32_t match_bonus, int64_t min_score, const awv_result* results, int64_t n_all,
                      const uint8_t* cigar_arena, uint64_t arena_bytes, uint64_t max_arena, const uint64_t* seg_first, awv_split_index* iout,
                      awv_clip_result* sout) {
  awv_penalties pen;
  if (int rc = check_args(pen_in, match_bonus, min_score, pen)) return rc;
  // before anything goes up: the layout ascends, every completed record's op bytes lie inside the caller's arena and its
  // region holds what an op string of its length may need
  if (!ascending(seg_first, n_all)) return awv_internal_fail(AWV_ERR_ARG, "split_cigars: seg_first must ascend");
  for (int64_t i = 0; i < n_all; ++i) {
    if (awvw::outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "split_cigars: a record's op bytes lie outside the CIGAR arena");
    const int64_t need = results[i].status == AWV_ST_COMPLETED ? slots(match_bonus, min_score, (int64_t)results[i].cigar_len) : 0;
    if (seg_first[i + 1] - seg_first[i] < (uint64_t)need)
      return awv_internal_fail(AWV_ERR_ARG, "split_cigars: record " + std::to_string(i) + " owns fewer slots than awv_split_slots(a, min_score, cigar_len)");
  }
  if (n_all > 0 && seg_first[n_all] > seg_first[0] && !sout) return awv_internal_fail(AWV_ERR_ARG, "split_cigars: null sout");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->stats = awv_split_stats{};
  // in pieces (record_pieces.hpp) that keep every string's offset modulo 16
  std::vector<uint8_t> stage;
  std::vector<awv_result> recs;
  for (int64_t first = 0; first < n_all;) {
    const awvw::Piece pc = awvw::pack_piece(results, n_all, first, cigar_arena, max_arena, true, recs, stage);
    AWV_TRY(st->d_arena.reserve((size_t)pc.bytes + 64));
    if (pc.bytes) AWV_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
    if (int rc = launch(v, st, pen, match_bonus, min_score, pc.n, recs.data(), st->d_arena.p, pc.bytes, seg_first + first, iout + first, sout)) return rc;
    first += pc.n;
  }
  return AWV_OK;
}

// seg_first from the (pattern, text) lengths of each entry
template <typename Lens>
int layout(int64_t n, int32_t match_bonus, int64_t min_score, uint64_t* seg_first, Lens lens) {
  if (slots(match_bonus, min_score, 0) < 0) return awv_internal_fail(AWV_ERR_ARG, "split_layout: need 1 <= match_bonus <= 32767 and min_score >= 1");
  if (n < 0 || !seg_first) return awv_internal_fail(AWV_ERR_ARG, "split_layout: bad argument");
  seg_first[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t pl = 0, tl = 0;
    if (!lens(i, pl, tl)) return awv_internal_fail(AWV_ERR_ARG, "split_layout: entry " + std::to_string(i) + " names a sequence index or an interval out of range");
    seg_first[i + 1] = seg_first[i] + (uint64_t)slots(match_bonus, min_score, std::min(pl, tl));
  }
  return AWV_OK;
}

}  // namespace

int split_batch(awv_engine* e, const awv_penalties* pen_in, int32_t match_bonus, int64_t min_score, int64_t n, const awv_result* results,
                const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* seg_first, awv_split_index* iout, awv_clip_result* sout) {
  awv_penalties pen;
  if (int rc = check_args(pen_in, match_bonus, min_score, pen)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  return launch(v, st, pen, match_bonus, min_score, n, results, d_arena, arena_bytes, seg_first, iout, sout);
}

}  // namespace awvs

extern "C" {

int64_t awv_split_slots(int32_t match_bonus, int64_t min_score, int64_t m) { return awvs::slots(match_bonus, min_score, m); }

int awv_split_layout_pairs(awv_engine* e, const awv_pair* pairs, int64_t n, int32_t match_bonus, int64_t min_score, uint64_t* seg_first) {
  if (!e) return awv_internal_fail(AWV_ERR_ARG, "null engine");
  if (n > 0 && !pairs) return awv_internal_fail(AWV_ERR_ARG, "split_layout_pairs: null pairs");
  awp::EngineView v;
  if (n > 0)
    if (int rc = awv_internal_view(e, &v)) return rc;
  AWV_GUARDED(return awvs::layout(n, match_bonus, min_score, seg_first, [&](int64_t i, int64_t& pl, int64_t& tl) {
    if (pairs[i].q_idx < 0 || pairs[i].q_idx >= v.n || pairs[i].t_idx < 0 || pairs[i].t_idx >= v.n) return false;
    pl = v.len_host[pairs[i].q_idx];
    tl = v.len_host[pairs[i].t_idx];
    return true;
  });)
}

int awv_split_layout_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, int32_t match_bonus, int64_t min_score, uint64_t* seg_first) {
  if (!e) return awv_internal_fail(AWV_ERR_ARG, "null engine");
  if (n > 0 && !ranges) return awv_internal_fail(AWV_ERR_ARG, "split_layout_ranges: null ranges");
  awp::EngineView v;
  if (n > 0)
    if (int rc = awv_internal_view(e, &v)) return rc;
  AWV_GUARDED(return awvs::layout(n, match_bonus, min_score, seg_first, [&](int64_t i, int64_t& pl, int64_t& tl) {
    awv_pair p;
    awvr::Span s;
    if (!awvr::split_range(v.len_host, v.n, ranges[i], p, s)) return false;
    pl = s.pe - s.pb;
    tl = s.te - s.tb;
    return true;
  });)
}

int awv_split_one_host(const awv_penalties* pen, int32_t match_bonus, int64_t min_score, const uint8_t* cigar, int64_t n, awv_clip_result* sout,
                       int64_t cap, int64_t* count, awv_split_index* index) {
  awv_penalties p;
  if (int rc = awvs::check_args(pen, match_bonus, min_score, p)) return rc;
  if (!count || cap < 0 || (cap > 0 && !sout) || n < 0 || n > (int64_t)UINT32_MAX || (n > 0 && !cigar))
    return awv_internal_fail(AWV_ERR_ARG, "split_one_host: bad argument");
  AWV_GUARDED(
    std::vector<awvs::Interval> stack((size_t)std::min<int64_t>(awvs::slots(match_bonus, min_score, n), n) + 1);
    const awv_split_index ix = awvs::split_one(p, match_bonus, min_score, cigar, n, sout, cap, stack.data());
    *count = ix.count;
    if (index) *index = ix;
    return AWV_OK;
  )
}

int awv_split_cigars(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, int64_t min_score, const awv_result* results, int64_t n,
                     const uint8_t* cigar_arena, uint64_t arena_bytes, const uint64_t* seg_first, awv_split_index* iout, awv_clip_result* sout) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || !seg_first || (n > 0 && (!results || !iout))) return awv_internal_fail(AWV_ERR_ARG, "split_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "split_cigars: null arena");
  AWV_GUARDED(return awvs::split_cigars_core(e, pen, match_bonus, min_score, results, n, cigar_arena, arena_bytes, awv_internal_max_arena(e), seg_first,
                                            iout, sout);)
}

int awv_engine_split_stats(const awv_engine* e, awv_split_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "split_stats: null argument");
  const awvs::State* st = awv_internal_split(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_split_stats{};
  return AWV_OK;
}

}  // extern "C"
