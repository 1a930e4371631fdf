// record_pass.hpp -- the host skeleton of a record pass: a kernel with one wave per alignment record,
// persistent waves taking records, longest op string first, from a cursor (awvw::take_record, wave_ops.hpp).  verify.hip,
// clip.hip, split.hip, normalize.hip, coverage.hip, variants.hip, lift.hip and msa.hip (namespaces awvf, awvc, awvs, awvn, awvcov,
// awvvar, awvl, awvmsa) each keep a State that derives from RecordPass next to the buffers and stats only that pass has; a launch is
// begin(), the pass's own uploads, clear_counters(), KParams, start(), the kernel, stop(), the pass's own copy-backs, finish().
// encode.hip and cs.hip (awve, awvcs) write text whose size depends on the data: their State derives from TextPass
// (text_pass.hpp), which puts measure, scan and emit on the stream with these parts.  Below the skeleton stand the checks that the
// calls on caller-supplied records with slices share (item_call.hpp: cs and the four passes made after it), as errors.
#pragma once

#include <algorithm>
#include <climits>
#include <numeric>
#include <string>
#include <vector>

#include "item_call.hpp"       // ItemCall, rectangle_ok, first_too_long
#include "planner_device.hpp"  // EngineView, awv_internal_view, AWV_TRY
#include "record_pieces.hpp"   // outside, pack_piece
#include "wave_ops.hpp"        // Buf

namespace awvw {

constexpr int WAVES_PER_CU = 16;  // persistent one-wave workgroups per CU: what a chunk does depends on its scans and loads, other waves fill the wait

struct RecordPass {
  Buf<awv_result> d_results;
  Buf<int32_t> d_order;
  Buf<unsigned long long> d_counters;  // [0] the cursor, [1..] the pass's own
  Buf<uint8_t> d_arena;                // awv_*_cigars: a piece of the caller's op bytes
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int num_cus = 0;

  void release() {
    d_results.release();
    d_order.release();
    d_counters.release();
    d_arena.release();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
  }

  // the engine's view, its device made current, the events and the CU count.  need_set: the pass reads sequences, so an
  // engine without a set is AWV_ERR_STATE; else the view of such an engine names no sequences and that is no error
  int open(awv_engine* e, awp::EngineView& v, bool need_set) {
    if (need_set) {
      if (int rc = awv_internal_view(e, &v)) return rc;
    } else {
      awv_internal_device_view(e, &v);
    }
    AWV_TRY(hipSetDevice(v.device));
    if (!ev0) AWV_TRY(hipEventCreate(&ev0));
    if (!ev1) AWV_TRY(hipEventCreate(&ev1));
    if (num_cus == 0) {
      int cus = 0;
      AWV_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, v.device));
      num_cus = std::max(cus, 1);
    }
    return AWV_OK;
  }

  // n > 0 records whose op bytes are on the device already.  Every op string's place in the arena is checked here, on the
  // host: the kernel reads what the records say.  Then the records and their dispatch order go up.
  int begin(const awp::EngineView& v, const char* name, int64_t n, const awv_result* results, uint64_t arena_bytes) {
    if (n > INT32_MAX) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": more than 2^31 - 1 records in one launch");
    for (int64_t i = 0; i < n; ++i)
      if (outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": a record's op bytes lie outside the CIGAR arena");
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    auto cols = [&](int32_t i) { return results[i].status == AWV_ST_COMPLETED ? results[i].cigar_len : 0u; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cols(a) > cols(b); });
    AWV_TRY(d_results.reserve((size_t)n));
    AWV_TRY(d_order.reserve((size_t)n));
    AWV_TRY(hipMemcpyAsync(d_results.p, results, (size_t)n * sizeof(awv_result), hipMemcpyHostToDevice, v.stream));
    AWV_TRY(hipMemcpyAsync(d_order.p, order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    return AWV_OK;
  }

  // one-wave workgroups: awv_engine_config.workgroups, or WAVES_PER_CU per CU, and never more than records
  unsigned grid(const awp::EngineView& v, int64_t n) const {
    return (unsigned)std::min<int64_t>(n, v.workgroups > 0 ? (int64_t)v.workgroups : (int64_t)num_cus * WAVES_PER_CU);
  }

  // behind every upload, the pass's own included, as each pass did on its own: d_counters is a State's last allocation and
  // the memset the stream's last operation before the kernel's bracket
  int clear_counters(const awp::EngineView& v, int n_counters) {
    AWV_TRY(d_counters.reserve((size_t)n_counters));
    AWV_TRY(hipMemsetAsync(d_counters.p, 0, (size_t)n_counters * sizeof(unsigned long long), v.stream));
    return AWV_OK;
  }

  // the bracket around the kernel launch
  int start(const awp::EngineView& v) {
    AWV_TRY(hipEventRecord(ev0, v.stream));
    return AWV_OK;
  }
  int stop(const awp::EngineView& v) {
    AWV_TRY(hipGetLastError());
    AWV_TRY(hipEventRecord(ev1, v.stream));
    return AWV_OK;
  }

  // awv_*_cigars / _ranges: the call in pieces (record_pieces.hpp) that keep every string's offset modulo 16.  A piece's op bytes go
  // up into d_arena, then launch_piece(first, n, recs, arena_bytes) is the pass's launch over records [first, first + n); pack_piece
  // takes one record or more, so `first` advances.
  template <typename LaunchPiece>
  int each_piece(const awp::EngineView& v, const awv_result* results, int64_t n_all, const uint8_t* cigar_arena, uint64_t max_arena, LaunchPiece&& launch_piece) {
    std::vector<uint8_t> stage;
    std::vector<awv_result> recs;
    for (int64_t first = 0; first < n_all;) {
      const Piece pc = pack_piece(results, n_all, first, cigar_arena, max_arena, true, recs, stage);
      AWV_TRY(d_arena.reserve((size_t)pc.bytes + 64));
      if (pc.bytes) AWV_TRY(hipMemcpyAsync(d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
      if (int rc = launch_piece(first, pc.n, recs.data(), pc.bytes)) return rc;
      first += pc.n;
    }
    return AWV_OK;
  }

  // behind the pass's own copy-backs: the counters come back to hc[0 .. n_counters), the stream is waited for, ms is the kernel's time
  int finish(const awp::EngineView& v, unsigned long long* hc, int n_counters, float& ms) {
    AWV_TRY(hipMemcpyAsync(hc, d_counters.p, (size_t)n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
    AWV_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    return AWV_OK;
  }
};

// What stands around every pass's State (a RecordPass with the pass's `stats`), once: the engine keeps one per pass in a slot of
// its own (engine.hip's awv_internal_*), made on first use; the functions a pass's *_device.hpp declares are one line each on these.
template <typename State>
int open_pass(State*& slot, awv_engine* e, awp::EngineView& v, State*& st, bool need_set) {
  if (!slot) slot = new State();
  st = slot;
  return st->open(e, v, need_set);
}
// the state of an engine whose pass accumulates (the pass's active(slot)): `who` before awv_engine_<pass>_begin is AWV_ERR_STATE
template <typename State>
int open_active(State*& slot, const char* who, const char* pass, awv_engine* e, awp::EngineView& v, State*& st) {
  if (!active(slot)) return awv_internal_fail(AWV_ERR_STATE, std::string(who) + " before awv_engine_" + pass + "_begin");
  return open_pass(slot, e, v, st, true);
}
template <typename State>
void release_pass(State* s) {  // frees the buffers and the object itself (nullptr: nothing)
  if (!s) return;
  s->release();
  delete s;
}
template <typename State>
void reset_stats(State* s) {  // (nullptr: nothing)
  if (s) s->stats = decltype(s->stats){};
}

// ---- the checks of a call on caller-supplied records with slices, as errors ---------------------------------------------------

// The head of an awv_*_cigars / _ranges call's argument check.  list: the pairs or ranges; outputs_ok: the pass's own outputs and
// counts are there.
inline int check_call_args(const char* name, int64_t n, const void* list, const awv_result* results, bool outputs_ok, const uint8_t* cigar_arena,
                           uint64_t arena_bytes) {
  if (n < 0 || !outputs_ok || (n > 0 && (!list || !results))) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": null arena");
  return AWV_OK;
}

// item_call.hpp's prologue on the engine's set: before anything goes up, every rectangle inside its sequences, every completed
// record's op bytes inside the caller's arena, every slice inside its string -- or AWV_ERR_ARG under `who`, the called function.
inline int resolve_call(ItemCall& c, const awp::EngineView& v, const char* who, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n,
                        const awv_result* results, uint64_t arena_bytes, const awv_cs_slice* slices) {
  if (c.resolve(v.len_host, v.n, pairs, ranges, n, results, arena_bytes, slices) != ItemCall::NONE) return awv_internal_fail(AWV_ERR_ARG, c.message(who));
  return AWV_OK;
}

// what fits a pass's 32-bit lengths and counts: refused before anything is launched
inline int check_lengths(const awv_result* recs, int64_t n, int64_t max_columns, const char* message) {
  return first_too_long(recs, n, max_columns) < 0 ? (int)AWV_OK : awv_internal_fail(AWV_ERR_ARG, message);
}

// Every index and rectangle of a launch, checked on the host: the kernels read what the items say.
inline int check_rectangles(const awp::EngineView& v, const char* name, const awv_pair* pairs, const Span* spans, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    if (!index_ok(pairs[i], v.n)) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": sequence index out of range");
    if (!rectangle_ok(v.len_host, pairs[i], spans[i])) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": an interval outside its sequence");
  }
  return AWV_OK;
}

// awv_*_one_host: the rectangle inside its two sequences,
inline int check_host_rectangle(const char* name, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb, int32_t te) {
  if (pb < 0 || pb > pe || pe > qlen || tb < 0 || tb > te || te > tlen) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": an interval outside its sequence");
  return AWV_OK;
}
// and the slice (nullable: the whole string of n columns) inside the string and no longer than max_columns: `out` is what is walked
struct HostSlice {
  int64_t beg, end, q_skip, t_skip;
};
inline int check_host_slice(const char* name, const awv_cs_slice* slice, int64_t n, int64_t max_columns, HostSlice& out) {
  out = HostSlice{0, n, 0, 0};
  if (slice) {
    if (slice->col_beg > slice->col_end || (int64_t)slice->col_end > n || slice->q_skip < 0 || slice->t_skip < 0)
      return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": the slice does not lie inside the op string, or skips a negative number of bases");
    out = HostSlice{slice->col_beg, slice->col_end, slice->q_skip, slice->t_skip};
  }
  if (out.end - out.beg > max_columns) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": an op string of more than 2^30 columns");
  return AWV_OK;
}

}  // namespace awvw
