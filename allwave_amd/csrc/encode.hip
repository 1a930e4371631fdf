// encode.hip -- run-length CIGAR text made on the device: the last per-batch step of awv_align_pairs_encoded /
// awv_align_ranges_encoded, awv_encode_cigars, awv_encode_one_host and awv_engine_encode_stats (include/allwave_hip.h).  What
// the text of an op string is is encode_device.hpp; this file gets the kernels to the same bytes.
//
// A text pass (text_pass.hpp): one wave per record, persistent waves taking records (longest op string first) from a cursor, and
// measure, scan and emit on the stream.  measure writes every record's text length and run count (awv_cigar_text.len / .runs).
// The walk is text_pass.hpp's: the lane that holds a break owns the run that ends there.  The characters a lane's runs take
// (digits + 1 each) go through an add-scan, with a carry, which gives every lane the text offset of its first run; a lane owns up
// to 16 runs and writes them one after the other.  The string's last run has no break behind it and is written when the chunks
// are done.
// The text is stored byte by byte, straight to global memory (DESIGN.md 4.29 has the reason and what it costs).
#include "encode_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "text_pass.hpp"  // the host skeleton and the device walk of a text pass: TextPass, lane_runs, text_dest, AWV_TRY

namespace awve {

struct KParams {
  const awv_result* results;     // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;          // dispatch slot -> record
  const uint8_t* arena;          // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_cigar_text* out;           // measure writes len and runs, the scan off, emit reads all three
  awvw::TextArena text;          // emit: where the launch's text goes
  unsigned long long* counters;  // [0] this kernel's cursor; measure: [1] runs, [2] columns
  long long npairs;
};

using awvw::byte_at;
using awvw::CHUNK;
using awvw::wave_scan_add;

template <bool EMIT>
__global__ __launch_bounds__(64) void awv_encode_kernel(KParams kp) {
  const int lane = threadIdx.x;
  unsigned long long t_runs = 0, t_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    const long long n = rec.status == AWV_ST_COMPLETED ? (long long)rec.cigar_len : 0;
    if (n == 0) {
      if (!EMIT && lane == 0) {
        kp.out[pair].len = 0;
        kp.out[pair].runs = 0;
      }
      continue;
    }
    awvw::TextDest d{nullptr, 0u};
    if (EMIT) {
      const awv_cigar_text t = kp.out[pair];
      d = awvw::text_dest(kp.text, t.off, t.len);
    }
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    awvw::RunCarry carry;
    unsigned c_text = 0;  // characters of the runs that ended in the chunks before (uniform, like everything carried)
    unsigned c_runs = 0;
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::LaneRuns r = awvw::lane_runs(ops, sh, span, base, lane, carry);
      // the characters and the count of the runs this lane owns
      int chars = 0;
      {
        long long start = r.rs0;
        for (unsigned m = r.brk; m != 0; m &= m - 1) {
          const long long col = r.b0 + __builtin_ctz(m) - sh;
          chars += (int)run_chars((unsigned)(col - start));
          start = col;
        }
      }
      const int packed = chars | (__popc(r.brk) << 16);  // (a lane's runs take at most 11 + 15 * 3 characters: a chunk's sums fit 16 bits each)
      const int s_in = wave_scan_add(packed);
      if (EMIT) {
        unsigned at = c_text + (unsigned)((s_in - packed) & 0xffff);
        long long start = r.rs0;
        for (unsigned m = r.brk; m != 0; m &= m - 1) {
          const int j = __builtin_ctz(m);
          const long long col = r.b0 + j - sh;
          const unsigned len = (unsigned)(col - start);
          const unsigned nc = run_chars(len);
          if (at + nc <= d.room) put_run(d.dst + at, len, j > 0 ? byte_at(r.w, j - 1) : r.prev);
          at += nc;
          start = col;
        }
      }
      awvw::carry_on(carry, r, sh, span, base);
      const int tot = __builtin_amdgcn_readlane(s_in, 63);
      c_text += (unsigned)(tot & 0xffff);
      c_runs += (unsigned)(tot >> 16);
    }
    // the last run ends with the string
    const unsigned last_len = (unsigned)(n - carry.start);
    const unsigned last_nc = run_chars(last_len);
    if (lane == 0) {
      if (EMIT) {
        if (c_text + last_nc <= d.room) put_run(d.dst + c_text, last_len, carry.prev);
      } else {
        kp.out[pair].len = c_text + last_nc;
        kp.out[pair].runs = c_runs + 1;
      }
    }
    t_runs += c_runs + 1;
    t_columns += (unsigned long long)n;
  }
  if (!EMIT && lane == 0) {
    if (t_runs) atomicAdd(&kp.counters[1], t_runs);
    if (t_columns) atomicAdd(&kp.counters[2], t_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct State : awvw::TextPass {
  awvw::Buf<awv_cigar_text> d_out;
  std::vector<awv_result> h_recs;   // a batch's records with their slices applied
  awv_encode_stats stats{};
  void release() {
    TextPass::release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
void stats_reset(State* s) { awvw::reset_stats(s); }

namespace {

constexpr const char* TOO_LONG = "encode: an op string of more than 2^31 - 1 columns";  // what fits awv_cigar_text.len

// (the text reads no sequence: an engine without a set will do, and is no error)
int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_encode(e), e, v, st, false); }

// One launch over n records whose op bytes are on the device already; a record's slice has been applied to it.  The records'
// texts take [text_base, *text_end) of the call's text arena, in record order; tout (host) is filled.  want_text: step 3 runs
// and the launch's text is in st->d_text afterwards, its first character the one at text_base.
int launch(const awp::EngineView& v, State* st, int64_t n, const awv_result* recs, const uint8_t* d_arena, uint64_t arena_bytes, uint64_t text_base,
           bool want_text, awv_cigar_text* tout, uint64_t* text_end) {
  *text_end = text_base;
  if (n == 0) return AWV_OK;
  if (int rc = st->begin(v, "encode", n, recs, arena_bytes)) return rc;
  AWV_TRY(st->d_out.reserve((size_t)n));
  KParams kp{};
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.npairs = n;
  awvw::TextLaunch done;
  const auto run = [&](bool emit, unsigned grid, unsigned long long* counters, const awvw::TextArena& text) {
    kp.counters = counters;
    kp.text = text;
    if (emit) hipLaunchKernelGGL(awv_encode_kernel<true>, dim3(grid), dim3(64), 0, v.stream, kp);
    else hipLaunchKernelGGL(awv_encode_kernel<false>, dim3(grid), dim3(64), 0, v.stream, kp);
  };
  if (int rc = st->measure_scan_emit(v, n, st->d_out.p, text_base, want_text, tout, run, done)) return rc;
  st->stats.kernel_ms += done.kernel_ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.runs += done.hc[1];
  st->stats.columns += done.hc[2];
  st->stats.text_bytes += done.bytes;
  *text_end = done.end;
  return AWV_OK;
}

int encode_cigars_core(awv_engine* e, const awv_result* results, int64_t n_all, const uint8_t* cigar_arena, uint64_t arena_bytes, const Slice* slices,
                       uint64_t max_arena, awv_cigar_text* tout, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->stats = awv_encode_stats{};
  // before anything goes up: every completed record's op bytes lie inside the caller's arena, and every slice inside its string
  for (int64_t i = 0; i < n_all; ++i) {
    if (awvw::outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "encode_cigars: a record's op bytes lie outside the CIGAR arena");
    if (slices && !slice_ok(results[i], slices[i].col_beg, slices[i].col_end))
      return awv_internal_fail(AWV_ERR_ARG, "encode_cigars: slice " + std::to_string(i) + " does not lie inside its op string");
  }
  // a slice is an op string of its own: the records that go up name the slices
  std::vector<awv_result> sliced;
  if (slices) {
    sliced.assign(results, results + n_all);
    for (int64_t i = 0; i < n_all; ++i) apply_slice(sliced[(size_t)i], slices[i].col_beg, slices[i].col_end);
    results = sliced.data();
  }
  if (int rc = awvw::check_lengths(results, n_all, MAX_COLUMNS, TOO_LONG)) return rc;
  return st->in_pieces(v, results, n_all, cigar_arena, max_arena, text_buf, text_cap, text_bytes,
                       [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes, uint64_t text_base, bool want_text, uint64_t* text_end) {
                         return launch(v, st, n, recs, st->d_arena.p, bytes, text_base, want_text, tout + first, text_end);
                       });
}

}  // namespace

int encode_batch(awv_engine* e, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes, const awv_clip_result* clips,
                 awv_cigar_text* tout, uint64_t* text_bytes) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  if (clips) {  // the clip's segment is the slice; a record without one has no text
    st->h_recs.assign(results, results + n);
    for (int64_t i = 0; i < n; ++i) {
      const bool ok = clips[i].code == AWV_CL_OK && slice_ok(results[i], clips[i].col_beg, clips[i].col_end);
      apply_slice(st->h_recs[(size_t)i], ok ? clips[i].col_beg : 0, ok ? clips[i].col_end : 0);
    }
    results = st->h_recs.data();
  }
  if (int rc = awvw::check_lengths(results, n, MAX_COLUMNS, TOO_LONG)) return rc;
  return launch(v, st, n, results, d_arena, arena_bytes, 0, true, tout, text_bytes);
}

const uint8_t* batch_text(awv_engine* e) {
  const State* st = awv_internal_encode(e);
  return st ? st->d_text.p : nullptr;
}

}  // namespace awve

extern "C" {

int awv_encode_one_host(const uint8_t* cigar, int64_t n, uint8_t* out_buf, uint64_t cap, awv_cigar_text* out) {
  if (!out || n < 0 || n > awve::MAX_COLUMNS || (n > 0 && !cigar) || (cap > 0 && !out_buf)) return awv_internal_fail(AWV_ERR_ARG, "encode_one_host: bad argument");
  *out = awve::encode_one(cigar, n, out_buf, cap);
  return AWV_OK;
}

int awv_encode_cigars(awv_engine* e, const awv_result* results, int64_t n, const uint8_t* cigar_arena, uint64_t arena_bytes, const uint32_t* slices,
                      awv_cigar_text* tout, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || !text_bytes || (n > 0 && (!results || !tout))) return awv_internal_fail(AWV_ERR_ARG, "encode_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "encode_cigars: null arena");
  if (text_cap > 0 && !text_buf) return awv_internal_fail(AWV_ERR_ARG, "encode_cigars: null text buffer");
  static_assert(sizeof(awve::Slice) == 2 * sizeof(uint32_t), "a slice is two columns");
  AWV_GUARDED(return awve::encode_cigars_core(e, results, n, cigar_arena, arena_bytes, (const awve::Slice*)slices, awv_internal_max_arena(e), tout, text_buf,
                                              text_cap, text_bytes);)
}

int awv_engine_encode_stats(const awv_engine* e, awv_encode_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "encode_stats: null argument");
  const awve::State* st = awv_internal_encode(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_encode_stats{};
  return AWV_OK;
}

}  // extern "C"
