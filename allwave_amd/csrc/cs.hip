// cs.hip -- minimap2's cs difference string made on the device: awv_cs_cigars / awv_cs_ranges, awv_cs_one_host and
// awv_engine_cs_stats (include/allwave_hip.h).  What the cs text of an op string is is cs_device.hpp; this file gets the kernels to
// the same bytes.
//
// A text pass (text_pass.hpp) with verify.hip's sequence walk: one wave per record, persistent waves taking records (longest op
// string first) from a cursor, and measure, scan and emit on the stream.  measure writes every record's text length and code
// (awv_cs_text.len / .code).
// The walk takes a string in chunks of 64 lanes x 16 op bytes, one aligned 16-byte load per lane.  A column's pattern position
// is the number of ops other than 'I' before it, its text position the number other than 'D': a lane counts both over its bytes,
// one packed add-scan over the lanes (16 bits each: a chunk holds 1,024 columns) and a carry from chunk to chunk place the lane,
// and a column inside the lane adds the popcount of the lane's masks below it.  From there a lane's columns touch at most 16
// consecutive pattern and 16 consecutive text bytes: five aligned dwords each, shifted into place.
// Who owns which characters: an 'X' column its three; a gap column its base, and the sign too when it starts its run (its op
// differs from the one before it); in long mode an 'M' column likewise.  In short mode an 'M' run's ":N" belongs to the lane that
// holds the break that ends the run (text_pass.hpp's run ownership), and the string's last run is written when the chunks are
// done.  A second add-scan over the lanes' character counts gives every lane its text offset.
// The text is stored byte by byte, straight to global memory, as encode.hip stores its text.
#include "cs_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "seq_load.hpp"   // load16
#include "text_pass.hpp"  // the host skeleton and the device walk of a text pass: TextPass, lane_runs, text_dest, AWV_TRY; resolve_call below it

namespace awvcs {

struct KParams {
  const uint8_t* fwd;         // the engine's forward copies
  const uint8_t* rc;          // and reverse-complement copies (the pattern of a q_revcomp pair)
  const uint64_t* seq_off;
  const awv_pair* pairs;
  const Span* spans;          // record i's pattern / text are these intervals of its sequences, behind the slice's skips (validated on the host;
                              // an interval of negative length: the skip alone is beyond the sequence)
  const awv_result* results;  // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;       // dispatch slot -> record
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_cs_text* out;           // measure writes len and code, the scan off, emit reads all three
  awvw::TextArena text;       // emit: where the launch's cs text goes
  unsigned long long* counters;  // [0] this kernel's cursor; measure: [1] failed records, [2] columns
  long long npairs;
};

using awvw::byte_at;
using awvw::CHUNK;
using awvw::LANE_BYTES;
using awvw::load16;
using awvw::u32x4;
using awvw::wave_scan_add;

__device__ __forceinline__ void put(uint8_t* dst, unsigned room, unsigned& at, unsigned ch) {  // never outside the record's own characters
  if (at < room) dst[at] = (uint8_t)ch;
  ++at;
}

template <bool EMIT, bool LONG>
__global__ __launch_bounds__(64) void awv_cs_kernel(KParams kp) {
  const int lane = threadIdx.x;
  unsigned long long t_failed = 0, t_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    if (rec.status != AWV_ST_COMPLETED) {
      if (!EMIT && lane == 0) kp.out[pair] = make_text(0, 0, AWV_CST_SKIPPED);
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    const awv_pair pr = kp.pairs[pair];
    const Span sp = kp.spans[pair];
    const int plen = sp.pe - sp.pb, tlen = sp.te - sp.tb;
    if (n == 0) {
      if (!EMIT) {
        const int code = whole_code(false, 0, 0, plen, tlen);
        if (lane == 0) kp.out[pair] = make_text(0, 0, code);
        t_failed += code != AWV_CST_OK;
      }
      continue;
    }
    // emit: only a record that measure found sound is walked again: its positions stay inside the two sequences (load16 clamps all
    // the same)
    uint8_t* dst = nullptr;
    unsigned room = 0;
    if (EMIT) {
      const awv_cs_text t = kp.out[pair];
      if (t.code == AWV_CST_OK) {
        const awvw::TextDest d = awvw::text_dest(kp.text, t.off, t.len);
        dst = d.dst;
        room = d.room;
      }
      if (room == 0) continue;
    }
    const uint8_t* const pattern = (pr.q_revcomp ? kp.rc : kp.fwd) + kp.seq_off[pr.q_idx] + sp.pb;
    const uint8_t* const text = kp.fwd + kp.seq_off[pr.t_idx] + sp.tb;
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    int cq = 0, ct = 0;  // bases consumed before the chunk (uniform, like everything carried)
    awvw::RunCarry carry;
    unsigned c_text = 0;  // characters of the columns and ended 'M' runs of the chunks before
    bool bad = false;
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::LaneRuns r = awvw::lane_runs(ops, sh, span, base, lane, carry);
      const long long b0 = r.b0;
      const u32x4 w = r.w;
      const unsigned brk = r.brk;
      awvw::OpMasks o = awvw::window_masks(r.jlo, r.jhi);  // (awvw::op_masks, written out: see there)
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) awvw::add_op(o, w, j);
      awvw::cut_to_window(o);
      const unsigned valid = o.valid, m_m = o.m, m_x = o.x, m_i = o.i, m_d = o.d;
      const unsigned gaps = m_i | m_d;
      const unsigned starts = brk | (b0 <= sh && sh < b0 + LANE_BYTES ? 1u << (int)(sh - b0) : 0u);  // columns that begin a run: the breaks and column 0
      const unsigned takes_p = valid & ~m_i, takes_t = valid & ~m_d;
      const bool lane_bad = (valid & ~(m_m | m_x | gaps)) != 0;

      // short mode: the breaks of this lane that end an 'M' run
      const unsigned end_m = LONG ? 0u : brk & ((m_m << 1) | (r.prev == 'M' ? 1u : 0u));
      int chars = 3 * __popc(m_x);
      if (LONG) {
        chars += __popc(valid & ~m_x) + __popc(starts & ~m_x);
      } else {
        chars += __popc(gaps) + __popc(starts & gaps);
        for (unsigned m = end_m; m != 0; m &= m - 1) {
          const int j = __builtin_ctz(m);
          chars += (int)match_chars((unsigned)(b0 + j - sh - awvw::run_start_before(r, sh, j)));
        }
      }
      const awvw::ConsumedScan pos = awvw::consumed_scan(o);
      const int s_ch = wave_scan_add(chars);
      if (EMIT) {
        const unsigned active = LONG ? valid : valid & ~m_m;  // the columns that own characters (an ended 'M' run's go with the column that ends it)
        if (active != 0) {
          const u32x4 pb16 = load16(pattern, plen, cq + (pos.ex & 0xffff)), tb16 = load16(text, tlen, ct + (pos.ex >> 16));
          unsigned at = c_text + (unsigned)(s_ch - chars);
          for (unsigned m = active; m != 0; m &= m - 1) {
            const int j = __builtin_ctz(m);
            const unsigned bit = 1u << j, below = bit - 1u;
            const unsigned op = byte_at(w, j);
            if (!LONG && (end_m & bit) != 0) {
              const unsigned len = (unsigned)(b0 + j - sh - awvw::run_start_before(r, sh, j)), nc = match_chars(len);
              if (at + nc <= room) put_match(dst + at, len);
              at += nc;
            }
            const unsigned pb = byte_at(pb16, __popc(takes_p & below)), tb = byte_at(tb16, __popc(takes_t & below));
            if (op == 'X') {
              put(dst, room, at, '*');
              put(dst, room, at, lower(tb));
              put(dst, room, at, lower(pb));
            } else {
              if ((starts & bit) != 0) put(dst, room, at, sign_of(op));
              put(dst, room, at, base_char(op, pb, tb));
            }
          }
        }
      }

      awvw::carry_on(carry, r, sh, span, base);
      cq += pos.tot & 0xffff;
      ct += pos.tot >> 16;
      c_text += (unsigned)__builtin_amdgcn_readlane(s_ch, 63);
      bad = bad || __ballot(lane_bad) != 0;
    }
    // short mode: an 'M' run that ends with the string
    const unsigned last_len = (unsigned)(n - carry.start);
    const unsigned last_nc = !LONG && carry.prev == 'M' ? match_chars(last_len) : 0u;
    if (EMIT) {
      if (lane == 0 && last_nc != 0 && c_text + last_nc <= room) put_match(dst + c_text, last_len);
    } else {
      const int code = whole_code(bad, cq, ct, plen, tlen);
      if (lane == 0) kp.out[pair] = make_text(0, code == AWV_CST_OK ? c_text + last_nc : 0u, code);
      t_failed += code != AWV_CST_OK;
      t_columns += (unsigned long long)n;
    }
  }
  if (!EMIT && lane == 0) {
    if (t_failed) atomicAdd(&kp.counters[1], t_failed);
    if (t_columns) atomicAdd(&kp.counters[2], t_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State : awvw::TextPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_cs_text> d_out;
  std::vector<awv_result> h_recs;  // a batch's records with their slices applied
  std::vector<Span> h_spans;       // and their rectangles
  awv_cs_stats stats{};
  void release() {
    TextPass::release();
    d_pairs.release();
    d_spans.release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
void stats_reset(State* s) { awvw::reset_stats(s); }

namespace {

constexpr const char* TOO_LONG = "cs: an op string of more than 2^30 columns";  // what fits awv_cs_text.len

int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_cs(e), e, v, st, true); }

void launch_kernel(bool emit, int32_t mode, unsigned grid, hipStream_t stream, const KParams& kp) {
  if (emit) {
    if (mode == AWV_CS_LONG) hipLaunchKernelGGL((awv_cs_kernel<true, true>), dim3(grid), dim3(64), 0, stream, kp);
    else hipLaunchKernelGGL((awv_cs_kernel<true, false>), dim3(grid), dim3(64), 0, stream, kp);
  } else {
    if (mode == AWV_CS_LONG) hipLaunchKernelGGL((awv_cs_kernel<false, true>), dim3(grid), dim3(64), 0, stream, kp);
    else hipLaunchKernelGGL((awv_cs_kernel<false, false>), dim3(grid), dim3(64), 0, stream, kp);
  }
}

// One launch over n records whose op bytes are on the device already; a record's slice has been applied to it and to its
// rectangle.  Every index and rectangle is checked here, on the host: the kernels read what the records say.  The
// records' texts take [text_base, *text_end) of the call's cs arena, in record order; csout (host) is filled.  want_text: step 3
// runs and the launch's text is in st->d_text afterwards, its first character the one at text_base.
int launch(const awp::EngineView& v, State* st, int32_t mode, const awv_pair* pairs, const Span* spans, int64_t n, const awv_result* recs,
           const uint8_t* d_arena, uint64_t arena_bytes, uint64_t text_base, bool want_text, awv_cs_text* csout, uint64_t* text_end) {
  *text_end = text_base;
  if (n == 0) return AWV_OK;
  if (int rc = awvw::check_rectangles(v, "cs", pairs, spans, n)) return rc;
  if (int rc = st->begin(v, "cs", n, recs, arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)n));
  AWV_TRY(st->d_spans.reserve((size_t)n));
  AWV_TRY(st->d_out.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, pairs, (size_t)n * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_spans.p, spans, (size_t)n * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  KParams kp{};
  kp.fwd = v.fwd;
  kp.rc = v.rc;
  kp.seq_off = v.off;
  kp.pairs = st->d_pairs.p;
  kp.spans = st->d_spans.p;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.npairs = n;
  awvw::TextLaunch done;
  const auto run = [&](bool emit, unsigned grid, unsigned long long* counters, const awvw::TextArena& text) {
    kp.counters = counters;
    kp.text = text;
    launch_kernel(emit, mode, grid, v.stream, kp);
  };
  if (int rc = st->measure_scan_emit(v, n, st->d_out.p, text_base, want_text, csout, run, done)) return rc;
  st->stats.kernel_ms += done.kernel_ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.failed += done.hc[1];
  st->stats.columns += done.hc[2];
  st->stats.text_bytes += done.bytes;
  *text_end = done.end;
  return AWV_OK;
}

// ranges (nullable; awv_cs_ranges): the call is on ranges[0..n_all) -- `pairs` is not read
int cs_cigars_core(awv_engine* e, int32_t mode, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n_all, const awv_result* results,
                   const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices, uint64_t max_arena, awv_cs_text* csout, uint8_t* text_buf,
                   uint64_t text_cap, uint64_t* text_bytes) {
  if (!mode_ok(mode)) return awv_internal_fail(AWV_ERR_ARG, "cs: mode must be AWV_CS_SHORT or AWV_CS_LONG");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->stats = awv_cs_stats{};
  awvw::ItemCall call;
  if (int rc = awvw::resolve_call(call, v, ranges ? "cs_ranges" : "cs_cigars", pairs, ranges, n_all, results, arena_bytes, slices)) return rc;
  if (int rc = awvw::check_lengths(call.recs, n_all, MAX_COLUMNS, TOO_LONG)) return rc;
  return st->in_pieces(v, call.recs, n_all, cigar_arena, max_arena, text_buf, text_cap, text_bytes,
                       [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes, uint64_t text_base, bool want_text, uint64_t* text_end) {
                         return launch(v, st, mode, call.pairs + first, call.spans.data() + first, n, recs, st->d_arena.p, bytes, text_base, want_text, csout + first,
                                       text_end);
                       });
}

// list: the pairs or ranges
int check_args(const char* name, int64_t n, const void* list, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_text* csout,
               const uint8_t* text_buf, uint64_t text_cap, const uint64_t* text_bytes) {
  if (int rc = awvw::check_call_args(name, n, list, results, text_bytes && (n <= 0 || csout), cigar_arena, arena_bytes)) return rc;
  if (text_cap > 0 && !text_buf) return awv_internal_fail(AWV_ERR_ARG, std::string(name) + ": null text buffer");
  return AWV_OK;
}

}  // namespace

int cs_batch(awv_engine* e, int32_t mode, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
             const awv_clip_result* clips, const Span* spans, awv_cs_text* csout, uint64_t* text_bytes) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->h_spans.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) st->h_spans[(size_t)i] = spans ? spans[i] : awvw::whole_span(v.len_host, pairs[i]);  // (the indices: checked by the aligning call)
  if (clips) {  // the clip's segment is the slice; a record without one has no text
    st->h_recs.assign(results, results + n);
    for (int64_t i = 0; i < n; ++i) {
      const awv_cs_slice sl{clips[i].col_beg, clips[i].col_end, clips[i].q_skip, clips[i].t_skip};
      if (clips[i].code == AWV_CL_OK && slice_ok(results[i], sl)) apply_slice(st->h_recs[(size_t)i], st->h_spans[(size_t)i], sl);
      else drop_record(st->h_recs[(size_t)i]);
    }
    results = st->h_recs.data();
  }
  if (int rc = awvw::check_lengths(results, n, MAX_COLUMNS, TOO_LONG)) return rc;
  return launch(v, st, mode, pairs, st->h_spans.data(), n, results, d_arena, arena_bytes, 0, true, csout, text_bytes);
}

const uint8_t* batch_text(awv_engine* e) {
  const State* st = awv_internal_cs(e);
  return st ? st->d_text.p : nullptr;
}

}  // namespace awvcs

extern "C" {

int awv_cs_one_host(int32_t mode, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen, const uint8_t* cigar, int64_t n,
                    const awv_cs_slice* slice, uint8_t* out_buf, uint64_t cap, awv_cs_text* out) {
  if (!out || !awvcs::mode_ok(mode) || plen < 0 || tlen < 0 || n < 0 || (plen > 0 && !pattern) || (tlen > 0 && !text) || (n > 0 && !cigar) ||
      (cap > 0 && !out_buf))
    return awv_internal_fail(AWV_ERR_ARG, "cs_one_host: bad argument");
  awvw::HostSlice sl;
  if (int rc = awvw::check_host_slice("cs_one_host", slice, n, awvcs::MAX_COLUMNS, sl)) return rc;
  *out = awvcs::cs_one(mode, pattern, plen, text, tlen, cigar + sl.beg, sl.end - sl.beg, sl.q_skip, sl.t_skip, out_buf, cap);
  return AWV_OK;
}

int awv_cs_cigars(awv_engine* e, int32_t mode, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                  uint64_t arena_bytes, const awv_cs_slice* slices, awv_cs_text* csout, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvcs::check_args("cs_cigars", n, pairs, results, cigar_arena, arena_bytes, csout, text_buf, text_cap, text_bytes)) return rc;
  AWV_GUARDED(return awvcs::cs_cigars_core(e, mode, pairs, nullptr, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), csout, text_buf,
                                          text_cap, text_bytes);)
}

int awv_cs_ranges(awv_engine* e, int32_t mode, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena,
                  uint64_t arena_bytes, const awv_cs_slice* slices, awv_cs_text* csout, uint8_t* text_buf, uint64_t text_cap, uint64_t* text_bytes) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvcs::check_args("cs_ranges", n, ranges, results, cigar_arena, arena_bytes, csout, text_buf, text_cap, text_bytes)) return rc;
  static const awv_range_pair none{};
  AWV_GUARDED(return awvcs::cs_cigars_core(e, mode, nullptr, n > 0 ? ranges : &none, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), csout,
                                          text_buf, text_cap, text_bytes);)
}

int awv_engine_cs_stats(const awv_engine* e, awv_cs_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "cs_stats: null argument");
  const awvcs::State* st = awv_internal_cs(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_cs_stats{};
  return AWV_OK;
}

}  // extern "C"
