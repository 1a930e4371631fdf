// encode.hip -- run-length CIGAR text made on the device: the last per-batch step of awv_align_pairs_encoded /
// awv_align_ranges_encoded, awv_encode_cigars, awv_encode_one_host and awv_engine_encode_stats (include/allwave_hip.h).  What
// the text of an op string is is encode_device.hpp; this file gets the kernels to the same bytes.
//
// verify.hip's shape: one wave per record, persistent waves taking records (longest op string first) from a cursor.  The size
// of the output depends on the data, so there are three steps on the stream:
//   1. measure: every record's text length and run count (awv_cigar_text.len / .runs);
//   2. scan: one workgroup's exclusive scan over `len` in record order gives every record its place (.off) in a dense text
//      arena and the arena's size, the only thing the host waits for before it sizes the text buffer;
//   3. emit: the same walk again, now writing every run's characters at its place.
// The walk takes a string in chunks of 64 lanes x 16 op bytes, one aligned 16-byte load per lane.  A run ends where a byte differs
// from the one before it (a "break"): the lane that holds the break owns the run that ends there.  Where that run began is the
// last break before it -- among the lane's own bytes, else from a max-scan over the lanes' last breaks, else the carry of the
// chunks before.  The characters a lane's runs take (digits + 1 each) go through an add-scan, with a carry, which gives every
// lane the text offset of its first run; a lane owns up to 16 runs and writes them one after the other.  The string's last run
// has no break behind it and is written when the chunks are done.
// The text is stored byte by byte, straight to global memory (DESIGN.md 4.29 has the reason and what it costs).
#include "encode_device.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "record_pass.hpp"  // the host skeleton of a record pass: RecordPass, pack_piece, AWV_TRY

namespace awve {

struct KParams {
  const awv_result* results;     // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;          // dispatch slot -> record
  const uint8_t* arena;          // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_cigar_text* out;           // measure writes len and runs, the scan off, emit reads all three
  uint8_t* text;                 // emit: the launch's text arena, text_bytes of it; text[0] is the character at offset text_base
  unsigned long long text_base, text_bytes;
  unsigned long long* counters;  // [0] this kernel's cursor; measure: [1] runs, [2] columns
  long long npairs;
};

using awvw::CHUNK;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::u32x4;
using awvw::wave_scan_add;
using awvw::wave_scan_max;

__device__ __forceinline__ unsigned byte_at(const u32x4& w, int j) {  // byte j of a lane's 16, j in a register
  const int k = j >> 2;
  const unsigned d = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
  return (d >> (8 * (j & 3))) & 0xffu;
}

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
    // emit: the record's characters are dst[0 .. room), inside the text arena by the scan -- checked all the same, so that nothing
    // is ever stored outside the buffer
    uint8_t* dst = nullptr;
    unsigned room = 0;
    if (EMIT) {
      const awv_cigar_text t = kp.out[pair];
      if (t.off >= kp.text_base && t.off - kp.text_base <= kp.text_bytes && (unsigned long long)t.len <= kp.text_bytes - (t.off - kp.text_base)) {
        dst = kp.text + (t.off - kp.text_base);
        room = t.len;
      }
    }
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    long long c_start = 0;  // the column the run in progress began at (uniform, like everything carried)
    unsigned c_prev = 0;    // the op before the chunk's first column
    unsigned c_text = 0;    // characters of the runs that ended in the chunks before
    unsigned c_runs = 0;
    for (long long base = 0; base < span; base += CHUNK) {
      const long long b0 = base + lane * LANE_BYTES;
      const int jlo = (int)min(max((long long)sh - b0, 0ll), (long long)LANE_BYTES), jhi = (int)min(max(span - b0, 0ll), (long long)LANE_BYTES);  // this lane's bytes [jlo, jhi) are columns
      u32x4 w = {0u, 0u, 0u, 0u};
      if (b0 < span) w = *(const u32x4*)(ops + b0);
      // the op before this lane's first byte: the lower lane's last byte, the chunk's carry in lane 0 (column 0 has none: it is no break)
      const unsigned prev = (unsigned)from_lower_lane((int)w[3], (int)(c_prev << 24)) >> 24;
      unsigned brk = 0;  // bit j: byte j is a column > 0 whose op differs from the one before it
      unsigned pv = prev;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j >= jlo && j < jhi) {
          if (op != pv && b0 + j > sh) brk |= 1u << j;
          pv = op;
        }
      }
      const int key = brk != 0 ? lane * LANE_BYTES + (31 - __builtin_clz(brk)) : -1;  // the lane's last break, as a byte position in the chunk
      const int kin = wave_scan_max(key);
      const int kex = from_lower_lane(kin, -1);
      const long long rs0 = kex >= 0 ? base + kex - sh : c_start;  // the run this lane begins in started here

      // the characters and the count of the runs this lane owns
      int chars = 0;
      {
        long long start = rs0;
        for (unsigned m = brk; m != 0; m &= m - 1) {
          const long long col = b0 + __builtin_ctz(m) - sh;
          chars += (int)run_chars((unsigned)(col - start));
          start = col;
        }
      }
      const int packed = chars | (__popc(brk) << 16);  // (a lane's runs take at most 11 + 15 * 3 characters: a chunk's sums fit 16 bits each)
      const int s_in = wave_scan_add(packed);
      if (EMIT) {
        unsigned at = c_text + (unsigned)((s_in - packed) & 0xffff);
        long long start = rs0;
        for (unsigned m = brk; m != 0; m &= m - 1) {
          const int j = __builtin_ctz(m);
          const long long col = b0 + j - sh;
          const unsigned len = (unsigned)(col - start);
          const unsigned nc = run_chars(len);
          if (at + nc <= room) put_run(dst + at, len, j > 0 ? byte_at(w, j - 1) : prev);
          at += nc;
          start = col;
        }
      }

      const int last_lane = (int)min(63ll, (span - 1 - base) >> 4);  // the lane that holds the chunk's last column
      c_prev = (unsigned)__builtin_amdgcn_readlane((int)pv, last_lane);
      const int kall = __builtin_amdgcn_readlane(kin, 63);
      if (kall >= 0) c_start = base + kall - sh;
      const int tot = __builtin_amdgcn_readlane(s_in, 63);
      c_text += (unsigned)(tot & 0xffff);
      c_runs += (unsigned)(tot >> 16);
    }
    // the last run ends with the string
    const unsigned last_len = (unsigned)(n - c_start);
    const unsigned last_nc = run_chars(last_len);
    if (lane == 0) {
      if (EMIT) {
        if (c_text + last_nc <= room) put_run(dst + c_text, last_len, c_prev);
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

// Step 2: out[i].off = base + the sum of out[0 .. i).len, in record order; *total = base + the sum of them all.  One workgroup of
// sixteen waves takes the records in tiles of 1,024: a wave scan, the waves' sums through LDS, the tiles' sum carried on.
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void awv_encode_scan_kernel(awv_cigar_text* out, long long n, unsigned long long base, unsigned long long* total) {
  __shared__ unsigned long long wave_sum[SCAN_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  unsigned long long carry = base;
  for (long long tile = 0; tile < n; tile += SCAN_THREADS) {
    const long long i = tile + tid;
    const unsigned long long len = i < n ? (unsigned long long)out[i].len : 0ull;
    const unsigned long long inc = (unsigned long long)wave_scan_add((long long)len);
    if ((tid & 63) == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < SCAN_THREADS / 64; ++k) {
      const unsigned long long s = wave_sum[k];
      if (k < wave) before += s;
      all += s;
    }
    if (i < n) out[i].off = carry + before + inc - len;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

constexpr int N_COUNTERS = 16;  // [0..2] the measure kernel's, [4] the scan's total, [8] the emit kernel's cursor

struct State : awvw::RecordPass {
  Buf<awv_cigar_text> d_out;
  Buf<uint8_t> d_text;              // the text arena of the launch in hand
  std::vector<awv_result> h_recs;   // a batch's records with their slices applied
  awv_encode_stats stats{};
  void release() {
    RecordPass::release();
    d_out.release();
    d_text.release();
  }
};

void state_release(State* s) {
  if (!s) return;
  s->release();
  delete s;
}

void stats_reset(State* s) {
  if (s) s->stats = awv_encode_stats{};
}

namespace {

// what fits awv_cigar_text.len: refused before anything is launched
int check_lengths(const awv_result* recs, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (recs[i].status == AWV_ST_COMPLETED && (int64_t)recs[i].cigar_len > MAX_COLUMNS)
      return awv_internal_fail(AWV_ERR_ARG, "encode: an op string of more than 2^31 - 1 columns");
  return AWV_OK;
}

int open_state(awv_engine* e, awp::EngineView& v, State*& st) {
  State*& slot = awv_internal_encode(e);
  if (!slot) slot = new State();
  st = slot;
  return st->open(e, v, false);  // (the text reads no sequence: an engine without a set will do, and is no error)
}

// One launch over n records whose op bytes are on the device already; a record's slice has been applied to it.  The records'
// texts take [text_base, *text_end) of the call's text arena, in record order; tout (host) is filled.  want_text: step 3 runs
// and the launch's text is in st->d_text afterwards, its first character the one at text_base.
int launch(const awp::EngineView& v, State* st, int64_t n, const awv_result* recs, const uint8_t* d_arena, uint64_t arena_bytes, uint64_t text_base,
           bool want_text, awv_cigar_text* tout, uint64_t* text_end) {
  *text_end = text_base;
  if (n == 0) return AWV_OK;
  if (int rc = st->begin(v, "encode", n, recs, arena_bytes)) return rc;
  AWV_TRY(st->d_out.reserve((size_t)n));
  if (int rc = st->clear_counters(v, N_COUNTERS)) return rc;
  KParams kp{};
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  const unsigned grid = st->grid(v, n);
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_encode_kernel<false>, dim3(grid), dim3(64), 0, v.stream, kp);
  hipLaunchKernelGGL(awv_encode_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, v.stream, st->d_out.p, (long long)n, (unsigned long long)text_base,
                     st->d_counters.p + 4);
  if (int rc = st->stop(v)) return rc;
  // the arena's size: all the host waits for before the text buffer is sized
  unsigned long long total = 0;
  float ms = 0, ms_emit = 0;
  AWV_TRY(hipMemcpyAsync(&total, st->d_counters.p + 4, sizeof(total), hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  AWV_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
  const uint64_t bytes = total - text_base;
  const bool emit = want_text && bytes > 0;
  if (emit) {
    AWV_TRY(st->d_text.reserve((size_t)bytes + 64));
    kp.text = st->d_text.p;
    kp.text_base = text_base;
    kp.text_bytes = bytes;
    kp.counters = st->d_counters.p + 8;
    if (int rc = st->start(v)) return rc;
    hipLaunchKernelGGL(awv_encode_kernel<true>, dim3(grid), dim3(64), 0, v.stream, kp);
    if (int rc = st->stop(v)) return rc;
  }
  unsigned long long hc[4] = {0, 0, 0, 0};
  AWV_TRY(hipMemcpyAsync(tout, st->d_out.p, (size_t)n * sizeof(awv_cigar_text), hipMemcpyDeviceToHost, v.stream));
  if (int rc = st->finish(v, hc, 4, ms_emit)) return rc;
  st->stats.kernel_ms += ms + (emit ? ms_emit : 0.f);
  st->stats.pairs += (uint64_t)n;
  st->stats.runs += hc[1];
  st->stats.columns += hc[2];
  st->stats.text_bytes += bytes;
  *text_end = total;
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
  if (int rc = check_lengths(results, n_all)) return rc;
  // in pieces (record_pieces.hpp) that keep every string's offset modulo 16; the offsets run on from piece to piece.  A piece's
  // text is kept here while the text so far fits the caller's buffer, which is written at the end, all of it or none.
  std::vector<uint8_t> stage, text;
  std::vector<awv_result> recs;
  uint64_t at = 0;
  bool fits = text_buf != nullptr;
  for (int64_t first = 0; first < n_all;) {
    const awvw::Piece pc = awvw::pack_piece(results, n_all, first, cigar_arena, max_arena, true, recs, stage);
    AWV_TRY(st->d_arena.reserve((size_t)pc.bytes + 64));
    if (pc.bytes) AWV_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
    uint64_t end = at;
    if (int rc = launch(v, st, pc.n, recs.data(), st->d_arena.p, pc.bytes, at, fits, tout + first, &end)) return rc;
    fits = fits && end <= text_cap;
    if (fits && end > at) {
      text.resize((size_t)end);
      AWV_TRY(hipMemcpyAsync(text.data() + at, st->d_text.p, (size_t)(end - at), hipMemcpyDeviceToHost, v.stream));
      AWV_TRY(hipStreamSynchronize(v.stream));
    }
    at = end;
    first += pc.n;
  }
  *text_bytes = at;
  if (fits && at > 0) std::memcpy(text_buf, text.data(), (size_t)at);
  return AWV_OK;
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
  if (int rc = check_lengths(results, n)) return rc;
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
