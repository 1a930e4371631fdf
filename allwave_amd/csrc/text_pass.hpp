// text_pass.hpp -- what a text pass shares on top of record_pass.hpp: a record pass whose output's size depends
// on the data, so that it takes three steps on the stream.  encode.hip (awv_cigar_text) and cs.hip (awv_cs_text) are the two;
// variants.hip, whose rows are placed the same way, takes the walk by runs and the scan kernel from here.
//   1. measure: the pass's kernel walks every record and writes its text length (Text.len, and the pass's own 32-bit field);
//   2. scan: awv_text_scan_kernel's exclusive scan over `len` in record order gives every record its place (Text.off) in a dense
//      text arena and the arena's size, the only thing the host waits for before it sizes the text buffer;
//   3. emit: the pass's kernel walks the records again, now writing every character at its place (text_dest).
// The walk takes a string in chunks of 64 lanes x 16 op bytes.  A run ends where a byte differs from the one before it (a "break"):
// the lane that holds the break owns the run that ends there, and the run began at the last break before it -- among the lane's own
// bytes, else from a max-scan over the lanes' last breaks, else the carry of the chunks before (lane_runs, run_start_before,
// carry_on).  The string's last run has no break behind it: it is n - RunCarry.start columns of RunCarry.prev when the chunks are done.
#pragma once

#include <cstring>
#include <vector>

#include "record_pass.hpp"  // RecordPass, pack_piece, AWV_TRY

namespace awvw {

// ---- device side ---------------------------------------------------------------------------------------------------------

// emit: the launch's text arena, `bytes` of it; text[0] is the character at offset `base` of the call's arena (measure: all zero)
struct TextArena {
  uint8_t* text;
  unsigned long long base, bytes;
};

struct TextDest {
  uint8_t* dst;   // a record's characters are dst[0 .. room)
  unsigned room;
};
// The place of a record's text {off, len}: inside the arena by the scan -- checked all the same, so that nothing is ever stored
// outside the buffer (no place: nullptr, 0).
__device__ __forceinline__ TextDest text_dest(const TextArena& a, unsigned long long off, unsigned len) {
  if (off >= a.base && off - a.base <= a.bytes && (unsigned long long)len <= a.bytes - (off - a.base)) return TextDest{a.text + (off - a.base), len};
  return TextDest{nullptr, 0u};
}

// What a wave carries from chunk to chunk of one op string (uniform, like everything carried).
struct RunCarry {
  long long start = 0;  // the column the run in progress began at
  unsigned prev = 0;    // the op before the chunk's first column
};

// One lane's 16 op bytes of a chunk and the breaks among them.  Op byte c of the string is ops[sh + c]: b0 is a position in that
// frame, and byte j of the lane is column b0 + j - sh.
struct LaneRuns {
  long long b0;   // the lane's first byte
  int jlo, jhi;   // this lane's bytes [jlo, jhi) are columns
  u32x4 w;        // the bytes (0 behind the string)
  unsigned prev;  // the op before the lane's first byte: the lower lane's last byte, the carry in lane 0 (column 0 has none: it is no break)
  unsigned last;  // the op of the lane's last column (prev: it has none)
  unsigned brk;   // bit j: byte j is a column > 0 whose op differs from the one before it
  int kin;        // the last break in this lane or a lower one, as a byte position in the chunk (-1: none)
  long long rs0;  // the column at which the run this lane begins in started
};

__device__ __forceinline__ LaneRuns lane_runs(const uint8_t* ops, int sh, long long span, long long base, int lane, const RunCarry& c) {
  LaneRuns r;
  r.b0 = base + lane * LANE_BYTES;
  r.jlo = (int)min(max((long long)sh - r.b0, 0ll), (long long)LANE_BYTES);
  r.jhi = (int)min(max(span - r.b0, 0ll), (long long)LANE_BYTES);
  r.w = u32x4{0u, 0u, 0u, 0u};
  if (r.b0 < span) r.w = *(const u32x4*)(ops + r.b0);
  r.prev = (unsigned)from_lower_lane((int)r.w[3], (int)(c.prev << 24)) >> 24;
  r.brk = 0;
  r.last = r.prev;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j) {
    const unsigned op = (r.w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    if (j >= r.jlo && j < r.jhi) {
      if (op != r.last && r.b0 + j > sh) r.brk |= 1u << j;
      r.last = op;
    }
  }
  const int key = r.brk != 0 ? lane * LANE_BYTES + (31 - __builtin_clz(r.brk)) : -1;  // the lane's last break
  r.kin = wave_scan_max(key);
  const int kex = from_lower_lane(r.kin, -1);
  r.rs0 = kex >= 0 ? base + kex - sh : c.start;
  return r;
}

// the column at which the run that ends at the lane's break j began: the last break before it
__device__ __forceinline__ long long run_start_before(const LaneRuns& r, int sh, int j) {
  const unsigned lower_brk = r.brk & ((1u << j) - 1u);
  return lower_brk != 0 ? r.b0 + (31 - __builtin_clz(lower_brk)) - sh : r.rs0;
}

// at the end of a chunk: the op of its last column and the chunk's last break go on to the next
__device__ __forceinline__ void carry_on(RunCarry& c, const LaneRuns& r, int sh, long long span, long long base) {
  c.prev = (unsigned)__builtin_amdgcn_readlane((int)r.last, last_column_lane(span, base));
  const int kall = __builtin_amdgcn_readlane(r.kin, 63);
  if (kall >= 0) c.start = base + kall - sh;
}

// Step 2: out[i].off = base + the sum of out[0 .. i).len, in record order; *total = base + the sum of them all.  One workgroup of
// sixteen waves takes the records in tiles of 1,024: a wave scan, the waves' sums through LDS, the tiles' sum carried on.
constexpr int SCAN_THREADS = 1024;
template <typename Text>
__global__ __launch_bounds__(SCAN_THREADS) void awv_text_scan_kernel(Text* out, long long n, unsigned long long base, unsigned long long* total) {
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

// ---- host side -----------------------------------------------------------------------------------------------------------

constexpr int TEXT_COUNTERS = 16;  // [0..2] the measure kernel's (cursor and the pass's two), [4] the scan's total, [8] the emit kernel's cursor

struct TextLaunch {              // what one measure_scan_emit did
  uint64_t end = 0;              // the records' texts take [text_base, end) of the call's arena
  uint64_t bytes = 0;            // end - text_base
  float kernel_ms = 0;           // measure + scan, and emit where it ran
  unsigned long long hc[4] = {0, 0, 0, 0};  // the measure kernel's counters
};

struct TextPass : RecordPass {
  Buf<uint8_t> d_text;  // the text arena of the launch in hand
  void release() {
    RecordPass::release();
    d_text.release();
  }

  // Behind begin() and the pass's own uploads and reserves: the three steps over n records whose Text records are d_out.
  // run(emit, grid, counters, arena) launches the pass's kernel on v.stream.  The texts take [text_base, out.end) of the call's
  // arena; tout (host) is filled.  want_text: step 3 runs and the launch's text is in d_text afterwards, its first character the
  // one at text_base.
  template <typename Text, typename Run>
  int measure_scan_emit(const awp::EngineView& v, int64_t n, Text* d_out, uint64_t text_base, bool want_text, Text* tout, Run&& run, TextLaunch& out) {
    if (int rc = clear_counters(v, TEXT_COUNTERS)) return rc;
    const unsigned grid = this->grid(v, n);
    if (int rc = start(v)) return rc;
    run(false, grid, d_counters.p, TextArena{nullptr, 0ull, 0ull});
    hipLaunchKernelGGL(awv_text_scan_kernel<Text>, dim3(1), dim3(SCAN_THREADS), 0, v.stream, d_out, (long long)n, (unsigned long long)text_base, d_counters.p + 4);
    if (int rc = stop(v)) return rc;
    // the arena's size: all the host waits for before the text buffer is sized
    unsigned long long total = 0;
    float ms = 0, ms_emit = 0;
    AWV_TRY(hipMemcpyAsync(&total, d_counters.p + 4, sizeof(total), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
    AWV_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    out.bytes = total - text_base;
    const bool emit = want_text && out.bytes > 0;
    if (emit) {
      AWV_TRY(d_text.reserve((size_t)out.bytes + 64));
      if (int rc = start(v)) return rc;
      run(true, grid, d_counters.p + 8, TextArena{d_text.p, (unsigned long long)text_base, (unsigned long long)out.bytes});
      if (int rc = stop(v)) return rc;
    }
    AWV_TRY(hipMemcpyAsync(tout, d_out, (size_t)n * sizeof(Text), hipMemcpyDeviceToHost, v.stream));
    if (int rc = finish(v, out.hc, 4, ms_emit)) return rc;
    out.kernel_ms = ms + (emit ? ms_emit : 0.f);
    out.end = total;
    return AWV_OK;
  }

  // awv_*_cigars: the call in pieces (each_piece); the offsets run on from piece to piece.  launch_piece(first, n, recs,
  // arena_bytes, text_base, want_text, &end) is the pass's launch over records [first, first + n), whose op bytes are in d_arena.
  // A piece's text is kept here while the text so far fits the caller's buffer, which is written at the end, all of it or none.
  template <typename LaunchPiece>
  int in_pieces(const awp::EngineView& v, const awv_result* results, int64_t n_all, const uint8_t* cigar_arena, uint64_t max_arena, uint8_t* text_buf,
                uint64_t text_cap, uint64_t* text_bytes, LaunchPiece&& launch_piece) {
    std::vector<uint8_t> text;
    uint64_t at = 0;
    bool fits = text_buf != nullptr;
    const auto piece = [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes) {
      uint64_t end = at;
      if (int rc = launch_piece(first, n, recs, bytes, at, fits, &end)) return rc;
      fits = fits && end <= text_cap;
      if (fits && end > at) {
        text.resize((size_t)end);
        AWV_TRY(hipMemcpyAsync(text.data() + at, d_text.p, (size_t)(end - at), hipMemcpyDeviceToHost, v.stream));
        AWV_TRY(hipStreamSynchronize(v.stream));
      }
      at = end;
      return (int)AWV_OK;
    };
    if (int rc = each_piece(v, results, n_all, cigar_arena, max_arena, piece)) return rc;
    *text_bytes = at;
    if (fits && at > 0) std::memcpy(text_buf, text.data(), (size_t)at);
    return AWV_OK;
  }
};

}  // namespace awvw
