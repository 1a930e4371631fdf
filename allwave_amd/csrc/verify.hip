// verify.hip -- alignments checked on the device: awv_align_pairs_verified's per-batch check, awv_verify_cigars,
// awv_verify_one_host and awv_engine_verify_stats (include/allwave_hip.h).  What "verified" means is verify_device.hpp;
// this file gets the kernel to the same answer without a serial walk over the op string.
//
// One wave per pair, persistent waves taking pairs (longest op string first) from a cursor.  Per iteration a wave takes a
// chunk of 64 lanes x 16 op bytes, one aligned 16-byte load per lane: the pair's op bytes are addressed from the 16-byte
// boundary at or below their first byte, and bytes outside the string are masked out.  A column's pattern position is the
// number of non-'I' ops before it, its text position the number of non-'D' ops: each lane counts both over its 16 bytes
// with packed byte compares, an exclusive scan over the lanes on the DPP network (row_shr 1/2/4/8, row_bcast15/31, as
// wave_max_i32 in biwfa_device.hpp) places the lane, and the chunk's carry is uniform.  A lane's 16 columns touch at most 16
// consecutive pattern and 16 consecutive text bytes from there on: five aligned dwords each, shifted into place with
// v_alignbyte, then consumed from a 128-bit shift register as the lane walks its columns in registers.
// A gap run's cost needs its length, and a run may span lanes and chunks: "the last column in this lane whose op differs
// from the one before it" goes through the same scan as a max, so every lane knows where the run it starts in began; the
// column that ends a run adds the run's cost to a lane-private sum, reduced once per pair.
// Each lane keeps its first offending column; lanes hold ascending columns, so the lowest lane with one wins.
#include "verify_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "record_pass.hpp"  // the host skeleton of a record pass: RecordPass, pack_piece, AWV_TRY

namespace awvf {

struct KParams {
  const uint8_t* fwd;       // the engine's forward copies
  const uint8_t* rc;        // and reverse-complement copies (the pattern of a q_revcomp pair)
  const uint64_t* seq_off;
  const int32_t* seq_len;
  const awv_pair* pairs;
  const Span* spans;          // nullable (range calls): pair i's pattern / text are these intervals of its sequences
  const awv_result* results;  // cigar_off relative to `arena`
  const int32_t* order;       // dispatch slot -> pair
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_verify_result* out;
  unsigned long long* counters;  // [0] cursor, [1] failed pairs, [2] columns of checked pairs
  long long npairs;
  awv_penalties pen;
};

using awvw::byte_range_mask;  // (wave_ops.hpp: the chunk, the scans and the byte counting shared with clip.hip)
using awvw::CHUNK;
using awvw::count_bytes;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::u32x4;
using awvw::wave_scan_add;
using awvw::wave_scan_max;
using awvw::wave_sum_i64;

// 16 bytes of a sequence from position `pos` on, as two 64-bit halves: five aligned dwords, shifted into place.  Dwords
// that start at or behind the sequence's end are not read; a dword that starts inside it ends at most 3 bytes behind it,
// inside the engine's padding.
static_assert(awp::SEQ_PAD_BYTES >= 3, "load16 reads whole dwords that start inside a sequence: the layout must pad every sequence by 3 bytes or more");
__device__ __forceinline__ void load16(const uint8_t* seq, int len, int pos, unsigned long long& lo, unsigned long long& hi) {
  const uintptr_t addr = (uintptr_t)seq + (uintptr_t)pos, end = (uintptr_t)seq + (uintptr_t)len;
  const unsigned* a = (const unsigned*)(addr & ~(uintptr_t)3);
  const unsigned s = (unsigned)(addr & 3);
  unsigned d[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) d[k] = (uintptr_t)(a + k) < end ? a[k] : 0u;
  unsigned x[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], s);
  lo = (unsigned long long)x[0] | ((unsigned long long)x[1] << 32);
  hi = (unsigned long long)x[2] | ((unsigned long long)x[3] << 32);
}

__global__ __launch_bounds__(64) void awv_verify_kernel(KParams kp) {
  const int lane = threadIdx.x;
  unsigned long long n_failed = 0, n_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result claimed = kp.results[pair];
    if (claimed.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[pair] = make_result(AWV_VF_SKIPPED, -1, -1);
      continue;
    }
    const awv_pair pr = kp.pairs[pair];
    int plen = kp.seq_len[pr.q_idx], tlen = kp.seq_len[pr.t_idx];
    const uint8_t* pattern = (pr.q_revcomp ? kp.rc : kp.fwd) + kp.seq_off[pr.q_idx];
    const uint8_t* text = kp.fwd + kp.seq_off[pr.t_idx];
    if (kp.spans) {  // (validated on the host: inside the sequences)
      const Span sp = kp.spans[pair];
      pattern += sp.pb;
      text += sp.tb;
      plen = sp.pe - sp.pb;
      tlen = sp.te - sp.tb;
    }
    // every passing column consumes a base: an op string longer than plen + tlen fails within its first plen + tlen + 1 columns
    const long long n_claimed = (long long)claimed.cigar_len;
    const int n = (int)min(n_claimed, (long long)plen + tlen + 1);
    const int sh = (int)(claimed.cigar_off & 15);
    const uint8_t* ops = kp.arena + (claimed.cigar_off & ~(uint64_t)15);
    const int span = sh + n;  // op byte c is ops[sh + c]
    n_columns += (unsigned long long)n;

    int cq = 0, ct = 0;         // bases consumed before the chunk (uniform)
    int c_start = 0;            // the column the run in progress began at
    unsigned c_prev = 0;        // the op before the chunk's first column (0: none)
    long long sum = 0;          // lane-private: mismatches and ended gap runs
    int nx = 0;                 // lane-private: 'X' columns
    bool failed = false;
    for (int base = 0; n > 0 && base < span; base += CHUNK) {
      const int b0 = base + lane * LANE_BYTES;
      const int jlo = min(max(sh - b0, 0), LANE_BYTES), jhi = min(max(span - b0, 0), LANE_BYTES);  // this lane's bytes [jlo, jhi) are columns
      const int nv = max(jhi - jlo, 0);
      u32x4 w = {0u, 0u, 0u, 0u};
      if (b0 < span) w = *(const u32x4*)(ops + b0);
      int n_i = 0, n_d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] &= byte_range_mask(jlo - 4 * k, jhi - 4 * k);
        n_i += count_bytes(w[k], 'I');
        n_d += count_bytes(w[k], 'D');
      }
      const int lq = nv - n_i, lt = nv - n_d;
      // the op before this lane's first column: the lower lane's last byte, the chunk's carry in lane 0, none at column 0
      unsigned prev = (unsigned)from_lower_lane((int)w[3], (int)(c_prev << 24)) >> 24;
      if (b0 <= sh) prev = 0;
      int last_break = -1;
      {
        unsigned pv = prev;
#pragma unroll
        for (int j = 0; j < LANE_BYTES; ++j) {
          const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
          const bool valid = j >= jlo && j < jhi;
          if (valid && op != pv) last_break = b0 + j - sh;
          if (valid) pv = op;
        }
      }
      const int iq = wave_scan_add(lq), it = wave_scan_add(lt), ib = wave_scan_max(last_break);
      int q = cq + iq - lq, t = ct + it - lt;
      int run_start = max(c_start, from_lower_lane(ib, -1));

      unsigned long long p_lo = 0, p_hi = 0, t_lo = 0, t_hi = 0;
      if (nv > 0) {
        load16(pattern, plen, q, p_lo, p_hi);
        load16(text, tlen, t, t_lo, t_hi);
      }
      int fail_code = 0, fail_col = 0;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j >= jlo && j < jhi && fail_code == 0) {
          const int col = b0 + j - sh;
          const int code = column_code(op, q < plen, t < tlen, (unsigned)p_lo & 0xffu, (unsigned)t_lo & 0xffu);
          if (code != AWV_VF_OK) {
            fail_code = code;
            fail_col = col;
          } else {
            if (op != prev) {
              sum += run_end_cost(kp.pen, prev, run_start, col);
              run_start = col;
              prev = op;
            }
            if (op == 'X') {
              sum += kp.pen.mismatch;
              ++nx;
            }
            if (takes_pattern(op)) {
              ++q;
              p_lo = (p_lo >> 8) | (p_hi << 56);
              p_hi >>= 8;
            }
            if (takes_text(op)) {
              ++t;
              t_lo = (t_lo >> 8) | (t_hi << 56);
              t_hi >>= 8;
            }
          }
        }
      }
      const unsigned long long bad = __ballot(fail_code != 0);
      if (bad != 0) {  // lanes hold ascending columns: the lowest lane's is the first
        const int l = __builtin_ctzll(bad);
        const int code = __builtin_amdgcn_readlane(fail_code, l), col = __builtin_amdgcn_readlane(fail_col, l);
        if (lane == 0) kp.out[pair] = make_result(code, col, -1);
        failed = true;
        break;
      }
      const int last_lane = min(63, (span - 1 - base) >> 4);  // the lane that holds the chunk's last column
      c_prev = (unsigned)__builtin_amdgcn_readlane((int)prev, last_lane);
      c_start = __builtin_amdgcn_readlane(run_start, last_lane);
      cq += __builtin_amdgcn_readlane(iq, 63);
      ct += __builtin_amdgcn_readlane(it, 63);
    }
    if (failed) {
      ++n_failed;
      continue;
    }
    const long long penalty = wave_sum_i64(sum) + run_end_cost(kp.pen, c_prev, c_start, n);
    const long long nx_all = wave_sum_i64(nx);
    const int code = whole_code(claimed, n_claimed, plen, tlen, cq, ct, nx_all, penalty);
    if (lane == 0) kp.out[pair] = make_result(code, -1, penalty);
    n_failed += code != AWV_VF_OK;
  }
  if (lane == 0) {
    if (n_failed) atomicAdd(&kp.counters[1], n_failed);
    if (n_columns) atomicAdd(&kp.counters[2], n_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_verify_result> d_out;
  awv_verify_stats stats{};
  void release() {
    RecordPass::release();
    d_pairs.release();
    d_spans.release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
void stats_reset(State* s) { awvw::reset_stats(s); }

namespace {

// the engine's own sign rules for penalties (engine.hip; re-scoring has no ring to fit, so any size goes), then the unused piece of a gap-affine set cleared
int check_penalties(const awv_penalties* p, awv_penalties& out) {
  if (int rc = awv_internal_check_penalties(p)) return rc;
  out = *p;
  out.two_piece = p->two_piece ? 1 : 0;
  if (!out.two_piece) out.gap_open2 = out.gap_ext2 = 0;
  return AWV_OK;
}

int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_verify(e), e, v, st, true); }

// One launch over n pairs whose op bytes are on the device already.  Every index is checked here, on the host, as
// RecordPass::begin checks every op string's place in the arena: the kernel reads what the records say.
int launch(const awp::EngineView& v, State* st, const awv_penalties& pen, const awv_pair* pairs, int64_t n, const awv_result* results,
           const uint8_t* d_arena, uint64_t arena_bytes, awv_verify_result* vout, const Span* spans = nullptr) {
  if (n == 0) return AWV_OK;
  for (int64_t i = 0; i < n; ++i)
    if (pairs[i].q_idx < 0 || pairs[i].q_idx >= v.n || pairs[i].t_idx < 0 || pairs[i].t_idx >= v.n)
      return awv_internal_fail(AWV_ERR_ARG, "verify: sequence index out of range");
  if (int rc = st->begin(v, "verify", n, results, arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)n));
  AWV_TRY(st->d_out.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, pairs, (size_t)n * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  if (spans) {
    AWV_TRY(st->d_spans.reserve((size_t)n));
    AWV_TRY(hipMemcpyAsync(st->d_spans.p, spans, (size_t)n * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  }
  if (int rc = st->clear_counters(v, 4)) return rc;
  KParams kp{};
  kp.fwd = v.fwd;
  kp.rc = v.rc;
  kp.seq_off = v.off;
  kp.seq_len = v.len;
  kp.pairs = st->d_pairs.p;
  kp.spans = spans ? st->d_spans.p : nullptr;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.pen = pen;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_verify_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  unsigned long long hc[4] = {0, 0, 0, 0};
  float ms = 0;
  AWV_TRY(hipMemcpyAsync(vout, st->d_out.p, (size_t)n * sizeof(awv_verify_result), hipMemcpyDeviceToHost, v.stream));
  if (int rc = st->finish(v, hc, 4, ms)) return rc;
  st->stats.kernel_ms += ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.failed += hc[1];
  st->stats.columns += hc[2];
  return AWV_OK;
}

// ranges (nullable; awv_verify_ranges): the call is on ranges[0..npairs) -- `pairs` is not read
int verify_cigars_core(awv_engine* e, const awv_penalties* pen_in, const awv_pair* pairs, int64_t npairs, const awv_result* results,
                       const uint8_t* cigar_arena, uint64_t arena_bytes, uint64_t max_arena, awv_verify_result* vout,
                       const awv_range_pair* ranges = nullptr) {
  awv_penalties pen;
  if (int rc = check_penalties(pen_in, pen)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->stats = awv_verify_stats{};
  std::vector<awv_pair> rpairs;
  std::vector<Span> spans;
  if (ranges) {
    rpairs.resize((size_t)npairs);
    spans.resize((size_t)npairs);
    for (int64_t i = 0; i < npairs; ++i)
      if (!awvr::split_range(v.len_host, v.n, ranges[i], rpairs[(size_t)i], spans[(size_t)i]))
        return awv_internal_fail(AWV_ERR_ARG, "verify_ranges: range " + std::to_string(i) + " names a sequence index or an interval out of range");
    pairs = rpairs.data();
  }
  // before anything goes up: every completed record's op bytes lie inside the caller's arena
  for (int64_t i = 0; i < npairs; ++i)
    if (awvw::outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "verify_cigars: a record's op bytes lie outside the CIGAR arena");
  // in pieces (record_pieces.hpp); this pass alone packs every string at the start of its slot
  std::vector<uint8_t> stage;
  std::vector<awv_result> recs;
  for (int64_t first = 0; first < npairs;) {
    const awvw::Piece pc = awvw::pack_piece(results, npairs, first, cigar_arena, max_arena, false, recs, stage);
    AWV_TRY(st->d_arena.reserve((size_t)pc.bytes + 64));
    if (pc.bytes) AWV_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
    if (int rc = launch(v, st, pen, pairs + first, pc.n, recs.data(), st->d_arena.p, pc.bytes, vout + first, ranges ? spans.data() + first : nullptr)) return rc;
    first += pc.n;
  }
  return AWV_OK;
}

}  // namespace

int verify_batch(awv_engine* e, const awv_penalties* pen_in, const awv_pair* pairs, int64_t n, const awv_result* results,
                 const uint8_t* d_arena, uint64_t arena_bytes, awv_verify_result* vout, const Span* spans) {
  awv_penalties pen;
  if (int rc = check_penalties(pen_in, pen)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  return launch(v, st, pen, pairs, n, results, d_arena, arena_bytes, vout, spans);
}

}  // namespace awvf

extern "C" {

int awv_verify_cigars(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const awv_result* results,
                      const uint8_t* cigar_arena, uint64_t arena_bytes, awv_verify_result* vout) {
  if (!e) return awv_internal_null_engine();
  if (npairs < 0 || (npairs > 0 && (!pairs || !results || !vout))) return awv_internal_fail(AWV_ERR_ARG, "verify_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "verify_cigars: null arena");
  AWV_GUARDED(return awvf::verify_cigars_core(e, pen, pairs, npairs, results, cigar_arena, arena_bytes, awv_internal_max_arena(e), vout);)
}

int awv_verify_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                      const uint8_t* cigar_arena, uint64_t arena_bytes, awv_verify_result* vout) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || (n > 0 && (!ranges || !results || !vout))) return awv_internal_fail(AWV_ERR_ARG, "verify_ranges: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "verify_ranges: null arena");
  AWV_GUARDED(return awvf::verify_cigars_core(e, pen, nullptr, n, results, cigar_arena, arena_bytes, awv_internal_max_arena(e), vout, ranges);)
}

int awv_verify_one_host(const awv_penalties* pen, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                        const uint8_t* cigar, int64_t n, const awv_result* claimed, awv_verify_result* out) {
  awv_penalties p;
  if (int rc = awvf::check_penalties(pen, p)) return rc;
  if (!claimed || !out || plen < 0 || tlen < 0 || n < 0 || (plen > 0 && !pattern) || (tlen > 0 && !text) || (n > 0 && !cigar))
    return awv_internal_fail(AWV_ERR_ARG, "verify_one_host: bad argument");
  *out = awvf::verify_one(p, pattern, plen, text, tlen, cigar, n, *claimed);
  return AWV_OK;
}

int awv_engine_verify_stats(const awv_engine* e, awv_verify_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "verify_stats: null argument");
  const awvf::State* st = awv_internal_verify(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_verify_stats{};
  return AWV_OK;
}

}  // extern "C"
