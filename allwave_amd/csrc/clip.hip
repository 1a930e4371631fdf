// clip.hip -- alignments clipped to their best-scoring segment on the device: awv_align_pairs_clipped's per-batch step,
// awv_clip_cigars, awv_clip_one_host and awv_engine_clip_stats (include/allwave_hip.h).  What "clipped" means is
// clip_device.hpp; this file gets the kernel to the same record without a serial walk over the op string.
//
// verify.hip's shape: one wave per record, persistent waves taking records (longest op string first) from a cursor; per
// iteration a chunk of 64 lanes x 16 op bytes, one aligned 16-byte load per lane, addressed from the 16-byte boundary at or
// below the string's first byte, bytes outside the string masked out.  No sequence is read.
// Per chunk:
//   - a gap column's delta needs its position in its run: "the last column in this lane whose op differs from the one
//     before it" goes through a max-scan over the lanes, the run in progress at the chunk's end is carried;
//   - each lane forms the prefix sums of its 16 column deltas; an add-scan over the lane totals plus the chunk's carry
//     gives S at every column;
//   - the running minimum before a lane's columns is a min-scan over (lane minimum of S, column) keys whose low bits order a
//     tie towards the LATER column, combined with the carried minimum, which a tie replaces;
//   - from there each lane walks its 16 sums once more for its best S - minS (the first column attaining it, and the
//     minimum's index at that moment); a max-reduction whose low bits order a tie towards the LOWER lane picks the chunk's,
//     and only a strictly larger value replaces the carried best.
// The record's skips and counts are differences of op counts before the argmin and the argmax column: the per-lane counts
// of 'I', 'D', 'X', 'M' bytes are scanned with the rest (two packed scans), and the counts before one column are the
// owning lane's exclusive scan plus a masked count of its bytes -- taken only when the minimum or the best moves.
// All sums are 64-bit: a column costs up to o + e < 2^32, so 1,024 of them pass 32 bits for penalties no check rules out.
#include "clip_scan.hpp"  // the chunk loop described above: scan_ops, shared with split.hip

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "record_pass.hpp"  // the host skeleton of a record pass: RecordPass, pack_piece, AWV_TRY

namespace awvc {

struct KParams {
  const awv_result* results;  // cigar_off relative to `arena`
  const int32_t* order;       // dispatch slot -> record
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_clip_result* out;
  unsigned long long* counters;  // [0] cursor, [1] empty clips, [2] columns of clipped records
  long long npairs;
  awv_penalties pen;
  int32_t match_bonus;
};

__global__ __launch_bounds__(64) void awv_clip_kernel(KParams kp) {
  const int lane = threadIdx.x;
  const long long a = kp.match_bonus;
  unsigned long long n_empty = 0, n_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[pair] = make_clip(AWV_CL_SKIPPED, 0, 0);
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    n_columns += (unsigned long long)n;
    const Scan sc = scan_ops(kp.pen, a, kp.arena, rec.cigar_off, n, lane);
    if (sc.bad_col >= 0) {
      if (lane == 0) kp.out[pair] = make_clip(AWV_CL_BAD_OP, (uint32_t)sc.bad_col, (uint32_t)sc.bad_col);
      continue;
    }
    if (lane == 0) kp.out[pair] = sc.best > 0 ? make_clip(a, sc.best, sc.beg, sc.end, sc.at_beg, sc.at_end) : make_clip(AWV_CL_EMPTY, 0, 0);
    n_empty += sc.best <= 0;
  }
  if (lane == 0) {
    if (n_empty) atomicAdd(&kp.counters[1], n_empty);
    if (n_columns) atomicAdd(&kp.counters[2], n_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State : awvw::RecordPass {
  Buf<awv_clip_result> d_out;
  awv_clip_stats stats{};
  void release() {
    RecordPass::release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
void stats_reset(State* s) { awvw::reset_stats(s); }

namespace {

// the engine's sign rules for penalties (re-scoring has no ring to fit, so any size goes), the unused piece of a gap-affine
// set cleared, and the bonus in range
int check_args(const awv_penalties* p, int32_t match_bonus, awv_penalties& out) {
  if (int rc = awv_internal_check_penalties(p)) return rc;
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS)
    return awv_internal_fail(AWV_ERR_ARG, "clip: match_bonus must be in [1, " + std::to_string(AWV_CLIP_MAX_BONUS) + "]");
  out = *p;
  out.two_piece = p->two_piece ? 1 : 0;
  if (!out.two_piece) out.gap_open2 = out.gap_ext2 = 0;
  return AWV_OK;
}

// (the clip reads no sequence: an engine without a set will do, and is no error)
int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_clip(e), e, v, st, false); }

// One launch over n records whose op bytes are on the device already.
int launch(const awp::EngineView& v, State* st, const awv_penalties& pen, int32_t match_bonus, int64_t n, const awv_result* results,
           const uint8_t* d_arena, uint64_t arena_bytes, awv_clip_result* cout) {
  if (n == 0) return AWV_OK;
  if (int rc = st->begin(v, "clip", n, results, arena_bytes)) return rc;
  AWV_TRY(st->d_out.reserve((size_t)n));
  if (int rc = st->clear_counters(v, 4)) return rc;
  KParams kp{};
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.pen = pen;
  kp.match_bonus = match_bonus;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_clip_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  unsigned long long hc[4] = {0, 0, 0, 0};
  float ms = 0;
  AWV_TRY(hipMemcpyAsync(cout, st->d_out.p, (size_t)n * sizeof(awv_clip_result), hipMemcpyDeviceToHost, v.stream));
  if (int rc = st->finish(v, hc, 4, ms)) return rc;
  st->stats.kernel_ms += ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.empty += hc[1];
  st->stats.columns += hc[2];
  return AWV_OK;
}

int clip_cigars_core(awv_engine* e, const awv_penalties* pen_in, int32_t match_bonus, const awv_result* results, int64_t n_all,
                     const uint8_t* cigar_arena, uint64_t arena_bytes, uint64_t max_arena, awv_clip_result* cout) {
  awv_penalties pen;
  if (int rc = check_args(pen_in, match_bonus, pen)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->stats = awv_clip_stats{};
  // before anything goes up: every completed record's op bytes lie inside the caller's arena
  for (int64_t i = 0; i < n_all; ++i)
    if (awvw::outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: a record's op bytes lie outside the CIGAR arena");
  // in pieces (record_pieces.hpp) that keep every string's offset modulo 16
  std::vector<uint8_t> stage;
  std::vector<awv_result> recs;
  for (int64_t first = 0; first < n_all;) {
    const awvw::Piece pc = awvw::pack_piece(results, n_all, first, cigar_arena, max_arena, true, recs, stage);
    AWV_TRY(st->d_arena.reserve((size_t)pc.bytes + 64));
    if (pc.bytes) AWV_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
    if (int rc = launch(v, st, pen, match_bonus, pc.n, recs.data(), st->d_arena.p, pc.bytes, cout + first)) return rc;
    first += pc.n;
  }
  return AWV_OK;
}

}  // namespace

int clip_batch(awv_engine* e, const awv_penalties* pen_in, int32_t match_bonus, int64_t n, const awv_result* results, const uint8_t* d_arena,
               uint64_t arena_bytes, awv_clip_result* cout) {
  awv_penalties pen;
  if (int rc = check_args(pen_in, match_bonus, pen)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  return launch(v, st, pen, match_bonus, n, results, d_arena, arena_bytes, cout);
}

}  // namespace awvc

extern "C" {

int awv_clip_cigars(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, const awv_result* results, int64_t n,
                    const uint8_t* cigar_arena, uint64_t arena_bytes, awv_clip_result* cout) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || (n > 0 && (!results || !cout))) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: null arena");
  AWV_GUARDED(return awvc::clip_cigars_core(e, pen, match_bonus, results, n, cigar_arena, arena_bytes, awv_internal_max_arena(e), cout);)
}

int awv_clip_one_host(const awv_penalties* pen, int32_t match_bonus, const uint8_t* cigar, int64_t n, awv_clip_result* out) {
  awv_penalties p;
  if (int rc = awvc::check_args(pen, match_bonus, p)) return rc;
  if (!out || n < 0 || (n > 0 && !cigar)) return awv_internal_fail(AWV_ERR_ARG, "clip_one_host: bad argument");
  *out = awvc::clip_one(p, match_bonus, cigar, n);
  return AWV_OK;
}

int awv_engine_clip_stats(const awv_engine* e, awv_clip_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "clip_stats: null argument");
  const awvc::State* st = awv_internal_clip(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_clip_stats{};
  return AWV_OK;
}

}  // extern "C"
