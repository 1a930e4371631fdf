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
#include "clip_device.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "planner_device.hpp"  // EngineView, awv_internal_fail
#include "wave_ops.hpp"

namespace awvc {

constexpr int LANE_BYTES = 16;
constexpr int CHUNK = 64 * LANE_BYTES;
constexpr int WAVES_PER_CU = 16;  // persistent one-wave workgroups per CU: a chunk's walks depend on its scans, other waves fill the wait

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

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

using awvw::byte_range_mask;  // (wave_ops.hpp: the scans and the byte counting shared with verify.hip)
using awvw::count_bytes;
using awvw::from_lower_lane;
using awvw::wave_scan_add;
using awvw::wave_scan_max;
using awvw::wave_scan_min;

__device__ __forceinline__ long long wave_max(long long v) {  // in every lane
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ long long read_lane(long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

constexpr int KEY_POS_BITS = 10;  // a column's byte position in its chunk, 0 .. CHUNK - 1
static_assert((1 << KEY_POS_BITS) == CHUNK, "a minimum's key keeps the chunk position in its low bits");

__global__ __launch_bounds__(64) void awv_clip_kernel(KParams kp) {
  const int lane = threadIdx.x;
  const long long a = kp.match_bonus;
  unsigned long long n_empty = 0, n_columns = 0;  // (uniform)
  for (;;) {
    unsigned slot_lo = 0, slot_hi = 0;
    if (lane == 0) {
      const unsigned long long s = atomicAdd(&kp.counters[0], 1ull);
      slot_lo = (unsigned)s;
      slot_hi = (unsigned)(s >> 32);
    }
    const unsigned long long slot = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)slot_lo) |
                                    ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)slot_hi) << 32);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[pair] = make_clip(AWV_CL_SKIPPED, 0, 0);
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    n_columns += (unsigned long long)n;
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);
    const long long span = sh + n;  // op byte c is ops[sh + c]

    // carried from chunk to chunk (uniform)
    long long S = 0, minS = 0, best = 0;
    unsigned minI = 0, beg = 0, end = 0;
    Prefix at_min{0, 0, 0, 0}, at_beg{0, 0, 0, 0}, at_end{0, 0, 0, 0};
    unsigned cI = 0, cD = 0, cX = 0, cM = 0;  // ops before the chunk, by kind
    long long c_start = 0;                    // the column the run in progress began at
    unsigned c_prev = 0;                      // the op before the chunk's first column (0: none)
    bool bad = false;
    for (long long base = 0; n > 0 && base < span; base += CHUNK) {
      const long long b0 = base + lane * LANE_BYTES;
      const int jlo = (int)min(max((long long)sh - b0, 0ll), (long long)LANE_BYTES), jhi = (int)min(max(span - b0, 0ll), (long long)LANE_BYTES);  // this lane's bytes [jlo, jhi) are columns
      const int nv = max(jhi - jlo, 0);
      const long long col0 = b0 - sh;  // the column of this lane's byte 0
      const long long chunk_cols = base == 0 ? 0 : base - sh;  // columns before the chunk
      u32x4 w = {0u, 0u, 0u, 0u};
      if (b0 < span) w = *(const u32x4*)(ops + b0);
      int n_i = 0, n_d = 0, n_x = 0, n_m = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] &= byte_range_mask(jlo - 4 * k, jhi - 4 * k);
        n_i += count_bytes(w[k], 'I');
        n_d += count_bytes(w[k], 'D');
        n_x += count_bytes(w[k], 'X');
        n_m += count_bytes(w[k], 'M');
      }
      const unsigned long long bad_lanes = __ballot(n_i + n_d + n_x + n_m != nv);
      if (bad_lanes != 0) {  // lanes hold ascending columns: the lowest lane's first is the smallest
        int first = LANE_BYTES;
#pragma unroll
        for (int j = LANE_BYTES - 1; j >= 0; --j) {
          const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
          if (j >= jlo && j < jhi && !is_op(op)) first = j;
        }
        const int l = __builtin_ctzll(bad_lanes);
        const unsigned col = (unsigned)(base + l * LANE_BYTES + __builtin_amdgcn_readlane(first, l) - sh);
        if (lane == 0) kp.out[pair] = make_clip(AWV_CL_BAD_OP, col, col);
        bad = true;
        break;
      }
      // the op before this lane's first column: the lower lane's last byte, the chunk's carry in lane 0, none at column 0
      unsigned prev = (unsigned)from_lower_lane((int)w[3], (int)(c_prev << 24)) >> 24;
      if (b0 <= sh) prev = 0;
      int last_break = -1;  // as a byte position in the chunk
      {
        unsigned pv = prev;
#pragma unroll
        for (int j = 0; j < LANE_BYTES; ++j) {
          const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
          const bool valid = j >= jlo && j < jhi;
          if (valid && op != pv) last_break = lane * LANE_BYTES + j;
          if (valid) pv = op;
        }
      }
      const int packed_id = n_i | (n_d << 16), packed_xm = n_x | (n_m << 16);  // (a chunk holds 1,024 columns: the sums fit 16 bits)
      const int s_id = wave_scan_add(packed_id), s_xm = wave_scan_add(packed_xm);
      const int ib = from_lower_lane(wave_scan_max(last_break), -1);
      long long run_start = ib >= 0 ? base + ib - sh : c_start;

      // first walk: the lane's prefix sums, its total, its minimum (the latest column attaining it)
      long long p[LANE_BYTES];
      long long acc = 0, lmin = LLONG_MAX;
      int lmin_j = 0;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j >= jlo && j < jhi) {
          const long long col = col0 + j;
          if (op != prev) {
            run_start = col;
            prev = op;
          }
          acc += column_delta(kp.pen, a, op, col - run_start + 1);
          if (acc <= lmin) {
            lmin = acc;
            lmin_j = j;
          }
        }
        p[j] = acc;
      }
      const long long incl = wave_scan_add(acc);
      const long long rel = incl - acc;  // S before this lane's columns, relative to the chunk's start
      // a tie between two columns goes to the later one: the smaller key
      const long long key = nv > 0 ? (rel + lmin) * CHUNK + (CHUNK - 1 - (lane * LANE_BYTES + lmin_j)) : LLONG_MAX;
      const long long kin = wave_scan_min(key);
      const long long kex = from_lower_lane(kin, LLONG_MAX);
      long long m = minS;
      unsigned mi = minI;
      if (kex != LLONG_MAX && S + (kex >> KEY_POS_BITS) <= m) {  // (a tie replaces the carried minimum: the chunk's columns are later)
        m = S + (kex >> KEY_POS_BITS);
        mi = (unsigned)(base + (CHUNK - 1 - (int)(kex & (CHUNK - 1))) - sh + 1);
      }
      // second walk: the serial rule from the minimum the lower lanes leave
      long long lv = 0;
      unsigned lb = 0, le = 0;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        if (j >= jlo && j < jhi) {
          const long long s = S + rel + p[j];
          const unsigned next_col = (unsigned)(col0 + j + 1);
          if (s <= m) {
            m = s;
            mi = next_col;
          }
          if (s - m > lv) {
            lv = s - m;
            lb = mi;
            le = next_col;
          }
        }
      }
      // ops before the column at byte position bp of this chunk, that column included (uniform bp)
      auto prefix_through = [&](int bp) {
        const int hi = min(jhi, (bp & (LANE_BYTES - 1)) + 1);
        int li = 0, ld = 0, lx = 0, lm = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned wk = w[k] & byte_range_mask(jlo - 4 * k, hi - 4 * k);
          li += count_bytes(wk, 'I');
          ld += count_bytes(wk, 'D');
          lx += count_bytes(wk, 'X');
          lm += count_bytes(wk, 'M');
        }
        const int ex_id = s_id - packed_id, ex_xm = s_xm - packed_xm;
        const unsigned cols = (unsigned)(base + bp - sh + 1);
        const unsigned ni = cI + (unsigned)(ex_id & 0xffff) + (unsigned)li, nd = cD + (unsigned)(ex_id >> 16) + (unsigned)ld;
        const unsigned nx = cX + (unsigned)(ex_xm & 0xffff) + (unsigned)lx, nm = cM + (unsigned)(ex_xm >> 16) + (unsigned)lm;
        const int l = bp >> 4;
        Prefix r;
        r.q = cols - (unsigned)__builtin_amdgcn_readlane((int)ni, l);
        r.t = cols - (unsigned)__builtin_amdgcn_readlane((int)nd, l);
        r.x = (unsigned)__builtin_amdgcn_readlane((int)nx, l);
        r.m = (unsigned)__builtin_amdgcn_readlane((int)nm, l);
        return r;
      };
      // a tie between two lanes goes to the lower one (the earlier columns): the larger key
      const long long kbest = wave_max(lv * 64 + (63 - lane));
      const long long chunk_best = read_lane(kbest, 0) >> 6;
      if (chunk_best > best) {  // (a tie never replaces the carried best)
        const int wl = 63 - (__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)kbest) & 63);
        best = chunk_best;
        beg = (unsigned)__builtin_amdgcn_readlane((int)lb, wl);
        end = (unsigned)__builtin_amdgcn_readlane((int)le, wl);
        at_end = prefix_through((int)((long long)end - 1 + sh - base));
        at_beg = (long long)beg > chunk_cols ? prefix_through((int)((long long)beg - 1 + sh - base)) : at_min;
      }
      const long long kall = read_lane(kin, 63);
      if (kall != LLONG_MAX && S + (kall >> KEY_POS_BITS) <= minS) {
        const int bp = CHUNK - 1 - (int)(kall & (CHUNK - 1));
        minS = S + (kall >> KEY_POS_BITS);
        minI = (unsigned)(base + bp - sh + 1);
        at_min = prefix_through(bp);
      }
      S += read_lane(incl, 63);
      const int last_lane = (int)min(63ll, (span - 1 - base) >> 4);  // the lane that holds the chunk's last column
      c_prev = (unsigned)__builtin_amdgcn_readlane((int)prev, last_lane);
      c_start = read_lane(run_start, last_lane);
      const int t_id = __builtin_amdgcn_readlane(s_id, 63), t_xm = __builtin_amdgcn_readlane(s_xm, 63);
      cI += (unsigned)(t_id & 0xffff);
      cD += (unsigned)(t_id >> 16);
      cX += (unsigned)(t_xm & 0xffff);
      cM += (unsigned)(t_xm >> 16);
    }
    if (bad) continue;
    if (lane == 0) kp.out[pair] = best > 0 ? make_clip(a, best, beg, end, at_beg, at_end) : make_clip(AWV_CL_EMPTY, 0, 0);
    n_empty += best <= 0;
  }
  if (lane == 0) {
    if (n_empty) atomicAdd(&kp.counters[1], n_empty);
    if (n_columns) atomicAdd(&kp.counters[2], n_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State {
  Buf<awv_result> d_results;
  Buf<int32_t> d_order;
  Buf<awv_clip_result> d_out;
  Buf<unsigned long long> d_counters;
  Buf<uint8_t> d_arena;  // awv_clip_cigars: the caller's op bytes
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int num_cus = 0;
  awv_clip_stats stats{};
  void release() {
    d_results.release();
    d_order.release();
    d_out.release();
    d_counters.release();
    d_arena.release();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
  }
};

void state_release(State* s) {
  if (!s) return;
  s->release();
  delete s;
}

void stats_reset(State* s) {
  if (s) s->stats = awv_clip_stats{};
}

namespace {

#define CL_TRY(expr)                                                                                              \
  do {                                                                                                            \
    hipError_t _e = (expr);                                                                                       \
    if (_e != hipSuccess)                                                                                         \
      return awv_internal_fail(_e == hipErrorOutOfMemory ? AWV_ERR_OOM : AWV_ERR_HIP,                             \
                               std::string(#expr) + ": " + hipGetErrorString(_e));                                \
  } while (0)

#define CL_GUARDED(body)                                                                                          \
  try {                                                                                                           \
    body                                                                                                          \
  } catch (const std::bad_alloc&) {                                                                               \
    return awv_internal_fail(AWV_ERR_OOM, "host memory exhausted");                                               \
  } catch (const std::exception& ex) {                                                                            \
    return awv_internal_fail(AWV_ERR_HIP, std::string("internal error: ") + ex.what());                           \
  } catch (...) {                                                                                                 \
    return awv_internal_fail(AWV_ERR_HIP, "internal error: unknown exception");                                   \
  }

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

int open_state(awv_engine* e, awp::EngineView& v, State*& st) {
  awv_internal_device_view(e, &v);  // (the clip reads no sequence: an engine without a set will do, and is no error)
  CL_TRY(hipSetDevice(v.device));
  State*& slot = awv_internal_clip(e);
  if (!slot) slot = new State();
  st = slot;
  if (!st->ev0) CL_TRY(hipEventCreate(&st->ev0));
  if (!st->ev1) CL_TRY(hipEventCreate(&st->ev1));
  if (st->num_cus == 0) {
    int cus = 0;
    CL_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, v.device));
    st->num_cus = std::max(cus, 1);
  }
  return AWV_OK;
}

bool outside(const awv_result& r, uint64_t arena_bytes) {
  return r.status == AWV_ST_COMPLETED && (r.cigar_off > arena_bytes || (uint64_t)r.cigar_len > arena_bytes - r.cigar_off);
}

// One launch over n records whose op bytes are on the device already.  Every op string's place in the arena is checked
// here, on the host: the kernel reads what the records say.
int launch(const awp::EngineView& v, State* st, const awv_penalties& pen, int32_t match_bonus, int64_t n, const awv_result* results,
           const uint8_t* d_arena, uint64_t arena_bytes, awv_clip_result* cout) {
  if (n == 0) return AWV_OK;
  if (n > INT32_MAX) return awv_internal_fail(AWV_ERR_ARG, "clip: more than 2^31 - 1 records in one launch");
  for (int64_t i = 0; i < n; ++i)
    if (outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "clip: a record's op bytes lie outside the CIGAR arena");
  std::vector<int32_t> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  auto cols = [&](int32_t i) { return results[i].status == AWV_ST_COMPLETED ? results[i].cigar_len : 0u; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cols(a) > cols(b); });
  CL_TRY(st->d_results.reserve((size_t)n));
  CL_TRY(st->d_order.reserve((size_t)n));
  CL_TRY(st->d_out.reserve((size_t)n));
  CL_TRY(st->d_counters.reserve(4));
  CL_TRY(hipMemcpyAsync(st->d_results.p, results, (size_t)n * sizeof(awv_result), hipMemcpyHostToDevice, v.stream));
  CL_TRY(hipMemcpyAsync(st->d_order.p, order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
  CL_TRY(hipMemsetAsync(st->d_counters.p, 0, 4 * sizeof(unsigned long long), v.stream));
  KParams kp{};
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.pen = pen;
  kp.match_bonus = match_bonus;
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)st->num_cus * WAVES_PER_CU);
  CL_TRY(hipEventRecord(st->ev0, v.stream));
  hipLaunchKernelGGL(awv_clip_kernel, dim3(grid), dim3(64), 0, v.stream, kp);
  CL_TRY(hipGetLastError());
  CL_TRY(hipEventRecord(st->ev1, v.stream));
  unsigned long long hc[4] = {0, 0, 0, 0};
  CL_TRY(hipMemcpyAsync(cout, st->d_out.p, (size_t)n * sizeof(awv_clip_result), hipMemcpyDeviceToHost, v.stream));
  CL_TRY(hipMemcpyAsync(hc, st->d_counters.p, sizeof(hc), hipMemcpyDeviceToHost, v.stream));
  CL_TRY(hipStreamSynchronize(v.stream));
  float ms = 0;
  CL_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
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
    if (outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: a record's op bytes lie outside the CIGAR arena");
  // pieces of at most max_arena op bytes (one record alone may exceed it) and 2^20 records: the op bytes of a piece are
  // packed into 16-byte slots of a staging buffer that keep every string's offset modulo 16 (the kernel's addressing is
  // part of what a caller may want to exercise), so records may share, overlap or leave out parts of the caller's arena
  std::vector<uint8_t> stage;
  std::vector<awv_result> recs;
  for (int64_t first = 0; first < n_all;) {
    int64_t n = 0;
    uint64_t bytes = 0;
    recs.clear();
    while (first + n < n_all && n < ((int64_t)1 << 20)) {
      const awv_result& r = results[first + n];
      const uint64_t sh = r.cigar_off & 15;
      const uint64_t need = r.status == AWV_ST_COMPLETED ? (sh + (uint64_t)r.cigar_len + 15) & ~(uint64_t)15 : 0;
      if (n > 0 && bytes + need > max_arena) break;
      recs.push_back(r);
      recs.back().cigar_off = bytes + sh;
      bytes += need;
      ++n;
    }
    stage.assign((size_t)bytes, 0);
    for (int64_t i = 0; i < n; ++i) {
      const awv_result& r = results[first + i];
      if (r.status == AWV_ST_COMPLETED && r.cigar_len) std::memcpy(stage.data() + recs[(size_t)i].cigar_off, cigar_arena + r.cigar_off, r.cigar_len);
    }
    CL_TRY(st->d_arena.reserve((size_t)bytes + 64));
    if (bytes) CL_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)bytes, hipMemcpyHostToDevice, v.stream));
    if (int rc = launch(v, st, pen, match_bonus, n, recs.data(), st->d_arena.p, bytes, cout + first)) return rc;
    first += n;
  }
  return AWV_OK;
}

int null_engine() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return awv_internal_fail(AWV_ERR_NO_DEVICE, "no HIP device available: liballwave_hip has no CPU fallback");
  return awv_internal_fail(AWV_ERR_ARG, "null engine");
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
  if (!e) return awvc::null_engine();
  if (n < 0 || (n > 0 && (!results || !cout))) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "clip_cigars: null arena");
  CL_GUARDED(return awvc::clip_cigars_core(e, pen, match_bonus, results, n, cigar_arena, arena_bytes, awv_internal_max_arena(e), cout);)
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
