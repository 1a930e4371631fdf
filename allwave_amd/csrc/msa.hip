// msa.hip -- target-anchored multiple alignments built on the device: awv_msa_cigars / awv_msa_ranges, awv_engine_msa_stats and
// the host yardstick awv_msa_host (include/allwave_hip.h).  What an item widens and where its bases go is msa_device.hpp; this
// file gets the kernels to the same bytes.
//
// A record pass (record_pass.hpp) with coverage.hip's walk: one wave per item, persistent waves taking items (longest op string
// first) from a cursor, a string in chunks of 64 lanes x 16 op bytes, one aligned 16-byte load per lane.  Three things are new.
// The accumulator is a maximum: per chosen target len + 1 uint32 slots, the widest 'D' run any sound item has at that text
// position.  A run is owned by the column that ends it -- the first column behind it that is no 'D', or the string's end, closed
// by lane 0 behind the chunks -- and that column makes one no-return atomicMax.  It knows the slot from the packed add-scan of the
// lanes' consumed bases, and the run's start from a max-scan of "one past the lane's last column that is no 'D'", carried across
// chunks: nothing else is carried.  Every item is walked twice in the width launch: the first walk only counts and so decides
// the code; the second, for a sound item only, widens -- that keeps items all or nothing without any protocol between waves.
// Then the slots are scanned per target into 64-bit columns (awv_msa_scan_kernel), the host reads one width per target and lays
// out the blocks, and -- the second novelty -- every sound item is walked again after all items have widened
// (awv_msa_emit_kernel), each base one byte store at a column the other items decided.  The arena was filled with '-' by a
// stream-ordered memset before, so no order between a wave's own stores matters.  The output, third, is a dense block.
#include "msa_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "record_pass.hpp"  // RecordPass, open_pass, each_piece, resolve_call, Buf, AWV_TRY

namespace awvmsa {

struct KParams {
  const int32_t* len;          // the resident sequences' lengths
  const uint64_t* seq_off;     // and where their bytes begin in fwd / rc
  const uint8_t* fwd;          // the engine's forward copies
  const uint8_t* rc;           // and the reverse complements
  const int32_t* tmap;         // sequence -> index into the call's targets, or -1
  const uint64_t* slot_off;    // target j owns slots [slot_off[j], slot_off[j] + len + 1) of ins and col
  const awv_pair* pairs;       // the launch's items
  const Span* spans;           // their rectangles, behind the slices' skips (validated on the host)
  const awv_result* results;   // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;        // dispatch slot -> item
  const uint8_t* arena;        // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  uint32_t* ins;               // the widths
  const uint64_t* col;         // (emit) the columns
  awv_msa_item* out;           // the launch's items
  Ends* ends;
  const uint64_t* row_at;      // (emit) where item i's row begins in buf; unused for an item without a row
  const int64_t* width;        // (emit) per target
  uint8_t* buf;                // (emit) the arena of blocks
  unsigned long long* counters;  // [0] the cursor, [1] failed items, [2] columns, [3] runs, [4] bases
  long long npairs;
};

using awvw::CHUNK;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::wave_scan_add;
using awvw::wave_scan_max;
using awvw::wave_max_i64;
using awvw::wave_min_i64;
using awvw::wave_sum_i64;

// the string column of a lane's byte 0
__device__ __forceinline__ int lane_k0(int sh, long long base, int lane) { return (int)(base + lane * LANE_BYTES - sh); }

// What a chunk's scans give a lane (all under full EXEC, from values computed right before them).
struct ChunkScan {
  int k0;            // the string column of the lane's byte 0 (negative in the first lane of a string that begins inside its 16 bytes)
  long long x0, y0;  // the pattern and text positions of that byte
  int start;         // the string column where the 'D' run going on at the lane's byte 0 began: one past the last column below the lane that is no 'D'
  unsigned ends;     // the lane's columns that end a 'D' run: no 'D', behind one
  int tot, inc_last; // (uniform) the chunk's consumed bases, packed; one past the chunk's last column that is no 'D', or INT_MIN
};
// k0: lane_k0; cq, ct: bases consumed before the chunk; run0: the run start carried into the chunk; prev_d: the column before the chunk is a 'D'
__device__ __forceinline__ ChunkScan chunk_scan(const awvw::OpMasks& o, int k0, long long xb, long long yb, int cq, int ct, int run0, unsigned prev_d) {
  const unsigned takes_t = o.valid & ~o.d;
  const int mine = takes_t != 0 ? k0 + (31 - __clz((int)takes_t)) + 1 : INT_MIN;
  const int top = (int)((o.d >> 15) & 1u);
  const awvw::ConsumedScan pos = awvw::consumed_scan(o);
  const int s_run = wave_scan_max(mine);
  const int below_run = from_lower_lane(s_run, INT_MIN);
  const unsigned pbit = (unsigned)from_lower_lane(top, (int)prev_d);
  ChunkScan c;
  c.k0 = k0;
  c.x0 = xb + cq + (pos.ex & 0xffff);
  c.y0 = yb + ct + (pos.ex >> 16);
  c.start = max(below_run, run0);
  c.ends = takes_t & ((o.d << 1) | pbit);
  c.tot = pos.tot;
  c.inc_last = __builtin_amdgcn_readlane(s_run, 63);
  return c;
}
// the start of the 'D' run that ends at, or holds, the lane's byte j
__device__ __forceinline__ int run_start(const awvw::OpMasks& o, const ChunkScan& c, int j) {
  const unsigned nd = o.valid & ~o.d & ((1u << j) - 1u);
  return nd != 0 ? c.k0 + (31 - __clz((int)nd)) + 1 : c.start;
}
// whether the chunk's last column is a 'D': what the next chunk's first column follows, and what closes the string
__device__ __forceinline__ unsigned chunk_last_d(const awvw::OpMasks& o, long long span, long long base) {
  const long long lastb = min(span - 1 - base, (long long)CHUNK - 1);
  return ((unsigned)__builtin_amdgcn_readlane((int)o.d, awvw::last_column_lane(span, base)) >> (int)(lastb & 15)) & 1u;
}

// one maximum into a target's slots: never outside the target's own len + 1
__device__ __forceinline__ void widen_slot(const KParams& kp, int target, int tlen, long long y, int run) {
  if (slot_ok(y, tlen) && run > 0) atomicMax(&kp.ins[kp.slot_off[target] + (unsigned long long)y], (unsigned)run);
}

__global__ __launch_bounds__(64) void awv_msa_width_kernel(KParams kp) {
  const int lane = threadIdx.x;
  unsigned long long t_failed = 0, t_columns = 0, t_runs = 0, t_bases = 0;  // (uniform)
  for (;;) {
    // (the body ends on `if (lane == 0)` stores and take_record begins on one: a convergent operation between them keeps the
    // compiler from threading the other lanes past both -- variants.hip has the story)
    __builtin_amdgcn_wave_barrier();
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int item = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_pair pr = kp.pairs[item];
    const int target = kp.tmap[pr.t_idx];
    if (target < 0) {  // not walked, whatever the record says
      if (lane == 0) kp.out[item] = make_item(AWV_MS_NOT_CHOSEN, -1, 0);
      continue;
    }
    const awv_result rec = kp.results[item];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[item] = make_item(AWV_MS_SKIPPED, target, 0);
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    const Span sp = kp.spans[item];
    const int plen = sp.pe - sp.pb, tlen_sp = sp.te - sp.tb;
    if (n == 0) {
      const int code = whole_code(false, 0, 0, plen, tlen_sp);
      if (lane == 0) {
        kp.out[item] = make_item(code, target, 0);
        kp.ends[item] = make_ends(-1, -1, false, 0, 0, sp.tb, 0);
      }
      t_failed += code != AWV_MS_OK;
      continue;
    }
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    // ---- the first walk only counts (lane-local, reduced once behind the chunks)
    unsigned long long l_pos = 0, l_bad = 0;  // pattern bases | text bases << 32; bad bytes
    long long l_first = LLONG_MAX, l_last = -1;  // the first and last column other than 'I', each << 1 | it is a 'D'
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
      const int k0 = lane_k0(sh, base, lane);
      const unsigned takes_p = o.valid & ~o.i;
      l_pos += (unsigned long long)__popc(takes_p) | ((unsigned long long)__popc(o.valid & ~o.d) << 32);
      l_bad += (unsigned long long)__popc(o.valid & ~(o.m | o.x | o.i | o.d));
      if (takes_p != 0) {
        const int jf = __builtin_ctz(takes_p), jl = 31 - __clz((int)takes_p);
        l_first = min(l_first, ((long long)(k0 + jf) << 1) | (long long)((o.d >> jf) & 1u));
        l_last = max(l_last, ((long long)(k0 + jl) << 1) | (long long)((o.d >> jl) & 1u));
      }
    }
    const unsigned long long pos = (unsigned long long)wave_sum_i64((long long)l_pos), bad = (unsigned long long)wave_sum_i64((long long)l_bad);
    const long long first = wave_min_i64(l_first), last = wave_max_i64(l_last);
    const int code = whole_code(bad != 0, (long long)(unsigned)pos, (long long)(pos >> 32), plen, tlen_sp);
    t_columns += (unsigned long long)n;
    if (code != AWV_MS_OK) {
      if (lane == 0) kp.out[item] = make_item(code, target, 0);
      ++t_failed;
      continue;
    }
    t_bases += (unsigned)pos;

    // ---- the second walk widens: a sound item's positions stay inside its rectangle (widen_slot checks all the same)
    const int tlen = kp.len[pr.t_idx];
    const long long kl = last >> 1;  // (a sound item's bad bytes are none: a column other than 'I' is 'M', 'X' or 'D')
    int cq = 0, ct = 0, run0 = 0;  // bases consumed before the chunk; one past the last column so far that is no 'D' (uniform; afresh per record)
    unsigned prev_d = 0;           // the column before the chunk is a 'D' (uniform)
    unsigned l_runs = 0;
    int l_last_run = 0;  // the run that column kl is the last of, in the lane that closes it
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
      const ChunkScan c = chunk_scan(o, lane_k0(sh, base, lane), sp.pb, sp.tb, cq, ct, run0, prev_d);
      const unsigned takes_t = o.valid & ~o.d;
      for (unsigned b = c.ends; b != 0; b &= b - 1) {
        const int j = __builtin_ctz(b);
        const long long y = c.y0 + __popc(takes_t & ((1u << j) - 1u));
        const int k = c.k0 + j, run = k - run_start(o, c, j);
        widen_slot(kp, target, tlen, y, run);
        ++l_runs;
        if ((long long)k == kl + 1) l_last_run = run;
      }
      cq += c.tot & 0xffff;
      ct += c.tot >> 16;
      run0 = max(run0, c.inc_last);
      prev_d = chunk_last_d(o, span, base);
    }
    int tail_run = 0;
    if (prev_d) {  // a run that ends with the string (uniform)
      tail_run = (int)n - run0;
      if (lane == 0) widen_slot(kp, target, tlen, (long long)sp.tb + ct, tail_run);
    }
    const unsigned runs = (unsigned)wave_sum_i64((long long)l_runs) + (prev_d ? 1u : 0u);
    const int closed_run = (int)wave_max_i64((long long)l_last_run);
    const int last_run = (last >= 0 && (last & 1)) ? (prev_d ? tail_run : closed_run) : 0;
    t_runs += runs;
    if (lane == 0) {
      kp.out[item] = make_item(AWV_MS_OK, target, (unsigned)pos);
      kp.ends[item] = make_ends(first == LLONG_MAX ? -1 : first >> 1, kl, first != LLONG_MAX && (first & 1), last_run, n, sp.tb, (long long)(pos >> 32));
    }
  }
  if (lane == 0) {
    if (t_failed) atomicAdd(&kp.counters[1], t_failed);
    if (t_columns) atomicAdd(&kp.counters[2], t_columns);
    if (t_runs) atomicAdd(&kp.counters[3], t_runs);
    if (t_bases) atomicAdd(&kp.counters[4], t_bases);
  }
}

// The same walk again, for the items with a row: every base one byte store at its column.
__global__ __launch_bounds__(64) void awv_msa_emit_kernel(KParams kp) {
  const int lane = threadIdx.x;
  for (;;) {
    __builtin_amdgcn_wave_barrier();
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int item = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_msa_item it = kp.out[item];
    if (it.code != AWV_MS_OK || it.row <= 0) continue;
    const awv_result rec = kp.results[item];
    const long long n = (long long)rec.cigar_len;
    if (n == 0) continue;
    const awv_pair pr = kp.pairs[item];
    const Span sp = kp.spans[item];
    const int target = it.target;
    const int qlen = kp.len[pr.q_idx], tlen = kp.len[pr.t_idx];
    const uint8_t* const pattern = (pr.q_revcomp ? kp.rc : kp.fwd) + kp.seq_off[pr.q_idx];
    const uint64_t* const col = kp.col + kp.slot_off[target];
    const uint32_t* const ins = kp.ins + kp.slot_off[target];
    const long long W = kp.width[target];
    uint8_t* const row = kp.buf + kp.row_at[item];
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);
    const long long span = sh + n;
    int cq = 0, ct = 0, run0 = 0;
    unsigned prev_d = 0;
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
      const ChunkScan c = chunk_scan(o, lane_k0(sh, base, lane), sp.pb, sp.tb, cq, ct, run0, prev_d);
      const unsigned takes_p = o.valid & ~o.i, takes_t = o.valid & ~o.d;
      for (unsigned b = takes_p; b != 0; b &= b - 1) {
        const int j = __builtin_ctz(b);
        const unsigned below = (1u << j) - 1u;
        const long long x = c.x0 + __popc(takes_p & below), y = c.y0 + __popc(takes_t & below);
        const bool is_d = (o.d >> j) & 1u;
        if (!base_ok(x, qlen) || !slot_ok(y, tlen) || (!is_d && y >= tlen)) continue;
        const long long at = is_d ? ins_column((long long)col[y], ins[y], (c.k0 + j) - run_start(o, c, j)) : (long long)col[y];
        if (at >= 0 && at < W) row[at] = (uint8_t)awvcs::upper(pattern[x]);
      }
      cq += c.tot & 0xffff;
      ct += c.tot >> 16;
      run0 = max(run0, c.inc_last);
      prev_d = chunk_last_d(o, span, base);
    }
  }
}

// col[j][p] = p + the sum of target j's slots [0, p], in 64 bits; width[j] = col[j][len].  A workgroup of sixteen waves takes a
// target in tiles of 1,024 slots (a wave scan, the waves' sums through LDS, the tiles' sum carried on), like awv_cov_scan_kernel.
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void awv_msa_scan_kernel(const uint32_t* ins, const uint64_t* slot_off, const int32_t* targets, const int32_t* len,
                                                                    int nt, uint64_t* col, int64_t* width) {
  __shared__ unsigned long long wave_sum[SCAN_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int j = blockIdx.x; j < nt; j += gridDim.x) {
    const unsigned long long off = slot_off[j];
    const long long L = len[targets[j]];
    unsigned long long carry = 0;
    for (long long tile = 0; tile <= L; tile += SCAN_THREADS) {
      const long long i = tile + tid;
      const long long v = i <= L ? (long long)ins[off + i] : 0ll;
      const unsigned long long inc = (unsigned long long)wave_scan_add(v);
      if ((tid & 63) == 63) wave_sum[wave] = inc;
      __syncthreads();
      unsigned long long before = 0, all = 0;
#pragma unroll
      for (int k = 0; k < SCAN_THREADS / 64; ++k) {
        const unsigned long long s = wave_sum[k];
        if (k < wave) before += s;
        all += s;
      }
      const unsigned long long c = (unsigned long long)i + carry + before + inc;
      if (i <= L) col[off + i] = c;
      if (i == L) width[j] = (long long)c;
      carry += all;
      __syncthreads();
    }
  }
}

// the items' column intervals, one thread each, once the columns stand
__global__ void awv_msa_item_kernel(const awv_pair* pairs, const int32_t* len, const uint64_t* slot_off, const uint32_t* ins, const uint64_t* col,
                                    const Ends* ends, awv_msa_item* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  awv_msa_item it = out[i];
  if (it.code != AWV_MS_OK) return;
  int64_t beg = 0, end = 0;
  const uint64_t off = slot_off[it.target];
  item_columns(ends[i], col + off, ins + off, len[pairs[i].t_idx], beg, end);
  it.col_beg = beg;
  it.col_end = end;
  out[i] = it;
}

// row 0 of every block: upper(text[p]) at col[p]
__global__ __launch_bounds__(256) void awv_msa_target_kernel(const uint8_t* fwd, const uint64_t* seq_off, const int32_t* len, const int32_t* targets,
                                                             const uint64_t* slot_off, const uint64_t* col, const uint64_t* block_off, const int64_t* width,
                                                             int nt, uint8_t* buf) {
  for (int j = blockIdx.y; j < nt; j += gridDim.y) {
    const int s = targets[j];
    const long long L = len[s], W = width[j];
    const uint8_t* const text = fwd + seq_off[s];
    const uint64_t* const c = col + slot_off[j];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < L; p += (long long)gridDim.x * blockDim.x) {
      const long long at = (long long)c[p];
      if (at >= 0 && at < W) buf[block_off[j] + (unsigned long long)at] = (uint8_t)awvcs::upper(text[p]);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

constexpr int COUNTERS = 5;

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;  // the whole call's
  Buf<Span> d_spans;
  Buf<awv_msa_item> d_out;
  Buf<Ends> d_ends;
  Buf<int32_t> d_tmap, d_targets;
  Buf<uint64_t> d_slot_off, d_col, d_row_at, d_block_off;
  Buf<uint32_t> d_ins;
  Buf<int64_t> d_width;
  Buf<uint8_t> d_buf;
  awv_msa_stats stats{};
  void release() {
    RecordPass::release();
    d_pairs.release();
    d_spans.release();
    d_out.release();
    d_ends.release();
    d_tmap.release();
    d_targets.release();
    d_slot_off.release();
    d_col.release();
    d_row_at.release();
    d_block_off.release();
    d_ins.release();
    d_width.release();
    d_buf.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }

namespace {

template <typename T>
int upload(const awp::EngineView& v, Buf<T>& b, const T* src, size_t n) {
  AWV_TRY(b.reserve(std::max<size_t>(n, 1)));
  if (n) AWV_TRY(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, v.stream));
  return AWV_OK;
}

// One launch of a record kernel over the piece [first, first + n) of the call's items, whose op bytes are on the device.
int launch(const awp::EngineView& v, State* st, bool emit, int64_t first, int64_t n, const awv_result* recs, uint64_t arena_bytes, unsigned long long* hc,
           float& ms) {
  if (int rc = st->begin(v, "msa", n, recs, arena_bytes)) return rc;
  if (int rc = st->clear_counters(v, COUNTERS)) return rc;
  KParams kp{};
  kp.len = v.len;
  kp.seq_off = v.off;
  kp.fwd = v.fwd;
  kp.rc = v.rc;
  kp.tmap = st->d_tmap.p;
  kp.slot_off = st->d_slot_off.p;
  kp.pairs = st->d_pairs.p + first;
  kp.spans = st->d_spans.p + first;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = st->d_arena.p;
  kp.ins = st->d_ins.p;
  kp.col = st->d_col.p;
  kp.out = st->d_out.p + first;
  kp.ends = st->d_ends.p + first;
  kp.row_at = emit ? st->d_row_at.p + first : nullptr;
  kp.width = st->d_width.p;
  kp.buf = st->d_buf.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  if (int rc = st->start(v)) return rc;
  if (emit)
    hipLaunchKernelGGL(awv_msa_emit_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  else
    hipLaunchKernelGGL(awv_msa_width_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  return st->finish(v, hc, COUNTERS, ms);
}

// ranges (nullable; awv_msa_ranges): the call is on ranges[0..n_all) -- `pairs` is not read
int msa_core(awv_engine* e, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n_all, const awv_result* results, const uint8_t* cigar_arena,
             uint64_t arena_bytes, const awv_cs_slice* slices, uint64_t max_arena, const int32_t* targets, int64_t nt, awv_msa_item* items,
             awv_msa_target* tgts, uint8_t* buf, uint64_t cap, uint64_t* msa_bytes) {
  awp::EngineView v;
  State* st = nullptr;
  const char* const who = ranges ? "msa_ranges" : "msa_cigars";
  if (int rc = awvw::open_pass(awv_internal_msa(e), e, v, st, true)) return rc;
  st->stats = awv_msa_stats{};
  // before anything goes up: every target in the set and named once, every rectangle inside its sequences, every completed
  // record's op bytes inside the caller's arena, every slice inside its string
  if (nt > INT32_MAX) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": more targets than sequences");
  std::vector<int32_t> tmap((size_t)v.n, -1);
  std::vector<uint64_t> slot_off((size_t)nt + 1, 0);
  for (int64_t j = 0; j < nt; ++j) {
    if (targets[j] < 0 || targets[j] >= v.n) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": target " + std::to_string(j) + " is no sequence of the set");
    if (tmap[(size_t)targets[j]] >= 0) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": sequence " + std::to_string(targets[j]) + " is named as a target twice");
    tmap[(size_t)targets[j]] = (int32_t)j;
    slot_off[(size_t)j + 1] = slot_off[(size_t)j] + (uint64_t)v.len_host[targets[j]] + 1;
  }
  awvw::ItemCall call;
  if (int rc = awvw::resolve_call(call, v, who, pairs, ranges, n_all, results, arena_bytes, slices)) return rc;
  if (awvw::first_too_long(call.recs, n_all, MAX_COLUMNS) >= 0) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": an op string of more than 2^30 columns");
  pairs = call.pairs;
  results = call.recs;

  // the call's tables
  const uint64_t slots = slot_off[(size_t)nt];
  if (int rc = upload(v, st->d_tmap, tmap.data(), tmap.size())) return rc;
  if (int rc = upload(v, st->d_targets, targets, (size_t)nt)) return rc;
  if (int rc = upload(v, st->d_slot_off, slot_off.data(), slot_off.size())) return rc;
  if (int rc = upload(v, st->d_pairs, pairs, (size_t)n_all)) return rc;
  if (int rc = upload(v, st->d_spans, call.spans.data(), (size_t)n_all)) return rc;
  AWV_TRY(st->d_out.reserve(std::max<size_t>((size_t)n_all, 1)));
  AWV_TRY(st->d_ends.reserve(std::max<size_t>((size_t)n_all, 1)));
  AWV_TRY(st->d_ins.reserve(std::max<size_t>((size_t)slots, 1)));
  AWV_TRY(st->d_col.reserve(std::max<size_t>((size_t)slots, 1)));
  AWV_TRY(st->d_width.reserve(std::max<size_t>((size_t)nt, 1)));
  if (slots) AWV_TRY(hipMemsetAsync(st->d_ins.p, 0, (size_t)slots * sizeof(uint32_t), v.stream));
  if (n_all) AWV_TRY(hipMemsetAsync(st->d_ends.p, 0, (size_t)n_all * sizeof(Ends), v.stream));

  // (1) the widths, in pieces
  const auto widen = [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes) {
    unsigned long long hc[COUNTERS] = {0, 0, 0, 0, 0};
    float ms = 0;
    if (int rc = launch(v, st, false, first, n, recs, bytes, hc, ms)) return rc;
    st->stats.width_ms += ms;
    st->stats.failed += hc[1];
    st->stats.columns += hc[2];
    st->stats.runs += hc[3];
    st->stats.bases += hc[4];
    return (int)AWV_OK;
  };
  if (int rc = st->each_piece(v, results, n_all, cigar_arena, max_arena, widen)) return rc;
  st->stats.items = (uint64_t)n_all;

  // (2) the columns, one width per target and the items' column intervals
  std::vector<int64_t> width((size_t)nt, 0);
  {
    AWV_TRY(hipEventRecord(st->ev0, v.stream));
    if (nt) {
      const unsigned grid = (unsigned)std::min<int64_t>(nt, (int64_t)st->num_cus * 2);
      hipLaunchKernelGGL(awv_msa_scan_kernel, dim3(grid), dim3(SCAN_THREADS), 0, v.stream, st->d_ins.p, st->d_slot_off.p, st->d_targets.p, v.len, (int)nt,
                         st->d_col.p, st->d_width.p);
    }
    if (n_all && nt)
      hipLaunchKernelGGL(awv_msa_item_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, v.stream, st->d_pairs.p, v.len, st->d_slot_off.p, st->d_ins.p,
                         st->d_col.p, st->d_ends.p, st->d_out.p, (long long)n_all);
    AWV_TRY(hipGetLastError());
    AWV_TRY(hipEventRecord(st->ev1, v.stream));
    if (nt) AWV_TRY(hipMemcpyAsync(width.data(), st->d_width.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost, v.stream));
    if (n_all) AWV_TRY(hipMemcpyAsync(items, st->d_out.p, (size_t)n_all * sizeof(awv_msa_item), hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
    float ms = 0;
    AWV_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
    st->stats.scan_ms += ms;
  }
  // the layout: rows in the call's item order, blocks in `targets` order
  std::vector<int32_t> rows((size_t)nt, 1);
  for (int64_t i = 0; i < n_all; ++i)
    if (items[i].code == AWV_MS_OK) items[i].row = rows[(size_t)items[i].target]++;
  std::vector<uint64_t> block_off((size_t)nt + 1, 0);
  for (int64_t j = 0; j < nt; ++j) {
    tgts[j].t_idx = targets[j];
    tgts[j].rows = rows[(size_t)j];
    tgts[j].width = width[(size_t)j];
    tgts[j].off = block_off[(size_t)j];
    block_off[(size_t)j + 1] = block_off[(size_t)j] + (uint64_t)rows[(size_t)j] * (uint64_t)width[(size_t)j];
  }
  const uint64_t bytes = block_off[(size_t)nt];
  *msa_bytes = bytes;
  st->stats.bytes = bytes;
  if (bytes > cap || bytes == 0) return AWV_OK;

  // (3) the fill, the targets' rows and the items' rows
  std::vector<uint64_t> row_at((size_t)n_all, 0);
  for (int64_t i = 0; i < n_all; ++i)
    if (items[i].row > 0) row_at[(size_t)i] = block_off[(size_t)items[i].target] + (uint64_t)items[i].row * (uint64_t)width[(size_t)items[i].target];
  if (int rc = upload(v, st->d_row_at, row_at.data(), row_at.size())) return rc;
  if (int rc = upload(v, st->d_block_off, block_off.data(), block_off.size())) return rc;
  if (n_all) AWV_TRY(hipMemcpyAsync(st->d_out.p, items, (size_t)n_all * sizeof(awv_msa_item), hipMemcpyHostToDevice, v.stream));  // (the rows)
  AWV_TRY(st->d_buf.reserve((size_t)bytes));
  {
    AWV_TRY(hipEventRecord(st->ev0, v.stream));
    AWV_TRY(hipMemsetAsync(st->d_buf.p, '-', (size_t)bytes, v.stream));
    int64_t longest = 1;
    for (int64_t j = 0; j < nt; ++j) longest = std::max<int64_t>(longest, v.len_host[targets[j]]);
    const dim3 grid((unsigned)std::min<int64_t>((longest + 255) / 256, 64), (unsigned)std::min<int64_t>(nt, 1024));
    hipLaunchKernelGGL(awv_msa_target_kernel, grid, dim3(256), 0, v.stream, v.fwd, v.off, v.len, st->d_targets.p, st->d_slot_off.p, st->d_col.p,
                       st->d_block_off.p, st->d_width.p, (int)nt, st->d_buf.p);
    AWV_TRY(hipGetLastError());
    AWV_TRY(hipEventRecord(st->ev1, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
    float ms = 0;
    AWV_TRY(hipEventElapsedTime(&ms, st->ev0, st->ev1));
    st->stats.emit_ms += ms;
  }
  const auto emit = [&](int64_t first, int64_t n, const awv_result* recs, uint64_t piece_bytes) {  // (the same pieces: d_arena holds each already)
    unsigned long long hc[COUNTERS] = {0, 0, 0, 0, 0};
    float ms = 0;
    if (int rc = launch(v, st, true, first, n, recs, piece_bytes, hc, ms)) return rc;
    st->stats.emit_ms += ms;
    return (int)AWV_OK;
  };
  if (int rc = st->each_piece(v, results, n_all, cigar_arena, max_arena, emit)) return rc;
  AWV_TRY(hipMemcpyAsync(buf, st->d_buf.p, (size_t)bytes, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

// an awv_msa_cigars / awv_msa_ranges call's own outputs and counts
bool outputs_ok(int64_t n, const int32_t* targets, int64_t nt, const awv_msa_item* items, const awv_msa_target* tgts, const uint8_t* buf, uint64_t cap,
                const uint64_t* msa_bytes) {
  return nt >= 0 && msa_bytes && (n <= 0 || items) && (nt == 0 || (targets && tgts)) && (cap == 0 || buf);
}

}  // namespace

}  // namespace awvmsa

extern "C" {

int awv_msa_host(const uint8_t* text, int32_t tlen, int64_t n, const uint8_t* const* patterns, const int32_t* plens, const int32_t* rects,
                 const uint8_t* const* cigars, const int64_t* cigar_lens, const awv_cs_slice* slices, uint32_t* ins, int64_t* width, int32_t* codes,
                 uint8_t* block, uint64_t cap, uint64_t* block_bytes) {
  using namespace awvmsa;
  if (tlen < 0 || n < 0 || !ins || !width || !block_bytes || (tlen > 0 && !text) || (n > 0 && (!patterns || !plens || !rects || !cigars || !cigar_lens || !codes)) ||
      (cap > 0 && !block))
    return awv_internal_fail(AWV_ERR_ARG, "msa_host: bad argument");
  std::vector<HostItem> its((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t pb = rects[4 * i], pe = rects[4 * i + 1], tb = rects[4 * i + 2], te = rects[4 * i + 3];
    if (plens[i] < 0 || pb < 0 || pb > pe || pe > plens[i] || tb < 0 || tb > te || te > tlen || (plens[i] > 0 && !patterns[i]))
      return awv_internal_fail(AWV_ERR_ARG, "msa_host: an interval outside its sequence");
    int64_t beg = 0, end = std::max<int64_t>(cigar_lens[i], 0), q_skip = 0, t_skip = 0;
    if (slices) {
      const awv_cs_slice& s = slices[i];
      if (s.q_skip < 0 || s.t_skip < 0 || (cigar_lens[i] >= 0 && (s.col_beg > s.col_end || (int64_t)s.col_end > end)))
        return awv_internal_fail(AWV_ERR_ARG, "msa_host: a slice does not lie inside its op string, or skips a negative number of bases");
      if (cigar_lens[i] >= 0) {
        beg = s.col_beg;
        end = s.col_end;
      }
      q_skip = s.q_skip;
      t_skip = s.t_skip;
    }
    if (end - beg > MAX_COLUMNS) return awv_internal_fail(AWV_ERR_ARG, "msa_host: an op string of more than 2^30 columns");
    if (end > beg && !cigars[i]) return awv_internal_fail(AWV_ERR_ARG, "msa_host: bad argument");
    its[(size_t)i] = HostItem{patterns[i], plens[i], Span{pb, pe, tb, te}, cigars[i] ? cigars[i] + beg : nullptr, cigar_lens[i] < 0 ? -1 : end - beg, q_skip, t_skip};
  }
  msa_target(text, tlen, its.data(), n, ins, width, codes, block, cap, block_bytes);
  return AWV_OK;
}

int awv_msa_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                   const awv_cs_slice* slices, const int32_t* targets, int64_t nt, awv_msa_item* items, awv_msa_target* tgts, uint8_t* buf, uint64_t cap,
                   uint64_t* msa_bytes) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("msa_cigars", n, pairs, results, awvmsa::outputs_ok(n, targets, nt, items, tgts, buf, cap, msa_bytes), cigar_arena, arena_bytes)) return rc;
  AWV_GUARDED(return awvmsa::msa_core(e, pairs, nullptr, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), targets, nt, items, tgts, buf,
                                      cap, msa_bytes);)
}

int awv_msa_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                   const awv_cs_slice* slices, const int32_t* targets, int64_t nt, awv_msa_item* items, awv_msa_target* tgts, uint8_t* buf, uint64_t cap,
                   uint64_t* msa_bytes) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("msa_ranges", n, ranges, results, awvmsa::outputs_ok(n, targets, nt, items, tgts, buf, cap, msa_bytes), cigar_arena, arena_bytes)) return rc;
  static const awv_range_pair none{};
  AWV_GUARDED(return awvmsa::msa_core(e, nullptr, n > 0 ? ranges : &none, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), targets, nt,
                                      items, tgts, buf, cap, msa_bytes);)
}

int awv_engine_msa_stats(const awv_engine* e, awv_msa_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "msa_stats: null argument");
  const awvmsa::State* st = awv_internal_msa(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_msa_stats{};
  return AWV_OK;
}

}  // extern "C"
