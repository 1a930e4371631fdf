// coverage.hip -- per-base alignment depth accumulated on the device: awv_engine_coverage_begin / _read / _stats,
// awv_coverage_cigars / awv_coverage_ranges and awv_coverage_one_host (include/allwave_hip.h).  What an item adds is
// coverage_device.hpp; this file gets the kernels to the same numbers.
//
// A record pass (record_pass.hpp) with the op-mask walk of wave_ops.hpp (lane_op_masks): one wave per item, persistent waves
// taking items (longest op string first) from a cursor, a string in chunks of 64 lanes x 16 op bytes, one aligned 16-byte load
// per lane.  It is the first pass whose output is indexed by sequence coordinate and summed over items, batches and calls, so it
// only ever adds.
// The accumulators are difference arrays: per track and sequence len + 1 uint32 slots (slot len is the interval end), laid out by
// cov_off.  A maximal run of aligned columns covers one interval of the target and one of the query: +1 at the interval's begin,
// -1 at its end, modulo 2^32; likewise a maximal 'M' run in the matched track.  A lane sees a boundary where a column's class
// differs from the class of the column before it -- the lower lane's last byte, or the carry of the chunk before -- and knows both
// positions there from the packed add-scan of the lanes' consumed bases: no run start is carried.  A run that ends with the string
// is closed by lane 0 behind the chunks.  Adds are no-return atomics, one per boundary bit and role.
// Every item is walked twice in one launch: the first walk only counts (a bad byte, the consumed lengths, the columns and the
// boundaries) and so decides the code; the second, for a sound item only, adds -- its op bytes come from L2.  That keeps items all
// or nothing without any protocol between waves.
// Reading (awv_cov_scan_kernel) is a segmented inclusive scan of the difference slots into depth buffers of their own; every
// sequence's scan must end on 0 in slot len.
#include "coverage_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "batch_items.hpp"  // contributing_items
#include "record_pass.hpp"  // RecordPass, open_pass, open_active, each_piece, resolve_call, Buf, AWV_TRY

namespace awvcov {

struct KParams {
  const int32_t* len;         // the resident sequences' lengths
  const uint64_t* cov_off;    // sequence s owns slots [cov_off[s], cov_off[s] + len[s]] of both tracks
  const awv_pair* pairs;
  const Span* spans;          // item i's rectangle, behind the slice's skips (validated on the host)
  const awv_result* results;  // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;       // dispatch slot -> item
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  uint32_t* acc_a;            // the difference tracks
  uint32_t* acc_m;
  awv_cov_item* out;
  unsigned long long* counters;  // [0] the cursor, [1] failed items, [2] columns, [3] boundaries
  long long npairs;
  int roles;
};

using awvw::CHUNK;
using awvw::from_lower_lane;
using awvw::wave_scan_add;
using awvw::wave_sum_i64;

// What coverage makes of a lane's masks (awvw::OpMasks): its two classes of columns, aligned ('M' or 'X') and matched ('M').
struct LaneClasses {
  unsigned a;     // bit j: column j is aligned (o.m: it is matched)
  unsigned top;   // the classes of the lane's last byte (bit 0: aligned, bit 1: matched): what the next lane's first column follows
  unsigned last;  // the classes of the lane's last column (0: it has none)
};
__device__ __forceinline__ LaneClasses classes_of(const awvw::OpMasks& o) {
  LaneClasses c;
  c.a = o.m | o.x;
  c.top = ((c.a >> 15) & 1u) | (((o.m >> 15) & 1u) << 1);
  const int jl = 31 - __clz((int)(o.valid | 1u));
  c.last = o.valid != 0 ? ((c.a >> jl) & 1u) | (((o.m >> jl) & 1u) << 1) : 0u;
  return c;
}

// the columns of a lane whose class bit differs from the one of the column before them (prev: before the lane's first byte)
__device__ __forceinline__ unsigned boundaries_of(unsigned cls, unsigned prev, unsigned valid) { return (cls ^ ((cls << 1) | prev)) & valid; }

// the classes of the chunk's last column: what the next chunk's first column follows, and what closes the string
__device__ __forceinline__ unsigned chunk_last(const LaneClasses& c, long long span, long long base) {
  return (unsigned)__builtin_amdgcn_readlane((int)c.last, awvw::last_column_lane(span, base));
}

// one add into a difference track: slot `slot` of sequence `seq`, never outside the sequence's own slots
__device__ __forceinline__ void add_slot(uint32_t* track, const KParams& kp, int seq, int len, long long slot, uint32_t v) {
  if (slot_ok(slot, len)) atomicAdd(&track[kp.cov_off[seq] + (unsigned long long)slot], v);
}
// a boundary of sign v (1 or -1 modulo 2^32) at pattern position x and text position y, for the roles of the launch
__device__ __forceinline__ void add_boundary(uint32_t* track, const KParams& kp, const awv_pair& pr, int qlen, int tlen, long long x, long long y, uint32_t v) {
  if (kp.roles & AWV_COV_TARGET) add_slot(track, kp, pr.t_idx, tlen, y, v);
  if (kp.roles & AWV_COV_QUERY) add_slot(track, kp, pr.q_idx, qlen, query_slot(pr.q_revcomp != 0, qlen, x), pr.q_revcomp ? 0u - v : v);
}

__global__ __launch_bounds__(64) void awv_coverage_kernel(KParams kp) {
  const int lane = threadIdx.x;
  unsigned long long t_failed = 0, t_columns = 0, t_bound = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int item = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[item];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[item] = make_item(AWV_CV_SKIPPED, 0, 0, 0);
      continue;
    }
    const long long n = (long long)rec.cigar_len;
    const awv_pair pr = kp.pairs[item];
    const Span sp = kp.spans[item];
    const int plen = sp.pe - sp.pb, tlen_sp = sp.te - sp.tb;
    if (n == 0) {
      const int code = whole_code(false, 0, 0, plen, tlen_sp);
      if (lane == 0) kp.out[item] = make_item(code, 0, 0, 0);
      t_failed += code != AWV_CV_OK;
      continue;
    }
    const int sh = (int)(rec.cigar_off & 15);
    const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
    const long long span = sh + n;

    // ---- the first walk only counts (lane-local sums, added up once behind the chunks)
    unsigned prev = 0;  // the classes of the column before the chunk (uniform)
    unsigned long long l_cols = 0, l_pos = 0, l_rest = 0;  // aligned | matched << 32; pattern bases | text bases << 32; boundaries | bad bytes << 32
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
      const LaneClasses c = classes_of(o);
      const unsigned pb = (unsigned)from_lower_lane((int)c.top, (int)prev);
      const unsigned ba = boundaries_of(c.a, pb & 1u, o.valid), bm = boundaries_of(o.m, pb >> 1, o.valid);
      l_cols += (unsigned long long)__popc(c.a) | ((unsigned long long)__popc(o.m) << 32);
      l_pos += (unsigned long long)__popc(o.valid & ~o.i) | ((unsigned long long)__popc(o.valid & ~o.d) << 32);
      l_rest += (unsigned long long)(__popc(ba) + __popc(bm)) | ((unsigned long long)__popc(o.valid & ~(o.m | o.x | o.i | o.d)) << 32);
      prev = chunk_last(c, span, base);
    }
    const unsigned long long cols = (unsigned long long)wave_sum_i64((long long)l_cols), pos = (unsigned long long)wave_sum_i64((long long)l_pos),
                             rest = (unsigned long long)wave_sum_i64((long long)l_rest);
    const unsigned bounds = (unsigned)rest + (prev & 1u) + (prev >> 1);  // the runs that end with the string
    const int code = whole_code((rest >> 32) != 0, (long long)(unsigned)pos, (long long)(pos >> 32), plen, tlen_sp);
    if (lane == 0) kp.out[item] = make_item(code, (unsigned)cols, (unsigned)(cols >> 32), bounds);
    t_columns += (unsigned long long)n;
    if (code != AWV_CV_OK) {
      ++t_failed;
      continue;
    }
    t_bound += bounds;

    // ---- the second walk adds: a sound item's positions stay inside its rectangle (add_slot checks all the same)
    const int qlen = kp.len[pr.q_idx], tlen = kp.len[pr.t_idx];
    int cq = 0, ct = 0;  // bases consumed before the chunk (uniform)
    prev = 0;
    for (long long base = 0; base < span; base += CHUNK) {
      const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
      const LaneClasses c = classes_of(o);
      const unsigned pb = (unsigned)from_lower_lane((int)c.top, (int)prev);
      const unsigned ba = boundaries_of(c.a, pb & 1u, o.valid), bm = boundaries_of(o.m, pb >> 1, o.valid);
      const unsigned takes_p = o.valid & ~o.i, takes_t = o.valid & ~o.d;
      const awvw::ConsumedScan pos = awvw::consumed_scan(o);
      const long long x0 = (long long)sp.pb + cq + (pos.ex & 0xffff), y0 = (long long)sp.tb + ct + (pos.ex >> 16);
      for (unsigned b = ba | bm; b != 0; b &= b - 1) {
        const int j = __builtin_ctz(b);
        const unsigned bit = 1u << j, below = bit - 1u;
        const long long x = x0 + __popc(takes_p & below), y = y0 + __popc(takes_t & below);
        if (ba & bit) add_boundary(kp.acc_a, kp, pr, qlen, tlen, x, y, (c.a & bit) ? 1u : 0u - 1u);
        if (bm & bit) add_boundary(kp.acc_m, kp, pr, qlen, tlen, x, y, (o.m & bit) ? 1u : 0u - 1u);
      }
      cq += pos.tot & 0xffff;
      ct += pos.tot >> 16;
      prev = chunk_last(c, span, base);
    }
    if (lane == 0) {  // a run that ends with the string
      const long long x = (long long)sp.pb + cq, y = (long long)sp.tb + ct;
      if (prev & 1u) add_boundary(kp.acc_a, kp, pr, qlen, tlen, x, y, 0u - 1u);
      if (prev & 2u) add_boundary(kp.acc_m, kp, pr, qlen, tlen, x, y, 0u - 1u);
    }
  }
  if (lane == 0) {
    if (t_failed) atomicAdd(&kp.counters[1], t_failed);
    if (t_columns) atomicAdd(&kp.counters[2], t_columns);
    if (t_bound) atomicAdd(&kp.counters[3], t_bound);
  }
}

// The read-out: depth[s][p] = the sum of sequence s's difference slots [0, p], for both tracks.  A workgroup of sixteen waves
// takes a sequence in tiles of 1,024 slots (a wave scan, the waves' sums through LDS, the tiles' sum carried on), like
// awv_text_scan_kernel; the depths are dense (no interval-end slot): sequence s begins at cov_off[s] - s.  The scan of every
// sequence ends on 0 in slot len: *violations counts the tracks where it does not.
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void awv_cov_scan_kernel(const uint32_t* acc_a, const uint32_t* acc_m, const uint64_t* cov_off, const int32_t* len,
                                                                    int nseq, uint32_t* depth_a, uint32_t* depth_m, unsigned long long* violations) {
  __shared__ unsigned wave_sum[2][SCAN_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int s = blockIdx.x; s < nseq; s += gridDim.x) {
    const unsigned long long off = cov_off[s], dense = off - (unsigned long long)s;
    const long long L = len[s];
    unsigned carry_a = 0, carry_m = 0;
    for (long long tile = 0; tile <= L; tile += SCAN_THREADS) {
      const long long i = tile + tid;
      const unsigned va = i <= L ? acc_a[off + i] : 0u, vm = i <= L ? acc_m[off + i] : 0u;
      const unsigned inc_a = (unsigned)wave_scan_add((int)va), inc_m = (unsigned)wave_scan_add((int)vm);
      if ((tid & 63) == 63) {
        wave_sum[0][wave] = inc_a;
        wave_sum[1][wave] = inc_m;
      }
      __syncthreads();
      unsigned before_a = 0, all_a = 0, before_m = 0, all_m = 0;
#pragma unroll
      for (int k = 0; k < SCAN_THREADS / 64; ++k) {
        const unsigned sa = wave_sum[0][k], sm = wave_sum[1][k];
        if (k < wave) {
          before_a += sa;
          before_m += sm;
        }
        all_a += sa;
        all_m += sm;
      }
      const unsigned da = carry_a + before_a + inc_a, dm = carry_m + before_m + inc_m;
      if (i < L) {
        depth_a[dense + i] = da;
        depth_m[dense + i] = dm;
      }
      if (i == L && (da != 0 || dm != 0)) atomicAdd(violations, (unsigned long long)(da != 0) + (unsigned long long)(dm != 0));
      carry_a += all_a;
      carry_m += all_m;
      __syncthreads();
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

constexpr int COUNTERS = 4;

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_cov_item> d_out;
  Buf<uint64_t> d_cov_off;
  Buf<uint32_t> d_acc_a, d_acc_m;      // the difference tracks: n_bases + nseq slots each
  Buf<uint32_t> d_depth_a, d_depth_m;  // a read's depths: n_bases each
  awvw::BatchItems items;              // a batch's items (batch_items.hpp)
  std::vector<awv_cov_item> h_items;
  int32_t roles = 0;  // 0: no coverage
  int64_t clip_min_score = 0;
  int32_t nseq = 0;
  uint64_t n_bases = 0;
  awv_cov_stats stats{};
  void end() {  // coverage ends: the accumulators go, the stats stay readable until the next begin
    roles = 0;
    d_cov_off.release();
    d_acc_a.release();
    d_acc_m.release();
    d_depth_a.release();
    d_depth_m.release();
  }
  void release() {
    RecordPass::release();
    end();
    d_pairs.release();
    d_spans.release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
bool active(const State* s) { return s && s->roles != 0; }

namespace {

constexpr const char* TOO_LONG = "coverage: an op string of more than 2^30 columns";  // what fits awv_cov_item's counts

int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_coverage(e), e, v, st, true); }
// the state of an engine that accumulates
int open_active(awv_engine* e, const char* who, awp::EngineView& v, State*& st) { return awvw::open_active(awv_internal_coverage(e), who, "coverage", e, v, st); }

// One launch over n items whose op bytes are on the device already; an item's slice has been applied to its record and to its
// rectangle.  Every index and rectangle is checked here, on the host: the kernel reads what the items say.  items (host,
// nullable) is filled.
int launch(const awp::EngineView& v, State* st, const awv_pair* pairs, const Span* spans, int64_t n, const awv_result* recs, const uint8_t* d_arena,
           uint64_t arena_bytes, awv_cov_item* items) {
  if (n == 0) return AWV_OK;
  if (v.n != st->nseq) return awv_internal_fail(AWV_ERR_STATE, "coverage: the sequence set changed since awv_engine_coverage_begin");
  if ((int64_t)st->stats.items + n > MAX_ITEMS) return awv_internal_fail(AWV_ERR_ARG, "coverage: more than 2^31 - 1 items since awv_engine_coverage_begin");
  if (int rc = awvw::check_rectangles(v, "coverage", pairs, spans, n)) return rc;
  if (int rc = awvw::check_lengths(recs, n, MAX_COLUMNS, TOO_LONG)) return rc;
  if (int rc = st->begin(v, "coverage", n, recs, arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)n));
  AWV_TRY(st->d_spans.reserve((size_t)n));
  AWV_TRY(st->d_out.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, pairs, (size_t)n * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_spans.p, spans, (size_t)n * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  if (int rc = st->clear_counters(v, COUNTERS)) return rc;
  KParams kp{};
  kp.len = v.len;
  kp.cov_off = st->d_cov_off.p;
  kp.pairs = st->d_pairs.p;
  kp.spans = st->d_spans.p;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.acc_a = st->d_acc_a.p;
  kp.acc_m = st->d_acc_m.p;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.roles = st->roles;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_coverage_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  if (!items) {
    st->h_items.resize((size_t)n);
    items = st->h_items.data();
  }
  AWV_TRY(hipMemcpyAsync(items, st->d_out.p, (size_t)n * sizeof(awv_cov_item), hipMemcpyDeviceToHost, v.stream));
  unsigned long long hc[COUNTERS] = {0, 0, 0, 0};
  float ms = 0;
  if (int rc = st->finish(v, hc, COUNTERS, ms)) return rc;
  st->stats.kernel_ms += ms;
  st->stats.items += (uint64_t)n;
  st->stats.failed += hc[1];
  st->stats.columns += hc[2];
  st->stats.boundaries += hc[3] * (uint64_t)__builtin_popcount((unsigned)st->roles);
  return AWV_OK;
}

// ranges (nullable; awv_coverage_ranges): the call is on ranges[0..n_all) -- `pairs` is not read
int coverage_cigars_core(awv_engine* e, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n_all, const awv_result* results,
                         const uint8_t* cigar_arena, uint64_t arena_bytes, const awv_cs_slice* slices, uint64_t max_arena, awv_cov_item* items) {
  const char* const who = ranges ? "coverage_ranges" : "coverage_cigars";
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, who, v, st)) return rc;
  awvw::ItemCall call;
  if (int rc = awvw::resolve_call(call, v, who, pairs, ranges, n_all, results, arena_bytes, slices)) return rc;
  if (int rc = awvw::check_lengths(call.recs, n_all, MAX_COLUMNS, TOO_LONG)) return rc;
  if ((int64_t)st->stats.items + n_all > MAX_ITEMS) return awv_internal_fail(AWV_ERR_ARG, "coverage: more than 2^31 - 1 items since awv_engine_coverage_begin");
  return st->each_piece(v, call.recs, n_all, cigar_arena, max_arena, [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes) {
    return launch(v, st, call.pairs + first, call.spans.data() + first, n, recs, st->d_arena.p, bytes, items + first);
  });
}

int begin_core(awv_engine* e, int32_t roles, int64_t clip_min_score) {
  if (roles == 0) {  // coverage ends
    if (State* st = awv_internal_coverage(e)) st->end();
    return AWV_OK;
  }
  if (!roles_ok(roles)) return awv_internal_fail(AWV_ERR_ARG, "coverage_begin: roles must be 0 or an AWV_COV_* mask");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  st->end();
  std::vector<uint64_t> off((size_t)v.n + 1, 0);
  for (int32_t s = 0; s < v.n; ++s) off[(size_t)s + 1] = off[(size_t)s] + (uint64_t)v.len_host[s] + 1;
  const uint64_t slots = off[(size_t)v.n];
  AWV_TRY(st->d_cov_off.reserve(off.size()));
  AWV_TRY(st->d_acc_a.reserve((size_t)slots));
  AWV_TRY(st->d_acc_m.reserve((size_t)slots));
  AWV_TRY(hipMemcpyAsync(st->d_cov_off.p, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemsetAsync(st->d_acc_a.p, 0, (size_t)slots * sizeof(uint32_t), v.stream));
  AWV_TRY(hipMemsetAsync(st->d_acc_m.p, 0, (size_t)slots * sizeof(uint32_t), v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  st->nseq = v.n;
  st->n_bases = slots - (uint64_t)v.n;
  st->clip_min_score = clip_min_score;
  st->stats = awv_cov_stats{};
  st->roles = roles;
  return AWV_OK;
}

int read_core(awv_engine* e, uint32_t* aligned, uint32_t* matched, uint64_t n_bases) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "coverage_read", v, st)) return rc;
  if (v.n != st->nseq) return awv_internal_fail(AWV_ERR_STATE, "coverage: the sequence set changed since awv_engine_coverage_begin");
  if (n_bases != st->n_bases) return awv_internal_fail(AWV_ERR_ARG, "coverage_read: n_bases is not the sum of the resident sequences' lengths");
  AWV_TRY(st->d_depth_a.reserve((size_t)std::max<uint64_t>(n_bases, 1)));
  AWV_TRY(st->d_depth_m.reserve((size_t)std::max<uint64_t>(n_bases, 1)));
  if (int rc = st->clear_counters(v, COUNTERS)) return rc;
  if (int rc = st->start(v)) return rc;
  const unsigned grid = (unsigned)std::min<int64_t>((int64_t)st->nseq, (int64_t)st->num_cus * 2);
  hipLaunchKernelGGL(awv_cov_scan_kernel, dim3(grid), dim3(SCAN_THREADS), 0, v.stream, st->d_acc_a.p, st->d_acc_m.p, st->d_cov_off.p, v.len, (int)st->nseq,
                     st->d_depth_a.p, st->d_depth_m.p, st->d_counters.p + 1);
  if (int rc = st->stop(v)) return rc;
  if (aligned && n_bases) AWV_TRY(hipMemcpyAsync(aligned, st->d_depth_a.p, (size_t)n_bases * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  if (matched && n_bases) AWV_TRY(hipMemcpyAsync(matched, st->d_depth_m.p, (size_t)n_bases * sizeof(uint32_t), hipMemcpyDeviceToHost, v.stream));
  unsigned long long hc[COUNTERS] = {0, 0, 0, 0};
  float ms = 0;
  if (int rc = st->finish(v, hc, COUNTERS, ms)) return rc;
  st->stats.kernel_ms += ms;
  st->stats.reads += 1;
  if (hc[1] != 0)
    return awv_internal_fail(AWV_ERR_HIP, "coverage_read: " + std::to_string(hc[1]) + " difference tracks do not end on 0 (a bug: an item was added in part)");
  return AWV_OK;
}

}  // namespace

int coverage_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
                   const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "coverage_batch", v, st)) return rc;
  awvw::contributing_items(v, pairs, n, results, clips, st->clip_min_score, seg_first, iout, sout, spans, st->items);
  return launch(v, st, st->items.pairs.data(), st->items.spans.data(), (int64_t)st->items.pairs.size(), st->items.recs.data(), d_arena, arena_bytes, nullptr);
}

}  // namespace awvcov

extern "C" {

int awv_coverage_one_host(int32_t roles, int32_t q_revcomp, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb, int32_t te, const uint8_t* cigar,
                          int64_t n, const awv_cs_slice* slice, uint32_t* q_aligned, uint32_t* q_matched, uint32_t* t_aligned, uint32_t* t_matched,
                          awv_cov_item* out) {
  if (!out || !awvcov::roles_ok(roles) || qlen < 0 || tlen < 0 || n < 0 || (n > 0 && !cigar))
    return awv_internal_fail(AWV_ERR_ARG, "coverage_one_host: bad argument");
  if (int rc = awvw::check_host_rectangle("coverage_one_host", qlen, tlen, pb, pe, tb, te)) return rc;
  awvw::HostSlice sl;
  if (int rc = awvw::check_host_slice("coverage_one_host", slice, n, awvcov::MAX_COLUMNS, sl)) return rc;
  *out = awvcov::cov_one(roles, q_revcomp != 0, qlen, tlen, awvcov::Span{pb, pe, tb, te}, cigar + sl.beg, sl.end - sl.beg, sl.q_skip, sl.t_skip, q_aligned, q_matched,
                         t_aligned, t_matched);
  return AWV_OK;
}

int awv_engine_coverage_begin(awv_engine* e, int32_t roles, int64_t clip_min_score) {
  if (!e) return awv_internal_null_engine();
  AWV_GUARDED(return awvcov::begin_core(e, roles, clip_min_score);)
}

int awv_engine_coverage_read(awv_engine* e, uint32_t* aligned, uint32_t* matched, uint64_t n_bases) {
  if (!e) return awv_internal_null_engine();
  AWV_GUARDED(return awvcov::read_core(e, aligned, matched, n_bases);)
}

int awv_coverage_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                        const awv_cs_slice* slices, awv_cov_item* items) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("coverage_cigars", n, pairs, results, n <= 0 || items, cigar_arena, arena_bytes)) return rc;
  AWV_GUARDED(return awvcov::coverage_cigars_core(e, pairs, nullptr, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), items);)
}

int awv_coverage_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                        const awv_cs_slice* slices, awv_cov_item* items) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("coverage_ranges", n, ranges, results, n <= 0 || items, cigar_arena, arena_bytes)) return rc;
  static const awv_range_pair none{};
  AWV_GUARDED(return awvcov::coverage_cigars_core(e, nullptr, n > 0 ? ranges : &none, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), items);)
}

int awv_engine_coverage_stats(const awv_engine* e, awv_cov_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "coverage_stats: null argument");
  const awvcov::State* st = awv_internal_coverage(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_cov_stats{};
  return AWV_OK;
}

}  // extern "C"
