// engine.hip -- host side of liballwave_hip.so: the C ABI of include/allwave_hip.h.
//
// Owns all device state for one GPU (what the reference keeps in per-thread cached WFA2
// aligners, /root/reference/src/alignment.rs:11-22,210-221): sequence copies, per-workgroup
// wavefront arenas sized for 288 GB of HBM, result/CIGAR arenas, one stream.  There is no CPU
// fallback: without a HIP device every entry point fails with AWV_ERR_NO_DEVICE.
#include "allwave_hip.h"
#include "host_errors.hpp"      // (AWV_TRY, AWV_GUARDED: the error plumbing every unit behind the C ABI shares)
// the device code, once per workgroup size: awv:: one wave per pair (throughput), awvw:: four waves per pair,
// awvx:: sixteen waves per pair (one pair per CU: the few pairs a large length difference makes enormous).  These three
// names and awvw_m / awvx_m below belong to biwfa_device.hpp's instantiations, whose types (KParams, ...) are defined anew in
// each: no other header included here may open one of them.  The passes' hooks live in awp (planner), awo (orient), awvf
// (verify), awvc (clip), awvs (split), awvn (normalize), awve (encode) and awvcs (cs); awvw is also wave_ops.hpp's name in the
// passes' own units, which this unit does not include.
#include "planner_device.hpp"  // (the sketches and scratch of device pair planning, planner.hip)
#include "verify_device.hpp"   // (the per-batch check of awv_align_pairs_verified, verify.hip)
#include "clip_device.hpp"     // (the per-batch clip of awv_align_pairs_clipped, clip.hip)
#include "split_device.hpp"    // (the per-batch split of awv_align_pairs_split, split.hip)
#include "normalize_device.hpp"  // (the per-batch normalization under awv_engine_set_normalize, normalize.hip)
#include "encode_device.hpp"   // (the per-batch run-length text of awv_align_pairs_encoded, encode.hip)
#include "cs_device.hpp"       // (the per-batch cs text of awv_align_pairs_cs, cs.hip)
#include "coverage_device.hpp" // (the per-batch depth accumulation under awv_engine_coverage_begin, coverage.hip)
#include "variants_device.hpp" // (the per-batch allele events under awv_engine_variants_begin, variants.hip)
#include "lift_device.hpp"     // (the per-batch lifts under awv_engine_lift_begin, lift.hip)
#include "msa_device.hpp"      // (the buffers of awv_msa_cigars / awv_msa_ranges, msa.hip)
#include "kernels_awv.hpp"  // (the awv:: kernels themselves are instantiated in kernels_awv.hip -- here only the types)
#define AWV_NS awv
#define AWV_WG 64
#include "biwfa_device.hpp"
#undef AWV_NS
#undef AWV_WG
#define AWV_NS awvw
#define AWV_WG 256
#include "biwfa_device.hpp"
#undef AWV_NS
#undef AWV_WG
#define AWV_NS awvx
#define AWV_WG 1024
#include "biwfa_device.hpp"
#undef AWV_NS
#undef AWV_WG
// awvw_m:: / awvx_m:: the same two with AWV_WIDE16: 16-bit rows for pairs of which only the shorter sequence fits 16
// bits (cells stored as min(h, v), 32-bit row metadata) -- only their 16-bit-row kernels are used
#define AWV_WIDE16 1
#define AWV_NS awvw_m
#define AWV_WG 256
#include "biwfa_device.hpp"
#undef AWV_NS
#undef AWV_WG
#define AWV_NS awvx_m
#define AWV_WG 1024
#include "biwfa_device.hpp"
#undef AWV_NS
#undef AWV_WG
#undef AWV_WIDE16

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "batch_plan.hpp"
#include "twin_plan.hpp"
#include "row_reuse.hpp"

namespace {
// the device constants batch_plan.hpp's rules are written over (biwfa_device.hpp)
const awvb::Limits LIMITS = {awv::TMAX, awv::TMAX32, awv::CHAIN_MAX, awv::MAX_RING, awv::MAX_SCOPE, awv::NCOMP, awv::COL_PAD,
                             awv::FALLBACK_MIN_SCORE, awv::FALLBACK_MIN_LENGTH, awv::WAVES_PER_SIMD, awv::STATIC_LDS_RESERVE,
                             (size_t)awv::EV_STACK_WORDS, (size_t)awv::EV_TWIN_WORDS, sizeof(awv::RowMeta), sizeof(awv::RowMeta16),
                             sizeof(awv::Breakpoint)};
static_assert(awv::EV_STACK_WORDS == (awv::STACK_CAP * sizeof(awv::Task) + 3) / 4 + 16, "DFS stack words");

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// deliberately not awvw::Buf (wave_ops.hpp): growth slack, a second attempt without it, and an AWV_* code with its own message
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  int reserve(size_t n) {
    if (n <= cap) return AWV_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + std::min<size_t>(n / 8, (size_t)64 << 20) + 64;  // growth slack, bounded for the big arenas
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e != hipSuccess) {
      want = n;
      e = hipMalloc((void**)&p, want * sizeof(T));
    }
    if (e != hipSuccess) {
      p = nullptr;
      return fail(AWV_ERR_OOM, std::string("hipMalloc ") + std::to_string(want * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    }
    cap = want;
    return AWV_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void adopt(T* q, size_t n) {
    release();
    p = q;
    cap = n;
  }
  size_t bytes() const { return cap * sizeof(T); }
};

struct SeqSet {
  int32_t n = 0;
  std::vector<uint64_t> off;   // padded device layout
  std::vector<int32_t> len;
  DevBuf<uint8_t> d_seq[4];
  DevBuf<uint64_t> d_off;
  DevBuf<int32_t> d_len;
  DevBuf<uint32_t> d_seq2[2];  // 2-bit packed forward / reverse-complement
  DevBuf<uint64_t> d_off2;     // word offsets
  DevBuf<uint8_t> d_ok2;       // bit0 forward packable, bit1 reverse-complement packable
  size_t total = 0;
  void release() {
    for (auto& b : d_seq) b.release();
    for (auto& b : d_seq2) b.release();
    d_off2.release();
    d_ok2.release();
    d_off.release();
    d_len.release();
    n = 0;
  }
};

// reverse_complement of /root/reference/src/alignment.rs:178-190
inline uint8_t rc_base(uint8_t b) {
  switch (b) {
    case 'A': case 'a': return 'T';
    case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    default: return 'N';
  }
}

}  // namespace

struct awv_engine {
  awv_engine_config cfg{};
  int device = 0;
  int num_cus = 0;
  int wall_clock_khz = 100000;  // rate of s_memrealtime (hipDeviceAttributeWallClockRate)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  SeqSet seqs;
  // scratch arenas (per persistent workgroup)
  DevBuf<uint8_t> ring_mem, hist_mem;
  DevBuf<uint32_t> ev_mem;
  DevBuf<uint8_t> reuse_mem;  // row archives of the top-level searches (row_reuse.hpp); reserved after every other arena
  // per-launch buffers
  DevBuf<int32_t> d_pair_q, d_pair_t, d_pair_rc;
  DevBuf<int32_t> d_pair_bound;  // score-only launches with a bound per pair
  DevBuf<int32_t> d_unit_first, d_unit_twin;  // twin units (twin_plan.hpp): per dispatch unit its entry and its swapped entry
  uint64_t twin_stats[4] = {0, 0, 0, 0};  // last call: awv_twin_stats
  DevBuf<awvr::Span> d_pair_span;  // range launches: the rectangle of every pair
  DevBuf<uint64_t> d_cigar_off;
  DevBuf<awv::DevResult> d_results;
  DevBuf<uint8_t> d_cigar;
  DevBuf<unsigned long long> d_counters;  // [0] work cursor, [1..] stats
  std::vector<uint8_t> h_cigar;
  std::vector<uint8_t> h_cs;  // a cs call: the batch's cs text, next to h_cigar and handed on like it
  // host sides of a launch's uploads and of its read-back: kept with the engine, like h_cigar, so that the copies of every call
  // start from / land in the same host memory (fresh allocations per call cost the runtime tens of milliseconds now and then)
  struct HostStage {
    std::vector<int32_t> hq, ht, hrc, hbound, hufirst, hutwin;
    std::vector<uint64_t> hoff;
    std::vector<awvr::Span> hspan;
    std::vector<awv_result> tres;
    unsigned long long hreuse[4] = {0, 0, 0, 0};
  } stage;
  awv_stats stats{};
  awp::PlanState* plan = nullptr;  // planner.hip: sketches of `seqs` and planning scratch (released with a new set)
  awvf::State* verify = nullptr;   // verify.hip: buffers and stats of the verify launches
  awvc::State* clip = nullptr;     // clip.hip: buffers and stats of the clip launches
  awvs::State* split = nullptr;    // split.hip: likewise for the split launches
  awvn::State* normalize = nullptr;  // normalize.hip: likewise for the normalize launches
  awve::State* encode = nullptr;   // encode.hip: likewise for the encode launches, and the text arena of the batch in hand
  awvcs::State* cs = nullptr;      // cs.hip: likewise for the cs launches, and the cs arena of the batch in hand
  awvcov::State* cov = nullptr;    // coverage.hip: the depth accumulators between awv_engine_coverage_begin and its end, and the launches' buffers
  bool cov_paused = false;         // (orient.hip: the strand alignments inside an orientation call do not count -- for the depth and for the allele table)
  awvvar::State* var = nullptr;    // variants.hip: the allele table between awv_engine_variants_begin and its end, and the launches' buffers
  awvl::State* lift = nullptr;     // lift.hip: the regions and rows between awv_engine_lift_begin and its end, and the launches' buffers
  awvmsa::State* msa = nullptr;    // msa.hip: the launches' buffers and the last call's stats
  int32_t norm_mode = AWV_NORM_OFF;  // awv_engine_set_normalize: read at the start of every aligning call
};

namespace {

int upload_seqset(awv_engine* e, SeqSet& s, int32_t n, const uint8_t* bytes, const uint64_t* offsets) {
  if (n < 0 || (n > 0 && (!bytes || !offsets))) return fail(AWV_ERR_ARG, "set_sequences: null input");
  s.n = 0;  // the set counts as loaded (awv_align_pairs passes its AWV_ERR_STATE check) only once every copy below has landed
  s.off.assign((size_t)n + 1, 0);
  s.len.assign((size_t)n, 0);
  uint64_t run = 0;
  for (int i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(AWV_ERR_ARG, "set_sequences: offsets not monotone");
    const uint64_t l = offsets[i + 1] - offsets[i];
    if (l > (uint64_t)(INT32_MAX / 4)) return fail(AWV_ERR_ARG, "set_sequences: sequence too long");
    s.off[i] = run;
    s.len[i] = (int32_t)l;
    run += l + awp::SEQ_PAD_BYTES;  // extend reads 8 bytes at a time: keep over-reads inside the allocation
  }
  s.off[n] = run;
  s.total = run + 64;
  std::vector<uint8_t> h[4];
  for (auto& v : h) v.assign(s.total, 0);
  for (int i = 0; i < n; ++i) {
    const uint8_t* src = bytes + offsets[i];
    const size_t l = (size_t)s.len[i];
    uint8_t* f = h[0].data() + s.off[i];
    uint8_t* r = h[1].data() + s.off[i];
    uint8_t* c = h[2].data() + s.off[i];
    uint8_t* cr = h[3].data() + s.off[i];
    for (size_t j = 0; j < l; ++j) {
      const uint8_t b = src[j];
      f[j] = b;
      r[l - 1 - j] = b;
      const uint8_t cb = rc_base(b);
      c[l - 1 - j] = cb;  // reverse complement
      cr[j] = cb;         // its reversal
    }
  }
  // 2-bit packed copies (A,C,G,T -> 0..3, 16 bases per word) for sequences made of upper-case ACGT only;
  // bytes are compared verbatim by the reference, so anything else keeps the raw-byte path
  // (two pad words in front of the first sequence, one behind every sequence and four at the end: the kernels' probes of
  // packed words in place -- seq_mode 2 -- read up to two words below a sequence's first and two beyond its last)
  std::vector<uint64_t> off2((size_t)n + 1, 2);
  std::vector<uint8_t> ok2((size_t)std::max(n, 1), 0);
  for (int i = 0; i < n; ++i) off2[i + 1] = off2[i] + ((size_t)s.len[i] + 15) / 16 + 1;
  std::vector<uint32_t> h2[2];
  for (auto& v : h2) v.assign(off2[n] + 4, 0u);
  auto code = [](uint8_t b) -> int { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1; };
  for (int i = 0; i < n; ++i) {
    for (int v = 0; v < 2; ++v) {
      const uint8_t* src = h[v ? 2 : 0].data() + s.off[i];
      uint32_t* dst = h2[v].data() + off2[i];
      bool ok = true;
      for (size_t j = 0; j < (size_t)s.len[i]; ++j) {
        const int c = code(src[j]);
        if (c < 0) { ok = false; break; }
        dst[j >> 4] |= (uint32_t)c << (2 * (j & 15));
      }
      if (ok) ok2[i] |= (uint8_t)(1 << v);
    }
  }
  AWV_TRY(hipSetDevice(e->device));
  for (int v = 0; v < 2; ++v) {
    if (int rc = s.d_seq2[v].reserve(h2[v].size())) return rc;
    AWV_TRY(hipMemcpyAsync(s.d_seq2[v].p, h2[v].data(), h2[v].size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  }
  if (int rc = s.d_off2.reserve((size_t)n + 1)) return rc;
  if (int rc = s.d_ok2.reserve(ok2.size())) return rc;
  AWV_TRY(hipMemcpyAsync(s.d_off2.p, off2.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipMemcpyAsync(s.d_ok2.p, ok2.data(), ok2.size(), hipMemcpyHostToDevice, e->stream));
  for (int v = 0; v < 4; ++v) {
    if (int rc = s.d_seq[v].reserve(s.total)) return rc;
    AWV_TRY(hipMemcpyAsync(s.d_seq[v].p, h[v].data(), s.total, hipMemcpyHostToDevice, e->stream));
  }
  if (int rc = s.d_off.reserve((size_t)n + 1)) return rc;
  if (int rc = s.d_len.reserve((size_t)std::max(n, 1))) return rc;
  AWV_TRY(hipMemcpyAsync(s.d_off.p, s.off.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
  if (n > 0) AWV_TRY(hipMemcpyAsync(s.d_len.p, s.len.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipStreamSynchronize(e->stream));
  s.n = n;
  return AWV_OK;
}

// what makes a penalty set meaningful at all (the verify check re-scores under any such set: awv_internal_check_penalties); what
// the alignment kernels can run is batch_plan.hpp's plan_penalties
int check_penalty_signs(const awv_penalties* p) {
  std::string msg;
  const int rc = awvb::check_signs(p, msg);
  return rc == AWV_OK ? rc : fail(rc, msg);
}

// ---- arena placement --------------------------------------------------------------------------
// Where a multi-GB arena lands in HBM is worth up to +-6 % of the row traffic's rate (measured: the
// same kernel on five arenas allocated one after the other ran 1315..1465 ms, each arena keeping its
// rate; scratch/src/memplace.hip shows the same split with nothing but the traffic).  So the ring
// arena is chosen: a few candidates are allocated, each is timed with a few milliseconds of the step
// kernel's traffic pattern (rows 1, 2, 5, 10 and 25 steps old read, five rows written, per 248-column
// window, one wave per workgroup slot), the fastest is kept and the others are freed.
__global__ __launch_bounds__(64, 4) void arena_probe_kernel(unsigned char* arena, size_t slot_stride, int row_bytes, int steps, int width_cols,
                                                             unsigned long long* sink) {
  const int lane = threadIdx.x;
  awv::rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(arena + (size_t)blockIdx.x * slot_stride, 0, (int)std::min<size_t>(slot_stride, 0x7FFFFFFF), 0x00020000);
  auto off = [&](int dir, int comp, int score) { return ((dir * 5 + comp) * 32 + (score & 31)) * row_bytes; };
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  unsigned acc = 0;
  for (int s = 32; s < 32 + steps; ++s) {
    for (int dir = 0; dir < 2; ++dir) {
      const int lo = 1024 + (s & 7) * 4;
      for (int cb = lo; cb < lo + width_cols; cb += 248) {
        const int voff = (cb + lane * 4) * 2;
        const u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 0, s - 5), 0);
        const u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 0, s - 10), 0);
        const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 0, s - 25), 0);
        const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 1, s - 2), 2);
        const u32x2 f = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 3, s - 2), 2);
        const u32x2 g = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 2, s - 1), 2);
        const u32x2 h = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, off(dir, 4, s - 1), 2);
        const u32x2 m = a + b + c;
        acc += m[0] ^ m[1];
        __builtin_amdgcn_raw_buffer_store_b64(b + d, rs, voff, off(dir, 1, s), 0);
        __builtin_amdgcn_raw_buffer_store_b64(b + f, rs, voff, off(dir, 3, s), 0);
        __builtin_amdgcn_raw_buffer_store_b64(c + g, rs, voff, off(dir, 2, s), 0);
        __builtin_amdgcn_raw_buffer_store_b64(c + h, rs, voff, off(dir, 4, s), 0);
        __builtin_amdgcn_raw_buffer_store_b64(m, rs, voff, off(dir, 0, s), 0);
      }
    }
  }
  if (acc == 0x12345678u) sink[0] = acc;
}

// ---- an aligning call: batch_plan.hpp decides, the stages below carry it out ----
struct SplitOut {
  int64_t min_score;
  const uint64_t* seg_first;
  awv_split_index* iout;
  awv_clip_result* sout;
};
// What one call asks for; every aligning entry point of the C ABI fills one.
struct AlignRequest {
  const awv_pair* pairs = nullptr;
  int64_t npairs = 0;
  awv_result* out = nullptr;
  awv_sink sink = nullptr;
  void* user = nullptr;
  // awv_score_pairs: the top-level search's score only, no CIGAR arena (so max_arena_bytes does not cut batches)
  bool score_only = false;
  // the call's bound (INT_MAX = none), or pair i's own bound instead (nullable; INT_MAX = none).  A full alignment may carry
  // bounds too (awv_align_pairs_bounded): they stop the pair's top-level search, nothing below it
  int max_penalty = INT_MAX;
  const int32_t* pair_bound = nullptr;
  // (nullable; awv_align_pairs_verified, on the engine's own sequence set): every batch's records and op bytes are checked on
  // the device before the batch's CIGARs are copied back
  awv_verify_result* vout = nullptr;
  // (nullable; the awv_*_ranges calls): pair i aligns the rectangle spans[i] of its two sequences, in pattern / text
  // coordinates and already validated, instead of the whole of them -- every length of the plan is then the rectangle's
  const awvr::Span* spans = nullptr;
  // (nullable; awv_align_pairs_clipped): every batch's op strings are clipped on the device under match_bonus, after the check
  // and before the batch's CIGARs are copied back
  awv_clip_result* cout = nullptr;
  int32_t match_bonus = 0;
  // (nullable; awv_align_pairs_split): likewise split into all segments of at least split->min_score, into the caller's slot
  // layout (already checked against the slot rule)
  const SplitOut* split = nullptr;
  // (nullable; awv_align_pairs_encoded): every batch's op strings -- their clips under match_bonus > 0 -- become run-length text
  // on the device, last of the record steps; the text is copied back and handed to the sink in the op bytes' place
  awv_cigar_text* tout = nullptr;
  // (nullable; awv_align_pairs_cs): every batch's op strings -- their clips under match_bonus > 0 -- become cs text on the device,
  // after the run-length text; it is copied to a host buffer of its own and handed to cs_sink, which stands in sink's place
  awv_cs_text* csout = nullptr;
  int32_t cs_mode = 0;
  awv_cs_sink cs_sink = nullptr;
};

// With several batches in a call, the sink of batch i (the caller's formatting and output) runs on a
// helper thread while batch i+1 is carved, launched and copied back.  It is joined before the next
// sink starts: sinks never overlap, come in batch order, and a batch's result / CIGAR buffers stay
// untouched until its sink has returned.  The last batch's sink runs on the calling thread.
struct SinkRunner {
  std::thread th;
  int rc = 0;
  std::vector<awv_result> res;
  std::vector<uint8_t> cig, cs;
  int wait() {
    if (th.joinable()) th.join();
    const int r = rc;
    rc = 0;
    return r;
  }
  ~SinkRunner() { if (th.joinable()) th.join(); }
};

// Everything one call carries from stage to stage.
struct AlignCall {
  awv_engine* e;
  SeqSet& s;
  const awv_penalties* pen;
  const AlignRequest& rq;
  awvb::PenaltyPlan pp;
  awvb::Config cfg;
  int32_t norm = AWV_NORM_OFF;
  bool twin_ok = false;
  int64_t max_batch = 0;
  uint64_t max_arena = 0;
  // experiment knobs (read_knobs)
  bool inline_sink = false, timing = false;
  int force_sixteen_len = INT_MAX;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  // the batch in hand: pairs [first, first + n) of the call, `arena` bytes of CIGARs, results in caller order
  int64_t first = 0, n = 0;
  uint64_t arena = 0;
  uint64_t text_bytes = 0;  // an encoded call: the batch's text arena
  uint64_t cs_bytes = 0;    // a cs call: the batch's cs arena
  std::vector<awvb::Entry> entries;
  std::vector<awv_result> hres;
  double kernel_ms = 0, h2d_ms = 0, d2h_ms = 0;
  unsigned long long stat_tot[awv::STAT_N_DEV] = {0};
  uint64_t launches = 0;
  awvrr::Layout reuse{0, 0, 0, 0};  // the running group's row archives (passes == 0: none)
  SinkRunner runner;
  bool want_cigar() const { return (rq.sink || rq.cs_sink) && !rq.score_only && !(e->cfg.flags & AWV_F_KEEP_ON_DEVICE); }
  void lap(const char* what) const {  // diagnostic: host-side stage times on stderr
    if (timing) fprintf(stderr, "[awv] %-22s %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
};

// Experiment knobs read from the environment exist only in a -DAWV_DEBUG_KNOBS build; the product library's
// behaviour depends on its arguments alone.
void read_knobs(AlignCall& c) {
#ifdef AWV_DEBUG_KNOBS
  if (const char* env = getenv("AWV_MAX_ARENA_MB")) c.max_arena = std::max<uint64_t>(1, (uint64_t)atoll(env)) << 20;
  c.inline_sink = getenv("AWV_INLINE_SINK") != nullptr;  // every sink on the calling thread
  c.timing = getenv("AWV_TIMING") != nullptr;
  if (const char* env = getenv("AWV_FORCE_SIXTEEN")) c.force_sixteen_len = atoi(env);  // experiment: sixteen waves per pair for sequences at least that long
#else
  (void)c;
#endif
}

// the two events around a stretch of stream work: its milliseconds are added to `acc`
int timer_wait(AlignCall& c, double& acc) {
  float ms = 0;
  AWV_TRY(hipEventSynchronize(c.e->ev1));
  AWV_TRY(hipEventElapsedTime(&ms, c.e->ev0, c.e->ev1));
  acc += ms;
  return AWV_OK;
}
int timer_stop(AlignCall& c, double& acc) {
  AWV_TRY(hipEventRecord(c.e->ev1, c.e->stream));
  return timer_wait(c, acc);
}

// ---- per batch: carve, order, buffers ----
// (the (pattern, text) lengths a pair is aligned over decide cost order, kernel flavour, row width, row capacity and the CIGAR arena)
bool carve_and_order(AlignCall& c) {
  const AlignRequest& rq = c.rq;
  const awvb::Carve cv = awvb::carve_batch(
      [&](int64_t gi, int32_t& ql, int32_t& tl) {
        if (rq.spans) {
          ql = rq.spans[gi].pe - rq.spans[gi].pb;
          tl = rq.spans[gi].te - rq.spans[gi].tb;
        } else {
          ql = c.s.len[rq.pairs[gi].q_idx];
          tl = c.s.len[rq.pairs[gi].t_idx];
        }
      },
      c.first, rq.npairs, c.max_batch, c.max_arena, rq.score_only, c.entries);
  c.n = cv.n;
  c.arena = cv.arena;
  for (awvb::Entry& en : c.entries) {
    const awv_pair& p = rq.pairs[c.first + en.batch_index];
    en.q = p.q_idx;
    en.t = p.t_idx;
    en.rc = p.q_revcomp ? 1 : 0;
  }
  return awvb::order_by_cost(c.entries);  // results and CIGARs keep their caller-order slots through Entry::batch_index
}

int reserve_batch_buffers(AlignCall& c) {
  awv_engine* e = c.e;
  const size_t n = (size_t)c.n;
  if (int rc = e->d_pair_q.reserve(n)) return rc;
  if (int rc = e->d_pair_t.reserve(n)) return rc;
  if (int rc = e->d_pair_rc.reserve(n)) return rc;
  if (int rc = e->d_cigar_off.reserve(n)) return rc;
  if (int rc = e->d_results.reserve(n)) return rc;
  if (int rc = e->d_cigar.reserve((size_t)c.arena + 64)) return rc;
  if (int rc = e->d_counters.reserve(1 + awv::STAT_N_DEV + awv::RR_DESC_WORDS)) return rc;  // (behind the counters: the row archives' descriptor)
  static_assert(sizeof(awv_result) == sizeof(awv::DevResult), "result layout");
  c.hres.assign(n, awv_result{});
  return AWV_OK;
}

// the pairs of a group whose length difference alone rules out rows within the 2 GiB limit end CAPACITY before any launch
void drop_beyond_span(AlignCall& c, std::vector<awvb::Entry>& ge, int width) {
  const long long span = awvb::capacity_span(LIMITS, awvb::wc_2g(LIMITS, c.pp.ring, width));
  size_t k = 0;
  for (size_t i = 0; i < ge.size(); ++i) {
    const awvb::Entry en = ge[i];
    if (awvb::beyond_span(en.ql, en.tl, span)) {
      awv_result r{};
      r.status = AWV_ST_CAPACITY;
      r.cigar_off = en.off;
      c.hres[(size_t)en.batch_index] = r;
      continue;
    }
    ge[k++] = en;
  }
  ge.resize(k);
}

// ---- arenas ----
// The ring arena grows: choose where it lies (see arena_probe_kernel).
int choose_ring_arena(AlignCall& c, const awvb::RowPlan& rp, int wc, int nslots) {
  awv_engine* e = c.e;
  const size_t ring_stride = rp.ring_stride(wc);
  const size_t want = ring_stride * (size_t)nslots + ((size_t)64 << 20);
  size_t free_b = 0, total_b = 0;
  e->ring_mem.release();
  (void)hipMemGetInfo(&free_b, &total_b);
  int ncand = (e->cfg.flags & AWV_F_NO_ARENA_PROBE) ? 1 : 4;
  while (ncand > 1 && (size_t)ncand * want > free_b / 10 * 8) --ncand;  // all candidates are alive at once
  const bool probe_ok = ncand > 1 && want >= ((size_t)1 << 30) && rp.esz == 2 && ring_stride >= (size_t)2 * 5 * 32 * 4096 &&
                        (size_t)wc * rp.esz >= 4096;
  if (!probe_ok) ncand = 1;
  uint8_t* cand[4] = {nullptr, nullptr, nullptr, nullptr};
  float cms[4] = {0, 0, 0, 0};
  int best = -1;
  for (int k = 0; k < ncand; ++k) {
    if (hipMalloc((void**)&cand[k], want) != hipSuccess) { cand[k] = nullptr; (void)hipGetLastError(); break; }
    if (ncand == 1) { best = 0; break; }
    float tbest = 1e30f;
    hipError_t perr = hipSuccess;
    for (int rep = 0; rep < 2 && perr == hipSuccess; ++rep) {
      float pms = 0;
      if ((perr = hipEventRecord(e->ev0, e->stream)) != hipSuccess) break;
      hipLaunchKernelGGL(arena_probe_kernel, dim3(nslots), dim3(64), 0, e->stream, cand[k], ring_stride, (int)((size_t)wc * rp.esz), 24,
                         std::min(1400, wc - 2048), e->d_counters.p);
      if ((perr = hipEventRecord(e->ev1, e->stream)) != hipSuccess) break;
      if ((perr = hipEventSynchronize(e->ev1)) != hipSuccess) break;
      if ((perr = hipEventElapsedTime(&pms, e->ev0, e->ev1)) != hipSuccess) break;
      tbest = std::min(tbest, pms);
    }
    if (perr != hipSuccess) {  // nothing may stay allocated behind an error return
      for (int j = 0; j < 4; ++j)
        if (cand[j]) (void)hipFree(cand[j]);
      return fail(AWV_ERR_HIP, std::string("ring arena probe: ") + hipGetErrorString(perr));
    }
    cms[k] = tbest;
    if (best < 0 || tbest < cms[best]) best = k;
    if (c.timing) fprintf(stderr, "[awv] ring arena candidate %d at %p: %.2f ms\n", k, (void*)cand[k], tbest);
  }
  if (best < 0) return fail(AWV_ERR_OOM, "hipMalloc " + std::to_string(want) + " bytes for the ring arena failed");
  for (int k = 0; k < 4; ++k)
    if (k != best && cand[k]) (void)hipFree(cand[k]);
  e->ring_mem.adopt(cand[best], want);
  return AWV_OK;
}

// the per-workgroup arenas of an attempt of `nslots` workgroups at row capacity wc (DevBuf::reserve only ever grows)
int ensure_arenas(AlignCall& c, const awvb::RowPlan& rp, int wc, int nslots) {
  awv_engine* e = c.e;
  if (rp.ring_stride(wc) * nslots > e->ring_mem.cap)
    if (int rc = choose_ring_arena(c, rp, wc, nslots)) return rc;
  if (int rc = e->hist_mem.reserve(rp.hist_stride * nslots)) return rc;
  if (int rc = e->ev_mem.reserve(rp.ev_stride(wc) * nslots)) return rc;
  return AWV_OK;
}

// The row archives of an attempt: only the one-wave kernels with 16-bit rows keep them, for whole pairs aligned
// in full, and only in what the scratch budget leaves after the arenas above.  No archive is no error: the kernel then
// computes every row.
void plan_row_archives(AlignCall& c, const std::vector<awvb::Entry>& ge, const awvb::RowPlan& rp, int wc, int nslots) {
  awv_engine* e = c.e;
  c.reuse = awvrr::Layout{0, 0, 0, 0};
  const AlignRequest& rq = c.rq;
  if (rp.waves != 1 || rp.width != 0 || (e->cfg.flags & AWV_F_NO_ROW_REUSE) || rq.spans || rq.score_only || rq.pair_bound ||
      rq.max_penalty != INT_MAX || c.pp.multi_T <= 0)
    return;
  int maxsum = 0;
  for (const awvb::Entry& p : ge) maxsum = std::max(maxsum, p.ql + p.tl);
  const int chain = std::min(std::max(c.pp.chain_max, 1), awv::CHAIN_MAX);
  const int T = chain > 1 ? awv::TMAX * chain : c.pp.multi_T;
  const int nid = 2 * c.pp.e1 + (c.pp.two_piece ? 2 * c.pp.e2 : 0);
  const size_t used = rp.per_slot(wc) * (size_t)nslots;
  const int passes = awvrr::plan_passes(maxsum, T, nid, nslots, rp.budget > used ? rp.budget - used : 0);
  if (passes == 0) {
    c.lap("row archives: none (no room, or pairs too short)");
    return;
  }
  const awvrr::Layout l = awvrr::make_layout(passes, T, nid);
  if (e->reuse_mem.reserve(l.bytes() * (size_t)nslots) != AWV_OK) {  // (awv_stats.prof[13] then stays 0 for the launch)
    (void)hipGetLastError();
    c.lap("row archives: none (allocation failed)");
    return;
  }
  c.reuse = l;
  if (c.timing) fprintf(stderr, "[awv] row archives: %d passes of %d scores, %zu MiB for %d workgroups\n", passes, T, (l.bytes() * (size_t)nslots) >> 20, nslots);
}

// ---- one attempt of a group: upload, launch, read back ----
// Twin units: an entry (q, t) and its swapped entry (t, q) of this launch share their breakpoint searches.
// Entries are in descending cost order and a twin costs what its partner costs, so units ordered by their summed cost are the
// twin units in entry order, then the single ones.
int upload_twin_units(AlignCall& c, const std::vector<awvb::Entry>& ge, int64_t& nunits) {
  awv_engine* e = c.e;
  awv_engine::HostStage& st = e->stage;
  const awvt::TwinPlan tp = awvt::plan_twins(st.hq.data(), st.ht.data(), st.hrc.data(), ge.size());
  std::vector<size_t> uo(tp.first.size());
  for (size_t u = 0; u < uo.size(); ++u) uo[u] = u;
  auto ucost = [&](size_t u) {
    const awvb::Entry& en = ge[(size_t)tp.first[u]];
    const uint64_t cost = awvb::pair_cost(en.ql, en.tl);
    return tp.twin[u] >= 0 ? 2 * cost : cost;
  };
  std::stable_sort(uo.begin(), uo.end(), [&](size_t a, size_t b) { return ucost(a) > ucost(b); });
  st.hufirst.resize(uo.size());
  st.hutwin.resize(uo.size());
  for (size_t u = 0; u < uo.size(); ++u) {
    st.hufirst[u] = tp.first[uo[u]];
    st.hutwin[u] = tp.twin[uo[u]];
  }
  nunits = (int64_t)uo.size();
  if (int rc = e->d_unit_first.reserve((size_t)nunits)) return rc;
  if (int rc = e->d_unit_twin.reserve((size_t)nunits)) return rc;
  AWV_TRY(hipMemcpyAsync(e->d_unit_first.p, st.hufirst.data(), (size_t)nunits * 4, hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipMemcpyAsync(e->d_unit_twin.p, st.hutwin.data(), (size_t)nunits * 4, hipMemcpyHostToDevice, e->stream));
  return AWV_OK;
}

// the group's entries, split into the device's arrays; nunits: the launch's dispatch units (entries, or entries with their twins)
int upload_group(AlignCall& c, const std::vector<awvb::Entry>& ge, const awvb::RowPlan& rp, int64_t& nunits) {
  awv_engine* e = c.e;
  awv_engine::HostStage& st = e->stage;
  const AlignRequest& rq = c.rq;
  const size_t m = ge.size();
  st.hq.resize(m); st.ht.resize(m); st.hrc.resize(m); st.hoff.resize(m);
  for (size_t i = 0; i < m; ++i) {
    st.hq[i] = ge[i].q; st.ht[i] = ge[i].t; st.hrc[i] = ge[i].rc; st.hoff[i] = ge[i].off;
  }
  AWV_TRY(hipEventRecord(e->ev0, e->stream));
  AWV_TRY(hipMemcpyAsync(e->d_pair_q.p, st.hq.data(), m * 4, hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipMemcpyAsync(e->d_pair_t.p, st.ht.data(), m * 4, hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipMemcpyAsync(e->d_pair_rc.p, st.hrc.data(), m * 4, hipMemcpyHostToDevice, e->stream));
  AWV_TRY(hipMemcpyAsync(e->d_cigar_off.p, st.hoff.data(), m * 8, hipMemcpyHostToDevice, e->stream));
  if (rq.pair_bound) {
    st.hbound.resize(m);
    for (size_t i = 0; i < m; ++i) st.hbound[i] = rq.pair_bound[c.first + ge[i].batch_index];
    if (int rc = e->d_pair_bound.reserve(m)) return rc;
    AWV_TRY(hipMemcpyAsync(e->d_pair_bound.p, st.hbound.data(), m * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (rq.spans) {
    st.hspan.resize(m);
    for (size_t i = 0; i < m; ++i) st.hspan[i] = rq.spans[c.first + ge[i].batch_index];
    if (int rc = e->d_pair_span.reserve(m)) return rc;
    AWV_TRY(hipMemcpyAsync(e->d_pair_span.p, st.hspan.data(), m * sizeof(awvr::Span), hipMemcpyHostToDevice, e->stream));
  }
  nunits = (int64_t)m;
  if (rp.twin_here)
    if (int rc = upload_twin_units(c, ge, nunits)) return rc;
  AWV_TRY(hipMemsetAsync(e->d_counters.p, 0, (1 + awv::STAT_N_DEV + awv::RR_DESC_WORDS) * sizeof(unsigned long long), e->stream));
  if (c.reuse.passes > 0) {  // the launch's row archives (biwfa_device.hpp, RR_DESC_WORDS)
    st.hreuse[0] = (unsigned long long)(uintptr_t)e->reuse_mem.p;
    st.hreuse[1] = (unsigned long long)c.reuse.bytes();
    st.hreuse[2] = (unsigned long long)(unsigned)c.reuse.passes | ((unsigned long long)(unsigned)c.reuse.T << 32);
    st.hreuse[3] = (unsigned long long)c.reuse.nid | ((unsigned long long)((e->cfg.flags & AWV_F_ROW_REUSE_LEVEL1) ? awvrr::LV_ONE : awvrr::LV_ALL) << 32);
    AWV_TRY(hipMemcpyAsync(e->d_counters.p + 1 + awv::STAT_N_DEV, st.hreuse, sizeof(st.hreuse), hipMemcpyHostToDevice, e->stream));
  }
  return timer_stop(c, c.h2d_ms);
}

awv::KParams fill_kparams(const AlignCall& c, const awvb::RowPlan& rp, int wc, int64_t nunits) {
  const awv_engine* e = c.e;
  const SeqSet& s = c.s;
  const bool narrow = rp.width != 1;
  awv::KParams kp{};
  for (int v = 0; v < 4; ++v) kp.seq[v] = s.d_seq[v].p;
  kp.seq_off = s.d_off.p;
  kp.seq_len = s.d_len.p;
  kp.seq2[0] = s.d_seq2[0].p;
  kp.seq2[1] = s.d_seq2[1].p;
  kp.seq2_off = s.d_off2.p;
  kp.seq2_ok = s.d_ok2.p;
  kp.pair_q = e->d_pair_q.p;
  kp.pair_t = e->d_pair_t.p;
  kp.pair_rc = e->d_pair_rc.p;
  kp.npairs = nunits;
  kp.unit_first = rp.twin_here ? e->d_unit_first.p : nullptr;
  kp.unit_twin = rp.twin_here ? e->d_unit_twin.p : nullptr;
  kp.twin_levels = (e->cfg.flags & AWV_F_TWIN_TOP_ONLY) ? 1 : INT_MAX;
  kp.twin_base = (e->cfg.flags & AWV_F_NO_TWIN_BASE) ? 0 : 1;
  kp.pen = awv::DevPenalties{c.pp.x, c.pp.o1, c.pp.e1, c.pp.o2, c.pp.e2, c.pp.two_piece, c.pp.scope};
  kp.ring = c.pp.ring;
  // 32-bit rows: sweeps of at most TMAX32 scores, at most CHAIN_MAX32 of them chained (a lane vector is four registers)
  kp.multi_T = narrow ? c.pp.multi_T : (std::min(c.pp.multi_T, awv::TMAX32) >= 2 ? std::min(c.pp.multi_T, awv::TMAX32) : 0);
  kp.deep_passes = (kp.multi_T > 0 && !(e->cfg.flags & AWV_F_NO_DEEP)) ? 1 : 0;
  kp.sub16 = (e->cfg.flags & AWV_F_FORCE_INT32) ? 0 : 1;  // (the pin means 32-bit rows throughout)
  // (32-bit rows: two sweeps chained through registers, a third when the kernel finds room for its chain rows in LDS -- the
  // kernel caps what it is offered: biwfa_device.hpp, multi_phase's lds_chain)
  kp.chain_max = narrow ? c.pp.chain_max : (awv::TMAX32 == awv::TMAX ? std::min(c.pp.chain_max, 3) : 1);
  kp.wcap = wc;
  kp.ring_mem = e->ring_mem.p;
  kp.ring_slot_stride = rp.ring_stride(wc);
  kp.lds_meta_bytes = (int)rp.lds_meta;
  kp.lds_seq_bytes = (int)rp.lds_seq;
  kp.sb_cap = c.pp.sb_cap;
  kp.wb_cap = c.pp.wb_cap;
  kp.hist_mem = e->hist_mem.p;
  kp.hist_slot_stride = rp.hist_stride;
  kp.hist_meta_offset = rp.hist_rows;
  kp.ev_mem = e->ev_mem.p;
  kp.ev_slot_stride = rp.ev_stride(wc);
  kp.cigar = e->d_cigar.p;
  kp.cigar_off = e->d_cigar_off.p;
  kp.results = e->d_results.p;
  kp.work_counter = e->d_counters.p;
  kp.stats = e->d_counters.p + 1;
  kp.score_only = c.rq.score_only ? 1 : 0;
  kp.max_penalty = c.rq.max_penalty;
  kp.pair_max_penalty = c.rq.pair_bound ? e->d_pair_bound.p : nullptr;
  return kp;
}

// The kernel of a multi-wave flavour: NS names one inclusion of biwfa_device.hpp; the choice runs over 2-piece x row type x
// ranged (range launches: the kernels' two-argument instantiations).  The AWV_WIDE16 inclusions hold only their 16-bit kernels.
// (kernels_awv.hip has the same choice for the one-wave flavour.)
struct LaunchShape {
  unsigned grid;
  int wg;
  size_t dyn_lds;
  hipStream_t stream;
  bool two_piece, narrow;
  const awvr::Span* d_span;
};
#define AWV_KERNELS_OF(NS)                                                                   \
  struct NS##_kernels {                                                                      \
    typedef NS::KParams KParams;                                                             \
    static constexpr bool only16 = NS::WENC;                                                 \
    template <bool P2, typename OffT, typename... S>                                         \
    static auto kernel() { return &NS::biwfa_align_kernel<P2, OffT, S...>; }                \
  }
AWV_KERNELS_OF(awvw);
AWV_KERNELS_OF(awvx);
AWV_KERNELS_OF(awvw_m);
AWV_KERNELS_OF(awvx_m);
#undef AWV_KERNELS_OF
template <typename K, typename KP, typename... PairSpan>
int launch_kernel(K kern, const LaunchShape& l, const KP& kparams, PairSpan... pair_span) {
  AWV_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.dyn_lds));
  hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.wg), l.dyn_lds, l.stream, kparams, pair_span...);
  return AWV_OK;
}
template <typename NS, bool P2, typename OffT>
int launch_ranged(const LaunchShape& l, const typename NS::KParams& k) {
  if (l.d_span) return launch_kernel(NS::template kernel<P2, OffT, const awvr::Span*>(), l, k, l.d_span);
  return launch_kernel(NS::template kernel<P2, OffT>(), l, k);
}
template <typename NS, bool P2>
int launch_rows(const LaunchShape& l, const typename NS::KParams& k) {
  if constexpr (NS::only16) return launch_ranged<NS, P2, int16_t>(l, k);
  else return l.narrow ? launch_ranged<NS, P2, int16_t>(l, k) : launch_ranged<NS, P2, int32_t>(l, k);
}
template <typename NS>
int launch_flavour(const LaunchShape& l, const awv::KParams& kp) {
  static_assert(sizeof(typename NS::KParams) == sizeof(awv::KParams), "same parameter block for every workgroup size");
  typename NS::KParams k;
  std::memcpy(&k, &kp, sizeof(k));
  return l.two_piece ? launch_rows<NS, true>(l, k) : launch_rows<NS, false>(l, k);
}

int launch_group(AlignCall& c, const awvb::RowPlan& rp, const awv::KParams& kp, int nslots) {
  awv_engine* e = c.e;
  const LaunchShape l{(unsigned)nslots, rp.wg, rp.dyn_lds, e->stream, kp.pen.two_piece != 0, rp.width != 1, c.rq.spans ? e->d_pair_span.p : nullptr};
  AWV_TRY(hipEventRecord(e->ev0, e->stream));
  if (rp.waves == 1) AWV_TRY((hipError_t)awv_launch_one_wave(l.two_piece, l.narrow ? 1 : 0, l.d_span, l.grid, l.dyn_lds, l.stream, &kp));
  else if (int rc = rp.width == 2 ? (rp.waves == 4 ? launch_flavour<awvw_m_kernels>(l, kp) : launch_flavour<awvx_m_kernels>(l, kp))
                                  : (rp.waves == 4 ? launch_flavour<awvw_kernels>(l, kp) : launch_flavour<awvx_kernels>(l, kp)))
    return rc;
  AWV_TRY(hipGetLastError());
  AWV_TRY(hipEventRecord(e->ev1, e->stream));
  // while the kernel runs: get the host CIGAR buffer's pages in place (0.2 s for config 2's 670 MB)
  if (c.want_cigar() && !c.rq.tout && e->h_cigar.size() < (size_t)c.arena + 64) e->h_cigar.resize((size_t)c.arena + 64);
  if (int rc = timer_wait(c, c.kernel_ms)) return rc;
  ++c.launches;
  c.lap("kernel done");
  return AWV_OK;
}

// D2H of the attempt's results and counters; every result goes to its caller-order slot
int read_back(AlignCall& c, const std::vector<awvb::Entry>& ge) {
  awv_engine* e = c.e;
  awv_engine::HostStage& st = e->stage;
  const size_t m = ge.size();
  st.tres.resize(m);
  AWV_TRY(hipEventRecord(e->ev0, e->stream));
  AWV_TRY(hipMemcpyAsync(st.tres.data(), e->d_results.p, m * sizeof(awv_result), hipMemcpyDeviceToHost, e->stream));
  unsigned long long hstat[1 + awv::STAT_N_DEV];
  AWV_TRY(hipMemcpyAsync(hstat, e->d_counters.p, sizeof(hstat), hipMemcpyDeviceToHost, e->stream));
  if (int rc = timer_stop(c, c.d2h_ms)) return rc;
  for (int i = 0; i < awv::STAT_N_DEV; ++i) c.stat_tot[i] += hstat[1 + i];
  for (size_t i = 0; i < m; ++i) c.hres[(size_t)ge[i].batch_index] = st.tres[i];
  return AWV_OK;
}

// keeps the pairs to re-run with wider rows: those that outgrew rows narrower than the widest a re-run may use
void select_reruns(const AlignCall& c, std::vector<awvb::Entry>& ge, bool wider_rows_left) {
  const awv_engine::HostStage& st = c.e->stage;
  size_t k = 0;
  if (wider_rows_left && !(c.e->cfg.flags & AWV_F_NO_RERUN))
    for (size_t i = 0; i < ge.size(); ++i)
      if (st.tres[i].status == AWV_ST_CAPACITY) ge[k++] = ge[i];
  ge.resize(k);
}

// One group of the batch = one kernel flavour x one row width.  Attempts: the whole group at row capacity rp.wcap, then only
// the pairs that outgrew it.
int run_group(AlignCall& c, std::vector<awvb::Entry>& ge, const awvb::RowPlan& rp) {
  for (int wc = rp.wcap; !ge.empty(); wc = rp.next_wc(wc)) {
    const int nslots = rp.slots(wc, (int64_t)ge.size());
    if (int rc = ensure_arenas(c, rp, wc, nslots)) return rc;
    plan_row_archives(c, ge, rp, wc, nslots);
    c.lap("arenas reserved");
    if (c.timing) fprintf(stderr, "[awv] ring arena %p (%zu MiB), hist %p, cigar %p\n", (void*)c.e->ring_mem.p, c.e->ring_mem.bytes() >> 20, (void*)c.e->hist_mem.p, (void*)c.e->d_cigar.p);
    int64_t nunits = 0;
    if (int rc = upload_group(c, ge, rp, nunits)) return rc;
    if (int rc = launch_group(c, rp, fill_kparams(c, rp, wc, nunits), nslots)) return rc;
    if (int rc = read_back(c, ge)) return rc;
    select_reruns(c, ge, wc < rp.wc_last);
  }
  return AWV_OK;
}

// The batch's pairs go to their groups; the arenas are reserved for the most demanding group first (one allocation covers
// them all); the groups run from the sixteen-wave flavour down.
int run_groups(AlignCall& c, bool skewed) {
  const awvb::GroupPlan gp = awvb::assign_groups(LIMITS, c.cfg, c.entries, skewed, c.force_sixteen_len);
  std::vector<awvb::Entry> ge[awvb::NG];
  for (int g = 0; g < awvb::NG; ++g) ge[g].reserve(gp.count[g]);
  for (size_t i = 0; i < c.entries.size(); ++i) ge[gp.group[i]].push_back(c.entries[i]);
  awvb::RowPlan rp[awvb::NG];
  for (int k = 0; k < awvb::NG; ++k) {
    const int g = gp.demand_order[k];
    drop_beyond_span(c, ge[g], awvb::width_of(g));
    if (ge[g].empty()) continue;
    rp[g] = awvb::plan_rows(LIMITS, c.cfg, c.pp, ge[g], awvb::waves_of(g), awvb::width_of(g), c.twin_ok);
    if (int rc = ensure_arenas(c, rp[g], rp[g].wcap, rp[g].slots(rp[g].wcap, (int64_t)ge[g].size()))) return rc;
  }
  for (int g = awvb::NG - 1; g >= 0; --g)
    if (int rc = run_group(c, ge[g], rp[g])) return rc;
  return AWV_OK;
}

// ---- after the groups: record steps, copy-back, delivery ----
// normalize first: the check, the clip and the split see the normalized bytes; the text last: it is of the normalized string, and
// of the clip where there is one.  (The groups of a batch overwrite d_results: the
// batch's records, as gathered in hres, go up once per step.)
int run_record_steps(AlignCall& c) {
  awv_engine* e = c.e;
  const AlignRequest& rq = c.rq;
  const SeqSet& s = c.s;
  const int64_t first = c.first, n = c.n;
  const uint64_t arena = c.arena;
  std::vector<awv_result>& hres = c.hres;
  if (c.norm != AWV_NORM_OFF) {
    const awvn::SeqView sv{s.n, s.d_seq[0].p, s.d_seq[2].p, s.d_off.p, s.d_len.p};
    if (int rc = awvn::normalize_batch(e, sv, c.norm, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.spans ? rq.spans + first : nullptr)) return rc;
    c.lap("batch normalized");
  }
  if (rq.vout) {
    if (int rc = awvf::verify_batch(e, c.pen, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.vout + first, rq.spans ? rq.spans + first : nullptr)) return rc;
    c.lap("batch verified");
  }
  if (rq.cout) {
    if (int rc = awvc::clip_batch(e, c.pen, rq.match_bonus, n, hres.data(), e->d_cigar.p, arena, rq.cout + first)) return rc;
    c.lap("batch clipped");
  }
  if (rq.split) {
    if (int rc = awvs::split_batch(e, c.pen, rq.match_bonus, rq.split->min_score, n, hres.data(), e->d_cigar.p, arena, rq.split->seg_first + first,
                                   rq.split->iout + first, rq.split->sout)) return rc;
    c.lap("batch split");
  }
  // (the engine's own set only: awv_align_one aligns a set of its own)
  if (awvcov::active(e->cov) && !e->cov_paused && !rq.score_only && &s == &e->seqs) {
    if (int rc = awvcov::coverage_batch(e, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.cout ? rq.cout + first : nullptr,
                                        rq.split ? rq.split->seg_first + first : nullptr, rq.split ? rq.split->iout + first : nullptr,
                                        rq.split ? rq.split->sout : nullptr, rq.spans ? rq.spans + first : nullptr)) return rc;
    c.lap("batch coverage");
  }
  if (e->var && awvvar::active(e->var) && !e->cov_paused && !rq.score_only && &s == &e->seqs) {
    if (int rc = awvvar::variants_batch(e, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.cout ? rq.cout + first : nullptr,
                                        rq.split ? rq.split->seg_first + first : nullptr, rq.split ? rq.split->iout + first : nullptr,
                                        rq.split ? rq.split->sout : nullptr, rq.spans ? rq.spans + first : nullptr)) return rc;
    c.lap("batch variants");
  }
  if (awvl::active(e->lift) && !e->cov_paused && !rq.score_only && &s == &e->seqs) {
    if (int rc = awvl::lift_batch(e, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.cout ? rq.cout + first : nullptr,
                                  rq.split ? rq.split->seg_first + first : nullptr, rq.split ? rq.split->iout + first : nullptr,
                                  rq.split ? rq.split->sout : nullptr, rq.spans ? rq.spans + first : nullptr)) return rc;
    c.lap("batch lifted");
  }
  if (rq.tout) {
    if (int rc = awve::encode_batch(e, n, hres.data(), e->d_cigar.p, arena, rq.cout ? rq.cout + first : nullptr, rq.tout + first, &c.text_bytes)) return rc;
    c.lap("batch encoded");
  }
  if (rq.csout) {
    if (int rc = awvcs::cs_batch(e, rq.cs_mode, rq.pairs + first, n, hres.data(), e->d_cigar.p, arena, rq.cout ? rq.cout + first : nullptr,
                                rq.spans ? rq.spans + first : nullptr, rq.csout + first, &c.cs_bytes)) return rc;
    c.lap("batch cs");
  }
  return AWV_OK;
}

int copy_cigars_back(AlignCall& c) {
  awv_engine* e = c.e;
  if (c.want_cigar()) {
    // an encoded call: the batch's text in the op bytes' place, in the same host buffer
    const uint8_t* src = c.rq.tout ? awve::batch_text(e) : e->d_cigar.p;
    const size_t bytes = (size_t)(c.rq.tout ? c.text_bytes : c.arena);
    e->h_cigar.resize(bytes + 64);
    c.lap("host cigar buffer");
    AWV_TRY(hipEventRecord(e->ev0, e->stream));
    if (bytes) AWV_TRY(hipMemcpyAsync(e->h_cigar.data(), src, bytes, hipMemcpyDeviceToHost, e->stream));
    if (c.rq.csout) {  // (inside the same bracket: one wait for both copies)
      e->h_cs.resize((size_t)c.cs_bytes + 64);
      if (c.cs_bytes) AWV_TRY(hipMemcpyAsync(e->h_cs.data(), awvcs::batch_text(e), (size_t)c.cs_bytes, hipMemcpyDeviceToHost, e->stream));
    }
    if (int rc = timer_stop(c, c.d2h_ms)) return rc;
  }
  c.lap("cigars on host");
  return AWV_OK;
}

// the batch's results to the caller's array and to the sink (SinkRunner)
int deliver(AlignCall& c) {
  const AlignRequest& rq = c.rq;
  if (rq.out) std::memcpy(rq.out + c.first, c.hres.data(), (size_t)c.n * sizeof(awv_result));
  if (!rq.sink && !rq.cs_sink) return AWV_OK;
  const bool want_cigar = c.want_cigar();
  // a cs call's sink also takes the batch's cs arena
  const awv_sink plain = rq.sink;
  const awv_cs_sink with_cs = rq.cs_sink;
  const auto sink = [plain, with_cs](void* u, int64_t f, int64_t m, const awv_result* r, const uint8_t* cig, const uint8_t* cs) {
    return with_cs ? with_cs(u, f, m, r, cig, cs) : plain(u, f, m, r, cig);
  };
  void* const user = rq.user;
  if (const int prc = c.runner.wait()) return fail(AWV_ERR_SINK, "sink callback returned " + std::to_string(prc));
  if (c.first + c.n >= rq.npairs || c.inline_sink) {  // the last (or only) batch: on the calling thread
    const int rc = sink(user, c.first, c.n, c.hres.data(), want_cigar ? c.e->h_cigar.data() : nullptr, want_cigar && with_cs ? c.e->h_cs.data() : nullptr);
    if (rc != 0) return fail(AWV_ERR_SINK, "sink callback returned " + std::to_string(rc));
    c.lap("sink returned");
    return AWV_OK;
  }
  // hand the batch's buffers to the helper thread and go on with the next batch
  c.runner.res.swap(c.hres);
  c.runner.cig.swap(c.e->h_cigar);
  c.runner.cs.swap(c.e->h_cs);
  const awv_result* rp = c.runner.res.data();
  const uint8_t* cp = want_cigar ? c.runner.cig.data() : nullptr;
  const uint8_t* xp = want_cigar && with_cs ? c.runner.cs.data() : nullptr;
  const int64_t f0 = c.first, n0 = c.n;
  SinkRunner* rn = &c.runner;
  try {
    c.runner.th = std::thread([rn, sink, user, f0, n0, rp, cp, xp]() { rn->rc = sink(user, f0, n0, rp, cp, xp); });
    c.lap("sink handed off");
  } catch (const std::exception&) {  // no thread to be had: this sink runs here, nothing may cross the C boundary
    const int rc = sink(user, f0, n0, rp, cp, xp);
    if (rc != 0) return fail(AWV_ERR_SINK, "sink callback returned " + std::to_string(rc));
  }
  return AWV_OK;
}

void publish_stats(AlignCall& c) {
  using namespace awv;
  awv_engine* e = c.e;
  const unsigned long long* stat_tot = c.stat_tot;
  e->stats.kernel_ms = c.kernel_ms;
  e->stats.h2d_ms = c.h2d_ms;
  e->stats.d2h_ms = c.d2h_ms;
  e->stats.launches = c.launches;
  e->stats.cell_steps = stat_tot[STAT_CELLS];
  e->stats.extend_steps = stat_tot[STAT_EXTEND];
  e->stats.n_breakpoints = stat_tot[STAT_BREAKPOINTS];
  e->stats.n_base = stat_tot[STAT_BASE];
  e->stats.overlap_scans = stat_tot[STAT_OVERLAP];
  e->stats.aligned_bp = stat_tot[STAT_ALIGNED_BP];
  e->stats.pairs_completed = stat_tot[STAT_PAIRS];
  e->stats.scratch_bytes = e->ring_mem.bytes() + e->hist_mem.bytes() + e->ev_mem.bytes() + e->reuse_mem.bytes();
  for (int i = 0; i < 14; ++i) e->stats.prof[i] = stat_tot[STAT_T_TOTAL + i];
  e->stats.restarts = stat_tot[STAT_RESTARTS];
  e->stats.multi_cell_steps = stat_tot[STAT_MULTI_CELLS];
  e->stats.windows[0] = stat_tot[STAT_WIN_SINGLE];
  e->stats.windows[1] = stat_tot[STAT_WIN_MULTI];
  e->stats.windows[2] = stat_tot[STAT_WIN_BASE];
  e->stats.windows[3] = stat_tot[STAT_WIN_BASE_MULTI];
  e->stats.clock_cycles = stat_tot[STAT_CLK_CYCLES];
  e->stats.clock_ticks = stat_tot[STAT_CLK_TICKS];
  e->stats.clock_tick_khz = (uint64_t)e->wall_clock_khz;
  e->stats.deep_cell_steps = stat_tot[STAT_DEEP_CELLS];
  for (int i = 0; i < 4; ++i) e->twin_stats[i] = stat_tot[STAT_TWIN_UNITS + i];
#if !defined(AWV_PROF) && !defined(AWV_DIAG)
  // row reuse: the product build stamps no cycles and counts no zones, so two of the slots that only the diagnostic builds fill carry
  // the cell-steps taken from a row archive (they are counted in cell_steps and multi_cell_steps too) and the searches that took some
  e->stats.prof[12] = stat_tot[STAT_REUSE_CELLS];
  e->stats.prof[13] = stat_tot[STAT_REUSE_SEARCHES];
  // ([12] / [13]: by the two searches right below a top-level search; [10] / [11]: by the searches further down)
  e->stats.prof[10] = stat_tot[STAT_REUSE_DEEP_CELLS];
  e->stats.prof[11] = stat_tot[STAT_REUSE_DEEP_SEARCHES];
#endif
}

int align_core(awv_engine* e, SeqSet& s, const awv_penalties* pen, const AlignRequest& rq) {
  // ---- the penalty plan (the list, the pair indices and the slot rule are checked, and the steps' counters reset, by align_call)
  AlignCall c{e, s, pen, rq};
  c.pp = awvb::plan_penalties(LIMITS, pen, e->cfg.flags);
  if (c.pp.code != AWV_OK && !c.pp.late) return fail(c.pp.code, c.pp.message);
  AWV_TRY(hipSetDevice(e->device));
  e->stats = awv_stats{};
  for (uint64_t& v : e->twin_stats) v = 0;
  c.norm = rq.score_only ? AWV_NORM_OFF : e->norm_mode;  // (off: no launch, no allocation, nothing below changes)
  if (rq.npairs == 0) return AWV_OK;
  if (c.pp.code != AWV_OK) return fail(c.pp.code, c.pp.message);
  c.cfg = awvb::Config{e->cfg.flags, e->num_cus, e->cfg.workgroups, (int64_t)e->cfg.max_scratch_bytes, e->cfg.first_row_cols};
  c.max_batch = e->cfg.max_batch_pairs > 0 ? e->cfg.max_batch_pairs : (int64_t)1 << 20;
  c.max_arena = e->cfg.max_arena_bytes > 0 ? (uint64_t)e->cfg.max_arena_bytes : (uint64_t)8 << 30;
  // twin units only where the plain alignment or the plain score is asked for: whole pairs, no bound, re-runs allowed
  c.twin_ok = rq.max_penalty == INT_MAX && !rq.pair_bound && !rq.spans && !rq.cout && !(e->cfg.flags & (AWV_F_NO_TWIN | AWV_F_NO_RERUN));
  read_knobs(c);
  // ---- batch by batch
  for (; c.first < rq.npairs; c.first += c.n) {
    const bool skewed = carve_and_order(c);
    if (int rc = reserve_batch_buffers(c)) return rc;
    if (int rc = run_groups(c, skewed)) return rc;
    c.lap("results on host");
    if (int rc = run_record_steps(c)) return rc;
    if (int rc = copy_cigars_back(c)) return rc;
    if (int rc = deliver(c)) return rc;
  }
  publish_stats(c);
  return AWV_OK;
}

// ---- what the entry points share (the table of forms and the order of the checks) ----
int require_sequences(const awv_engine* e, int64_t n, const char* who) {
  if (e->seqs.n == 0 && n > 0) return fail(AWV_ERR_STATE, std::string(who) + " before set_sequences");
  return AWV_OK;
}
// (a bound of 2^30 or more cannot be met by any pair the engine accepts: it is no bound)
int32_t norm_bound(int32_t b) { return b < 0 || b >= (1 << 30) ? INT_MAX : b; }
// a caller's nullable array of n bounds as align_core takes them: normalized, in `store`; no array (or no pairs) stays null
const int32_t* normalized_bounds(const int32_t* bounds, int64_t n, std::vector<int32_t>& store) {
  if (!bounds || n <= 0) return nullptr;
  store.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) store[(size_t)i] = norm_bound(bounds[i]);
  return store.data();
}
// Each range becomes the pair and the rectangle (pattern / text coordinates) align_core works on
int split_ranges(const SeqSet& s, const awv_range_pair* ranges, int64_t n, std::vector<awv_pair>& pairs, std::vector<awvr::Span>& spans,
                 const char* who) {
  pairs.resize((size_t)n);
  spans.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (!awvr::split_range(s.len.data(), s.n, ranges[i], pairs[(size_t)i], spans[(size_t)i]))
      return fail(AWV_ERR_ARG, std::string(who) + ": range " + std::to_string(i) + " names a sequence index or an interval out of range");
  return AWV_OK;
}
// what every clipping call refuses before anything is launched
int check_clip_args(const awv_clip_result* cout, int32_t match_bonus) {
  if (!cout) return fail(AWV_ERR_ARG, "align_clipped: null cout");
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS) return fail(AWV_ERR_ARG, "align_clipped: match_bonus must be in [1, 32767]");
  return AWV_OK;
}
// what every encoding call refuses; match_bonus == 0: no clip, cout is not read
int check_encode_args(const awv_cigar_text* tout, awv_clip_result*& cout, int32_t match_bonus) {
  if (!tout) return fail(AWV_ERR_ARG, "align_encoded: null tout");
  if (match_bonus == 0) {
    cout = nullptr;
    return AWV_OK;
  }
  return check_clip_args(cout, match_bonus);
}
// what every cs call refuses; match_bonus == 0: no clip, cout is not read
int check_cs_args(int32_t cs_mode, const awv_cs_text* csout, awv_clip_result*& cout, int32_t match_bonus) {
  if (!awvcs::mode_ok(cs_mode)) return fail(AWV_ERR_ARG, "align_cs: cs_mode must be AWV_CS_SHORT or AWV_CS_LONG");
  if (!csout) return fail(AWV_ERR_ARG, "align_cs: null csout");
  if (match_bonus == 0) {
    cout = nullptr;
    return AWV_OK;
  }
  return check_clip_args(cout, match_bonus);
}
// what every splitting call refuses, and the slot rule for one entry
int check_split_args(int32_t match_bonus, const SplitOut& sp, int64_t n) {
  if (match_bonus < 1 || match_bonus > AWV_CLIP_MAX_BONUS) return fail(AWV_ERR_ARG, "align_split: match_bonus must be in [1, 32767]");
  if (sp.min_score < 1) return fail(AWV_ERR_ARG, "align_split: min_score must be >= 1");
  if (!sp.seg_first || (n > 0 && !sp.iout)) return fail(AWV_ERR_ARG, "align_split: null seg_first or iout");
  for (int64_t i = 0; i < n; ++i)
    if (sp.seg_first[i + 1] < sp.seg_first[i]) return fail(AWV_ERR_ARG, "align_split: seg_first must ascend");
  if (n > 0 && sp.seg_first[n] > sp.seg_first[0] && !sp.sout) return fail(AWV_ERR_ARG, "align_split: null sout");
  return AWV_OK;
}
int check_split_slots(const SplitOut& sp, int64_t i, int32_t match_bonus, int64_t shorter) {
  if (sp.seg_first[i + 1] - sp.seg_first[i] < (uint64_t)awvs::slots(match_bonus, sp.min_score, shorter))
    return fail(AWV_ERR_ARG, "align_split: entry " + std::to_string(i) + " owns fewer slots than awv_split_slots(a, min_score, min(plen, tlen))");
  return AWV_OK;
}

// The request's outputs exactly as the caller gave them; the pairs and rectangles are align_call's to set
AlignRequest request(awv_result* out, awv_sink sink, void* user, const int32_t* bounds = nullptr, awv_verify_result* vout = nullptr,
                     int32_t match_bonus = 0, awv_clip_result* cout = nullptr, awv_cigar_text* tout = nullptr) {
  AlignRequest rq;
  rq.out = out;
  rq.sink = sink;
  rq.user = user;
  rq.pair_bound = bounds;
  rq.vout = vout;
  rq.match_bonus = match_bonus;
  rq.cout = cout;
  rq.tout = tout;
  return rq;
}
// the encoded call's request plus the cs step; the sink that takes both arenas stands in the plain sink's place
AlignRequest cs_request(AlignRequest rq, int32_t cs_mode, awv_cs_text* csout, awv_cs_sink sink) {
  rq.cs_mode = cs_mode;
  rq.csout = csout;
  rq.cs_sink = sink;
  return rq;
}
// the bounded call's request plus the split step; sp outlives the call
AlignRequest split_request(AlignRequest rq, const SplitOut& sp) {
  rq.split = &sp;
  return rq;
}
// The list a call works on -- pairs, or ranges -- and the name its messages carry
struct Subject {
  const awv_pair* pairs;
  const awv_range_pair* ranges;
  bool by_range;
  int64_t n;
  const char* who;
};
Subject over_pairs(const awv_pair* pairs, int64_t n, const char* who = "align_pairs") { return {pairs, nullptr, false, n, who}; }
Subject over_ranges(const awv_range_pair* ranges, int64_t n, const char* who = "align_ranges") { return {nullptr, ranges, true, n, who}; }
// What a form requires of its arguments beyond the list, and the name its own messages carry
enum : unsigned { NEED_VOUT = 1, NEED_BOUNDS = 2, NEED_CLIP = 4, NEED_SPLIT = 8, NEED_TEXT = 16, NEED_CS = 32 };
struct Form {
  const char* name;
  unsigned needs;
};

// The one path from an entry point to align_core.  Every check comes before anything is launched or reset, in this order: the
// engine, the form's own arguments, the list, the sequence set, the ranges, the pair indices, the slot rule.  An accepted call
// resets the counters of the steps it asks for and of no other.
int align_call(awv_engine* e, const awv_penalties* pen, const Subject& sub, AlignRequest rq, const Form& form) {
  if (!e) return fail(AWV_ERR_ARG, "null engine");
  const int64_t n = sub.n;
  if ((form.needs & NEED_VOUT) && !rq.vout) return fail(AWV_ERR_ARG, std::string(form.name) + ": null vout");
  if ((form.needs & NEED_BOUNDS) && n > 0 && !rq.pair_bound) return fail(AWV_ERR_ARG, std::string(form.name) + ": null max_penalty");
  if (form.needs & NEED_CLIP)
    if (int rc = check_clip_args(rq.cout, rq.match_bonus)) return rc;
  if (form.needs & NEED_TEXT)
    if (int rc = check_encode_args(rq.tout, rq.cout, rq.match_bonus)) return rc;
  if (form.needs & NEED_CS)
    if (int rc = check_cs_args(rq.cs_mode, rq.csout, rq.cout, rq.match_bonus)) return rc;
  if (form.needs & NEED_SPLIT)
    if (int rc = check_split_args(rq.match_bonus, *rq.split, n)) return rc;
  if (n < 0 || (n > 0 && !(sub.by_range ? (const void*)sub.ranges : (const void*)sub.pairs)))
    return fail(AWV_ERR_ARG, sub.by_range ? std::string(sub.who) + ": null ranges" : std::string("align_pairs: null pairs"));
  if (int rc = require_sequences(e, n, sub.who)) return rc;
  AWV_GUARDED(
    const SeqSet& s = e->seqs;
    std::vector<awv_pair> pairs;
    std::vector<awvr::Span> spans;
    std::vector<int32_t> pb;
    rq.pairs = sub.pairs;
    rq.npairs = n;
    if (sub.by_range) {
      if (int rc = split_ranges(s, sub.ranges, n, pairs, spans, sub.who)) return rc;
      rq.pairs = pairs.data();
      rq.spans = n > 0 ? spans.data() : nullptr;
    }
    for (int64_t i = 0; i < n; ++i) {
      const awv_pair& p = rq.pairs[i];
      if (p.q_idx < 0 || p.q_idx >= s.n || p.t_idx < 0 || p.t_idx >= s.n) return fail(AWV_ERR_ARG, "align_pairs: sequence index out of range");
      if (!rq.split) continue;  // the slot rule over the two lengths the pair aligns: the intervals', or the sequences'
      const int64_t shorter = rq.spans ? std::min(rq.spans[i].pe - rq.spans[i].pb, rq.spans[i].te - rq.spans[i].tb)
                                       : std::min(s.len[p.q_idx], s.len[p.t_idx]);
      if (int rc = check_split_slots(*rq.split, i, rq.match_bonus, shorter)) return rc;
    }
    // the call's batches add to them (a call without pairs launches nothing: its stats are empty)
    if (rq.vout) awvf::stats_reset(e->verify);
    if (rq.cout) awvc::stats_reset(e->clip);
    if (rq.split) awvs::stats_reset(e->split);
    if (rq.tout) awve::stats_reset(e->encode);
    if (rq.csout) awvcs::stats_reset(e->cs);
    if (!rq.score_only && e->norm_mode != AWV_NORM_OFF) awvn::stats_reset(e->normalize);
    rq.max_penalty = norm_bound(rq.max_penalty);
    rq.pair_bound = normalized_bounds(rq.pair_bound, n, pb);
    return align_core(e, e->seqs, pen, rq);
  )
}
// awv_score_pairs / awv_score_pairs_bounded / awv_score_ranges.  rq: the bounds as the caller gave them -- one for the call
// (max_penalty), or one per pair (pair_bound).
int score_core(awv_engine* e, const awv_penalties* pen, const Subject& sub, AlignRequest rq, awv_score_result* out, const Form& form) {
  if (!e) return awv_internal_null_engine();  // (without a GPU there is no engine to pass: say so, as awv_engine_create does)
  if (!out) return fail(AWV_ERR_ARG, std::string(sub.who) + ": null out");
  if (sub.n < 0) return fail(AWV_ERR_ARG, sub.by_range ? "score_ranges: null ranges" : "score_pairs: npairs < 0");
  AWV_GUARDED(
    std::vector<awv_result> res((size_t)sub.n);
    rq.out = res.data();
    rq.score_only = true;
    const int rc = align_call(e, pen, sub, rq, form);
    if (rc != AWV_OK) return rc;
    for (int64_t i = 0; i < sub.n; ++i) {
      out[i].status = res[(size_t)i].status;
      out[i].penalty = res[(size_t)i].penalty;
    }
    return AWV_OK;
  )
}

}  // namespace

extern "C" {

int awv_abi_version(void) { return AWV_ABI_VERSION; }

const char* awv_last_error(void) { return g_last_error.c_str(); }

int awv_engine_create(const awv_engine_config* cfg, awv_engine** out) {
  if (!out) return fail(AWV_ERR_ARG, "engine_create: null out");
  *out = nullptr;
  int ndev = 0;
  hipError_t err = hipGetDeviceCount(&ndev);
  if (err != hipSuccess || ndev <= 0)
    return fail(AWV_ERR_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(err) +
                                       "): liballwave_hip has no CPU fallback");
  awv_engine* e = new awv_engine();
  if (cfg) e->cfg = *cfg;
  e->device = e->cfg.device;
  if (e->device < 0 || e->device >= ndev) {
    delete e;
    return fail(AWV_ERR_ARG, "engine_create: device ordinal out of range");
  }
  auto bail = [&](hipError_t he, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(he);
    awv_engine_destroy(e);
    return fail(AWV_ERR_HIP, m);
  };
  hipError_t he;
  if ((he = hipSetDevice(e->device)) != hipSuccess) return bail(he, "hipSetDevice");
  hipDeviceProp_t prop;
  if ((he = hipGetDeviceProperties(&prop, e->device)) != hipSuccess) return bail(he, "hipGetDeviceProperties");
  e->num_cus = prop.multiProcessorCount;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device) == hipSuccess && khz > 0) e->wall_clock_khz = khz;
    else (void)hipGetLastError();
  }
  if ((he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail(he, "hipStreamCreate");
  if ((he = hipEventCreate(&e->ev0)) != hipSuccess) return bail(he, "hipEventCreate");
  if ((he = hipEventCreate(&e->ev1)) != hipSuccess) return bail(he, "hipEventCreate");
  *out = e;
  return AWV_OK;
}

void awv_engine_destroy(awv_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  awp::plan_state_release(e->plan);
  e->plan = nullptr;
  awvf::state_release(e->verify);
  e->verify = nullptr;
  awvc::state_release(e->clip);
  e->clip = nullptr;
  awvs::state_release(e->split);
  e->split = nullptr;
  awvn::state_release(e->normalize);
  e->normalize = nullptr;
  awve::state_release(e->encode);
  e->encode = nullptr;
  awvcs::state_release(e->cs);
  e->cs = nullptr;
  awvcov::state_release(e->cov);
  e->cov = nullptr;
  awvvar::state_release(e->var);
  e->var = nullptr;
  awvl::state_release(e->lift);
  e->lift = nullptr;
  awvmsa::state_release(e->msa);
  e->msa = nullptr;
  e->seqs.release();
  e->ring_mem.release();
  e->hist_mem.release();
  e->ev_mem.release();
  e->reuse_mem.release();
  e->d_pair_q.release();
  e->d_pair_t.release();
  e->d_pair_rc.release();
  e->d_pair_bound.release();
  e->d_pair_span.release();
  e->d_cigar_off.release();
  e->d_results.release();
  e->d_cigar.release();
  e->d_counters.release();
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int awv_engine_set_sequences(awv_engine* e, int32_t n, const uint8_t* concat_bytes, const uint64_t* offsets) {
  if (!e) return fail(AWV_ERR_ARG, "null engine");
  awp::plan_state_release(e->plan);  // (sketches of the previous set are stale)
  e->plan = nullptr;
  (void)hipSetDevice(e->device);
  awvcov::state_release(e->cov);  // (coverage is of the previous set: it ends)
  e->cov = nullptr;
  awvvar::state_release(e->var);  // (and so does the allele table)
  e->var = nullptr;
  awvl::state_release(e->lift);   // (and the lift table)
  e->lift = nullptr;
  AWV_GUARDED(return upload_seqset(e, e->seqs, n, concat_bytes, offsets);)
}

// ---- the aligning calls: each fills the request from its arguments, names what its form requires, and takes the one path.
// The _ranges forms are the same calls over sub-intervals of the resident sequences.
int awv_align_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, awv_result* out,
                    awv_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), request(out, sink, user), {"align_pairs", 0});
}

int awv_align_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, awv_result* out,
                     awv_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), request(out, sink, user), {"align_ranges", 0});
}

int awv_align_pairs_verified(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, awv_result* out,
                             awv_verify_result* vout, awv_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), request(out, sink, user, nullptr, vout), {"align_pairs_verified", NEED_VOUT});
}

int awv_align_ranges_verified(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, awv_result* out,
                              awv_verify_result* vout, awv_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), request(out, sink, user, nullptr, vout), {"align_ranges_verified", NEED_VOUT});
}

int awv_align_pairs_bounded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const int32_t* max_penalty,
                            awv_result* out, awv_verify_result* vout, awv_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), request(out, sink, user, max_penalty, vout), {"align_pairs_bounded", NEED_BOUNDS});
}

int awv_align_ranges_bounded(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty,
                             awv_result* out, awv_verify_result* vout, awv_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), request(out, sink, user, max_penalty, vout), {"align_ranges_bounded", 0});
}

int awv_align_pairs_clipped(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const int32_t* max_penalty,
                            int32_t match_bonus, awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), request(out, sink, user, max_penalty, vout, match_bonus, cout), {"align_pairs_clipped", NEED_CLIP});
}

int awv_align_ranges_clipped(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty,
                             int32_t match_bonus, awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), request(out, sink, user, max_penalty, vout, match_bonus, cout), {"align_ranges_clipped", NEED_CLIP});
}

int awv_align_pairs_encoded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const int32_t* max_penalty,
                            int32_t match_bonus, awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_cigar_text* tout,
                            awv_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), request(out, sink, user, max_penalty, vout, match_bonus, cout, tout), {"align_pairs_encoded", NEED_TEXT});
}

int awv_align_ranges_encoded(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty,
                             int32_t match_bonus, awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_cigar_text* tout,
                             awv_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), request(out, sink, user, max_penalty, vout, match_bonus, cout, tout), {"align_ranges_encoded", NEED_TEXT});
}

int awv_align_pairs_cs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const int32_t* max_penalty, int32_t match_bonus,
                       awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_cigar_text* tout, int32_t cs_mode, awv_cs_text* csout,
                       awv_cs_sink sink, void* user) {
  return align_call(e, pen, over_pairs(pairs, npairs), cs_request(request(out, nullptr, user, max_penalty, vout, match_bonus, cout, tout), cs_mode, csout, sink),
                    {"align_pairs_cs", NEED_CS});
}

int awv_align_ranges_cs(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty, int32_t match_bonus,
                        awv_result* out, awv_verify_result* vout, awv_clip_result* cout, awv_cigar_text* tout, int32_t cs_mode, awv_cs_text* csout,
                        awv_cs_sink sink, void* user) {
  return align_call(e, pen, over_ranges(ranges, n), cs_request(request(out, nullptr, user, max_penalty, vout, match_bonus, cout, tout), cs_mode, csout, sink),
                    {"align_ranges_cs", NEED_CS});
}

int awv_align_pairs_split(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, const int32_t* max_penalty,
                          int32_t match_bonus, int64_t min_score, awv_result* out, awv_verify_result* vout, const uint64_t* seg_first,
                          awv_split_index* iout, awv_clip_result* sout, awv_sink sink, void* user) {
  const SplitOut sp{min_score, seg_first, iout, sout};
  return align_call(e, pen, over_pairs(pairs, npairs), split_request(request(out, sink, user, max_penalty, vout, match_bonus), sp), {"align_pairs_split", NEED_SPLIT});
}

int awv_align_ranges_split(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty,
                           int32_t match_bonus, int64_t min_score, awv_result* out, awv_verify_result* vout, const uint64_t* seg_first,
                           awv_split_index* iout, awv_clip_result* sout, awv_sink sink, void* user) {
  const SplitOut sp{min_score, seg_first, iout, sout};
  return align_call(e, pen, over_ranges(ranges, n), split_request(request(out, sink, user, max_penalty, vout, match_bonus), sp), {"align_ranges_split", NEED_SPLIT});
}

int32_t awv_divergence_bound(const awv_penalties* pen, int32_t plen, int32_t tlen, double d) {
  if (check_penalty_signs(pen) != AWV_OK) return INT32_MIN;
  if (!(d >= 0.0) || plen < 0 || tlen < 0) {  // (NaN fails the comparison too)
    (void)fail(AWV_ERR_ARG, "divergence_bound: need d >= 0 and lengths >= 0");
    return INT32_MIN;
  }
  if (d >= 1.0) return -1;
  // E <= d (plen + tlen) / (2 - d) edit columns (columns = plen + #I = tlen + #D), each at most cmax; one more absorbs the
  // rounding of the quotient -- the bound only has to err upwards, an exact filter on the counts follows it
  long long gap1 = (long long)pen->gap_open1 + pen->gap_ext1;
  if (pen->two_piece) gap1 = std::min(gap1, (long long)pen->gap_open2 + pen->gap_ext2);
  const long long cmax = std::max<long long>(pen->mismatch, gap1);
  const double edits = std::floor(d * ((double)plen + (double)tlen) / (2.0 - d));
  const double B = (double)cmax * (edits + 1.0);
  return B > (double)INT32_MAX ? -1 : (int32_t)B;
}

// ---- the score calls: score_core converts the results and takes the same path
int awv_score_pairs(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs, int32_t max_penalty,
                    awv_score_result* out) {
  AlignRequest rq;
  rq.max_penalty = max_penalty;
  return score_core(e, pen, over_pairs(pairs, npairs, "score_pairs"), rq, out, {"score_pairs", 0});
}

int awv_score_pairs_bounded(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t npairs,
                            const int32_t* max_penalty, awv_score_result* out) {
  return score_core(e, pen, over_pairs(pairs, npairs, "score_pairs"), request(nullptr, nullptr, nullptr, max_penalty), out, {"score_pairs_bounded", NEED_BOUNDS});
}

int awv_score_ranges(awv_engine* e, const awv_penalties* pen, const awv_range_pair* ranges, int64_t n, const int32_t* max_penalty,
                     awv_score_result* out) {
  return score_core(e, pen, over_ranges(ranges, n, "score_ranges"), request(nullptr, nullptr, nullptr, max_penalty), out, {"score_ranges", 0});
}

namespace {
int align_one_core(awv_engine* e, const awv_penalties* pen, const uint8_t* pattern, int32_t plen, const uint8_t* text,
                   int32_t tlen, awv_result* result, uint8_t* cigar_buf, size_t cigar_cap);
struct OneSink {
  uint8_t* buf;
  size_t cap;
  int rc;
};
int one_sink(void* user, int64_t, int64_t n, const awv_result* r, const uint8_t* arena) {
  OneSink* o = (OneSink*)user;
  if (n != 1 || !arena) return 1;
  if (r[0].status == AWV_ST_COMPLETED) {
    if (r[0].cigar_len > o->cap) { o->rc = AWV_ERR_ARG; return 2; }
    std::memcpy(o->buf, arena + r[0].cigar_off, r[0].cigar_len);
  }
  return 0;
}
}  // namespace

int awv_align_one(awv_engine* e, const awv_penalties* pen, const uint8_t* pattern, int32_t plen, const uint8_t* text,
                  int32_t tlen, awv_result* result, uint8_t* cigar_buf, size_t cigar_cap) {
  if (!e || !result || plen < 0 || tlen < 0 || (plen > 0 && !pattern) || (tlen > 0 && !text))
    return fail(AWV_ERR_ARG, "align_one: bad argument");
  if (cigar_cap < (size_t)plen + (size_t)tlen) return fail(AWV_ERR_ARG, "align_one: cigar buffer needs plen + tlen bytes");
  AWV_GUARDED(return align_one_core(e, pen, pattern, plen, text, tlen, result, cigar_buf, cigar_cap);)
}
}  // extern "C"

namespace {
int align_one_core(awv_engine* e, const awv_penalties* pen, const uint8_t* pattern, int32_t plen, const uint8_t* text,
                   int32_t tlen, awv_result* result, uint8_t* cigar_buf, size_t cigar_cap) {
  struct Scope {  // the temporary sequence set and the engine's flags go back whichever way this function is left
    awv_engine* e;
    int32_t saved_flags;
    SeqSet tmp;
    ~Scope() {
      e->cfg.flags = saved_flags;
      tmp.release();
    }
  } sc{e, e->cfg.flags, {}};
  std::vector<uint8_t> cat((size_t)plen + (size_t)tlen + 1);
  if (plen) std::memcpy(cat.data(), pattern, (size_t)plen);
  if (tlen) std::memcpy(cat.data() + plen, text, (size_t)tlen);
  const uint64_t offs[3] = {0, (uint64_t)plen, (uint64_t)plen + (uint64_t)tlen};
  int rc = upload_seqset(e, sc.tmp, 2, cat.data(), offs);
  if (rc == AWV_OK) {
    const awv_pair p{0, 1, 0};
    OneSink os{cigar_buf, cigar_cap, AWV_OK};
    e->cfg.flags &= ~AWV_F_KEEP_ON_DEVICE;
    AlignRequest rq = request(result, one_sink, &os);
    rq.pairs = &p;
    rq.npairs = 1;
    if (e->norm_mode != AWV_NORM_OFF) awvn::stats_reset(e->normalize);  // (the one call that does not come through align_call)
    rc = align_core(e, sc.tmp, pen, rq);
    if (rc == AWV_ERR_SINK && os.rc != AWV_OK) rc = fail(os.rc, "align_one: cigar buffer too small");
  }
  return rc;
}
}  // namespace

extern "C" {

int awv_twin_stats(const awv_engine* e, uint64_t out[4]) {
  if (!e || !out) return fail(AWV_ERR_ARG, "twin_stats: null argument");
  for (int i = 0; i < 4; ++i) out[i] = e->twin_stats[i];
  return AWV_OK;
}

int awv_engine_stats(const awv_engine* e, awv_stats* out) {
  if (!e || !out) return fail(AWV_ERR_ARG, "stats: null argument");
  *out = e->stats;
  return AWV_OK;
}

}  // extern "C"

// ---- what planner.hip reads of an engine (planner_device.hpp) ----
void awv_internal_device_view(awv_engine* e, awp::EngineView* v) {
  v->device = e->device;
  v->stream = e->stream;
  v->n = e->seqs.n;
  v->fwd = e->seqs.d_seq[0].p;
  v->rc = e->seqs.d_seq[2].p;
  v->off = e->seqs.d_off.p;
  v->len = e->seqs.d_len.p;
  v->len_host = e->seqs.len.data();
  v->workgroups = e->cfg.workgroups;
}
int awv_internal_view(awv_engine* e, awp::EngineView* v) {
  if (!e || !v) return fail(AWV_ERR_ARG, "null engine");
  awv_internal_device_view(e, v);
  if (e->seqs.n == 0) return fail(AWV_ERR_STATE, "no sequence set: call awv_engine_set_sequences first");
  return AWV_OK;
}
awp::PlanState*& awv_internal_plan(awv_engine* e) { return e->plan; }
// ---- what verify.hip keeps in an engine, and the arena budget awv_verify_cigars splits its call by (verify_device.hpp) ----
awvf::State*& awv_internal_verify(awv_engine* e) { return e->verify; }
awvc::State*& awv_internal_clip(awv_engine* e) { return e->clip; }
awvs::State*& awv_internal_split(awv_engine* e) { return e->split; }
awvn::State*& awv_internal_normalize(awv_engine* e) { return e->normalize; }
awve::State*& awv_internal_encode(awv_engine* e) { return e->encode; }
awvcs::State*& awv_internal_cs(awv_engine* e) { return e->cs; }
awvcov::State*& awv_internal_coverage(awv_engine* e) { return e->cov; }
awvvar::State*& awv_internal_variants(awv_engine* e) { return e->var; }
awvl::State*& awv_internal_lift(awv_engine* e) { return e->lift; }
awvmsa::State*& awv_internal_msa(awv_engine* e) { return e->msa; }
bool& awv_internal_coverage_paused(awv_engine* e) { return e->cov_paused; }
int32_t& awv_internal_normalize_mode(awv_engine* e) { return e->norm_mode; }
uint64_t awv_internal_max_arena(const awv_engine* e) { return e->cfg.max_arena_bytes > 0 ? (uint64_t)e->cfg.max_arena_bytes : (uint64_t)8 << 30; }
int awv_internal_fail(int code, const std::string& msg) { return fail(code, msg); }
int awv_internal_check_penalties(const awv_penalties* pen) { return check_penalty_signs(pen); }
// ---- what orient.hip needs beyond that (orient_device.hpp): the stats of a call made of several engine calls
void awv_internal_set_stats(awv_engine* e, const awv_stats* st) { e->stats = *st; }
