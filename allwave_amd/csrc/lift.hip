// lift.hip -- intervals lifted through alignments on the device: awv_lift_cigars / awv_lift_ranges, awv_engine_lift_begin / _read /
// _stats and awv_lift_one_host (include/allwave_hip.h).  What the lift of one interval is stands in lift_device.hpp; this file gets
// the kernel to the same results.
//
// A record pass (record_pass.hpp) with the op-mask walk of wave_ops.hpp (lane_op_masks): persistent one-wave workgroups take
// records -- not queries --, longest op string first, from a cursor; a string goes by in chunks of 64 lanes x 16 op bytes, one
// aligned 16-byte load per lane.  Only records that have a query are dispatched, and a record is walked once however many queries
// it has.
// The host turns a record's queries into probes.  A probe is a source offset r (counted from the item's first source base) and
// asks for the first aligned ('M' / 'X') column whose source offset is r or more: a query's begin wants that column, its end the
// aligned column before it.  Both are the same search, and its answer is monotone in r, so a record's probes are sorted by r, per
// side (offsets count text bases on the target side and pattern bases on the query side), and the walk keeps one cursor per side
// into them.  Per chunk one packed add-scan (four 16-bit fields in 64 bits: a chunk holds 1,024 columns) gives every lane the
// 'M', 'X', 'I' and 'D' bytes before it; with the uniform carries of the chunks before, that is the source offset, both skips and
// the four counts at any column.  Every lane leaves its masks, its prefix, the running maximum of the lanes' last aligned source
// offsets and the nearest lower lane that has an aligned column in LDS.  Then up to 64 pending probes are resolved per step, one
// per lane: a binary search of the running maxima finds the lane whose 16 bytes hold the column, a walk of that lane's masks the
// column.  A probe beyond the chunk's last aligned column stays pending; the probes behind it are beyond it too.  The aligned
// column before a chunk's first one is the last aligned column of the chunks before: one uniform carry.  What is pending when the
// string ends has no column at or after it.  All of that starts afresh at every record.
// The answers (a column and the four counts before it) go to global memory at the probes' indices; behind the string the lanes
// take the record's queries, and lift_device.hpp's compose() makes each result from its two answers and what the whole string
// decided (a bad byte anywhere, the consumed lengths).  Results are plain stores at host-assigned indices; the only atomics are the
// cursor and the two stats counters.
#include "lift_device.hpp"

#include <algorithm>
#include <climits>
#include <new>
#include <string>
#include <vector>

#include "batch_items.hpp"  // contributing_items
#include "record_pass.hpp"  // RecordPass, open_pass, open_active, each_piece, resolve_call, Buf, AWV_TRY

namespace awvl {

constexpr unsigned KIND_END = 0x80000000u;  // of a probe word: the answer is the aligned column before; the low 31 bits are r

struct RecDesc {
  int32_t q0, q1;        // the record's queries
  int32_t p0[2], p1[2];  // its probes, per side (0: from the target, 1: from the query), ascending by r
};
struct DevQuery {
  int32_t from;
  int32_t a, b;    // the interval in the item's coordinates (to_item)
  int32_t pb, pe;  // the probes of its begin and of its end
};

struct KParams {
  const int32_t* len;  // the resident sequences' lengths
  const awv_pair* pairs;
  const Span* spans;          // record i's rectangle, behind its slice's skips (validated on the host)
  const awv_cs_slice* bases;  // its slice of the caller's string (zero: the whole string): only added to what is reported
  const awv_result* results;  // cigar_off relative to `arena`; a slice is a record of its own here
  const int32_t* order;       // dispatch slot -> record
  const uint8_t* arena;       // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  const RecDesc* recs;
  const DevQuery* queries;
  const uint32_t* probes;
  Prefix* answers;  // one per probe
  awv_lift_result* out;  // one per query
  unsigned long long* counters;  // [0] the cursor, [1] records walked, [2] columns
  long long npairs;
};

using awvw::CHUNK;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::wave_scan_add;
using awvw::wave_scan_max;

// the columns of a lane below bit j
__device__ __forceinline__ unsigned below(int j) { return (1u << j) - 1u; }

// What a lane left in LDS for the probes: its masks and the op bytes of each kind before it, the carry of the chunks before added.
struct LaneView {
  unsigned m, x, i, d;
  unsigned cm, cx, ci, cd;
};
// lane l's words, the carries tm, tx, ti, td of the chunks before added
__device__ __forceinline__ LaneView lane_view(const unsigned* s_mx, const unsigned* s_id, const unsigned long long* s_pre, int l, unsigned tm, unsigned tx, unsigned ti,
                                              unsigned td) {
  const unsigned mx = s_mx[l], id = s_id[l];
  const unsigned long long pre = s_pre[l];
  return LaneView{mx & 0xffffu, mx >> 16, id & 0xffffu, id >> 16, tm + (unsigned)(pre & 0xffffu), tx + (unsigned)((pre >> 16) & 0xffffu),
                  ti + (unsigned)((pre >> 32) & 0xffffu), td + (unsigned)(pre >> 48)};
}
// the answer "before column j of that lane" (col: of the string)
__device__ __forceinline__ Prefix before_bit(const LaneView& v, long long col0, int j) {
  const unsigned bl = below(j);
  return Prefix{(uint32_t)(col0 + j), v.cm + (unsigned)__popc(v.m & bl), v.cx + (unsigned)__popc(v.x & bl), v.ci + (unsigned)__popc(v.i & bl),
                v.cd + (unsigned)__popc(v.d & bl)};
}
// the answer "behind the aligned column j of that lane"
__device__ __forceinline__ Prefix behind_bit(const LaneView& v, long long col0, int j) {
  Prefix p = before_bit(v, col0, j);
  p.col += 1u;
  p.m += (v.m >> j) & 1u;
  p.x += (v.x >> j) & 1u;
  return p;
}

__global__ __launch_bounds__(64) void awv_lift_kernel(KParams kp) {
  __shared__ int s_pm[2][64];             // per side: the largest source offset of an aligned column in the lanes up to this one (-1: none)
  __shared__ unsigned s_mx[64], s_id[64];  // the lanes' masks: m | x << 16, i | d << 16
  __shared__ unsigned long long s_pre[64]; // the chunk's op bytes before the lane: four 16-bit fields, m x i d
  __shared__ int s_prev[64];               // the nearest lower lane with an aligned column (-1: none in this chunk)
  const int lane = threadIdx.x;
  unsigned long long t_records = 0, t_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int item = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[item];
    const RecDesc rd = kp.recs[item];
    const awv_pair pr = kp.pairs[item];
    const Span sp = kp.spans[item];
    int code = AWV_LF_SKIPPED;
    unsigned tm = 0u, tx = 0u, ti = 0u, td = 0u;  // the 'M', 'X', 'I', 'D' bytes of the chunks before (uniform); behind the string: of the string

    if (rec.status == AWV_ST_COMPLETED) {
      const long long n = (long long)rec.cigar_len;
      const int sh = (int)(rec.cigar_off & 15);
      const uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]
      const long long span = n > 0 ? sh + n : 0;
      int pp[2] = {rd.p0[0], rd.p0[1]};          // the first pending probe of each side (uniform)
      Prefix last_a{0u, 0u, 0u, 0u, 0u};          // behind the last aligned column so far (col 0: there is none) (uniform)
      unsigned bad = 0;                           // (lane-local)
      for (long long base = 0; base < span; base += CHUNK) {
        const awvw::OpMasks o = awvw::lane_op_masks(ops, sh, span, base, lane);
        bad |= o.valid & ~(o.m | o.x | o.i | o.d);
        const unsigned al = o.m | o.x;
        const long long cnt = (long long)((unsigned long long)__popc(o.m) | ((unsigned long long)__popc(o.x) << 16) | ((unsigned long long)__popc(o.i) << 32) |
                                          ((unsigned long long)__popc(o.d) << 48));
        const long long inc = wave_scan_add(cnt);
        const unsigned long long exc = (unsigned long long)(inc - cnt);
        const int inc_lane = wave_scan_max(al != 0u ? lane : -1);
        s_mx[lane] = o.m | (o.x << 16);
        s_id[lane] = o.i | (o.d << 16);
        s_pre[lane] = exc;
        s_prev[lane] = from_lower_lane(inc_lane, -1);
        const unsigned em = tm + (unsigned)(exc & 0xffffu), ex = tx + (unsigned)((exc >> 16) & 0xffffu), ei = ti + (unsigned)((exc >> 32) & 0xffffu),
                       ed = td + (unsigned)(exc >> 48);
        const int top = al != 0u ? 31 - __clz((int)al) : 0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          // the source offset of the lane's last aligned column
          const unsigned consumes = al | (side == 0 ? o.i : o.d);
          const int before = (int)(em + ex + (side == 0 ? ei : ed));
          const int last = al != 0u ? before + __popc(consumes & below(top)) : -1;
          s_pm[side][lane] = wave_scan_max(last);
        }
        __syncthreads();

#pragma unroll
        for (int side = 0; side < 2; ++side) {
          while (pp[side] < rd.p1[side]) {  // (uniform) up to 64 pending probes per step, one per lane
            const int idx = pp[side] + lane;
            const bool mine = idx < rd.p1[side];
            const unsigned word = mine ? kp.probes[idx] : 0u;
            const int r = mine ? (int)(word & ~KIND_END) : INT_MAX;
            const bool found = mine && s_pm[side][63] >= r;
            if (found) {
              int L = 0;  // the first lane whose running maximum reaches r
#pragma unroll
              for (int step = 32; step >= 1; step >>= 1)
                if (s_pm[side][L + step - 1] < r) L += step;
              const LaneView v = lane_view(s_mx, s_id, s_pre, L, tm, tx, ti, td);
              const unsigned va = v.m | v.x, consumes = va | (side == 0 ? v.i : v.d);
              const int before = (int)(v.cm + v.cx + (side == 0 ? v.ci : v.cd));
              int j = 31 - __clz((int)(va | 1u));  // (the lane's last aligned column reaches r: the walk ends there at the latest)
              for (unsigned bits = va; bits != 0u; bits &= bits - 1u) {
                const int t = __builtin_ctz(bits);
                if (before + __popc(consumes & below(t)) >= r) {
                  j = t;
                  break;
                }
              }
              const long long col0 = base + (long long)L * LANE_BYTES - sh;
              Prefix ans;
              if (!(word & KIND_END)) {
                ans = before_bit(v, col0, j);
              } else {  // the aligned column before: in this lane, in the nearest lower lane that has one, or in a chunk before
                const unsigned lower = va & below(j);
                const int L2 = s_prev[L];
                if (lower != 0u) {
                  ans = behind_bit(v, col0, 31 - __clz((int)lower));
                } else if (L2 >= 0) {
                  const LaneView v2 = lane_view(s_mx, s_id, s_pre, L2, tm, tx, ti, td);
                  ans = behind_bit(v2, base + (long long)L2 * LANE_BYTES - sh, 31 - __clz((int)((v2.m | v2.x) | 1u)));
                } else {
                  ans = last_a;
                }
              }
              kp.answers[idx] = ans;
            }
            const int nres = __popcll(__ballot(found));
            pp[side] += nres;
            if (nres < 64) break;
          }
        }

        // the carries: the last aligned column so far (every lane reads the same words), then the counts
        const int last_lane = __builtin_amdgcn_readlane(inc_lane, 63);
        if (last_lane >= 0) {
          const LaneView v = lane_view(s_mx, s_id, s_pre, last_lane, tm, tx, ti, td);
          const Prefix p = behind_bit(v, base + (long long)last_lane * LANE_BYTES - sh, 31 - __clz((int)((v.m | v.x) | 1u)));
          last_a.col = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.col);
          last_a.m = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.m);
          last_a.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.x);
          last_a.i = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.i);
          last_a.d = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.d);
        }
        const unsigned tlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)inc, 63);
        const unsigned thi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)inc >> 32), 63);
        tm += tlo & 0xffffu;
        tx += tlo >> 16;
        ti += thi & 0xffffu;
        td += thi >> 16;
        __syncthreads();  // (the next chunk writes the LDS words again)
      }
      // what is pending behind the string: no aligned column at or after r
      const Prefix none{(uint32_t)n, tm, tx, ti, td};
#pragma unroll
      for (int side = 0; side < 2; ++side)
        for (int idx = pp[side] + lane; idx < rd.p1[side]; idx += 64) kp.answers[idx] = (kp.probes[idx] & KIND_END) ? last_a : none;
      const bool any_bad = __ballot(bad != 0u) != 0ull;
      code = whole_code(any_bad, (long long)tm + tx + td, (long long)tm + tx + ti, (long long)sp.pe - sp.pb, (long long)sp.te - sp.tb);
      ++t_records;
      t_columns += (unsigned long long)n;
    }
    __syncthreads();  // the answers are in memory

    // lanes over the record's queries
    const awv_cs_slice bs = kp.bases[item];
    const long long qlen = kp.len[pr.q_idx];
    for (int qi = rd.q0 + lane; qi < rd.q1; qi += 64) {
      const DevQuery q = kp.queries[qi];
      awv_lift_result res = make_code(code);
      if (code == AWV_LF_OK) {
        const Prefix pb = kp.answers[q.pb], pe = kp.answers[q.pe];
        const long long consumed = (long long)tm + tx + (q.from == AWV_LIFT_FROM_TARGET ? ti : td);
        res = compose(code, q.from, pr.q_revcomp != 0, qlen, sp, bs, consumed, q.a, q.b, pb, pe);
      }
      kp.out[qi] = res;
    }
  }
  if (lane == 0) {
    if (t_records) atomicAdd(&kp.counters[1], t_records);
    if (t_columns) atomicAdd(&kp.counters[2], t_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

constexpr int COUNTERS = 3;

// a query as the launches take it: on record `rec` of the launch's records; the launch's queries are sorted by rec
struct HostQuery {
  int64_t rec;
  int32_t from, beg, end;
  int64_t tag;  // the caller's: where the answer goes
};

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_cs_slice> d_bases;
  Buf<RecDesc> d_recs;
  Buf<DevQuery> d_queries;
  Buf<uint32_t> d_probes;
  Buf<Prefix> d_answers;
  Buf<awv_lift_result> d_out;
  awvw::BatchItems items;  // a batch's items (batch_items.hpp)
  std::vector<HostQuery> h_queries;
  std::vector<awv_lift_result> h_out;
  // the table of an engine that lifts its own alignments
  int32_t from_mask = 0;  // 0: no table
  int64_t clip_min_score = 0;
  int32_t nseq = 0;
  std::vector<awv_region> regions;
  std::vector<int32_t> by_seq;     // the regions' indices, by sequence, then begin
  std::vector<int64_t> seq_first;  // sequence s owns by_seq[seq_first[s], seq_first[s + 1])
  std::vector<int32_t> seq_reach;  // the longest region of each sequence
  std::vector<awv_lift_row> rows;
  awv_lift_stats stats{};
  void end() {  // the table ends: the stats stay readable until the next begin
    from_mask = 0;
    regions = {};
    by_seq = {};
    seq_first = {};
    seq_reach = {};
    rows = {};
  }
  void release() {
    RecordPass::release();
    end();
    d_pairs.release();
    d_spans.release();
    d_bases.release();
    d_recs.release();
    d_queries.release();
    d_probes.release();
    d_answers.release();
    d_out.release();
  }
};

void state_release(State* s) { awvw::release_pass(s); }
bool active(const State* s) { return s && s->from_mask != 0; }

namespace {

constexpr const char* TOO_LONG = "lift: an op string of more than 2^30 columns";  // what the kernel's 32-bit columns and counts hold

int open_state(awv_engine* e, awp::EngineView& v, State*& st) { return awvw::open_pass(awv_internal_lift(e), e, v, st, true); }
// the state of an engine that keeps a table
int open_active(awv_engine* e, const char* who, awp::EngineView& v, State*& st) { return awvw::open_active(awv_internal_lift(e), who, "lift", e, v, st); }

// One launch over the records, of n, that hq[0 .. nq) (sorted by rec) name; their op bytes are on the device already, and a
// record's slice has been applied to it and to its rectangle (bases, nullable: what the slices were).  Every index, rectangle and
// interval is checked here, on the host: the kernel reads what the records and the probes say.  out[k] answers hq[k].
int launch(const awp::EngineView& v, State* st, const awv_pair* pairs, const Span* spans, const awv_cs_slice* bases, int64_t n, const awv_result* recs,
           const uint8_t* d_arena, uint64_t arena_bytes, const HostQuery* hq, int64_t nq, awv_lift_result* out) {
  if (nq == 0) return AWV_OK;
  if (nq > MAX_QUERIES) return awv_internal_fail(AWV_ERR_ARG, "lift: 2^30 queries or more in one launch");
  // the records that are walked: the ones with a query
  std::vector<awv_pair> cpairs;
  std::vector<Span> cspans;
  std::vector<awv_cs_slice> cbases;
  std::vector<awv_result> crecs;
  std::vector<RecDesc> descs;
  std::vector<DevQuery> dq((size_t)nq);
  std::vector<uint32_t> probes((size_t)nq * 2);
  struct Key {
    uint32_t r;
    int32_t q;  // query, and whether the probe is its end
    bool end;
  };
  std::vector<Key> keys[2];
  for (int64_t k = 0; k < nq;) {
    const int64_t i = hq[k].rec;
    if (i < 0 || i >= n || (k > 0 && i < hq[k - 1].rec)) return awv_internal_fail(AWV_ERR_ARG, "lift: a query's record is out of range");
    if (int rc = awvw::check_rectangles(v, "lift", pairs + i, spans + i, 1)) return rc;
    const Span& sp = spans[i];
    const int64_t qlen = v.len_host[pairs[i].q_idx], tlen = v.len_host[pairs[i].t_idx];
    int64_t k1 = k;
    keys[0].clear();
    keys[1].clear();
    for (; k1 < nq && hq[k1].rec == i; ++k1) {
      const HostQuery& h = hq[k1];
      if (!from_ok(h.from)) return awv_internal_fail(AWV_ERR_ARG, "lift: a query's side is neither AWV_LIFT_FROM_TARGET nor AWV_LIFT_FROM_QUERY");
      if (h.beg < 0 || h.beg >= h.end || h.end > (h.from == AWV_LIFT_FROM_TARGET ? tlen : qlen))
        return awv_internal_fail(AWV_ERR_ARG, "lift: a query's interval is empty or outside its source sequence");
      int64_t a, b;
      to_item(h.from, pairs[i].q_revcomp != 0, qlen, h.beg, h.end, a, b);
      const int side = h.from == AWV_LIFT_FROM_TARGET ? 0 : 1;
      const int64_t s0 = side == 0 ? sp.tb : sp.pb;
      dq[(size_t)k1] = DevQuery{h.from, (int32_t)a, (int32_t)b, 0, 0};
      keys[side].push_back(Key{(uint32_t)std::max<int64_t>(a - s0, 0), (int32_t)k1, false});
      keys[side].push_back(Key{(uint32_t)std::max<int64_t>(b - s0, 0), (int32_t)k1, true});
    }
    RecDesc d{};
    d.q0 = (int32_t)k;
    d.q1 = (int32_t)k1;
    int32_t p = (int32_t)(2 * k);
    for (int side = 0; side < 2; ++side) {
      std::sort(keys[side].begin(), keys[side].end(), [](const Key& u, const Key& w) { return u.r < w.r; });
      d.p0[side] = p;
      for (const Key& key : keys[side]) {
        probes[(size_t)p] = key.r | (key.end ? KIND_END : 0u);
        (key.end ? dq[(size_t)key.q].pe : dq[(size_t)key.q].pb) = p;
        ++p;
      }
      d.p1[side] = p;
    }
    descs.push_back(d);
    cpairs.push_back(pairs[i]);
    cspans.push_back(sp);
    cbases.push_back(bases ? bases[i] : awv_cs_slice{0u, 0u, 0, 0});
    crecs.push_back(recs[i]);
    k = k1;
  }
  const int64_t m = (int64_t)crecs.size();
  if (int rc = awvw::check_lengths(crecs.data(), m, MAX_COLUMNS, TOO_LONG)) return rc;
  if (int rc = st->begin(v, "lift", m, crecs.data(), arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)m));
  AWV_TRY(st->d_spans.reserve((size_t)m));
  AWV_TRY(st->d_bases.reserve((size_t)m));
  AWV_TRY(st->d_recs.reserve((size_t)m));
  AWV_TRY(st->d_queries.reserve((size_t)nq));
  AWV_TRY(st->d_probes.reserve((size_t)nq * 2));
  AWV_TRY(st->d_answers.reserve((size_t)nq * 2));
  AWV_TRY(st->d_out.reserve((size_t)nq));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, cpairs.data(), (size_t)m * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_spans.p, cspans.data(), (size_t)m * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_bases.p, cbases.data(), (size_t)m * sizeof(awv_cs_slice), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_recs.p, descs.data(), (size_t)m * sizeof(RecDesc), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_queries.p, dq.data(), (size_t)nq * sizeof(DevQuery), hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(st->d_probes.p, probes.data(), (size_t)nq * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  if (int rc = st->clear_counters(v, COUNTERS)) return rc;
  KParams kp{};
  kp.len = v.len;
  kp.pairs = st->d_pairs.p;
  kp.spans = st->d_spans.p;
  kp.bases = st->d_bases.p;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.recs = st->d_recs.p;
  kp.queries = st->d_queries.p;
  kp.probes = st->d_probes.p;
  kp.answers = st->d_answers.p;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = m;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_lift_kernel, dim3(st->grid(v, m)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  AWV_TRY(hipMemcpyAsync(out, st->d_out.p, (size_t)nq * sizeof(awv_lift_result), hipMemcpyDeviceToHost, v.stream));
  unsigned long long hc[COUNTERS] = {0, 0, 0};
  float ms = 0;
  if (int rc = st->finish(v, hc, COUNTERS, ms)) return rc;
  awv_lift_stats& s = st->stats;
  s.kernel_ms += ms;
  s.records += hc[1];
  s.columns += hc[2];
  s.queries += (uint64_t)nq;
  for (int64_t k = 0; k < nq; ++k) {
    uint64_t* const by_code[6] = {&s.ok, &s.skipped, &s.bad_op, &s.lengths, &s.unaligned, &s.outside};
    if (out[k].code >= 0 && out[k].code < 6) ++*by_code[out[k].code];
  }
  return AWV_OK;
}

// ranges (nullable; awv_lift_ranges): the call is on ranges[0..n_all) -- `pairs` is not read
int lift_cigars_core(awv_engine* e, const awv_pair* pairs, const awv_range_pair* ranges, int64_t n_all, const awv_result* results, const uint8_t* cigar_arena,
                     uint64_t arena_bytes, const awv_cs_slice* slices, uint64_t max_arena, const awv_lift_query* queries, int64_t nq, awv_lift_result* lout) {
  const char* const who = ranges ? "lift_ranges" : "lift_cigars";
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  // before anything goes up: the call's own checks (item_call.hpp), then every query on a record of the call and inside its
  // source sequence
  awvw::ItemCall call;
  if (int rc = awvw::resolve_call(call, v, who, pairs, ranges, n_all, results, arena_bytes, slices)) return rc;
  pairs = call.pairs;
  if (nq > MAX_QUERIES) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": 2^30 queries or more");
  for (int64_t j = 0; j < nq; ++j) {
    const awv_lift_query& q = queries[j];
    if (q.record < 0 || q.record >= n_all) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": query " + std::to_string(j) + " names a record outside the call");
    if (!from_ok(q.from)) return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": query " + std::to_string(j) + ": `from` is neither AWV_LIFT_FROM_TARGET nor AWV_LIFT_FROM_QUERY");
    const int64_t len = v.len_host[q.from == AWV_LIFT_FROM_TARGET ? pairs[q.record].t_idx : pairs[q.record].q_idx];
    if (q.beg < 0 || q.beg >= q.end || q.end > len)
      return awv_internal_fail(AWV_ERR_ARG, std::string(who) + ": query " + std::to_string(j) + ": the interval is empty or outside its source sequence");
  }
  // the queries by record; the records that have one, with their slices applied (a slice is an op string of its own)
  std::vector<int64_t> by_rec((size_t)nq);
  for (int64_t j = 0; j < nq; ++j) by_rec[(size_t)j] = j;
  std::stable_sort(by_rec.begin(), by_rec.end(), [&](int64_t a, int64_t b) { return queries[a].record < queries[b].record; });
  std::vector<awv_pair> cpairs;
  std::vector<Span> cspans;
  std::vector<awv_cs_slice> cbases;
  std::vector<awv_result> crecs;
  std::vector<HostQuery> hq((size_t)nq);
  for (int64_t k = 0; k < nq; ++k) {
    const awv_lift_query& q = queries[by_rec[(size_t)k]];
    if (k == 0 || q.record != queries[by_rec[(size_t)k - 1]].record) {
      const int64_t i = q.record;
      cpairs.push_back(pairs[i]);
      cspans.push_back(call.spans[(size_t)i]);
      crecs.push_back(call.recs[i]);
      cbases.push_back(slices && results[i].status == AWV_ST_COMPLETED ? slices[i] : awv_cs_slice{0u, 0u, 0, 0});
    }
    hq[(size_t)k] = HostQuery{(int64_t)crecs.size() - 1, q.from, q.beg, q.end, by_rec[(size_t)k]};
  }
  const int64_t m = (int64_t)crecs.size();
  if (int rc = awvw::check_lengths(crecs.data(), m, MAX_COLUMNS, TOO_LONG)) return rc;
  // in pieces, a piece's queries re-based to its first record
  std::vector<awv_lift_result> out;
  std::vector<HostQuery> piece_q;
  int64_t k = 0;
  return st->each_piece(v, crecs.data(), m, cigar_arena, max_arena, [&](int64_t first, int64_t n, const awv_result* recs, uint64_t bytes) {
    piece_q.clear();
    for (; k < nq && hq[(size_t)k].rec < first + n; ++k) {
      piece_q.push_back(hq[(size_t)k]);
      piece_q.back().rec -= first;
    }
    out.resize(piece_q.size());
    if (int rc = launch(v, st, cpairs.data() + first, cspans.data() + first, cbases.data() + first, n, recs, st->d_arena.p, bytes, piece_q.data(), (int64_t)piece_q.size(),
                        out.data()))
      return rc;
    for (size_t t = 0; t < piece_q.size(); ++t) lout[piece_q[t].tag] = out[t];
    return (int)AWV_OK;
  });
}

int begin_core(awv_engine* e, const awv_region* regions, int64_t n_regions, int32_t from_mask, int64_t clip_min_score) {
  if (from_mask == 0) {  // the table ends
    if (State* st = awv_internal_lift(e)) st->end();
    return AWV_OK;
  }
  if (from_mask < AWV_LIFT_FROM_TARGET || from_mask > AWV_LIFT_FROM_BOTH) return awv_internal_fail(AWV_ERR_ARG, "lift_begin: from_mask must be 0 or an AWV_LIFT_FROM_* mask");
  if (n_regions < 0 || n_regions > INT32_MAX || (n_regions > 0 && !regions)) return awv_internal_fail(AWV_ERR_ARG, "lift_begin: bad region list");
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st)) return rc;
  for (int64_t r = 0; r < n_regions; ++r) {
    const awv_region& g = regions[r];
    if (g.seq < 0 || g.seq >= v.n || g.beg < 0 || g.beg >= g.end || g.end > v.len_host[g.seq])
      return awv_internal_fail(AWV_ERR_ARG, "lift_begin: region " + std::to_string(r) + " names a sequence out of range, or an interval that is empty or outside its sequence");
  }
  st->end();
  st->regions.assign(regions, regions + n_regions);
  st->by_seq.resize((size_t)n_regions);
  for (int64_t r = 0; r < n_regions; ++r) st->by_seq[(size_t)r] = (int32_t)r;
  const std::vector<awv_region>& g = st->regions;
  std::stable_sort(st->by_seq.begin(), st->by_seq.end(),
                   [&](int32_t a, int32_t b) { return g[(size_t)a].seq != g[(size_t)b].seq ? g[(size_t)a].seq < g[(size_t)b].seq : g[(size_t)a].beg < g[(size_t)b].beg; });
  st->seq_first.assign((size_t)v.n + 1, 0);
  st->seq_reach.assign((size_t)v.n, 0);
  for (const awv_region& r : g) {
    ++st->seq_first[(size_t)r.seq + 1];
    st->seq_reach[(size_t)r.seq] = std::max(st->seq_reach[(size_t)r.seq], r.end - r.beg);
  }
  for (int32_t s = 0; s < v.n; ++s) st->seq_first[(size_t)s + 1] += st->seq_first[(size_t)s];
  st->nseq = v.n;
  st->clip_min_score = clip_min_score;
  st->stats = awv_lift_stats{};
  st->from_mask = from_mask;
  return AWV_OK;
}

int read_core(awv_engine* e, awv_lift_row* rows, uint64_t cap, uint64_t* n_rows) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "lift_read", v, st)) return rc;
  std::sort(st->rows.begin(), st->rows.end(), row_less);
  *n_rows = (uint64_t)st->rows.size();
  if (*n_rows <= cap && rows && *n_rows) std::copy(st->rows.begin(), st->rows.end(), rows);
  return AWV_OK;
}

// the regions of sequence seq that overlap [lo, hi): a query each
void match_regions(const State* st, int64_t item, int32_t from, int32_t seq, int64_t lo, int64_t hi, std::vector<HostQuery>& out) {
  if (lo >= hi) return;
  const std::vector<awv_region>& g = st->regions;
  const int32_t* const first = st->by_seq.data() + st->seq_first[(size_t)seq];
  const int32_t* const last = st->by_seq.data() + st->seq_first[(size_t)seq + 1];
  // a region that overlaps begins after lo - (the longest region's length) and before hi
  const int64_t from_beg = lo - st->seq_reach[(size_t)seq];
  const int32_t* it = std::partition_point(first, last, [&](int32_t r) { return (int64_t)g[(size_t)r].beg <= from_beg; });
  for (; it != last && (int64_t)g[(size_t)*it].beg < hi; ++it)
    if ((int64_t)g[(size_t)*it].end > lo) out.push_back(HostQuery{item, from, g[(size_t)*it].beg, g[(size_t)*it].end, (int64_t)*it});
}

}  // namespace

int lift_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
               const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans) {
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_active(e, "lift_batch", v, st)) return rc;
  if (v.n != st->nseq) return awv_internal_fail(AWV_ERR_STATE, "lift: the sequence set changed since awv_engine_lift_begin");
  awvw::contributing_items(v, pairs, n, results, clips, st->clip_min_score, seg_first, iout, sout, spans, st->items);
  const awvw::BatchItems& it = st->items;
  std::vector<HostQuery>& hq = st->h_queries;
  hq.clear();
  for (size_t i = 0; i < it.pairs.size(); ++i) {
    const awv_pair& p = it.pairs[i];
    const Span& sp = it.spans[i];
    if (st->from_mask & AWV_LIFT_FROM_TARGET) match_regions(st, (int64_t)i, AWV_LIFT_FROM_TARGET, p.t_idx, sp.tb, sp.te, hq);
    if (st->from_mask & AWV_LIFT_FROM_QUERY) {
      const int64_t qlen = v.len_host[p.q_idx];
      match_regions(st, (int64_t)i, AWV_LIFT_FROM_QUERY, p.q_idx, p.q_revcomp ? qlen - sp.pe : (int64_t)sp.pb, p.q_revcomp ? qlen - sp.pb : (int64_t)sp.pe, hq);
    }
  }
  st->h_out.resize(hq.size());
  if (int rc = launch(v, st, it.pairs.data(), it.spans.data(), nullptr, (int64_t)it.pairs.size(), it.recs.data(), d_arena, arena_bytes, hq.data(), (int64_t)hq.size(),
                      st->h_out.data()))
    return rc;
  for (size_t k = 0; k < hq.size(); ++k) {
    const awv_lift_result& r = st->h_out[k];
    if (r.code != AWV_LF_OK) continue;
    const awv_pair& p = it.pairs[(size_t)hq[k].rec];
    st->rows.push_back(awv_lift_row{(int32_t)hq[k].tag, p.q_idx, p.t_idx, (p.q_revcomp ? AWV_LIFT_ROW_REVCOMP : 0) | (hq[k].from == AWV_LIFT_FROM_QUERY ? AWV_LIFT_ROW_FROM_QUERY : 0),
                                    r.src_beg, r.src_end, r.dst_beg, r.dst_end, r.num_matches, r.num_mismatches, r.num_ins, r.num_del});
  }
  return AWV_OK;
}

}  // namespace awvl

extern "C" {

int awv_lift_one_host(int32_t from, int32_t q_revcomp, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb, int32_t te, const uint8_t* cigar, int64_t n,
                      const awv_cs_slice* slice, int32_t beg, int32_t end, awv_lift_result* out) {
  if (!out || !awvl::from_ok(from) || qlen < 0 || tlen < 0 || n < 0 || (n > 0 && !cigar)) return awv_internal_fail(AWV_ERR_ARG, "lift_one_host: bad argument");
  if (int rc = awvw::check_host_rectangle("lift_one_host", qlen, tlen, pb, pe, tb, te)) return rc;
  if (beg < 0 || beg >= end || end > (from == AWV_LIFT_FROM_TARGET ? tlen : qlen))
    return awv_internal_fail(AWV_ERR_ARG, "lift_one_host: the interval is empty or outside its source sequence");
  awvw::HostSlice sl;
  if (int rc = awvw::check_host_slice("lift_one_host", slice, n, awvl::MAX_COLUMNS, sl)) return rc;
  const awv_cs_slice base{(uint32_t)sl.beg, (uint32_t)sl.end, (int32_t)sl.q_skip, (int32_t)sl.t_skip};
  awvl::Span sp{pb, pe, tb, te};
  sp.pb = (int32_t)std::min<int64_t>((int64_t)sp.pb + base.q_skip, (int64_t)sp.pe + 1);  // (awvcs::apply_slice's rectangle)
  sp.tb = (int32_t)std::min<int64_t>((int64_t)sp.tb + base.t_skip, (int64_t)sp.te + 1);
  *out = awvl::lift_one(from, q_revcomp != 0, qlen, sp, cigar + base.col_beg, (int64_t)base.col_end - base.col_beg, base, beg, end);
  return AWV_OK;
}

int awv_lift_cigars(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                    const awv_cs_slice* slices, const awv_lift_query* queries, int64_t nq, awv_lift_result* lout) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("lift_cigars", n, pairs, results, nq >= 0 && (nq == 0 || (queries && lout)), cigar_arena, arena_bytes)) return rc;
  AWV_GUARDED(return awvl::lift_cigars_core(e, pairs, nullptr, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), queries, nq, lout);)
}

int awv_lift_ranges(awv_engine* e, const awv_range_pair* ranges, int64_t n, const awv_result* results, const uint8_t* cigar_arena, uint64_t arena_bytes,
                    const awv_cs_slice* slices, const awv_lift_query* queries, int64_t nq, awv_lift_result* lout) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awvw::check_call_args("lift_ranges", n, ranges, results, nq >= 0 && (nq == 0 || (queries && lout)), cigar_arena, arena_bytes)) return rc;
  static const awv_range_pair none{};
  AWV_GUARDED(return awvl::lift_cigars_core(e, nullptr, n > 0 ? ranges : &none, n, results, cigar_arena, arena_bytes, slices, awv_internal_max_arena(e), queries, nq, lout);)
}

int awv_engine_lift_begin(awv_engine* e, const awv_region* regions, int64_t n_regions, int32_t from_mask, int64_t clip_min_score) {
  if (!e) return awv_internal_null_engine();
  AWV_GUARDED(return awvl::begin_core(e, regions, n_regions, from_mask, clip_min_score);)
}

int awv_engine_lift_read(awv_engine* e, awv_lift_row* rows, uint64_t cap, uint64_t* n_rows) {
  if (!e) return awv_internal_null_engine();
  if (!n_rows) return awv_internal_fail(AWV_ERR_ARG, "lift_read: null argument");
  AWV_GUARDED(return awvl::read_core(e, rows, cap, n_rows);)
}

int awv_engine_lift_stats(const awv_engine* e, awv_lift_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "lift_stats: null argument");
  const awvl::State* st = awv_internal_lift(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_lift_stats{};
  return AWV_OK;
}

}  // extern "C"
