// normalize.hip -- gap runs moved to their left- (or right-) normal place on the device: the per-batch step of an aligning
// call under awv_engine_set_normalize, awv_normalize_cigars / _ranges, awv_normalize_one_host and awv_engine_normalize_stats
// (include/allwave_hip.h).  What "normalized" means is normalize_device.hpp; this file gets the kernel to the same bytes.
//
// verify.hip's shape: one wave per record, persistent waves taking records (longest op string first) from a cursor.
// Per record:
//   1. a counting pass over the op bytes (chunks of 64 lanes x 16 bytes, packed byte counts) finds a byte that is no op and
//      the bases the ops consume: any code but AWV_NM_OK ends the record before a byte is changed.  It also proves what the
//      second pass relies on: every run's bases lie inside its sequence.
//   2. one pass in the direction of normalization, again in chunks of 64 x 16 bytes with one aligned 16-byte load per lane.
//      A right-normalizing wave walks the mirrored string: its chunks come from the string's end, every lane's 16 bytes are
//      reversed in registers, and a column or base index is mirrored where memory is touched; nothing else knows.
//      Per chunk each lane marks where an op differs from the one before it ("breaks"), which breaks begin a gap run and which
//      end one.  The consumed pattern / text bases before a lane are a packed add-scan of its counts, as in verify.hip; the
//      start of the op run a lane begins in, and the op before that run, come from a max-scan over (last break, op before it)
//      keys, carried from chunk to chunk.  The wave then takes the chunk's events in column order, lowest lane first: the
//      owning lane works out the event's column and, for a run's start, its m (from its own breaks or the scanned ones),
//      whether it is linked, and its own sequence's position; five readlanes make that uniform.  A run is decided at its end
//      (the next break, or the end of the string): b from shift_bound and the carried shift of the run before, a by the whole
//      wave comparing seq[p - j] with seq[p + L - j] for 64 values of j per trip, capped at b, a ballot finding the first
//      difference.  The lanes then patch the zone with byte stores: min(s, L) columns at either end.
// The zone lies at or before the run's last column, which the pass has read: in the chunk in registers or an earlier one.  So
// patching in place never disturbs a later read, and b, m and the types always come from the input string, as the closed
// form wants.  Work: O(cigar_len / 64 + runs + sum of s_i / 64) wave steps.
#include "normalize_device.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "record_pass.hpp"  // the host skeleton of a record pass: RecordPass, pack_piece, scatter_back, AWV_TRY

namespace awvn {

struct KParams {
  const uint8_t* fwd;
  const uint8_t* rc;
  const uint64_t* seq_off;
  const int32_t* seq_len;
  const awv_pair* pairs;
  const Span* spans;          // nullable (range calls)
  const awv_result* results;  // cigar_off relative to `arena`
  const int32_t* order;       // dispatch slot -> record
  uint8_t* arena;             // 16-byte aligned, readable up to the 16-byte boundary behind every op string
  awv_norm_result* out;
  unsigned long long* counters;  // [0] cursor, [1] records moved, [2] runs, [3] runs moved, [4] columns moved, [5] columns
  long long npairs;
  int mirror;                 // 0: left, 1: right
};

using awvw::byte_at;
using awvw::byte_range_mask;
using awvw::CHUNK;
using awvw::count_bytes;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::u32x4;
using awvw::wave_scan_add;
using awvw::wave_scan_max;
using awvw::wave_sum_i64;

__global__ __launch_bounds__(64) void awv_normalize_kernel(KParams kp) {
  const int lane = threadIdx.x;
  const bool mirror = kp.mirror != 0;
  unsigned long long t_records = 0, t_runs = 0, t_runs_moved = 0, t_cols_moved = 0, t_columns = 0;  // (uniform)
  for (;;) {
    const unsigned long long slot = awvw::take_record(kp.counters, lane);
    if (slot >= (unsigned long long)kp.npairs) break;
    const int pair = __builtin_amdgcn_readfirstlane(kp.order[slot]);
    const awv_result rec = kp.results[pair];
    if (rec.status != AWV_ST_COMPLETED) {
      if (lane == 0) kp.out[pair] = make_norm(AWV_NM_SKIPPED, 0, 0, 0);
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
    const long long n64 = (long long)rec.cigar_len;
    t_columns += (unsigned long long)n64;
    const int sh = (int)(rec.cigar_off & 15);
    uint8_t* const ops = kp.arena + (rec.cigar_off & ~(uint64_t)15);  // op byte c is ops[sh + c]

    // ---- pass 1: codes, before anything is written
    {
      const long long span = sh + n64;
      long long cnt_i = 0, cnt_d = 0, bad_col = -1;  // counts: lane-private
      for (long long base = 0; base < span; base += CHUNK) {
        const long long b0 = base + lane * LANE_BYTES;
        const int jlo = (int)min(max((long long)sh - b0, 0ll), (long long)LANE_BYTES), jhi = (int)min(max(span - b0, 0ll), (long long)LANE_BYTES);
        const int nv = max(jhi - jlo, 0);
        u32x4 w = {0u, 0u, 0u, 0u};
        if (b0 < span) w = *(const u32x4*)(ops + b0);
        int n_i = 0, n_d = 0, n_mx = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          w[k] &= byte_range_mask(jlo - 4 * k, jhi - 4 * k);
          n_i += count_bytes(w[k], 'I');
          n_d += count_bytes(w[k], 'D');
          n_mx += count_bytes(w[k], 'X') + count_bytes(w[k], 'M');
        }
        const unsigned long long bad_lanes = __ballot(n_i + n_d + n_mx != nv);
        if (bad_lanes != 0) {  // lanes hold ascending columns: the lowest lane's first is the smallest
          int first = LANE_BYTES;
#pragma unroll
          for (int j = LANE_BYTES - 1; j >= 0; --j) {
            const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            if (j >= jlo && j < jhi && !is_op(op)) first = j;
          }
          const int l = __builtin_ctzll(bad_lanes);
          bad_col = base + l * LANE_BYTES + __builtin_amdgcn_readlane(first, l) - sh;
          break;
        }
        cnt_i += n_i;
        cnt_d += n_d;
      }
      if (bad_col >= 0) {
        if (lane == 0) kp.out[pair] = make_norm(AWV_NM_BAD_OP, 0, bad_col, 0);
        continue;
      }
      if (lengths_code(n64, wave_sum_i64(cnt_i), wave_sum_i64(cnt_d), plen, tlen) != AWV_NM_OK) {
        if (lane == 0) kp.out[pair] = make_norm(AWV_NM_LENGTHS, 0, 0, 0);
        continue;
      }
    }

    // ---- pass 2 (n = plen + #I <= 2^31 - 2 from here on: columns fit an int)
    const int n = (int)n64;
    const int frame_end = (sh + n + 15) & ~15;                  // the 16-byte boundary behind the string
    const int shm = mirror ? frame_end - (sh + n) : sh;          // column k is byte shm + k of the frame the wave walks
    const int span = shm + n;
    auto store_op = [&](int col, unsigned op) { ops[mirror ? frame_end - 1 - (shm + col) : shm + col] = (uint8_t)op; };

    int cq = 0, ct = 0;        // bases consumed before the chunk (uniform, like everything carried)
    int c_start = 0;           // the column the op run in progress began at
    unsigned c_prev = 0;       // the op before the chunk's first column (0: none)
    unsigned c_pp = 0;         // the op before column c_start (0: none)
    // the gap run in progress
    unsigned cur_g = 0;
    int cur_c = 0, cur_m = 0, cur_p = 0;
    bool cur_linked = false;
    // the gap run before it
    unsigned prev_type = 0;
    int prev_s = 0;
    int runs = 0, runs_moved = 0, max_shift = 0;
    long long cols_moved = 0;

    // a run [cur_c, col_end) of cur_g is complete: decide its shift and patch its zone (all lanes, uniform arguments)
    auto finish_run = [&](int col_end) {
      const int L = col_end - cur_c;
      const bool del = cur_g == 'D';
      const uint8_t* seq = del ? pattern : text;
      const int slen = del ? plen : tlen;
      long long b = shift_bound(cur_m, cur_linked, cur_g, prev_type, prev_s);
      int cap = (int)min(b, (long long)min(cur_p, cur_c));
      if (cap < 0 || L <= 0 || (long long)cur_p + L > slen) cap = 0;  // (pass 1 rules these out; never read outside a sequence)
      int s = cap;
      for (int t0 = 0; t0 < cap; t0 += 64) {
        const int j = t0 + lane + 1;
        bool differs = false;
        if (j <= cap) {
          const int lo = cur_p - j, hi = cur_p + L - j;  // 0 <= lo < hi < slen
          differs = seq[mirror ? slen - 1 - lo : lo] != seq[mirror ? slen - 1 - hi : hi];
        }
        const unsigned long long d = __ballot(differs);
        if (d != 0) {
          s = t0 + __builtin_ctzll(d);
          break;
        }
      }
      ++runs;
      if (s > 0) {
        const int w = min(s, L);
        for (int i = lane; i < w; i += 64) {
          store_op(cur_c - s + i, cur_g);
          store_op(cur_c + L - w + i, 'M');
        }
        ++runs_moved;
        cols_moved += s;
        max_shift = max(max_shift, s);
      }
      prev_type = cur_g;
      prev_s = s;
    };

    for (int base = 0; n > 0 && base < span; base += CHUNK) {
      const int b0 = base + lane * LANE_BYTES;
      const int jlo = min(max(shm - b0, 0), LANE_BYTES), jhi = min(max(span - b0, 0), LANE_BYTES);  // this lane's bytes [jlo, jhi) are columns
      const int nv = max(jhi - jlo, 0);
      u32x4 w = {0u, 0u, 0u, 0u};
      if (b0 < span) {
        if (!mirror) {
          w = *(const u32x4*)(ops + b0);
        } else {  // the frame's bytes [b0, b0 + 16) are memory's [frame_end - b0 - 16, frame_end - b0), last first
          const u32x4 r = *(const u32x4*)(ops + (frame_end - b0 - LANE_BYTES));
          w[0] = __builtin_bswap32(r[3]);
          w[1] = __builtin_bswap32(r[2]);
          w[2] = __builtin_bswap32(r[1]);
          w[3] = __builtin_bswap32(r[0]);
        }
      }
      int n_i = 0, n_d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] &= byte_range_mask(jlo - 4 * k, jhi - 4 * k);
        n_i += count_bytes(w[k], 'I');
        n_d += count_bytes(w[k], 'D');
      }
      const int packed = (nv - n_i) | ((nv - n_d) << 16);  // (a chunk holds 1,024 columns: the sums fit 16 bits)
      const int s_qt = wave_scan_add(packed);
      const int q0 = cq + ((s_qt - packed) & 0xffff), t0 = ct + ((s_qt - packed) >> 16);  // bases consumed before this lane's columns
      // the op before this lane's first column: the lower lane's last byte, the chunk's carry in lane 0, none at column 0
      unsigned prev = (unsigned)from_lower_lane((int)w[3], (int)(c_prev << 24)) >> 24;
      if (b0 <= shm) prev = 0;
      unsigned brk = 0, starts = 0, ends = 0;  // bit j: byte j's op differs from the one before it / begins a gap run / follows one
      int key = -1;                            // (last break's byte position in the chunk) << 8 | the op before it
      unsigned pv = prev;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j >= jlo && j < jhi) {
          if (op != pv) {
            brk |= 1u << j;
            if (is_gap(op)) starts |= 1u << j;
            if (is_gap(pv)) ends |= 1u << j;
            key = ((lane * LANE_BYTES + j) << 8) | (int)pv;
          }
          pv = op;
        }
      }
      const int kin = wave_scan_max(key);
      const int kex = from_lower_lane(kin, -1);
      const int rs0 = kex >= 0 ? base + (kex >> 8) - shm : c_start;  // the op run this lane begins in started here
      const unsigned pp0 = kex >= 0 ? (unsigned)(kex & 0xff) : c_pp;  // and this op came before it

      unsigned ev = starts | ends;
      for (;;) {
        const unsigned long long have = __ballot(ev != 0);
        if (have == 0) break;
        const int l = __builtin_ctzll(have);
        // every lane works on its own next event; lane l's is the wave's
        const int j = __builtin_ctz(ev | 0x10000u) & 15;
        const unsigned op_j = byte_at(w, j);
        const unsigned pv_j = j > jlo ? byte_at(w, j - 1) : prev;
        const int col = b0 + j - shm;
        int m = 0;
        bool linked = is_gap(pv_j);
        if (pv_j == 'M') {  // the 'M' run before column col: from this lane's own breaks, else from the scan
          const unsigned below = brk & ((1u << j) - 1u);
          int m_start = rs0;
          unsigned pp = pp0;
          if (below != 0) {
            const int hb = 31 - __builtin_clz(below);
            m_start = b0 + hb - shm;
            pp = hb > jlo ? byte_at(w, hb - 1) : prev;
          }
          m = col - m_start;
          linked = is_gap(pp);
        }
        int li = 0, ld = 0;  // 'I' / 'D' among this lane's columns before byte j
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned wk = w[k] & byte_range_mask(jlo - 4 * k, j - 4 * k);
          li += count_bytes(wk, 'I');
          ld += count_bytes(wk, 'D');
        }
        const int before = max(j - jlo, 0);
        const int p = op_j == 'D' ? q0 + before - li : t0 + before - ld;
        const int info = (int)op_j | (int)(((ends >> j) & 1u) << 8) | (int)(((starts >> j) & 1u) << 9) | (linked ? 1 << 10 : 0);
        const int u_info = __builtin_amdgcn_readlane(info, l);
        const int u_col = __builtin_amdgcn_readlane(col, l);
        if (u_info & (1 << 8)) finish_run(u_col);
        if (u_info & (1 << 9)) {
          cur_g = (unsigned)(u_info & 0xff);
          cur_c = u_col;
          cur_m = __builtin_amdgcn_readlane(m, l);
          cur_p = __builtin_amdgcn_readlane(p, l);
          cur_linked = (u_info & (1 << 10)) != 0;
        }
        if (lane == l) ev &= ev - 1;
      }

      const int last_lane = min(63, (span - 1 - base) >> 4);  // the lane that holds the chunk's last column
      c_prev = (unsigned)__builtin_amdgcn_readlane((int)pv, last_lane);
      const int kall = __builtin_amdgcn_readlane(kin, 63);
      if (kall >= 0) {
        c_start = base + (kall >> 8) - shm;
        c_pp = (unsigned)(kall & 0xff);
      }
      const int tot = __builtin_amdgcn_readlane(s_qt, 63);
      cq += tot & 0xffff;
      ct += tot >> 16;
    }
    if (is_gap(c_prev)) finish_run(n);  // the string ends with a gap run

    if (lane == 0) kp.out[pair] = make_norm(AWV_NM_OK, runs_moved, cols_moved, max_shift);
    t_records += runs_moved > 0;
    t_runs += (unsigned long long)runs;
    t_runs_moved += (unsigned long long)runs_moved;
    t_cols_moved += (unsigned long long)cols_moved;
  }
  if (lane == 0) {
    if (t_records) atomicAdd(&kp.counters[1], t_records);
    if (t_runs) atomicAdd(&kp.counters[2], t_runs);
    if (t_runs_moved) atomicAdd(&kp.counters[3], t_runs_moved);
    if (t_cols_moved) atomicAdd(&kp.counters[4], t_cols_moved);
    if (t_columns) atomicAdd(&kp.counters[5], t_columns);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

using awvw::Buf;

struct State : awvw::RecordPass {
  Buf<awv_pair> d_pairs;
  Buf<Span> d_spans;
  Buf<awv_norm_result> d_out;
  std::vector<awv_norm_result> h_out;  // a batch's records, which an aligning call does not hand out
  awv_norm_stats stats{};
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

int check_direction(int32_t direction) {
  if (direction != AWV_NORM_LEFT && direction != AWV_NORM_RIGHT)
    return awv_internal_fail(AWV_ERR_ARG, "normalize: direction must be AWV_NORM_LEFT or AWV_NORM_RIGHT");
  return AWV_OK;
}

int open_state(awv_engine* e, awp::EngineView& v, State*& st, bool need_set) { return awvw::open_pass(awv_internal_normalize(e), e, v, st, need_set); }

// One launch over n records whose op bytes are on the device already.  Every index is checked here, on the host, as
// RecordPass::begin checks every op string's place in the arena: the kernel reads and writes where the records say.
int launch(const awp::EngineView& v, const SeqView& seqs, State* st, int32_t direction, const awv_pair* pairs, int64_t n, const awv_result* results,
           uint8_t* d_arena, uint64_t arena_bytes, awv_norm_result* nout, const Span* spans) {
  if (n == 0) return AWV_OK;
  for (int64_t i = 0; i < n; ++i)
    if (pairs[i].q_idx < 0 || pairs[i].q_idx >= seqs.n || pairs[i].t_idx < 0 || pairs[i].t_idx >= seqs.n)
      return awv_internal_fail(AWV_ERR_ARG, "normalize: sequence index out of range");
  if (int rc = st->begin(v, "normalize", n, results, arena_bytes)) return rc;
  AWV_TRY(st->d_pairs.reserve((size_t)n));
  AWV_TRY(st->d_out.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(st->d_pairs.p, pairs, (size_t)n * sizeof(awv_pair), hipMemcpyHostToDevice, v.stream));
  if (spans) {
    AWV_TRY(st->d_spans.reserve((size_t)n));
    AWV_TRY(hipMemcpyAsync(st->d_spans.p, spans, (size_t)n * sizeof(Span), hipMemcpyHostToDevice, v.stream));
  }
  if (int rc = st->clear_counters(v, 8)) return rc;
  KParams kp{};
  kp.fwd = seqs.fwd;
  kp.rc = seqs.rc;
  kp.seq_off = seqs.off;
  kp.seq_len = seqs.len;
  kp.pairs = st->d_pairs.p;
  kp.spans = spans ? st->d_spans.p : nullptr;
  kp.results = st->d_results.p;
  kp.order = st->d_order.p;
  kp.arena = d_arena;
  kp.out = st->d_out.p;
  kp.counters = st->d_counters.p;
  kp.npairs = n;
  kp.mirror = direction == AWV_NORM_RIGHT ? 1 : 0;
  if (int rc = st->start(v)) return rc;
  hipLaunchKernelGGL(awv_normalize_kernel, dim3(st->grid(v, n)), dim3(64), 0, v.stream, kp);
  if (int rc = st->stop(v)) return rc;
  unsigned long long hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float ms = 0;
  AWV_TRY(hipMemcpyAsync(nout, st->d_out.p, (size_t)n * sizeof(awv_norm_result), hipMemcpyDeviceToHost, v.stream));
  if (int rc = st->finish(v, hc, 8, ms)) return rc;
  st->stats.kernel_ms += ms;
  st->stats.pairs += (uint64_t)n;
  st->stats.records_moved += hc[1];
  st->stats.runs += hc[2];
  st->stats.runs_moved += hc[3];
  st->stats.columns_moved += hc[4];
  st->stats.columns += hc[5];
  return AWV_OK;
}

// ranges (nullable; awv_normalize_ranges): the call is on ranges[0..npairs) -- `pairs` is not read
int normalize_cigars_core(awv_engine* e, int32_t direction, const awv_pair* pairs, int64_t npairs, const awv_result* results, uint8_t* cigar_arena,
                          uint64_t arena_bytes, uint64_t max_arena, awv_norm_result* nout, const awv_range_pair* ranges) {
  if (int rc = check_direction(direction)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st, true)) return rc;
  st->stats = awv_norm_stats{};
  const SeqView seqs{v.n, v.fwd, v.rc, v.off, v.len};
  std::vector<awv_pair> rpairs;
  std::vector<Span> spans;
  if (ranges) {
    rpairs.resize((size_t)npairs);
    spans.resize((size_t)npairs);
    for (int64_t i = 0; i < npairs; ++i)
      if (!awvr::split_range(v.len_host, v.n, ranges[i], rpairs[(size_t)i], spans[(size_t)i]))
        return awv_internal_fail(AWV_ERR_ARG, "normalize_ranges: range " + std::to_string(i) + " names a sequence index or an interval out of range");
    pairs = rpairs.data();
  }
  // before anything goes up: every index is in range and every completed record's op bytes lie inside the caller's arena
  for (int64_t i = 0; i < npairs; ++i) {
    if (pairs[i].q_idx < 0 || pairs[i].q_idx >= v.n || pairs[i].t_idx < 0 || pairs[i].t_idx >= v.n)
      return awv_internal_fail(AWV_ERR_ARG, "normalize_cigars: sequence index out of range");
    if (awvw::outside(results[i], arena_bytes)) return awv_internal_fail(AWV_ERR_ARG, "normalize_cigars: a record's op bytes lie outside the CIGAR arena");
  }
  // in pieces (record_pieces.hpp) that keep every string's offset modulo 16; a piece comes back whole and every string
  // returns to its place
  std::vector<uint8_t> stage;
  std::vector<awv_result> recs;
  for (int64_t first = 0; first < npairs;) {
    const awvw::Piece pc = awvw::pack_piece(results, npairs, first, cigar_arena, max_arena, true, recs, stage);
    AWV_TRY(st->d_arena.reserve((size_t)pc.bytes + 64));
    if (pc.bytes) AWV_TRY(hipMemcpyAsync(st->d_arena.p, stage.data(), (size_t)pc.bytes, hipMemcpyHostToDevice, v.stream));
    if (int rc = launch(v, seqs, st, direction, pairs + first, pc.n, recs.data(), st->d_arena.p, pc.bytes, nout + first, ranges ? spans.data() + first : nullptr)) return rc;
    if (pc.bytes) {
      AWV_TRY(hipMemcpyAsync(stage.data(), st->d_arena.p, (size_t)pc.bytes, hipMemcpyDeviceToHost, v.stream));
      AWV_TRY(hipStreamSynchronize(v.stream));
    }
    awvw::scatter_back(results + first, nout + first, pc.n, recs, stage, cigar_arena);
    first += pc.n;
  }
  return AWV_OK;
}

}  // namespace

int normalize_batch(awv_engine* e, const SeqView& seqs, int32_t direction, const awv_pair* pairs, int64_t n, const awv_result* results,
                    uint8_t* d_arena, uint64_t arena_bytes, const Span* spans) {
  if (int rc = check_direction(direction)) return rc;
  awp::EngineView v;
  State* st = nullptr;
  if (int rc = open_state(e, v, st, false)) return rc;
  st->h_out.resize((size_t)n);
  return launch(v, seqs, st, direction, pairs, n, results, d_arena, arena_bytes, st->h_out.data(), spans);
}

}  // namespace awvn

extern "C" {

int awv_normalize_cigars(awv_engine* e, int32_t direction, const awv_pair* pairs, int64_t n, const awv_result* results, uint8_t* cigar_arena,
                         uint64_t arena_bytes, awv_norm_result* nout) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || (n > 0 && (!pairs || !results || !nout))) return awv_internal_fail(AWV_ERR_ARG, "normalize_cigars: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "normalize_cigars: null arena");
  AWV_GUARDED(return awvn::normalize_cigars_core(e, direction, pairs, n, results, cigar_arena, arena_bytes, awv_internal_max_arena(e), nout, nullptr);)
}

int awv_normalize_ranges(awv_engine* e, int32_t direction, const awv_range_pair* ranges, int64_t n, const awv_result* results, uint8_t* cigar_arena,
                         uint64_t arena_bytes, awv_norm_result* nout) {
  if (!e) return awv_internal_null_engine();
  if (n < 0 || (n > 0 && (!ranges || !results || !nout))) return awv_internal_fail(AWV_ERR_ARG, "normalize_ranges: null argument");
  if (arena_bytes > 0 && !cigar_arena) return awv_internal_fail(AWV_ERR_ARG, "normalize_ranges: null arena");
  AWV_GUARDED(return awvn::normalize_cigars_core(e, direction, nullptr, n, results, cigar_arena, arena_bytes, awv_internal_max_arena(e), nout, ranges);)
}

int awv_normalize_one_host(int32_t direction, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen, const uint8_t* cigar,
                           int64_t n, uint8_t* out_cigar, awv_norm_result* out) {
  if (int rc = awvn::check_direction(direction)) return rc;
  if (!out || plen < 0 || tlen < 0 || n < 0 || (plen > 0 && !pattern) || (tlen > 0 && !text) || (n > 0 && (!cigar || !out_cigar)))
    return awv_internal_fail(AWV_ERR_ARG, "normalize_one_host: bad argument");
  if (out_cigar != cigar && n > 0) std::memmove(out_cigar, cigar, (size_t)n);  // (any code but AWV_NM_OK: the input, untouched)
  *out = awvn::normalize_one(direction == AWV_NORM_RIGHT, pattern, plen, text, tlen, cigar, n, out_cigar);
  return AWV_OK;
}

int awv_engine_set_normalize(awv_engine* e, int32_t mode) {
  if (!e) return awv_internal_fail(AWV_ERR_ARG, "set_normalize: null engine");
  if (mode != AWV_NORM_OFF && mode != AWV_NORM_LEFT && mode != AWV_NORM_RIGHT)
    return awv_internal_fail(AWV_ERR_ARG, "set_normalize: mode must be AWV_NORM_OFF, AWV_NORM_LEFT or AWV_NORM_RIGHT");
  awv_internal_normalize_mode(e) = mode;
  return AWV_OK;
}

int awv_engine_normalize_stats(const awv_engine* e, awv_norm_stats* out) {
  if (!e || !out) return awv_internal_fail(AWV_ERR_ARG, "normalize_stats: null argument");
  const awvn::State* st = awv_internal_normalize(const_cast<awv_engine*>(e));
  *out = st ? st->stats : awv_norm_stats{};
  return AWV_OK;
}

}  // extern "C"
