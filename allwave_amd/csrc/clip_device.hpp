// clip_device.hpp -- what "clipped" means for one op string (include/allwave_hip.h, above awv_align_pairs_clipped), once, for
// the host and the device: awv_clip_one_host is clip_one below, and the clip kernel (clip.hip) reaches the same record from
// wave scans over the same column deltas.
//
// A column adds column_delta to a running sum S: +a for 'M', -x for 'X', and for the L-th column of a gap run what the run's
// cost grows by, gap_cost(L) - gap_cost(L - 1).  The clip is the segment [b, e) of maximal S(e) - S(b), the smallest such e
// and for it the largest b; empty when nothing scores above 0.  It begins and ends with an 'M' (dropping any other column
// at either end raises the score), so no gap run is ever cut and the segment's score is a * #M minus the segment re-scored
// as an op string of its own.  Needs no sequence.
#pragma once

#include "verify_device.hpp"  // awvf::gap_cost, awvf::is_gap: the re-scoring rule, not restated here

namespace awvc {

__host__ __device__ inline bool is_op(uint32_t op) { return op == 'M' || op == 'X' || op == 'I' || op == 'D'; }

// What a column adds to S.  run_pos: for a gap column its 1-based position in its maximal run of equal gap ops.
__host__ __device__ inline int64_t column_delta(const awv_penalties& pen, int64_t a, uint32_t op, int64_t run_pos) {
  if (op == 'M') return a;
  if (op == 'X') return -(int64_t)pen.mismatch;
  return (run_pos > 1 ? awvf::gap_cost(pen, run_pos - 1) : 0) - awvf::gap_cost(pen, run_pos);
}

// ops before a column, by kind: q = not 'I' (pattern bases consumed), t = not 'D' (text bases), x = 'X', m = 'M'
struct Prefix {
  uint32_t q, t, x, m;
};

__host__ __device__ inline awv_clip_result make_clip(int code, uint32_t col_beg, uint32_t col_end) {  // a record without a segment
  awv_clip_result r;
  r.code = code;
  r.reserved = 0;
  r.score = 0;
  r.col_beg = col_beg;
  r.col_end = col_end;
  r.q_skip = r.t_skip = 0;
  r.num_matches = r.num_mismatches = r.num_ins = r.num_del = 0;
  r.penalty = 0;
  r.reserved2 = 0;
  return r;
}

// The segment [b, e) of score `score` > 0: `at_b` / `at_e` count the ops before column b / column e.
__host__ __device__ inline awv_clip_result make_clip(int64_t a, int64_t score, uint32_t b, uint32_t e, const Prefix& at_b, const Prefix& at_e) {
  awv_clip_result r = make_clip(AWV_CL_OK, b, e);
  const uint32_t cols = e - b;
  r.score = score;
  r.q_skip = (int32_t)at_b.q;
  r.t_skip = (int32_t)at_b.t;
  r.num_matches = (int32_t)(at_e.m - at_b.m);
  r.num_mismatches = (int32_t)(at_e.x - at_b.x);
  r.num_ins = (int32_t)(cols - (at_e.q - at_b.q));
  r.num_del = (int32_t)(cols - (at_e.t - at_b.t));
  r.penalty = (int32_t)(a * (int64_t)r.num_matches - score);
  return r;
}

// The contract as a serial walk (the host yardstick).  A tie replaces the minimum's index and never replaces the best.
__host__ __device__ inline awv_clip_result clip_one(const awv_penalties& pen, int64_t a, const uint8_t* cigar, int64_t n) {
  int64_t S = 0, minS = 0, best = 0, run_start = 0;
  uint32_t min_i = 0, b = 0, e = 0, prev = 0;
  Prefix now{0, 0, 0, 0}, at_min{0, 0, 0, 0}, at_b{0, 0, 0, 0}, at_e{0, 0, 0, 0};
  for (int64_t c = 0; c < n; ++c) {
    const uint32_t op = cigar[c];
    if (!is_op(op)) return make_clip(AWV_CL_BAD_OP, (uint32_t)c, (uint32_t)c);
    if (op != prev) {
      run_start = c;
      prev = op;
    }
    S += column_delta(pen, a, op, c - run_start + 1);
    now.q += op != 'I';
    now.t += op != 'D';
    now.x += op == 'X';
    now.m += op == 'M';
    if (S <= minS) {
      minS = S;
      min_i = (uint32_t)(c + 1);
      at_min = now;
    }
    if (S - minS > best) {
      best = S - minS;
      at_b = at_min;
      at_e = now;
      b = min_i;
      e = (uint32_t)(c + 1);
    }
  }
  return best > 0 ? make_clip(a, best, b, e, at_b, at_e) : make_clip(AWV_CL_EMPTY, 0, 0);
}

struct State;                  // clip.hip: the clip launches' device buffers, events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);    // (nullptr: nothing)

// engine.hip's hook: clips one batch of awv_align_pairs_clipped on the engine's stream.  `results`, `cout`: the batch's n
// entries (host); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it.  Adds to the stats the caller reset
// at the start of its call (stats_reset).
int clip_batch(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, int64_t n, const awv_result* results, const uint8_t* d_arena,
               uint64_t arena_bytes, awv_clip_result* cout);

}  // namespace awvc

// engine.hip
awvc::State*& awv_internal_clip(awv_engine* e);
