// verify_device.hpp -- what "verified" means for one pair (include/allwave_hip.h, above awv_align_pairs_verified), once, for
// the host and the device: awv_verify_one_host walks an op string with these functions, and the verify kernel (verify.hip)
// applies the same ones to the columns a lane holds and to the totals a wave has gathered.
//
// The checks, in order of precedence: the first offending column in string order (within one column: an op byte that is
// not M/X/I/D, a base needed beyond the end of a sequence, an 'M' over differing bytes, an 'X' over equal bytes); then, on
// the whole string: both sequences consumed, the record's counts, the record's penalty.  Bytes compare verbatim; 'I'
// consumes the text and 'D' the pattern.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "allwave_hip.h"
#include "range_span.hpp"

struct awv_engine;

namespace awvf {

__host__ __device__ inline bool is_gap(uint32_t op) { return op == 'I' || op == 'D'; }
__host__ __device__ inline bool takes_pattern(uint32_t op) { return op != 'I'; }  // M, X, D (an unknown byte never gets that far)
__host__ __device__ inline bool takes_text(uint32_t op) { return op != 'D'; }

// One column: `p_in` / `t_in` say whether the pattern / text still has a base at this column's position, pb / tb are those
// bases (read only when both are in).
__host__ __device__ inline int column_code(uint32_t op, bool p_in, bool t_in, uint32_t pb, uint32_t tb) {
  if (op != 'M' && op != 'X' && op != 'I' && op != 'D') return AWV_VF_BAD_OP;
  if ((takes_pattern(op) && !p_in) || (takes_text(op) && !t_in)) return AWV_VF_OVERRUN;
  if (op == 'M' && pb != tb) return AWV_VF_M_DIFFERS;
  if (op == 'X' && pb == tb) return AWV_VF_X_EQUAL;
  return AWV_VF_OK;
}

// a maximal run of L > 0 equal gap ops
__host__ __device__ inline int64_t gap_cost(const awv_penalties& p, int64_t L) {
  int64_t g = p.gap_open1 + L * p.gap_ext1;
  if (p.two_piece) {
    const int64_t g2 = p.gap_open2 + L * p.gap_ext2;
    if (g2 < g) g = g2;
  }
  return g;
}

// what a column adds to the penalty when it is known to differ from the one before it: the gap run that ended there
// (`prev` the op before this column, `run_start` the column that run began at)
__host__ __device__ inline int64_t run_end_cost(const awv_penalties& p, uint32_t prev, int64_t run_start, int64_t col) {
  return is_gap(prev) ? gap_cost(p, col - run_start) : 0;
}

// The whole string, once every column has passed: n ops that consumed `q` pattern and `t` text bases, `nx` of them 'X',
// re-scored to `penalty`.
__host__ __device__ inline int whole_code(const awv_result& c, int64_t n, int64_t plen, int64_t tlen, int64_t q, int64_t t,
                                          int64_t nx, int64_t penalty) {
  if (q != plen || t != tlen) return AWV_VF_SHORT;
  const int64_t ni = n - q, nd = n - t, nm = n - ni - nd - nx;
  if ((int64_t)c.cigar_len != n || c.num_matches != nm || c.num_mismatches != nx || c.num_ins != ni || c.num_del != nd ||
      c.q_end != q || c.t_end != t)
    return AWV_VF_COUNTS;
  if ((int64_t)c.penalty != penalty || (int64_t)c.score != -(int64_t)c.penalty) return AWV_VF_PENALTY;
  return AWV_VF_OK;
}

__host__ __device__ inline awv_verify_result make_result(int code, int64_t column, int64_t penalty) {
  awv_verify_result r;
  r.code = code;
  r.reserved = 0;
  r.column = column;
  r.penalty = penalty;
  return r;
}

// The contract as a serial walk (the host yardstick; the kernel reaches the same answer from scanned positions).
__host__ __device__ inline awv_verify_result verify_one(const awv_penalties& pen, const uint8_t* pattern, int64_t plen,
                                                        const uint8_t* text, int64_t tlen, const uint8_t* cigar, int64_t n,
                                                        const awv_result& claimed) {
  if (claimed.status != AWV_ST_COMPLETED) return make_result(AWV_VF_SKIPPED, -1, -1);
  int64_t q = 0, t = 0, nx = 0, penalty = 0, run_start = 0;
  uint32_t prev = 0;
  for (int64_t c = 0; c < n; ++c) {
    const uint32_t op = cigar[c];
    const bool p_in = q < plen, t_in = t < tlen;
    const int code = column_code(op, p_in, t_in, p_in ? pattern[q] : 0u, t_in ? text[t] : 0u);
    if (code != AWV_VF_OK) return make_result(code, c, -1);
    if (op != prev) {
      penalty += run_end_cost(pen, prev, run_start, c);
      run_start = c;
      prev = op;
    }
    if (op == 'X') {
      penalty += pen.mismatch;
      ++nx;
    }
    q += takes_pattern(op);
    t += takes_text(op);
  }
  penalty += run_end_cost(pen, prev, run_start, n);
  return make_result(whole_code(claimed, n, plen, tlen, q, t, nx, penalty), -1, penalty);
}

using awvr::Span;  // (range_span.hpp: the rectangle of a range call's pair)

struct State;                    // verify.hip: the verify launches' device buffers, events and the last call's stats
void state_release(State* s);    // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);      // (nullptr: nothing)

// engine.hip's hook: checks one batch of awv_align_pairs_verified on the engine's stream.  `pairs`, `results`, `vout`: the
// batch's n entries (host); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it.  Adds to the stats the
// caller reset at the start of its call (stats_reset).  `spans` (nullable): the batch's rectangles of a range call.
int verify_batch(awv_engine* e, const awv_penalties* pen, const awv_pair* pairs, int64_t n, const awv_result* results,
                 const uint8_t* d_arena, uint64_t arena_bytes, awv_verify_result* vout, const Span* spans = nullptr);

}  // namespace awvf

// engine.hip
awvf::State*& awv_internal_verify(awv_engine* e);
uint64_t awv_internal_max_arena(const awv_engine* e);  // the CIGAR arena budget of a launch (awv_engine_config.max_arena_bytes or its default)
