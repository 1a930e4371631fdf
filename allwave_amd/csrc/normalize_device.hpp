// normalize_device.hpp -- what "normalized" means for one op string (include/allwave_hip.h, above awv_normalize_one_host),
// once, for the host and the device: awv_normalize_one_host is normalize_one below, and the normalize kernel
// (normalize.hip) applies the same functions to the runs a wave finds in its chunks.
//
// Left and right are one rule seen through a Frame: right-normalization is left-normalization of the reversed op string over
// the reversed sequences, so a frame maps a column k to n - 1 - k and a base i to len - 1 - i and everything else is shared.
// A gap run's final shift is s = min(a, b): b from shift_bound (the 'M' columns before it, plus what the run it is linked to
// has vacated), a the number of bases that agree between the run's own bases and the bases before them, compared no further
// than b.  Only the bytes that change are written: min(s, L) columns at the run's new start and as many at its old end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "allwave_hip.h"
#include "verify_device.hpp"  // awvf::is_gap, awvr::Span

struct awv_engine;

namespace awvn {

using awvf::is_gap;
using awvr::Span;

__host__ __device__ inline bool is_op(uint32_t op) { return op == 'M' || op == 'X' || op == 'I' || op == 'D'; }

__host__ __device__ inline awv_norm_result make_norm(int code, int32_t runs_moved, int64_t columns_moved, int32_t max_shift) {
  awv_norm_result r;
  r.code = code;
  r.runs_moved = runs_moved;
  r.columns_moved = columns_moved;
  r.max_shift = max_shift;
  r.reserved = 0;
  return r;
}

// The up-front code of a string whose bytes are all ops, from its counts of 'I' and 'D'.
__host__ __device__ inline int lengths_code(int64_t n, int64_t n_i, int64_t n_d, int32_t plen, int32_t tlen) {
  return n - n_i == (int64_t)plen && n - n_d == (int64_t)tlen ? AWV_NM_OK : AWV_NM_LENGTHS;
}

// b_i: how far run i may go at most.  m: the 'M' columns directly before it; linked: only those lie between it and the run
// before, whose type and final shift are prev_type / prev_s.
__host__ __device__ inline int64_t shift_bound(int64_t m, bool linked, uint32_t type, uint32_t prev_type, int64_t prev_s) {
  return linked ? m + prev_s - (type == prev_type ? 1 : 0) : m;
}

// one sequence seen from the left (mirror = false) or from the right
struct SeqFrame {
  const uint8_t* s;
  int32_t len;
  bool mirror;
  __host__ __device__ inline uint32_t at(int64_t i) const { return s[mirror ? (int64_t)len - 1 - i : i]; }
};

// The contract as a serial walk (the host yardstick): `in` and `out` hold n bytes each and may be the same array.  A zone only
// covers columns the walk has read already.
__host__ __device__ inline awv_norm_result normalize_one(bool mirror, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                                                         const uint8_t* in, int64_t n, uint8_t* out) {
  int64_t n_i = 0, n_d = 0;
  for (int64_t c = 0; c < n; ++c) {
    if (!is_op(in[c])) return make_norm(AWV_NM_BAD_OP, 0, c, 0);
    n_i += in[c] == 'I';
    n_d += in[c] == 'D';
  }
  if (lengths_code(n, n_i, n_d, plen, tlen) != AWV_NM_OK) return make_norm(AWV_NM_LENGTHS, 0, 0, 0);
  if (out != in)
    for (int64_t c = 0; c < n; ++c) out[c] = in[c];
  auto col = [&](int64_t k) { return mirror ? n - 1 - k : k; };
  const SeqFrame P{pattern, plen, mirror}, T{text, tlen, mirror};
  int64_t q = 0, t = 0, m = 0, prev_s = 0, moved = 0;
  int32_t runs_moved = 0, max_shift = 0;
  uint32_t prev_type = 0;
  bool linked = false;
  for (int64_t k = 0; k < n;) {
    const uint32_t op = in[col(k)];
    if (!is_gap(op)) {
      if (op == 'M') {
        ++m;
      } else {
        m = 0;
        linked = false;
      }
      ++q, ++t, ++k;
      continue;
    }
    int64_t L = 1;
    while (k + L < n && in[col(k + L)] == op) ++L;
    const SeqFrame& S = op == 'D' ? P : T;
    const int64_t p = op == 'D' ? q : t;
    int64_t cap = shift_bound(m, linked, op, prev_type, prev_s);
    if (cap > p) cap = p;  // (never binds: the columns a run passes consume its own sequence)
    if (cap > k) cap = k;
    int64_t s = 0;
    while (s < cap && S.at(p - 1 - s) == S.at(p + L - 1 - s)) ++s;
    if (s > 0) {
      const int64_t w = s < L ? s : L;
      for (int64_t i = 0; i < w; ++i) {  // (reads of `in` at or before k + L - 1 are done: k + L is the next column read)
        out[col(k - s + i)] = (uint8_t)op;
        out[col(k + L - w + i)] = 'M';
      }
      ++runs_moved;
      moved += s;
      if (s > max_shift) max_shift = (int32_t)s;
    }
    prev_type = op;
    prev_s = s;
    m = 0;
    linked = true;
    (op == 'D' ? q : t) += L;
    k += L;
  }
  return make_norm(AWV_NM_OK, runs_moved, moved, max_shift);
}

struct State;                  // normalize.hip: the launches' device buffers, events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);    // (nullptr: nothing)

// the resident copies a launch reads: the engine's own set, or awv_align_one's temporary one
struct SeqView {
  int32_t n;
  const uint8_t* fwd;     // device
  const uint8_t* rc;      // device
  const uint64_t* off;    // device
  const int32_t* len;     // device
};

// engine.hip's hook: normalizes one batch of an aligning call in place on the engine's stream.  `results`: the batch's n
// records (host); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it; spans: nullable (range calls).
// Adds to the stats the caller reset at the start of its call (stats_reset).
int normalize_batch(awv_engine* e, const SeqView& seqs, int32_t direction, const awv_pair* pairs, int64_t n, const awv_result* results,
                    uint8_t* d_arena, uint64_t arena_bytes, const Span* spans);

}  // namespace awvn

// engine.hip
awvn::State*& awv_internal_normalize(awv_engine* e);
int32_t& awv_internal_normalize_mode(awv_engine* e);
