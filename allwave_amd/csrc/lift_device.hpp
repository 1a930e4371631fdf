// lift_device.hpp -- what the lift of one interval through one item is (include/allwave_hip.h, above awv_lift_one_host), once, for
// the host and the device: awv_lift_one_host is lift_one below, and the lift kernel (lift.hip) finds the same two columns with its
// probes and makes the result with the same compose().
//
// The op string c[0 .. n) over M X I D aligns a pattern (the query, or its reverse complement) with a text (the target).  Column k
// sits at pattern position x = pb + q_skip + #(ops other than 'I' before k) and text position y = tb + t_skip + #(ops other than
// 'D' before k).  The interval [a, b) of the source (the text under AWV_LIFT_FROM_TARGET, the pattern under AWV_LIFT_FROM_QUERY)
// is lifted to its aligned core: from the first 'M' / 'X' column at or after a to the last one before b.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "allwave_hip.h"
#include "cs_device.hpp"  // is_op, whole_code's rule, slice_ok, apply_slice, Span

struct awv_engine;

namespace awvl {

using awvr::Span;

constexpr int64_t MAX_COLUMNS = awvcs::MAX_COLUMNS;  // of one string or slice: every count and column then fits 32 bits
constexpr int64_t MAX_QUERIES = ((int64_t)1 << 30) - 1;  // of one call: two probes a query, indexed with 31 bits

__host__ __device__ inline bool from_ok(int32_t from) { return from == AWV_LIFT_FROM_TARGET || from == AWV_LIFT_FROM_QUERY; }

// what the totals of a string decide: the rule of the cs text (awvcs::whole_code), in this pass's codes
__host__ __device__ inline int whole_code(bool bad, int64_t q, int64_t t, int64_t plen, int64_t tlen) {
  const int c = awvcs::whole_code(bad, q, t, plen, tlen);
  return c == AWV_CST_OK ? AWV_LF_OK : c == AWV_CST_BAD_OP ? AWV_LF_BAD_OP : AWV_LF_LENGTHS;
}

// a result that is its code alone
__host__ __device__ inline awv_lift_result make_code(int32_t code) {
  awv_lift_result r;
  r.code = code;
  r.reserved = 0;
  r.col_beg = r.col_end = 0u;
  r.q_skip = r.t_skip = 0;
  r.src_beg = r.src_end = r.dst_beg = r.dst_end = 0;
  r.num_matches = r.num_mismatches = r.num_ins = r.num_del = 0;
  return r;
}

// [beg, end) on the source's forward strand in the item's own coordinates: the text's are the target's; the pattern of a
// q_revcomp pair runs the other way
__host__ __device__ inline void to_item(int32_t from, bool revcomp, int64_t qlen, int64_t beg, int64_t end, int64_t& a, int64_t& b) {
  const bool turn = from == AWV_LIFT_FROM_QUERY && revcomp;
  a = turn ? qlen - end : beg;
  b = turn ? qlen - beg : end;
}

// A column of the string (of the item: 0 is its first) and the op bytes of each kind before it: what a probe answers.
struct Prefix {
  uint32_t col, m, x, i, d;
};

// The result from the two columns.  item_code: what the whole string decided; sp: the item's rectangle, behind its skips; base: the
// item's own slice of its record's string (zero: the whole string); consumed: the source bases the string consumes; [a, b): the
// interval in the item's coordinates (to_item); pb: col_beg and the counts before it; pe: col_end and the counts before it.
__host__ __device__ inline awv_lift_result compose(int32_t item_code, int32_t from, bool revcomp, int64_t qlen, const Span& sp, const awv_cs_slice& base,
                                                   int64_t consumed, int64_t a, int64_t b, const Prefix& pb, const Prefix& pe) {
  if (item_code != AWV_LF_OK) return make_code(item_code);
  const int64_t s0 = from == AWV_LIFT_FROM_TARGET ? sp.tb : sp.pb;
  const int64_t lo = a > s0 ? a : s0, hi = b < s0 + consumed ? b : s0 + consumed;
  if (lo >= hi) return make_code(AWV_LF_OUTSIDE);
  if (pb.col >= pe.col) return make_code(AWV_LF_UNALIGNED);
  awv_lift_result r = make_code(AWV_LF_OK);
  r.col_beg = base.col_beg + pb.col;
  r.col_end = base.col_beg + pe.col;
  const int64_t qb = (int64_t)pb.m + pb.x + pb.d, tb = (int64_t)pb.m + pb.x + pb.i;  // bases consumed before col_beg
  const int64_t qe = (int64_t)pe.m + pe.x + pe.d, te = (int64_t)pe.m + pe.x + pe.i;  // ... before col_end
  r.q_skip = (int32_t)(base.q_skip + qb);
  r.t_skip = (int32_t)(base.t_skip + tb);
  const int64_t x0 = sp.pb + qb, x1 = sp.pb + qe;  // the pattern interval; forward strand: turned back
  const int32_t q_beg = (int32_t)(revcomp ? qlen - x1 : x0), q_end = (int32_t)(revcomp ? qlen - x0 : x1);
  const int32_t t_beg = (int32_t)(sp.tb + tb), t_end = (int32_t)(sp.tb + te);
  const bool from_t = from == AWV_LIFT_FROM_TARGET;
  r.src_beg = from_t ? t_beg : q_beg;
  r.src_end = from_t ? t_end : q_end;
  r.dst_beg = from_t ? q_beg : t_beg;
  r.dst_end = from_t ? q_end : t_end;
  r.num_matches = (int32_t)(pe.m - pb.m);
  r.num_mismatches = (int32_t)(pe.x - pb.x);
  r.num_ins = (int32_t)(pe.i - pb.i);
  r.num_del = (int32_t)(pe.d - pb.d);
  return r;
}

// The contract as a serial walk (the host yardstick): c[0 .. n), n <= MAX_COLUMNS, over the rectangle sp (behind the skips) of a
// query of qlen bases; [beg, end) on the source's forward strand.
__host__ __device__ inline awv_lift_result lift_one(int32_t from, bool revcomp, int64_t qlen, const Span& sp, const uint8_t* c, int64_t n,
                                                    const awv_cs_slice& base, int64_t beg, int64_t end) {
  int64_t a, b;
  to_item(from, revcomp, qlen, beg, end, a, b);
  const bool from_t = from == AWV_LIFT_FROM_TARGET;
  bool bad = false, have_beg = false;
  Prefix cnt{0u, 0u, 0u, 0u, 0u}, pb{0u, 0u, 0u, 0u, 0u}, pe{0u, 0u, 0u, 0u, 0u};
  int64_t x = sp.pb, y = sp.tb;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    bad = bad || !awvcs::is_op(op);
    const int64_t src = from_t ? y : x;
    if (op == 'M' || op == 'X') {
      if (!have_beg && src >= a) {
        pb = cnt;
        pb.col = (uint32_t)k;
        have_beg = true;
      }
      if (src < b) {
        pe = cnt;
        pe.col = (uint32_t)k + 1u;
        pe.m += op == 'M';
        pe.x += op == 'X';
      }
    }
    cnt.m += op == 'M';
    cnt.x += op == 'X';
    cnt.i += op == 'I';
    cnt.d += op == 'D';
    x += op != 'I';
    y += op != 'D';
  }
  if (!have_beg) {
    pb = cnt;
    pb.col = (uint32_t)n;
  }
  const int64_t q = x - sp.pb, t = y - sp.tb;
  const int code = whole_code(bad, q, t, (int64_t)sp.pe - sp.pb, (int64_t)sp.te - sp.tb);
  return compose(code, from, revcomp, qlen, sp, base, from_t ? t : q, a, b, pb, pe);
}

// the total order of the table's rows: all fields in their order, region first
__host__ __device__ inline bool row_less(const awv_lift_row& p, const awv_lift_row& q) {
  const int32_t u[12] = {p.region, p.q_idx, p.t_idx, p.flags, p.src_beg, p.src_end, p.dst_beg, p.dst_end, p.num_matches, p.num_mismatches, p.num_ins, p.num_del};
  const int32_t w[12] = {q.region, q.q_idx, q.t_idx, q.flags, q.src_beg, q.src_end, q.dst_beg, q.dst_end, q.num_matches, q.num_mismatches, q.num_ins, q.num_del};
  for (int k = 0; k < 12; ++k)
    if (u[k] != w[k]) return u[k] < w[k];
  return false;
}

struct State;                  // lift.hip: the regions and the rows of a table, the pass's device buffers and the stats since begin
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
bool active(const State* s);   // between a begin with from_mask != 0 and the end of the table

// engine.hip's hook: one batch of an aligning call, on the engine's stream, after the clip / split step; the arguments are
// awvcov::coverage_batch's.
int lift_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
               const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans);

}  // namespace awvl

// engine.hip
awvl::State*& awv_internal_lift(awv_engine* e);
