// coverage_device.hpp -- what one item adds to the per-base depth tracks (include/allwave_hip.h, above awv_coverage_one_host),
// once, for the host and the device: awv_coverage_one_host is cov_one below, and the coverage kernel (coverage.hip) decides an
// item's code, maps a pattern position to the query's forward strand and guards its slots with the same functions.
//
// The op string c[0 .. n) over M X I D aligns a pattern (the query, or its reverse complement) with a text (the target).  Column k
// sits at pattern position x = pb + q_skip + #(ops other than 'I' before k) and text position y = tb + t_skip + #(ops other than
// 'D' before k).  An 'M' or 'X' column adds 1 to `aligned` of the target's base y and of the query's forward-strand base
// (x, or len - 1 - x under q_revcomp); an 'M' column to `matched` as well.  An item adds everything or nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "allwave_hip.h"
#include "cs_device.hpp"  // is_op, whole_code's rule, slice_ok, apply_slice, drop_record, Span

struct awv_engine;

namespace awvcov {

using awvr::Span;

constexpr int64_t MAX_COLUMNS = awvcs::MAX_COLUMNS;  // of one string or slice: its counts then fit awv_cov_item's 32 bits
constexpr int64_t MAX_ITEMS = INT32_MAX;             // between two begins: an item adds at most 2 to a base's depth (a self pair, both roles)

__host__ __device__ inline bool roles_ok(int32_t roles) { return roles >= AWV_COV_TARGET && roles <= AWV_COV_BOTH; }

// what the totals of a string decide: the rule of the cs text (awvcs::whole_code), in this pass's codes
__host__ __device__ inline int whole_code(bool bad, int64_t q, int64_t t, int64_t plen, int64_t tlen) {
  const int c = awvcs::whole_code(bad, q, t, plen, tlen);
  return c == AWV_CST_OK ? AWV_CV_OK : c == AWV_CST_BAD_OP ? AWV_CV_BAD_OP : AWV_CV_LENGTHS;
}

__host__ __device__ inline awv_cov_item make_item(int32_t code, uint32_t aligned, uint32_t matched, uint32_t boundaries) {
  awv_cov_item it;
  it.code = code;
  it.aligned_cols = code == AWV_CV_OK ? aligned : 0u;
  it.matched_cols = code == AWV_CV_OK ? matched : 0u;
  it.boundaries = code == AWV_CV_OK ? boundaries : 0u;
  return it;
}

// the query's forward-strand base of pattern position x (qlen: the whole sequence's length)
__host__ __device__ inline int64_t query_base(bool revcomp, int64_t qlen, int64_t x) { return revcomp ? qlen - 1 - x : x; }
// A run of columns over pattern positions [x0, x1) is the forward-strand interval [len - x1, len - x0) of a reverse-complement
// query: a boundary at pattern position x is the difference slot len - x there, with the opposite sign.
__host__ __device__ inline int64_t query_slot(bool revcomp, int64_t qlen, int64_t x) { return revcomp ? qlen - x : x; }

// the guard of every store: base p of a sequence of len bases (difference slots: slot len, the interval end, included)
__host__ __device__ inline bool base_ok(int64_t p, int64_t len) { return p >= 0 && p < len; }
__host__ __device__ inline bool slot_ok(int64_t p, int64_t len) { return p >= 0 && p <= len; }

// The contract as a serial walk (the host yardstick): c[0 .. n), n <= MAX_COLUMNS, over the rectangle sp of a query of qlen and a
// target of tlen bases, from x = sp.pb + q_skip and y = sp.tb + t_skip on.  First the code, then -- only for AWV_CV_OK -- one add
// per contributing column into the depth tracks (a null track is not kept).
__host__ __device__ inline awv_cov_item cov_one(int32_t roles, bool revcomp, int64_t qlen, int64_t tlen, const Span& sp, const uint8_t* c, int64_t n,
                                                int64_t q_skip, int64_t t_skip, uint32_t* q_aligned, uint32_t* q_matched, uint32_t* t_aligned,
                                                uint32_t* t_matched) {
  bool bad = false;
  int64_t q = 0, t = 0;
  uint32_t aligned = 0, matched = 0, boundaries = 0;
  bool in_a = false, in_m = false;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    bad = bad || !awvcs::is_op(op);
    const bool a = op == 'M' || op == 'X', m = op == 'M';
    boundaries += (uint32_t)(a != in_a) + (uint32_t)(m != in_m);
    in_a = a;
    in_m = m;
    aligned += a;
    matched += m;
    q += op != 'I';
    t += op != 'D';
  }
  boundaries += (uint32_t)in_a + (uint32_t)in_m;  // the runs that end with the string
  const int code = whole_code(bad, q, t, (int64_t)sp.pe - sp.pb - q_skip, (int64_t)sp.te - sp.tb - t_skip);
  if (code != AWV_CV_OK) return make_item(code, 0, 0, 0);
  int64_t x = (int64_t)sp.pb + q_skip, y = (int64_t)sp.tb + t_skip;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    if (op == 'M' || op == 'X') {
      const int64_t f = query_base(revcomp, qlen, x);
      if ((roles & AWV_COV_TARGET) && base_ok(y, tlen)) {
        if (t_aligned) ++t_aligned[y];
        if (t_matched && op == 'M') ++t_matched[y];
      }
      if ((roles & AWV_COV_QUERY) && base_ok(f, qlen)) {
        if (q_aligned) ++q_aligned[f];
        if (q_matched && op == 'M') ++q_matched[f];
      }
    }
    x += op != 'I';
    y += op != 'D';
  }
  return make_item(AWV_CV_OK, aligned, matched, boundaries);
}

struct State;                  // coverage.hip: the accumulators, the pass's device buffers and the stats since begin
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
bool active(const State* s);   // between a begin with roles != 0 and the end of coverage

// engine.hip's hook: one batch of an aligning call, on the engine's stream, after the clip / split step.  `pairs`, `results`: the
// batch's n entries (host); `d_arena`: the batch's CIGAR arena on the device; clips (nullable): the batch's clips, whose slices
// contribute when their score reaches the begin's clip_min_score; seg_first / iout / sout (nullable): the call's split layout,
// seg_first and iout already offset to the batch, whose segments all contribute; spans (nullable): the batch's rectangles.
int coverage_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
                   const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans);

}  // namespace awvcov

// engine.hip
awvcov::State*& awv_internal_coverage(awv_engine* e);
bool& awv_internal_coverage_paused(awv_engine* e);  // set around the full strand alignments of an orientation call (orient.hip): they add nothing
