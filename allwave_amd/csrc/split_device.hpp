// split_device.hpp -- what "split" means for one op string (include/allwave_hip.h, above awv_split_slots), once, for the host
// and the device: awv_split_one_host is split_one below, the recursion over clip_one (clip_device.hpp) with an explicit stack;
// the split kernel (split.hip) walks the same intervals with the clip kernel's wave scan in clip_one's place.
#pragma once

#include "clip_device.hpp"

namespace awvs {

// A pending interval [lo, hi) of the op string and the pattern / text bases consumed before column lo.
struct Interval {
  uint32_t lo, hi, q_before, t_before;
};

// floor(a * m / min_score): each segment holds at least ceil(min_score / a) 'M' columns.  a <= 32767 and m < 2^32 for an op
// string, so the product fits; a caller's m beyond that saturates instead of wrapping.
__host__ __device__ inline int64_t slots(int64_t a, int64_t min_score, int64_t m) {
  if (a < 1 || a > AWV_CLIP_MAX_BONUS || min_score < 1 || m < 0) return -1;
  if (m > INT64_MAX / a) return INT64_MAX / min_score;
  return a * m / min_score;
}

// An interval can hold a segment only when all its columns as matches would reach min_score.
__host__ __device__ inline bool worth(int64_t a, int64_t min_score, uint32_t lo, uint32_t hi) {
  return hi > lo && a * (int64_t)(hi - lo) >= min_score;
}

// The clip of c[lo..hi) as a segment of the whole string.
__host__ __device__ inline awv_clip_result lift(awv_clip_result r, const Interval& iv) {
  r.col_beg += iv.lo;
  r.col_end += iv.lo;
  r.q_skip += (int32_t)iv.q_before;
  r.t_skip += (int32_t)iv.t_before;
  return r;
}

// The contract (the host yardstick): segments(0, n), as a depth-first walk with an explicit stack -- after an interval's clip
// the right remainder waits on the stack while the left one is walked, so the stack holds at most one interval per segment
// found (`stack`: room for min(slots, n) + 1).  The segments are written as they are found, the first `cap` of them, and put
// into ascending col_beg at the end; the returned count is that of ALL segments found.
__host__ __device__ inline awv_split_index split_one(const awv_penalties& pen, int64_t a, int64_t min_score, const uint8_t* cigar, int64_t n,
                                                     awv_clip_result* sout, int64_t cap, Interval* stack) {
  awv_split_index ix;
  ix.code = AWV_CL_EMPTY;
  ix.count = 0;
  ix.column = -1;
  int64_t sp = 0, count = 0;
  Interval cur{0, (uint32_t)n, 0, 0};
  bool have = n > 0, first = true;
  for (;;) {
    if (!have) {
      if (sp == 0) break;
      cur = stack[--sp];
    }
    have = false;
    const awv_clip_result r = awvc::clip_one(pen, a, cigar + cur.lo, (int64_t)cur.hi - cur.lo);
    if (first && r.code == AWV_CL_BAD_OP) {  // the first scan covers the whole string: this is the clip's answer
      ix.code = AWV_CL_BAD_OP;
      ix.column = (int64_t)r.col_beg;
      return ix;
    }
    first = false;
    if (r.code != AWV_CL_OK || r.score < min_score) continue;
    if (count < cap) sout[count] = lift(r, cur);
    ++count;
    const uint32_t b = cur.lo + r.col_beg, e = cur.lo + r.col_end, cols = r.col_end - r.col_beg;
    const Interval right{e, cur.hi, cur.q_before + (uint32_t)r.q_skip + cols - (uint32_t)r.num_ins,
                         cur.t_before + (uint32_t)r.t_skip + cols - (uint32_t)r.num_del};
    if (right.hi > right.lo) stack[sp++] = right;
    if (b > cur.lo) {
      cur = Interval{cur.lo, b, cur.q_before, cur.t_before};
      have = true;
    }
  }
  const int64_t w = count < cap ? count : cap;
  for (int64_t i = 1; i < w; ++i) {  // insertion sort: the walk leaves runs that are nearly in order
    const awv_clip_result v = sout[i];
    int64_t k = i;
    for (; k > 0 && sout[k - 1].col_beg > v.col_beg; --k) sout[k] = sout[k - 1];
    sout[k] = v;
  }
  ix.count = (int32_t)count;
  ix.code = count > 0 ? AWV_CL_OK : AWV_CL_EMPTY;
  return ix;
}

struct State;                  // split.hip: the split launches' device buffers, events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);    // (nullptr: nothing)

// engine.hip's hook: splits one batch of awv_align_*_split on the engine's stream.  `results`, `iout`: the batch's n entries
// (host); seg_first: the batch's n + 1 entries of the call's layout; sout: the call's segment storage (record i's slots are
// sout[seg_first[i] ..)); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it.
int split_batch(awv_engine* e, const awv_penalties* pen, int32_t match_bonus, int64_t min_score, int64_t n, const awv_result* results,
                const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* seg_first, awv_split_index* iout, awv_clip_result* sout);

}  // namespace awvs

// engine.hip
awvs::State*& awv_internal_split(awv_engine* e);
