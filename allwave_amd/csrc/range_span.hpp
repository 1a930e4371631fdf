// range_span.hpp -- the rectangle a range call (awv_align_ranges, awv_score_ranges, awv_verify_ranges; include/allwave_hip.h)
// aligns of one pair, as the engine's host side builds it and the alignment and verify kernels read it.
#pragma once

#include <cstdint>

#include "allwave_hip.h"

namespace awvr {

// pattern[pb, pe) against text[tb, te), in pattern / text coordinates: the pattern's are those of the reverse-complement copy
// for a q_revcomp pair.  One 16-byte load on the device.
struct alignas(16) Span { int32_t pb, pe, tb, te; };

// awv_range_pair -> (pair, span), validated against the resident set's lengths: false (and nothing is launched by the caller)
// for an index out of range or an interval outside its sequence.  The one place the forward-strand query interval of a
// q_revcomp range is mapped onto the reverse-complement copy.
inline bool split_range(const int32_t* len, int32_t nseq, const awv_range_pair& r, awv_pair& pair, Span& span) {
  if (r.q_idx < 0 || r.q_idx >= nseq || r.t_idx < 0 || r.t_idx >= nseq) return false;
  const int32_t ql = len[r.q_idx], tl = len[r.t_idx];
  if (r.q_beg < 0 || r.q_beg > r.q_end || r.q_end > ql || r.t_beg < 0 || r.t_beg > r.t_end || r.t_end > tl) return false;
  pair = awv_pair{r.q_idx, r.t_idx, r.q_revcomp ? 1 : 0};
  span = r.q_revcomp ? Span{ql - r.q_end, ql - r.q_beg, r.t_beg, r.t_end} : Span{r.q_beg, r.q_end, r.t_beg, r.t_end};
  return true;
}

}  // namespace awvr
