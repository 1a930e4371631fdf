// cs_slice.hpp -- the two rules of a slice of an op string (awv_cs_slice; include/allwave_hip.h above awv_cs_one_host), for every
// pass that takes slices and for the host prologue of their calls (item_call.hpp): pure host code, no HIP.
#pragma once

#include <algorithm>
#include <cstdint>

#include "allwave_hip.h"
#include "range_span.hpp"

namespace awvcs {

// a slice that lies inside a record's op string and skips no negative number of bases (a record that is not completed has no
// string: any columns will do)
inline bool slice_ok(const awv_result& r, const awv_cs_slice& s) {
  if (s.q_skip < 0 || s.t_skip < 0) return false;
  return r.status != AWV_ST_COMPLETED || (s.col_beg <= s.col_end && s.col_end <= r.cigar_len);
}
// A slice is an op string of its own: the record as the kernels take it names the slice's bytes, and the rectangle begins behind
// the skips (a skip beyond its sequence leaves a rectangle of negative length: AWV_CST_LENGTHS).
inline void apply_slice(awv_result& r, awvr::Span& sp, const awv_cs_slice& s) {
  if (r.status != AWV_ST_COMPLETED) return;
  r.cigar_off += s.col_beg;
  r.cigar_len = s.col_end - s.col_beg;
  sp.pb = (int32_t)std::min<int64_t>((int64_t)sp.pb + s.q_skip, (int64_t)sp.pe + 1);
  sp.tb = (int32_t)std::min<int64_t>((int64_t)sp.tb + s.t_skip, (int64_t)sp.te + 1);
}

}  // namespace awvcs
