// variants.hip -- the alleles of all alignments per target site: the host yardsticks awv_variants_one_host and
// awv_variants_fold_host (include/allwave_hip.h).  Which events an item carries and how they fold is variants_device.hpp, whose hash,
// combine and key order are __host__ __device__ for the device pass that is to tally the same table.
#include "variants_device.hpp"

#include <string>

#include "planner_device.hpp"  // awv_internal_fail

extern "C" {

int awv_variants_one_host(int32_t q_idx, int32_t t_idx, int32_t q_revcomp, const uint8_t* pattern, int32_t qlen, int32_t tlen, int32_t pb, int32_t pe, int32_t tb,
                          int32_t te, const uint8_t* cigar, int64_t n, const awv_cs_slice* slice, awv_variant* events, uint64_t cap, uint64_t* n_events,
                          awv_var_item* out) {
  if (!out || !n_events || q_idx < 0 || t_idx < 0 || qlen < 0 || tlen < 0 || n < 0 || (qlen > 0 && !pattern) || (n > 0 && !cigar) || (cap > 0 && !events))
    return awv_internal_fail(AWV_ERR_ARG, "variants_one_host: bad argument");
  if (pb < 0 || pb > pe || pe > qlen || tb < 0 || tb > te || te > tlen) return awv_internal_fail(AWV_ERR_ARG, "variants_one_host: an interval outside its sequence");
  int64_t beg = 0, end = n, q_skip = 0, t_skip = 0;
  if (slice) {
    if (slice->col_beg > slice->col_end || (int64_t)slice->col_end > n || slice->q_skip < 0 || slice->t_skip < 0)
      return awv_internal_fail(AWV_ERR_ARG, "variants_one_host: the slice does not lie inside the op string, or skips a negative number of bases");
    beg = slice->col_beg;
    end = slice->col_end;
    q_skip = slice->q_skip;
    t_skip = slice->t_skip;
  }
  if (end - beg > awvvar::MAX_COLUMNS) return awv_internal_fail(AWV_ERR_ARG, "variants_one_host: an op string of more than 2^30 columns");
  *out = awvvar::var_one(q_idx, t_idx, q_revcomp != 0, pattern, awvvar::Span{pb, pe, tb, te}, cigar + beg, end - beg, q_skip, t_skip, events, cap, n_events);
  return AWV_OK;
}

int awv_variants_fold_host(awv_variant* rows, uint64_t n, uint64_t* n_rows) {
  if (!n_rows || (n > 0 && !rows)) return awv_internal_fail(AWV_ERR_ARG, "variants_fold_host: null argument");
  *n_rows = awvvar::fold_rows(rows, n);
  return AWV_OK;
}

}  // extern "C"
