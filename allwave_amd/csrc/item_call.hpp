// item_call.hpp -- a call on caller-supplied records with slices (awv_cs_cigars / _ranges and the same two of coverage, variants,
// lift and msa) resolved and checked before anything goes up: pure host code, no HIP, so a CPU program can run it
// (tests/item_call_driver.cpp).  Here are the rectangle of a pair call's record and ItemCall: the pairs (the caller's, or the ones
// made from ranges), the rectangles and the records with the slices applied (cs_slice.hpp), or the first refusal.
//
// The checks, in the order a caller can observe: every range or index of the whole list; then record by record the op bytes'
// place in the caller's arena and then the slice; the length limit on the sliced records comes last and apart (first_too_long),
// since a pass may have checks of its own before it.  Each refusal is AWV_ERR_ARG under the called function's name
// (record_pass.hpp's resolve_call makes the error of it).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "allwave_hip.h"
#include "cs_slice.hpp"       // slice_ok, apply_slice
#include "range_span.hpp"     // Span, split_range
#include "record_pieces.hpp"  // outside

namespace awvw {

using awvr::Span;

inline bool index_ok(const awv_pair& p, int32_t nseq) { return p.q_idx >= 0 && p.q_idx < nseq && p.t_idx >= 0 && p.t_idx < nseq; }
// the whole of both sequences: the rectangle of a pair call's record (len: the resident sequences' lengths)
inline Span whole_span(const int32_t* len, const awv_pair& p) { return Span{0, len[p.q_idx], 0, len[p.t_idx]}; }
// a rectangle as the kernels may take it: inside its sequences, an interval at most emptied by a slice's skip (pb = pe + 1)
inline bool rectangle_ok(const int32_t* len, const awv_pair& p, const Span& sp) {
  return sp.pb >= 0 && sp.tb >= 0 && sp.pe <= len[p.q_idx] && sp.te <= len[p.t_idx] && (int64_t)sp.pb <= (int64_t)sp.pe + 1 && (int64_t)sp.tb <= (int64_t)sp.te + 1;
}
// the first completed record of more than max_columns columns (-1: none): what a pass's 32-bit counts hold
inline int64_t first_too_long(const awv_result* recs, int64_t n, int64_t max_columns) {
  for (int64_t i = 0; i < n; ++i)
    if (recs[i].status == AWV_ST_COMPLETED && (int64_t)recs[i].cigar_len > max_columns) return i;
  return -1;
}

struct ItemCall {
  enum Refusal { NONE, RANGE, INDEX, ARENA, SLICE };

  ItemCall() = default;
  ItemCall(const ItemCall&) = delete;  // (pairs and recs may point into the object's own vectors)
  ItemCall& operator=(const ItemCall&) = delete;

  const awv_pair* pairs = nullptr;   // the caller's, or `rpairs`
  const awv_result* recs = nullptr;  // the caller's, or `sliced`
  std::vector<Span> spans;           // the records' rectangles, behind the slices' skips
  std::vector<awv_pair> rpairs;      // a range call's pairs
  std::vector<awv_result> sliced;    // a slice is an op string of its own: the records that go up name the slices
  Refusal refused = NONE;
  int64_t at = -1;  // the record the refusal names

  // ranges (nullable): the call is on ranges[0 .. n) and `pairs_in` is not read; slices: nullable.  len, nseq: the resident set.
  Refusal resolve(const int32_t* len, int32_t nseq, const awv_pair* pairs_in, const awv_range_pair* ranges, int64_t n, const awv_result* results,
                  uint64_t arena_bytes, const awv_cs_slice* slices) {
    const auto refuse = [&](Refusal why, int64_t i) {
      at = i;
      return refused = why;
    };
    spans.resize((size_t)n);
    if (ranges) {
      rpairs.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i)
        if (!awvr::split_range(len, nseq, ranges[i], rpairs[(size_t)i], spans[(size_t)i])) return refuse(RANGE, i);
      pairs_in = rpairs.data();
    } else {
      for (int64_t i = 0; i < n; ++i) {
        if (!index_ok(pairs_in[i], nseq)) return refuse(INDEX, i);
        spans[(size_t)i] = whole_span(len, pairs_in[i]);
      }
    }
    for (int64_t i = 0; i < n; ++i) {
      if (outside(results[i], arena_bytes)) return refuse(ARENA, i);
      if (slices && !awvcs::slice_ok(results[i], slices[i])) return refuse(SLICE, i);
    }
    if (slices) {
      sliced.assign(results, results + n);
      for (int64_t i = 0; i < n; ++i) awvcs::apply_slice(sliced[(size_t)i], spans[(size_t)i], slices[i]);
      results = sliced.data();
    }
    pairs = pairs_in;
    recs = results;
    return refused = NONE;
  }

  // the refusal in words, under the name of the called function
  std::string message(const char* who) const {
    const std::string head = std::string(who) + ": ";
    switch (refused) {
      case RANGE: return head + "range " + std::to_string(at) + " names a sequence index or an interval out of range";
      case INDEX: return head + "sequence index out of range";
      case ARENA: return head + "a record's op bytes lie outside the CIGAR arena";
      case SLICE: return head + "slice " + std::to_string(at) + " does not lie inside its op string, or skips a negative number of bases";
      default: return head + "no refusal";
    }
  }
};

}  // namespace awvw
