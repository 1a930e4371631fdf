// cs_device.hpp -- what the cs difference string of one op string is (include/allwave_hip.h, above awv_cs_one_host), once, for
// the host and the device: awv_cs_one_host is cs_one below, and the cs kernels (cs.hip) write the same items with the same
// functions.
//
// The op string c[0 .. n) over M X I D aligns a pattern (the query, or its reverse complement) with a text (the target); p and t
// are the pattern and text positions consumed so far.  Maximal runs of equal op bytes, left to right:
//   a run of L 'M'   short: ':' + L in decimal            long: '=' + upper(text[t .. t + L))         p and t advance by L
//   each 'X' column  '*' + lower(text[t]) + lower(pattern[p])   (target base first)                   both by 1
//   a run of L 'I'   '-' + lower(text[t .. t + L))        ('I' consumes the text)                     t by L
//   a run of L 'D'   '+' + lower(pattern[p .. p + L))     ('D' consumes the pattern)                  p by L
// An 'I' run directly followed by a 'D' run is two items.  Whether an 'M' column's bases are equal or an 'X' column's differ is
// not judged here (that is verification).  A slice of a string is an op string of its own that starts at p = q_skip,
// t = t_skip: a run that the slice cuts is cut.  No penalties.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "allwave_hip.h"
#include "encode_device.hpp"  // digits
#include "cs_slice.hpp"       // slice_ok, apply_slice
#include "range_span.hpp"

struct awv_engine;

namespace awvcs {

constexpr int64_t MAX_COLUMNS = (int64_t)1 << 30;  // of one string or slice: its text (at most three characters a column) then fits awv_cs_text.len

__host__ __device__ inline bool mode_ok(int32_t mode) { return mode == AWV_CS_SHORT || mode == AWV_CS_LONG; }
__host__ __device__ inline bool is_op(uint32_t op) { return op == 'M' || op == 'X' || op == 'I' || op == 'D'; }
__host__ __device__ inline uint32_t lower(uint32_t b) { return b >= 'A' && b <= 'Z' ? b + 32u : b; }
__host__ __device__ inline uint32_t upper(uint32_t b) { return b >= 'a' && b <= 'z' ? b - 32u : b; }

using awve::digits;  // decimal digits of a run length (>= 1, <= MAX_COLUMNS)

// the characters of a short-mode 'M' run: ':' and its length
__host__ __device__ inline uint32_t match_chars(uint32_t len) { return (uint32_t)digits(len) + 1u; }
// writes them at dst
__host__ __device__ inline void put_match(uint8_t* dst, uint32_t len) {
  const int nd = digits(len);
  dst[0] = ':';
  for (int k = nd; k >= 1; --k) {
    dst[k] = (uint8_t)('0' + len % 10u);
    len /= 10u;
  }
}
// the sign that opens a run of `op` other than 'X' (long mode's 'M' included)
__host__ __device__ inline uint32_t sign_of(uint32_t op) { return op == 'M' ? '=' : op == 'I' ? '-' : '+'; }
// the one base character a column of `op` other than 'X' owns: pb / tb are the pattern's and the text's base at the column
__host__ __device__ inline uint32_t base_char(uint32_t op, uint32_t pb, uint32_t tb) { return op == 'M' ? upper(tb) : op == 'I' ? lower(tb) : lower(pb); }

__host__ __device__ inline awv_cs_text make_text(uint64_t off, uint32_t len, int32_t code) {
  awv_cs_text t;
  t.off = off;
  t.len = len;
  t.code = code;
  return t;
}

// what the totals of a string decide: `bad` says a byte outside MXID was seen, q / t are the bases the string consumes, plen / tlen
// what is left of the two sequences behind the skips (negative: the skip alone is beyond the sequence)
__host__ __device__ inline int whole_code(bool bad, int64_t q, int64_t t, int64_t plen, int64_t tlen) {
  if (bad) return AWV_CST_BAD_OP;
  if (q > plen || t > tlen) return AWV_CST_LENGTHS;
  return AWV_CST_OK;
}

// The contract as a serial walk (the host yardstick): the text of c[0 .. n), n <= MAX_COLUMNS, over pattern[0 .. plen) and
// text[0 .. tlen), from p = q_skip and t = t_skip on.  The text is measured always and written to out[0 .. len) only when the
// code is AWV_CST_OK and it fits cap.
__host__ __device__ inline awv_cs_text cs_one(int32_t mode, const uint8_t* pattern, int64_t plen, const uint8_t* text, int64_t tlen, const uint8_t* c,
                                               int64_t n, int64_t q_skip, int64_t t_skip, uint8_t* out, uint64_t cap) {
  const bool is_long = mode == AWV_CS_LONG;
  bool bad = false;
  int64_t q = 0, t = 0;
  uint32_t len = 0;
  for (int64_t i = 0; i < n;) {
    int64_t j = i + 1;
    while (j < n && c[j] == c[i]) ++j;
    const uint32_t L = (uint32_t)(j - i), op = c[i];
    bad = bad || !is_op(op);
    len += op == 'X' ? 3u * L : op == 'M' && !is_long ? match_chars(L) : L + 1u;
    q += op != 'I' ? L : 0;
    t += op != 'D' ? L : 0;
    i = j;
  }
  const int code = whole_code(bad, q, t, plen - q_skip, tlen - t_skip);
  if (code != AWV_CST_OK) return make_text(0, 0, code);
  if ((uint64_t)len <= cap && out) {
    uint32_t w = 0;
    int64_t p = q_skip;
    t = t_skip;
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t op = c[i];
      const bool starts = i == 0 || c[i - 1] != op;
      if (op == 'X') {
        out[w++] = '*';
        out[w++] = (uint8_t)lower(text[t]);
        out[w++] = (uint8_t)lower(pattern[p]);
      } else if (op == 'M' && !is_long) {
        if (starts) {
          int64_t j = i + 1;
          while (j < n && c[j] == 'M') ++j;
          put_match(out + w, (uint32_t)(j - i));
          w += match_chars((uint32_t)(j - i));
        }
      } else {
        if (starts) out[w++] = (uint8_t)sign_of(op);
        out[w++] = (uint8_t)base_char(op, op != 'I' ? pattern[p] : 0u, op != 'D' ? text[t] : 0u);
      }
      p += op != 'I';
      t += op != 'D';
    }
  }
  return make_text(0, len, AWV_CST_OK);
}

// A record without a clip has no text (AWV_CST_SKIPPED): the kernels take it as one that is not completed.
inline void drop_record(awv_result& r) {
  if (r.status == AWV_ST_COMPLETED) r.status = AWV_ST_ABOVE_BOUND;
}

using awvr::Span;

struct State;                  // cs.hip: the cs launches' device buffers (the text among them), events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);    // (nullptr: nothing)

// engine.hip's hook: the cs text of one batch of awv_align_pairs_cs on the engine's stream, last of the record steps.  `pairs`,
// `results`, `csout`: the batch's n entries (host); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it; clips
// (nullable): the batch's clips, whose segments and skips are the slices (AWV_CST_SKIPPED for a code other than AWV_CL_OK);
// spans (nullable): the batch's rectangles of a range call.  csout comes back filled, relative to the batch's cs arena, which
// stays on the device: *text_bytes of it at batch_text().  Adds to the stats the caller reset at the start of its call.
int cs_batch(awv_engine* e, int32_t mode, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
             const awv_clip_result* clips, const Span* spans, awv_cs_text* csout, uint64_t* text_bytes);
const uint8_t* batch_text(awv_engine* e);  // the last cs_batch's text, on the device

}  // namespace awvcs

// engine.hip
awvcs::State*& awv_internal_cs(awv_engine* e);
uint64_t awv_internal_max_arena(const awv_engine* e);  // the CIGAR arena budget of a launch: awv_cs_cigars cuts its call by it
