// encode_device.hpp -- what the run-length text of one op string is (include/allwave_hip.h, above awv_encode_one_host), once,
// for the host and the device: awv_encode_one_host is encode_one below, and the encode kernels (encode.hip) put the same
// runs through the same put_run.
//
// Every maximal run of equal bytes becomes its length in decimal and one character: 'M' -> '=', 'X' -> 'X', 'I' -> 'D',
// 'D' -> 'I' (the reference's cigar_bytes_to_string, which swaps the gap letters), any other byte -> '?'.  A slice of a string is
// encoded as a string of its own: a run that the slice cuts is cut.  Needs no sequence and no penalties.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "allwave_hip.h"

struct awv_engine;

namespace awve {

constexpr int64_t MAX_COLUMNS = INT32_MAX;  // of one string or slice: its text (at most two characters a column) then fits awv_cigar_text.len

__host__ __device__ inline uint8_t op_char(uint32_t op) { return op == 'M' ? '=' : op == 'X' ? 'X' : op == 'I' ? 'D' : op == 'D' ? 'I' : '?'; }

// decimal digits of a run length (>= 1)
__host__ __device__ inline int digits(uint32_t len) {
  return len < 10u ? 1 : len < 100u ? 2 : len < 1000u ? 3 : len < 10000u ? 4 : len < 100000u ? 5 : len < 1000000u ? 6 : len < 10000000u ? 7 : len < 100000000u ? 8
       : len < 1000000000u ? 9 : 10;
}

// the characters one run takes
__host__ __device__ inline uint32_t run_chars(uint32_t len) { return (uint32_t)digits(len) + 1u; }

// writes a run's run_chars(len) characters at dst
__host__ __device__ inline void put_run(uint8_t* dst, uint32_t len, uint32_t op) {
  const int nd = digits(len);
  dst[nd] = op_char(op);
  for (int k = nd - 1; k >= 0; --k) {
    dst[k] = (uint8_t)('0' + len % 10u);
    len /= 10u;
  }
}

__host__ __device__ inline awv_cigar_text make_text(uint64_t off, uint32_t len, uint32_t runs) {
  awv_cigar_text t;
  t.off = off;
  t.len = len;
  t.runs = runs;
  return t;
}

// The contract as a serial walk (the host yardstick): the text of c[0 .. n), n <= MAX_COLUMNS.  The text is measured always
// and written to out[0 .. len) only when it fits cap.
__host__ __device__ inline awv_cigar_text encode_one(const uint8_t* c, int64_t n, uint8_t* out, uint64_t cap) {
  uint32_t len = 0, runs = 0;
  for (int64_t i = 0; i < n;) {
    int64_t j = i + 1;
    while (j < n && c[j] == c[i]) ++j;
    len += run_chars((uint32_t)(j - i));
    ++runs;
    i = j;
  }
  if ((uint64_t)len <= cap && out) {
    uint32_t w = 0;
    for (int64_t i = 0; i < n;) {
      int64_t j = i + 1;
      while (j < n && c[j] == c[i]) ++j;
      put_run(out + w, (uint32_t)(j - i), c[i]);
      w += run_chars((uint32_t)(j - i));
      i = j;
    }
  }
  return make_text(0, len, runs);
}

struct Slice {  // awv_encode_cigars' slices: columns [col_beg, col_end) of a record's op string
  uint32_t col_beg, col_end;
};
// a slice that lies inside a record's op string (a record that is not completed has no string: any slice will do)
inline bool slice_ok(const awv_result& r, uint32_t col_beg, uint32_t col_end) {
  return r.status != AWV_ST_COMPLETED || (col_beg <= col_end && col_end <= r.cigar_len);
}
// A slice is an op string of its own: the record as the kernels take it names the slice's bytes.
inline void apply_slice(awv_result& r, uint32_t col_beg, uint32_t col_end) {
  if (r.status != AWV_ST_COMPLETED) return;
  r.cigar_off += col_beg;
  r.cigar_len = col_end - col_beg;
}

struct State;                  // encode.hip: the encode launches' device buffers (the text among them), events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
void stats_reset(State* s);    // (nullptr: nothing)

// engine.hip's hook: encodes one batch of awv_align_pairs_encoded on the engine's stream, last of the record steps.  `results`,
// `tout`: the batch's n entries (host); `d_arena`: the batch's CIGAR arena on the device, `arena_bytes` of it; clips (nullable):
// the batch's clips, whose segments are the slices to encode (no text for a code other than AWV_CL_OK).  tout comes back filled,
// relative to the batch's text arena, which stays on the device: *text_bytes of it at batch_text().  Adds to the stats the
// caller reset at the start of its call (stats_reset).
int encode_batch(awv_engine* e, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes, const awv_clip_result* clips,
                 awv_cigar_text* tout, uint64_t* text_bytes);
const uint8_t* batch_text(awv_engine* e);  // the last encode_batch's text, on the device

}  // namespace awve

// engine.hip
awve::State*& awv_internal_encode(awv_engine* e);
uint64_t awv_internal_max_arena(const awv_engine* e);  // the CIGAR arena budget of a launch: awv_encode_cigars cuts its call by it
