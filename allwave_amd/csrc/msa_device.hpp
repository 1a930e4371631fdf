// msa_device.hpp -- what a target-anchored multiple alignment is (include/allwave_hip.h, above awv_msa_host), once, for the host
// and the device: awv_msa_host is msa_target below, and the kernels (msa.hip) decide an item's code, guard their slots, place an
// insertion's bases and close an item's column interval with the same functions.
//
// The op string c[0 .. n) over M X I D aligns a pattern (the query, or its reverse complement) with a text (the target).  Column k
// sits at pattern position x = pb + q_skip + #(ops other than 'I' before k) and text position y = tb + t_skip + #(ops other than
// 'D' before k).  The 'D' columns at one text position y are one run; the widest run of any sound item at y is ins[y], the
// columns are col[p] = p + the sum of ins[0 .. p], and an item's bases go to col[y] ('M', 'X') or col[y] - ins[y] + j (the j-th
// 'D' of its run).  An item widens and places everything or nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "allwave_hip.h"
#include "cs_device.hpp"  // is_op, upper, whole_code's rule, slice_ok, apply_slice, Span

struct awv_engine;

namespace awvmsa {

using awvr::Span;

constexpr int64_t MAX_COLUMNS = awvcs::MAX_COLUMNS;  // of one string or slice: its counts then fit 32 bits

// what the totals of a string decide: the rule of the cs text (awvcs::whole_code), in this pass's codes
__host__ __device__ inline int whole_code(bool bad, int64_t q, int64_t t, int64_t plen, int64_t tlen) {
  const int c = awvcs::whole_code(bad, q, t, plen, tlen);
  return c == AWV_CST_OK ? AWV_MS_OK : c == AWV_CST_BAD_OP ? AWV_MS_BAD_OP : AWV_MS_LENGTHS;
}

// the guard of every store into a target's slots (slot len, behind the last base, included) and of every read of a base
__host__ __device__ inline bool slot_ok(int64_t p, int64_t len) { return p >= 0 && p <= len; }
__host__ __device__ inline bool base_ok(int64_t p, int64_t len) { return p >= 0 && p < len; }

// the column of the j-th 'D' of a run at a slot whose base column is col_y and whose width is ins_y: left-justified
__host__ __device__ inline int64_t ins_column(int64_t col_y, int64_t ins_y, int64_t j) { return col_y - ins_y + j; }

// What the walk leaves of a sound item for its column interval: the text positions of its first and last column other than 'I'
// (everything before the first and behind the last is 'I', so they follow from the columns' indices), and how the two ends look.
struct Ends {
  int32_t y_first, y_last;  // (undefined when any == 0)
  int32_t first_is_d;       // the first such column is a 'D': the row begins at its slot's first insertion column
  int32_t last_run;         // the last such column is a 'D', the last of a run of this many; 0: it is an 'M' or 'X'
  int32_t any;              // the item has a column other than 'I'
  int32_t reserved;
};
// kf, kl: the indices of the first and last column other than 'I' (kf < 0: none); y0: the text position of column 0; t: the text
// bases the string consumes
__host__ __device__ inline Ends make_ends(int64_t kf, int64_t kl, bool first_is_d, int64_t last_run, int64_t n, int64_t y0, int64_t t) {
  Ends e{0, 0, 0, 0, 0, 0};
  if (kf < 0) return e;
  e.any = 1;
  e.y_first = (int32_t)(y0 + kf);
  e.y_last = (int32_t)(y0 + t - (n - 1 - kl) - (last_run > 0 ? 0 : 1));
  e.first_is_d = first_is_d;
  e.last_run = (int32_t)last_run;
  return e;
}
// the item's first and one-past-last non-gap column: col, ins are the target's own slots
__host__ __device__ inline void item_columns(const Ends& e, const uint64_t* col, const uint32_t* ins, int64_t tlen, int64_t& beg, int64_t& end) {
  beg = end = 0;
  if (!e.any || !slot_ok(e.y_first, tlen) || !slot_ok(e.y_last, tlen)) return;
  beg = e.first_is_d ? ins_column((int64_t)col[e.y_first], ins[e.y_first], 0) : (int64_t)col[e.y_first];
  end = e.last_run > 0 ? ins_column((int64_t)col[e.y_last], ins[e.y_last], e.last_run) : (int64_t)col[e.y_last] + 1;
}

__host__ __device__ inline awv_msa_item make_item(int32_t code, int32_t target, uint32_t bases) {
  awv_msa_item it;
  it.code = code;
  it.target = target;
  it.row = 0;
  it.bases = code == AWV_MS_OK ? bases : 0u;
  it.col_beg = it.col_end = 0;
  return it;
}

// ---- the contract as serial walks (the host yardstick) -----------------------------------------------------------------------

// the code of c[0 .. n) over what is left of the rectangle behind the skips; *bases: the pattern bases it consumes
__host__ __device__ inline int code_one(const uint8_t* c, int64_t n, int64_t plen, int64_t tlen, uint32_t* bases) {
  bool bad = false;
  int64_t q = 0, t = 0;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    bad = bad || !awvcs::is_op(op);
    q += op != 'I';
    t += op != 'D';
  }
  *bases = (uint32_t)q;
  return whole_code(bad, q, t, plen, tlen);
}

// a sound item widens: ins[y] = max(ins[y], the 'D' columns at y), y from y0 on; returns its 'D' runs
__host__ __device__ inline uint64_t widen_one(const uint8_t* c, int64_t n, int64_t y0, int64_t tlen, uint32_t* ins) {
  uint64_t runs = 0;
  int64_t y = y0, run = 0;
  for (int64_t k = 0; k <= n; ++k) {
    const uint32_t op = k < n ? c[k] : 0u;
    if (op == 'D') {
      ++run;
      continue;
    }
    if (run > 0) {  // the column that ends the run, or the string's end
      if (slot_ok(y, tlen) && ins[y] < (uint32_t)run) ins[y] = (uint32_t)run;
      ++runs;
      run = 0;
    }
    ++y;
  }
  return runs;
}

// a sound item's row: row[0 .. W) of the block, over col / ins of its target; x0, y0 the positions of column 0
__host__ __device__ inline void place_one(const uint8_t* c, int64_t n, const uint8_t* pattern, int64_t plen, int64_t x0, int64_t y0, int64_t tlen,
                                          const uint64_t* col, const uint32_t* ins, uint8_t* row, int64_t W) {
  int64_t x = x0, y = y0, j = 0;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    j = op == 'D' ? j : 0;
    if (op != 'I' && base_ok(x, plen) && slot_ok(y, tlen)) {
      const int64_t at = op == 'D' ? ins_column((int64_t)col[y], ins[y], j) : (int64_t)col[y];
      if (at >= 0 && at < W && (op == 'D' || y < tlen)) row[at] = (uint8_t)awvcs::upper(pattern[x]);
    }
    j += op == 'D';
    x += op != 'I';
    y += op != 'D';
  }
}

// One item of the yardstick: c[0 .. n) is the slice's own bytes (n < 0: a record that is not completed), sp the rectangle before the skips
struct HostItem {
  const uint8_t* pattern;
  int64_t plen;
  Span sp;
  const uint8_t* c;
  int64_t n, q_skip, t_skip;
};
// One target's items, whole (awv_msa_host behind its argument checks): ins[0 .. tlen], *width, codes[0 .. n) and *block_bytes always;
// block[0 .. *block_bytes) only when it fits cap.
inline void msa_target(const uint8_t* text, int64_t tlen, const HostItem* it, int64_t n, uint32_t* ins, int64_t* width, int32_t* codes, uint8_t* block,
                       uint64_t cap, uint64_t* block_bytes) {
  for (int64_t p = 0; p <= tlen; ++p) ins[p] = 0;
  int64_t rows = 1;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t bases = 0;
    codes[i] = it[i].n < 0 ? AWV_MS_SKIPPED
                           : code_one(it[i].c, it[i].n, (int64_t)it[i].sp.pe - it[i].sp.pb - it[i].q_skip, (int64_t)it[i].sp.te - it[i].sp.tb - it[i].t_skip, &bases);
    rows += codes[i] == AWV_MS_OK;
  }
  for (int64_t i = 0; i < n; ++i)
    if (codes[i] == AWV_MS_OK) widen_one(it[i].c, it[i].n, (int64_t)it[i].sp.tb + it[i].t_skip, tlen, ins);
  std::vector<uint64_t> col((size_t)tlen + 1);
  uint64_t sum = 0;
  for (int64_t p = 0; p <= tlen; ++p) {
    sum += ins[p];
    col[(size_t)p] = (uint64_t)p + sum;
  }
  const int64_t W = (int64_t)col[(size_t)tlen];
  *width = W;
  *block_bytes = (uint64_t)rows * (uint64_t)W;
  if (*block_bytes > cap || *block_bytes == 0) return;
  for (uint64_t b = 0; b < *block_bytes; ++b) block[b] = '-';
  for (int64_t p = 0; p < tlen; ++p) block[col[(size_t)p]] = (uint8_t)awvcs::upper(text[p]);
  int64_t row = 1;
  for (int64_t i = 0; i < n; ++i) {
    if (codes[i] != AWV_MS_OK) continue;
    place_one(it[i].c, it[i].n, it[i].pattern, it[i].plen, (int64_t)it[i].sp.pb + it[i].q_skip, (int64_t)it[i].sp.tb + it[i].t_skip, tlen, col.data(), ins,
              block + row * W, W);
    ++row;
  }
}

struct State;                  // msa.hip: the launches' device buffers, events and the last call's stats
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)

}  // namespace awvmsa

// engine.hip
awvmsa::State*& awv_internal_msa(awv_engine* e);
