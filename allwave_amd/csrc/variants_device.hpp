// variants_device.hpp -- which (site, allele) events one item carries and how events fold into rows (include/allwave_hip.h, above
// awv_variants_one_host), once, for the host and the device: awv_variants_one_host is var_one below, awv_variants_fold_host is
// fold_rows; the hash, its combine, the key order and an item's code are __host__ __device__, for kernels that tally the same table.
//
// The op string c[0 .. n) over M X I D aligns a pattern (the query, or its reverse complement) with a text (the target).  Column k
// sits at pattern position x = pb + q_skip + #(ops other than 'I' before k) and text position y = tb + t_skip + #(ops other than
// 'D' before k).  An 'X' column is an SNV at y whose allele is pattern[x]; a maximal 'I' run of L a deletion of L at the y of its
// first column; a maximal 'D' run of L an insertion of pattern[x .. x + L) before y.  An item appends everything or nothing.
//
// The allele hash is a polynomial modulo the Mersenne prime 2^61 - 1 with base B = AWV_VAR_HASH_BASE = 0x1b873593a5c1f2e7, over
// the upper-cased bytes.  B is part of the contract: tables from several devices are merged by key.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "allwave_hip.h"
#include "cs_device.hpp"  // is_op, upper, whole_code's rule, slice_ok, apply_slice, Span

namespace awvvar {

using awvr::Span;

constexpr int64_t MAX_COLUMNS = awvcs::MAX_COLUMNS;  // of one string or slice: its event counts then fit awv_var_item's 32 bits
constexpr int64_t MAX_ITEMS = INT32_MAX;             // between two begins: an item carries a row's event at most once, so no count wraps
constexpr uint64_t MOD61 = ((uint64_t)1 << 61) - 1;
constexpr uint64_t HASH_BASE = AWV_VAR_HASH_BASE;
static_assert(HASH_BASE < MOD61, "the base is a residue");

// x < 2^62 + 2^61 -> x mod (2^61 - 1)
__host__ __device__ inline uint64_t reduce61(uint64_t x) {
  x = (x & MOD61) + (x >> 61);
  return x >= MOD61 ? x - MOD61 : x;
}
// a * b mod (2^61 - 1) for residues a, b: the 122-bit product's bits above 61 count once more, since 2^61 = 1
__host__ __device__ inline uint64_t mulmod61(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t hi = __umul64hi(a, b), lo = a * b;
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  const uint64_t hi = (uint64_t)(p >> 64), lo = (uint64_t)p;
#endif
  return reduce61(((hi << 3) | (lo >> 61)) + (lo & MOD61));
}
// h(s.c) from h(s)
__host__ __device__ inline uint64_t hash_push(uint64_t h, uint32_t c) { return reduce61(mulmod61(h, HASH_BASE) + (uint64_t)awvcs::upper(c)); }
// h(a.b) from h(a), h(b) and B^|b|
__host__ __device__ inline uint64_t hash_combine(uint64_t ha, uint64_t hb, uint64_t pow_b) { return reduce61(mulmod61(ha, pow_b) + hb); }
__host__ __device__ inline uint64_t hash_pow(uint64_t len) {  // B^len
  uint64_t r = 1, b = HASH_BASE;
  for (; len != 0; len >>= 1) {
    if (len & 1) r = mulmod61(r, b);
    b = mulmod61(b, b);
  }
  return r;
}

// the table's order: (t_idx, pos, type, len, hash) ascending
__host__ __device__ inline bool key_less(const awv_variant& a, const awv_variant& b) {
  if (a.t_idx != b.t_idx) return a.t_idx < b.t_idx;
  if (a.pos != b.pos) return a.pos < b.pos;
  if (a.type != b.type) return a.type < b.type;
  if (a.len != b.len) return a.len < b.len;
  return a.hash < b.hash;
}
__host__ __device__ inline bool key_equal(const awv_variant& a, const awv_variant& b) {
  return a.t_idx == b.t_idx && a.pos == b.pos && a.type == b.type && a.len == b.len && a.hash == b.hash;
}
// The key's three sort words, most significant first.  Every field of an event is non-negative, so the unsigned order of the
// words is the key's order.
__host__ __device__ inline uint64_t key_word(const awv_variant& r, int k) {
  return k == 0 ? ((uint64_t)(uint32_t)r.t_idx << 32) | (uint32_t)r.pos : k == 1 ? ((uint64_t)(uint32_t)r.type << 32) | (uint32_t)r.len : r.hash;
}

__host__ __device__ inline uint64_t make_rep(int32_t q_idx, bool revcomp, int64_t p_beg) {
  return ((uint64_t)(uint32_t)q_idx << 32) | ((uint64_t)revcomp << 31) | (uint64_t)(uint32_t)p_beg;
}
__host__ __device__ inline awv_variant make_event(int32_t t_idx, int64_t pos, int32_t type, int64_t len, uint64_t hash, uint64_t rep) {
  awv_variant r;
  r.t_idx = t_idx;
  r.pos = (int32_t)pos;
  r.type = type;
  r.len = (int32_t)len;
  r.hash = hash;
  r.rep = rep;
  r.count = 1;
  r.reserved = 0;
  return r;
}

// what the totals of a string decide: the rule of the cs text (awvcs::whole_code), in this pass's codes
__host__ __device__ inline int whole_code(bool bad, int64_t q, int64_t t, int64_t plen, int64_t tlen) {
  const int c = awvcs::whole_code(bad, q, t, plen, tlen);
  return c == AWV_CST_OK ? AWV_VR_OK : c == AWV_CST_BAD_OP ? AWV_VR_BAD_OP : AWV_VR_LENGTHS;
}
__host__ __device__ inline awv_var_item make_item(int32_t code, uint32_t snv, uint32_t ins, uint32_t del) {
  awv_var_item it;
  it.code = code;
  it.snv = code == AWV_VR_OK ? snv : 0u;
  it.ins = code == AWV_VR_OK ? ins : 0u;
  it.del = code == AWV_VR_OK ? del : 0u;
  return it;
}

// The contract as a serial walk (the host yardstick): c[0 .. n), n <= MAX_COLUMNS, over the rectangle sp of the aligned copy
// `pattern` of query q_idx, from x = sp.pb + q_skip and y = sp.tb + t_skip on.  First the code, then -- only for AWV_VR_OK -- the
// events in column order, at most cap of them into out; *n_events counts them all.
inline awv_var_item var_one(int32_t q_idx, int32_t t_idx, bool revcomp, const uint8_t* pattern, const Span& sp, const uint8_t* c, int64_t n, int64_t q_skip,
                            int64_t t_skip, awv_variant* out, uint64_t cap, uint64_t* n_events) {
  bool bad = false;
  int64_t q = 0, t = 0;
  uint32_t snv = 0, ins = 0, del = 0;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    bad = bad || !awvcs::is_op(op);
    const bool ends = k + 1 == n || c[k + 1] != op;  // the column ends its run
    snv += op == 'X';
    del += op == 'I' && ends;
    ins += op == 'D' && ends;
    q += op != 'I';
    t += op != 'D';
  }
  *n_events = 0;
  const int code = whole_code(bad, q, t, (int64_t)sp.pe - sp.pb - q_skip, (int64_t)sp.te - sp.tb - t_skip);
  if (code != AWV_VR_OK) return make_item(code, 0, 0, 0);
  int64_t x = (int64_t)sp.pb + q_skip, y = (int64_t)sp.tb + t_skip;
  uint64_t w = 0;
  const auto put = [&](const awv_variant& ev) {
    if (w < cap && out) out[w] = ev;
    ++w;
  };
  int64_t x0 = x, y0 = y;  // where the run in progress began
  uint64_t h = 0;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t op = c[k];
    if (k == 0 || c[k - 1] != op) {
      x0 = x;
      y0 = y;
      h = 0;
    }
    const bool ends = k + 1 == n || c[k + 1] != op;
    if (op == 'X') put(make_event(t_idx, y, AWV_VAR_SNV, 1, hash_push(0, pattern[x]), make_rep(q_idx, revcomp, x)));
    if (op == 'D') h = hash_push(h, pattern[x]);
    x += op != 'I';
    y += op != 'D';
    if (op == 'I' && ends) put(make_event(t_idx, y0, AWV_VAR_DEL, y - y0, 0, make_rep(q_idx, revcomp, x0)));
    if (op == 'D' && ends) put(make_event(t_idx, y0, AWV_VAR_INS, x - x0, h, make_rep(q_idx, revcomp, x0)));
  }
  *n_events = w;
  return make_item(AWV_VR_OK, snv, ins, del);
}

// ---- the walk in lanes and chunks (variants.hip's kernel; tests/variants_walk_driver.cpp runs the same functions serially) --------
// The kernel takes a string in chunks of 64 lanes x 16 op bytes (text_pass.hpp).  What is new relative to the cs walk stands here
// on plain values: the allele hash of a 'D' run that crosses lanes or chunks, which events a lane owns and in which order, and a
// run's pos / p_beg from the positions at its end.

// The segmented hash scan's element: of a stretch of columns, the hash and B^length of the 'D' bytes behind its last column other
// than 'D' (`reset`: it holds one; else the stretch lies wholly inside a run and is a pass-through).
struct HashSeg {
  uint64_t h, pw;
  uint32_t reset;
};
__host__ __device__ inline HashSeg seg_identity() { return HashSeg{0, 1, 0u}; }
// a then b; associative, with seg_identity() on both sides
__host__ __device__ inline HashSeg seg_combine(const HashSeg& a, const HashSeg& b) {
  if (b.reset) return b;
  return HashSeg{hash_combine(a.h, b.h, b.pw), mulmod61(a.pw, b.pw), a.reset};
}
// the hash of the 'D' run in progress behind a stretch, `carry` the one in progress before it
__host__ __device__ inline uint64_t seg_behind(uint64_t carry, const HashSeg& s) { return s.reset ? s.h : hash_combine(carry, s.h, s.pw); }

// A lane's 16 bytes as masks (bit j: byte j), all inside `valid`, the bytes that are columns -- a contiguous range.
struct LaneCols {
  uint32_t valid, x, i, d;  // ... an 'X', an 'I', a 'D'
  uint32_t brk;             // a column > 0 whose op differs from the one before it
  uint32_t prev_i, prev_d;  // 1: the op before the lane's first byte is an 'I' / a 'D'
};
__host__ __device__ inline int popc32(uint32_t m) { return __builtin_popcount(m); }
__host__ __device__ inline int top_bit(uint32_t m) { return 31 - __builtin_clz(m); }  // m != 0
// the breaks that end an 'I' run / a 'D' run: the lane that holds the break owns the run's event
__host__ __device__ inline uint32_t ends_i(const LaneCols& c) { return c.brk & ((c.i << 1) | c.prev_i); }
__host__ __device__ inline uint32_t ends_d(const LaneCols& c) { return c.brk & ((c.d << 1) | c.prev_d); }
__host__ __device__ inline uint32_t lane_event_count(const LaneCols& c) { return (uint32_t)(popc32(c.x) + popc32(ends_i(c)) + popc32(ends_d(c))); }
// the 'D' columns at the lane's upper end: their run goes on into the next lane (or ends with the string)
__host__ __device__ inline uint32_t tail_d(const LaneCols& c) {
  const uint32_t other = c.valid & ~c.d;
  return other == 0 ? c.d : c.d & ~(((uint32_t)2 << top_bit(other)) - 1u);
}
// the lane's element of the scan; byte(k): the k-th of the pattern bytes the lane's columns consume
template <typename Byte>
__host__ __device__ inline HashSeg lane_seg(const LaneCols& c, Byte&& byte) {
  const uint32_t tail = tail_d(c), takes_p = c.valid & ~c.i;
  uint64_t h = 0;
  for (uint32_t m = tail; m != 0; m &= m - 1) h = hash_push(h, byte(popc32(takes_p & ((m & (0u - m)) - 1u))));  // at most 16 trips: a 16-bit mask
  return HashSeg{h, hash_pow((uint64_t)popc32(tail)), (uint32_t)((c.valid & ~tail) != 0)};
}
// a gap run's event from the positions (x, y) behind its last column and its length
__host__ __device__ inline awv_variant gap_event(int32_t q_idx, int32_t t_idx, bool revcomp, bool is_d, int64_t x, int64_t y, int64_t len, uint64_t hash) {
  return is_d ? make_event(t_idx, y, AWV_VAR_INS, len, hash, make_rep(q_idx, revcomp, x - len))
              : make_event(t_idx, y - len, AWV_VAR_DEL, len, 0, make_rep(q_idx, revcomp, x));
}
// The lane's events in order, each handed to put(event): ascending by byte; at a break the run that ends there, then the byte's own
// SNV.  col0: the column of byte 0 (may be negative); rs0: the column at which the run the lane begins in started; (x0, y0): the
// positions at the lane's first column; in_h: the hash of the 'D' run in progress before the lane (seg_behind of the lower lanes).
template <typename Byte, typename Put>
__host__ __device__ inline void lane_events(const LaneCols& c, int32_t q_idx, int32_t t_idx, bool revcomp, int64_t col0, int64_t rs0, int64_t x0, int64_t y0,
                                            uint64_t in_h, Byte&& byte, Put&& put) {
  const uint32_t e_i = ends_i(c), e_d = ends_d(c), takes_p = c.valid & ~c.i, takes_t = c.valid & ~c.d;
  const uint32_t head_d = c.d & ~tail_d(c);  // the 'D' columns whose run ends inside the lane
  uint64_t h = 0;     // of the 'D' run in progress, its bytes in this lane
  uint32_t cnt = 0;   // how many they are
  bool begun = false; // the run began inside the lane
  for (uint32_t m = c.x | e_i | e_d | head_d; m != 0; m &= m - 1) {  // at most 16 trips: a 16-bit mask
    const uint32_t bit = m & (0u - m), below = bit - 1u;
    const int j = top_bit(bit);
    const int kp = popc32(takes_p & below);
    const int64_t x = x0 + kp, y = y0 + popc32(takes_t & below);
    if ((e_i | e_d) & bit) {
      const uint32_t lower = c.brk & below;
      const int64_t len = col0 + j - (lower != 0 ? col0 + top_bit(lower) : rs0);
      const bool is_d = (e_d & bit) != 0;
      put(gap_event(q_idx, t_idx, revcomp, is_d, x, y, len, is_d ? (begun ? h : hash_combine(in_h, h, hash_pow(cnt))) : 0));
    }
    if (c.x & bit) put(make_event(t_idx, y, AWV_VAR_SNV, 1, hash_push(0, byte(kp)), make_rep(q_idx, revcomp, x)));
    if (head_d & bit) {
      if (c.brk & bit) {
        h = 0;
        cnt = 0;
        begun = true;
      }
      h = hash_push(h, byte(kp));
      ++cnt;
    }
  }
}

// The fold as the host does it (the yardstick, and the merge of several engines' tables): rows[0 .. n) sorted by key, equal keys
// reduced to one row (sum of count, min of rep), compacted to the front; returns the number of rows left.
inline uint64_t fold_rows(awv_variant* rows, uint64_t n) {
  std::sort(rows, rows + n, [](const awv_variant& a, const awv_variant& b) { return key_less(a, b); });
  uint64_t w = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (w > 0 && key_equal(rows[w - 1], rows[i])) {
      rows[w - 1].count += rows[i].count;
      rows[w - 1].rep = std::min(rows[w - 1].rep, rows[i].rep);
    } else {
      rows[w++] = rows[i];
    }
  }
  return w;
}

struct State;                  // variants.hip: the accumulated table, the pass's device buffers and the stats since begin
void state_release(State* s);  // frees them and the object itself (nullptr: nothing)
bool active(const State* s);   // between awv_engine_variants_begin and the end of its table

// engine.hip's hook: one batch of an aligning call, on the engine's stream, after the clip / split step; the arguments are
// awvcov::coverage_batch's, the items awvw::contributing_items' under the begin's clip_min_score.  Appends the batch's events to the table.
int variants_batch(awv_engine* e, const awv_pair* pairs, int64_t n, const awv_result* results, const uint8_t* d_arena, uint64_t arena_bytes,
                   const awv_clip_result* clips, const uint64_t* seg_first, const awv_split_index* iout, const awv_clip_result* sout, const Span* spans);

// variants_fold.hip: the fold on the device.  d_rows[0 .. n), events or rows in any order, become fold_rows' rows in place, on
// `stream`; *n_out is their number and *ms gains the HIP-event time.  The scratch only ever grows.
struct FoldScratch;
FoldScratch* fold_scratch_new();
void fold_scratch_release(FoldScratch* fs);  // (nullptr: nothing)
constexpr uint64_t MAX_FOLD_ROWS = (uint64_t)1 << 31;  // the sort's permutation is 32 bits wide
int fold_device(hipStream_t stream, FoldScratch* fs, awv_variant* d_rows, uint64_t n, uint64_t* n_out, float* ms);

}  // namespace awvvar

// engine.hip
awvvar::State*& awv_internal_variants(awv_engine* e);
