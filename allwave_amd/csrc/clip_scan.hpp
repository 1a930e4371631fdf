// clip_scan.hpp -- the scan of one op string by one wave (device only): the chunk loop clip.hip describes, as the function
// the clip kernel (clip.hip) and the split kernel (split.hip) both call.  An interval of an op string is scanned as an op
// string of its own: the bytes at `off`, `n` of them, addressed from the 16-byte boundary at or below the first one.
#pragma once

#include <climits>

#include "clip_device.hpp"
#include "wave_ops.hpp"

namespace awvc {

using awvw::byte_range_mask;  // (wave_ops.hpp: the chunk, the scans and the byte counting shared with verify.hip)
using awvw::CHUNK;
using awvw::count_bytes;
using awvw::from_lower_lane;
using awvw::LANE_BYTES;
using awvw::u32x4;
using awvw::wave_scan_add;
using awvw::wave_scan_max;
using awvw::wave_scan_min;

__device__ __forceinline__ long long wave_max(long long v) {  // in every lane
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ long long read_lane(long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

constexpr int KEY_POS_BITS = 10;  // a column's byte position in its chunk, 0 .. CHUNK - 1
static_assert((1 << KEY_POS_BITS) == CHUNK, "a minimum's key keeps the chunk position in its low bits");

// What one scan leaves, uniform across the wave: the clip_one walk's best (0: no segment), its segment [beg, end) and the ops
// before either end, all counted from the string's first column; bad_col >= 0: the smallest column whose byte is no op (the
// rest is then meaningless).
struct Scan {
  long long best;
  unsigned beg, end;
  Prefix at_beg, at_end;
  long long bad_col;
};

// arena: 16-byte aligned, readable up to the 16-byte boundary behind the string.  Called by all 64 lanes with uniform arguments.
__device__ __forceinline__ Scan scan_ops(const awv_penalties& pen, const long long a, const uint8_t* arena, const uint64_t off, const long long n,
                                         const int lane) {
  const int sh = (int)(off & 15);
  const uint8_t* ops = arena + (off & ~(uint64_t)15);
  const long long span = sh + n;  // op byte c is ops[sh + c]
  long long bad_col = -1;
  // carried from chunk to chunk (uniform)
  long long S = 0, minS = 0, best = 0;
  unsigned minI = 0, beg = 0, end = 0;
  Prefix at_min{0, 0, 0, 0}, at_beg{0, 0, 0, 0}, at_end{0, 0, 0, 0};
  unsigned cI = 0, cD = 0, cX = 0, cM = 0;  // ops before the chunk, by kind
  long long c_start = 0;                    // the column the run in progress began at
  unsigned c_prev = 0;                      // the op before the chunk's first column (0: none)
  for (long long base = 0; n > 0 && base < span; base += CHUNK) {
    const long long b0 = base + lane * LANE_BYTES;
    const int jlo = (int)min(max((long long)sh - b0, 0ll), (long long)LANE_BYTES), jhi = (int)min(max(span - b0, 0ll), (long long)LANE_BYTES);  // this lane's bytes [jlo, jhi) are columns
    const int nv = max(jhi - jlo, 0);
    const long long col0 = b0 - sh;  // the column of this lane's byte 0
    const long long chunk_cols = base == 0 ? 0 : base - sh;  // columns before the chunk
    u32x4 w = {0u, 0u, 0u, 0u};
    if (b0 < span) w = *(const u32x4*)(ops + b0);
    int n_i = 0, n_d = 0, n_x = 0, n_m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w[k] &= byte_range_mask(jlo - 4 * k, jhi - 4 * k);
      n_i += count_bytes(w[k], 'I');
      n_d += count_bytes(w[k], 'D');
      n_x += count_bytes(w[k], 'X');
      n_m += count_bytes(w[k], 'M');
    }
    const unsigned long long bad_lanes = __ballot(n_i + n_d + n_x + n_m != nv);
    if (bad_lanes != 0) {  // lanes hold ascending columns: the lowest lane's first is the smallest
      int first = LANE_BYTES;
#pragma unroll
      for (int j = LANE_BYTES - 1; j >= 0; --j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j >= jlo && j < jhi && !is_op(op)) first = j;
      }
      const int l = __builtin_ctzll(bad_lanes);
      const unsigned col = (unsigned)(base + l * LANE_BYTES + __builtin_amdgcn_readlane(first, l) - sh);
      bad_col = (long long)col;
      break;
    }
    // the op before this lane's first column: the lower lane's last byte, the chunk's carry in lane 0, none at column 0
    unsigned prev = (unsigned)from_lower_lane((int)w[3], (int)(c_prev << 24)) >> 24;
    if (b0 <= sh) prev = 0;
    int last_break = -1;  // as a byte position in the chunk
    {
      unsigned pv = prev;
#pragma unroll
      for (int j = 0; j < LANE_BYTES; ++j) {
        const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const bool valid = j >= jlo && j < jhi;
        if (valid && op != pv) last_break = lane * LANE_BYTES + j;
        if (valid) pv = op;
      }
    }
    const int packed_id = n_i | (n_d << 16), packed_xm = n_x | (n_m << 16);  // (a chunk holds 1,024 columns: the sums fit 16 bits)
    const int s_id = wave_scan_add(packed_id), s_xm = wave_scan_add(packed_xm);
    const int ib = from_lower_lane(wave_scan_max(last_break), -1);
    long long run_start = ib >= 0 ? base + ib - sh : c_start;

    // first walk: the lane's prefix sums, its total, its minimum (the latest column attaining it)
    long long p[LANE_BYTES];
    long long acc = 0, lmin = LLONG_MAX;
    int lmin_j = 0;
#pragma unroll
    for (int j = 0; j < LANE_BYTES; ++j) {
      const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
      if (j >= jlo && j < jhi) {
        const long long col = col0 + j;
        if (op != prev) {
          run_start = col;
          prev = op;
        }
        acc += column_delta(pen, a, op, col - run_start + 1);
        if (acc <= lmin) {
          lmin = acc;
          lmin_j = j;
        }
      }
      p[j] = acc;
    }
    const long long incl = wave_scan_add(acc);
    const long long rel = incl - acc;  // S before this lane's columns, relative to the chunk's start
    // a tie between two columns goes to the later one: the smaller key
    const long long key = nv > 0 ? (rel + lmin) * CHUNK + (CHUNK - 1 - (lane * LANE_BYTES + lmin_j)) : LLONG_MAX;
    const long long kin = wave_scan_min(key);
    const long long kex = from_lower_lane(kin, LLONG_MAX);
    long long m = minS;
    unsigned mi = minI;
    if (kex != LLONG_MAX && S + (kex >> KEY_POS_BITS) <= m) {  // (a tie replaces the carried minimum: the chunk's columns are later)
      m = S + (kex >> KEY_POS_BITS);
      mi = (unsigned)(base + (CHUNK - 1 - (int)(kex & (CHUNK - 1))) - sh + 1);
    }
    // second walk: the serial rule from the minimum the lower lanes leave
    long long lv = 0;
    unsigned lb = 0, le = 0;
#pragma unroll
    for (int j = 0; j < LANE_BYTES; ++j) {
      if (j >= jlo && j < jhi) {
        const long long s = S + rel + p[j];
        const unsigned next_col = (unsigned)(col0 + j + 1);
        if (s <= m) {
          m = s;
          mi = next_col;
        }
        if (s - m > lv) {
          lv = s - m;
          lb = mi;
          le = next_col;
        }
      }
    }
    // ops before the column at byte position bp of this chunk, that column included (uniform bp)
    auto prefix_through = [&](int bp) {
      const int hi = min(jhi, (bp & (LANE_BYTES - 1)) + 1);
      int li = 0, ld = 0, lx = 0, lm = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned wk = w[k] & byte_range_mask(jlo - 4 * k, hi - 4 * k);
        li += count_bytes(wk, 'I');
        ld += count_bytes(wk, 'D');
        lx += count_bytes(wk, 'X');
        lm += count_bytes(wk, 'M');
      }
      const int ex_id = s_id - packed_id, ex_xm = s_xm - packed_xm;
      const unsigned cols = (unsigned)(base + bp - sh + 1);
      const unsigned ni = cI + (unsigned)(ex_id & 0xffff) + (unsigned)li, nd = cD + (unsigned)(ex_id >> 16) + (unsigned)ld;
      const unsigned nx = cX + (unsigned)(ex_xm & 0xffff) + (unsigned)lx, nm = cM + (unsigned)(ex_xm >> 16) + (unsigned)lm;
      const int l = bp >> 4;
      Prefix r;
      r.q = cols - (unsigned)__builtin_amdgcn_readlane((int)ni, l);
      r.t = cols - (unsigned)__builtin_amdgcn_readlane((int)nd, l);
      r.x = (unsigned)__builtin_amdgcn_readlane((int)nx, l);
      r.m = (unsigned)__builtin_amdgcn_readlane((int)nm, l);
      return r;
    };
    // a tie between two lanes goes to the lower one (the earlier columns): the larger key
    const long long kbest = wave_max(lv * 64 + (63 - lane));
    const long long chunk_best = read_lane(kbest, 0) >> 6;
    if (chunk_best > best) {  // (a tie never replaces the carried best)
      const int wl = 63 - (__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)kbest) & 63);
      best = chunk_best;
      beg = (unsigned)__builtin_amdgcn_readlane((int)lb, wl);
      end = (unsigned)__builtin_amdgcn_readlane((int)le, wl);
      at_end = prefix_through((int)((long long)end - 1 + sh - base));
      at_beg = (long long)beg > chunk_cols ? prefix_through((int)((long long)beg - 1 + sh - base)) : at_min;
    }
    const long long kall = read_lane(kin, 63);
    if (kall != LLONG_MAX && S + (kall >> KEY_POS_BITS) <= minS) {
      const int bp = CHUNK - 1 - (int)(kall & (CHUNK - 1));
      minS = S + (kall >> KEY_POS_BITS);
      minI = (unsigned)(base + bp - sh + 1);
      at_min = prefix_through(bp);
    }
    S += read_lane(incl, 63);
    const int last_lane = (int)min(63ll, (span - 1 - base) >> 4);  // the lane that holds the chunk's last column
    c_prev = (unsigned)__builtin_amdgcn_readlane((int)prev, last_lane);
    c_start = read_lane(run_start, last_lane);
    const int t_id = __builtin_amdgcn_readlane(s_id, 63), t_xm = __builtin_amdgcn_readlane(s_xm, 63);
    cI += (unsigned)(t_id & 0xffff);
    cD += (unsigned)(t_id >> 16);
    cX += (unsigned)(t_xm & 0xffff);
    cM += (unsigned)(t_xm >> 16);
  }
  return Scan{best, beg, end, at_beg, at_end, bad_col};
}

}  // namespace awvc
