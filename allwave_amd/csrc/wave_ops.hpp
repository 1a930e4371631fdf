// wave_ops.hpp -- what the kernels of the ten record passes (verify.hip, clip.hip, split.hip, normalize.hip, encode.hip, cs.hip,
// coverage.hip, variants.hip, lift.hip, msa.hip: namespaces awvf, awvc, awvs, awvn, awve, awvcs, awvcov, awvvar, awvl, awvmsa) share on
// the device, in namespace awvw: the take of the next record from the cursor, the chunk a wave reads (64 lanes x 16 op bytes),
// wave64 reductions and inclusive scans on the DPP network, one byte of a lane's 16 and packed byte counting over them, a lane's
// 16 op bytes as bit masks with the packed scan of the bases they consume (cs.hip and the four passes made after it); and the
// device buffer their host sides keep (record_pass.hpp).  What only the passes that look at runs share on the device is
// text_pass.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

namespace awvw {

constexpr int LANE_BYTES = 16;
constexpr int CHUNK = 64 * LANE_BYTES;  // the op bytes a wave takes per iteration, one aligned 16-byte load per lane

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The next dispatch slot, uniform across the wave: lane 0 advances the 64-bit cursor counters[0].  A kernel's persistent
// waves call it at the top of their loop and leave when the slot is npairs or more.
__device__ __forceinline__ unsigned long long take_record(unsigned long long* counters, int lane) {
  unsigned slot_lo = 0, slot_hi = 0;
  if (lane == 0) {
    const unsigned long long s = atomicAdd(&counters[0], 1ull);
    slot_lo = (unsigned)s;
    slot_hi = (unsigned)(s >> 32);
  }
  return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)slot_lo) |
         ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)slot_hi) << 32);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {  // in every lane
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ long long wave_min_i64(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ long long wave_max_i64(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp32(int ident, int v) {  // lanes without a source (or outside ROWS) get `ident`
  return __builtin_amdgcn_update_dpp(ident, v, CTRL, ROWS, 0xf, false);
}
// 64-bit values travel as two halves
template <int CTRL, int ROWS>
__device__ __forceinline__ long long dpp64(long long ident, long long v) {
  const unsigned lo = (unsigned)dpp32<CTRL, ROWS>((int)(unsigned)(unsigned long long)ident, (int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)dpp32<CTRL, ROWS>((int)(unsigned)((unsigned long long)ident >> 32), (int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// wave64 inclusive scans: row_shr 1/2/4/8 within the rows of 16, then row_bcast15 / row_bcast31 across them
__device__ __forceinline__ int wave_scan_add(int v) {
  v += dpp32<0x111, 0xf>(0, v);
  v += dpp32<0x112, 0xf>(0, v);
  v += dpp32<0x114, 0xf>(0, v);
  v += dpp32<0x118, 0xf>(0, v);
  v += dpp32<0x142, 0xa>(0, v);
  v += dpp32<0x143, 0xc>(0, v);
  return v;
}
__device__ __forceinline__ int wave_scan_max(int v) {
  v = max(v, dpp32<0x111, 0xf>(INT_MIN, v));
  v = max(v, dpp32<0x112, 0xf>(INT_MIN, v));
  v = max(v, dpp32<0x114, 0xf>(INT_MIN, v));
  v = max(v, dpp32<0x118, 0xf>(INT_MIN, v));
  v = max(v, dpp32<0x142, 0xa>(INT_MIN, v));
  v = max(v, dpp32<0x143, 0xc>(INT_MIN, v));
  return v;
}
__device__ __forceinline__ long long wave_scan_add(long long v) {
  v += dpp64<0x111, 0xf>(0, v);
  v += dpp64<0x112, 0xf>(0, v);
  v += dpp64<0x114, 0xf>(0, v);
  v += dpp64<0x118, 0xf>(0, v);
  v += dpp64<0x142, 0xa>(0, v);
  v += dpp64<0x143, 0xc>(0, v);
  return v;
}
__device__ __forceinline__ long long wave_scan_min(long long v) {
  v = min(v, dpp64<0x111, 0xf>(LLONG_MAX, v));
  v = min(v, dpp64<0x112, 0xf>(LLONG_MAX, v));
  v = min(v, dpp64<0x114, 0xf>(LLONG_MAX, v));
  v = min(v, dpp64<0x118, 0xf>(LLONG_MAX, v));
  v = min(v, dpp64<0x142, 0xa>(LLONG_MAX, v));
  v = min(v, dpp64<0x143, 0xc>(LLONG_MAX, v));
  return v;
}
// the value of the lane below (wave_shr 1); lane 0 keeps `lane0`
__device__ __forceinline__ int from_lower_lane(int v, int lane0) { return dpp32<0x138, 0xf>(lane0, v); }
__device__ __forceinline__ long long from_lower_lane(long long v, long long lane0) { return dpp64<0x138, 0xf>(lane0, v); }

// byte j of a lane's 16, j in a register
__device__ __forceinline__ unsigned byte_at(const u32x4& w, int j) {
  const int k = j >> 2;
  const unsigned d = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
  return (d >> (8 * (j & 3))) & 0xffu;
}

// 0xff in every byte j of a dword with lo <= j < hi (any lo, hi)
__device__ __forceinline__ unsigned byte_range_mask(int lo, int hi) {
  lo = min(max(lo, 0), 4);
  hi = min(max(hi, 0), 4);
  const unsigned long long below_hi = (1ull << (8 * hi)) - 1, below_lo = (1ull << (8 * lo)) - 1;
  return (unsigned)(below_hi & ~below_lo);
}
// how many bytes of w equal b
__device__ __forceinline__ int count_bytes(unsigned w, unsigned b) {
  const unsigned x = w ^ (b * 0x01010101u);
  const unsigned nonzero = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
  return 4 - __popc(nonzero);
}

// One lane's 16 op bytes of a chunk as masks over its columns.  Op byte c of the string is ops[sh + c]; a pass's bad-byte test is
// valid & ~(m | x | i | d).
struct OpMasks {
  unsigned valid;       // bit j: byte j is a column
  unsigned m, x, i, d;  // ... an 'M', an 'X', an 'I', a 'D' (cut to valid)
};
// The three steps that build them: the window [jlo, jhi) of the lane's bytes that are columns (0 <= jlo, jhi <= 16; none when
// jhi <= jlo), every byte's op, the cut to the window.
__device__ __forceinline__ OpMasks window_masks(int jlo, int jhi) { return OpMasks{((1u << jhi) - 1u) & ~((1u << jlo) - 1u), 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ void add_op(OpMasks& o, const u32x4& w, int j) {
  const unsigned op = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
  o.m |= (unsigned)(op == 'M') << j;
  o.x |= (unsigned)(op == 'X') << j;
  o.i |= (unsigned)(op == 'I') << j;
  o.d |= (unsigned)(op == 'D') << j;
}
__device__ __forceinline__ void cut_to_window(OpMasks& o) {
  o.m &= o.valid;
  o.x &= o.valid;
  o.i &= o.valid;
  o.d &= o.valid;
}
// from the lane's bytes w.  cs.hip and variants.hip, which have the bytes from text_pass.hpp's lane_runs, write these four lines in
// their chunk loop instead of calling this: compiled with the call, the four cs kernels take 75 to 87 VGPRs (5 or 6 waves per
// SIMD) in place of 57 to 62 (8), and with the loop in the kernel they take what they took (observed).
__device__ __forceinline__ OpMasks op_masks(const u32x4& w, int jlo, int jhi) {
  OpMasks o = window_masks(jlo, jhi);
#pragma unroll
  for (int j = 0; j < LANE_BYTES; ++j) add_op(o, w, j);
  cut_to_window(o);
  return o;
}
// the window and the aligned load first: lane `lane` of the chunk at `base` of a string that takes bytes [sh, span)
__device__ __forceinline__ OpMasks lane_op_masks(const uint8_t* ops, int sh, long long span, long long base, int lane) {
  const long long b0 = base + lane * LANE_BYTES;
  const int jlo = (int)min(max((long long)sh - b0, 0ll), (long long)LANE_BYTES);
  const int jhi = (int)min(max(span - b0, 0ll), (long long)LANE_BYTES);
  u32x4 w = u32x4{0u, 0u, 0u, 0u};
  if (b0 < span) w = *(const u32x4*)(ops + b0);
  return op_masks(w, jlo, jhi);
}
// the lane that holds the chunk's last column
__device__ __forceinline__ int last_column_lane(long long span, long long base) { return (int)min(63ll, (span - 1 - base) >> 4); }

// The bases a chunk's columns consume, packed: pattern bases (every column but an 'I') in the low 16 bits, text bases (every
// column but a 'D') in the high ones -- a chunk holds 1,024 columns, so the sums fit 16 bits each.  One add-scan over the lanes.
struct ConsumedScan {
  int ex;   // by the lanes below this one
  int tot;  // by the whole chunk (uniform)
};
__device__ __forceinline__ ConsumedScan consumed_scan(const OpMasks& o) {
  const int counts = __popc(o.valid & ~o.i) | (__popc(o.valid & ~o.d) << 16);
  const int s_pos = wave_scan_add(counts);
  return ConsumedScan{s_pos - counts, __builtin_amdgcn_readlane(s_pos, 63)};
}

// a device buffer that only ever grows
template <typename T>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = n;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace awvw
