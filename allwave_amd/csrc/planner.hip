// planner.hip -- device pair planning over an engine's resident sequences (include/allwave_hip.h, awv_sketch*, awv_keep_pairs).
//
// Everything here is integer work whose results equal the host planner's (csrc/host/planner.cpp) bit for bit:
//   awp_sketch_kernel        mash / stranded sketches: SipHash-1-3 of every ACGT-only k-mer, the s smallest with
//                            duplicates (tile by tile: bitonic sort in LDS, merged into the running s smallest), deduplicated
//   awp_rows_kernel          |A n B| of one row's sketch against every column's (all against all, a block of rows at a time)
//   awp_pair_counts_kernel   |A n B| for a pair list (pairs grouped by their A sequence, whose sketch sits in LDS)
//   awp_knn_kernel           per row the k nearest / farthest columns by Jaccard, compared exactly by cross-multiplication
//   awp_keep_kernel          the hashed keep test of iterator.rs's sparsifiers as one bit per (i, j), rows of 32-bit words
// No kernel writes outside the buffers sized here: every store is guarded by the counts the host derived from lengths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "allwave_hip.h"
#include "planner_device.hpp"
#include "wave_ops.hpp"

namespace awp {

constexpr int SK_WG = 1024;    // sketch workgroup: one per sequence
constexpr int SK_TILE = 2048;  // k-mer positions per tile (2 per thread)
constexpr int ROW_WG = 256;    // rows / pair counts: 4 waves, one column (pair) per wave at a time
constexpr int ROW_COLS = 256;  // columns per rows workgroup
constexpr int PAIR_SEG = 256;  // pairs per pair-count workgroup at the most
constexpr int KNN_WG = 256;    // kNN: one row per wave

// ---- SipHash-1-3, zero keys (Rust's DefaultHasher) -----------------------------------------------------------------------
struct Sip {
  uint64_t v0 = 0x736f6d6570736575ULL, v1 = 0x646f72616e646f6dULL, v2 = 0x6c7967656e657261ULL, v3 = 0x7465646279746573ULL;
  __device__ static uint64_t rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
  __device__ void round() {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  }
  __device__ void block(uint64_t m) { v3 ^= m; round(); v0 ^= m; }
  __device__ uint64_t finish(uint64_t b) {  // b: the tail bytes | total length << 56
    v3 ^= b; round(); v0 ^= b;
    v2 ^= 0xff;
    round(); round(); round();
    return v0 ^ v1 ^ v2 ^ v3;
  }
};

// SipHash of an n-byte message whose bytes come from byte(p)
template <typename F>
__device__ inline uint64_t sip_message(int n, F byte) {
  Sip s;
  const int full = n >> 3;
  for (int w = 0; w < full; ++w) {
    uint64_t m = 0;
    for (int b = 0; b < 8; ++b) m |= (uint64_t)byte(8 * w + b) << (8 * b);
    s.block(m);
  }
  uint64_t t = (uint64_t)n << 56;
  for (int b = 0; b < (n & 7); ++b) t |= (uint64_t)byte(8 * full + b) << (8 * b);
  return s.finish(t);
}

// <[u8] as Hash> through DefaultHasher: the length as a u64 (LE) and then the k bytes
template <typename F>
__device__ inline uint64_t hash_kmer(int k, F byte) {
  return sip_message(k + 8, [&](int p) -> uint8_t { return p < 8 ? (uint8_t)((uint64_t)k >> (8 * p)) : byte(p - 8); });
}

__device__ inline bool is_base(uint8_t b) {
  const uint8_t u = (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
__device__ inline uint8_t comp_upper(uint8_t b) {  // (only ever applied to ACGTacgt)
  const uint8_t u = (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
  return u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : 'C';
}

__device__ inline int lower_bound(const uint64_t* a, int n, uint64_t v) {  // first index with a[i] >= v
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ inline int upper_bound(const uint64_t* a, int n, uint64_t v) {  // first index with a[i] > v
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- sketches ------------------------------------------------------------------------------------------------------------
// One workgroup per sequence.  The host's rule is "sort all k-mer hashes, truncate to s, deduplicate": the s smallest WITH
// duplicates are kept in LDS (best[0, nb)), and every tile's sorted hashes are merged into them (merge positions by binary
// search, the first s kept).  Invalid positions sort last as ~0 but are never counted (tv), so a real hash of ~0 is safe.
// slot[i]: where sequence i's sketch goes (min(s, positions) slots, host prefix sum); cnt[i]: its length after deduplication.
// Dynamic LDS: (2 s + SK_TILE) u64 + SK_TILE + 64 bytes.
__global__ __launch_bounds__(SK_WG) void awp_sketch_kernel(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off,
                                                           const int32_t* __restrict__ len, const uint64_t* __restrict__ slot, int k,
                                                           int s, int canonical, uint64_t* __restrict__ hashes,
                                                           uint32_t* __restrict__ cnt) {
  extern __shared__ uint64_t lds[];
  __shared__ int s_valid;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int npos = len[i] - k + 1;
  if (npos <= 0) {  // (block-uniform)
    if (tid == 0) cnt[i] = 0;
    return;
  }
  uint64_t* best = lds;
  uint64_t* nxt = lds + s;
  uint64_t* tile = lds + 2 * s;
  uint8_t* tb = (uint8_t*)(tile + SK_TILE);
  const uint8_t* src = seq + off[i];
  int nb = 0;
  for (int t0 = 0; t0 < npos; t0 += SK_TILE) {
    const int tn = min(SK_TILE, npos - t0);
    __syncthreads();  // (every thread has read the previous tile's s_valid)
    for (int x = tid; x < tn + k - 1; x += SK_WG) tb[x] = src[t0 + x];
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int mine = 0;
    for (int p = tid; p < SK_TILE; p += SK_WG) {
      uint64_t h = ~0ULL;
      if (p < tn) {
        bool ok = true;
        for (int x = 0; x < k; ++x) ok = ok && is_base(tb[p + x]);
        if (ok) {
          h = hash_kmer(k, [&](int x) { return tb[p + x]; });
          if (canonical) h = min(h, hash_kmer(k, [&](int x) { return comp_upper(tb[p + k - 1 - x]); }));
          ++mine;
        }
      }
      tile[p] = h;
    }
    if (mine) atomicAdd(&s_valid, mine);
    __syncthreads();
    const int tv = s_valid;
    if (tv > 0) {
      for (int size = 2; size <= SK_TILE; size <<= 1) {  // bitonic sort, ascending
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          const int lo = (tid / stride) * stride * 2 + (tid % stride), hi = lo + stride;
          const uint64_t a = tile[lo], b = tile[hi];
          if ((a > b) == ((lo & size) == 0)) {
            tile[lo] = b;
            tile[hi] = a;
          }
          __syncthreads();
        }
      }
      for (int x = tid; x < nb; x += SK_WG) {
        const uint64_t v = best[x];
        const int pos = x + lower_bound(tile, tv, v);
        if (pos < s) nxt[pos] = v;
      }
      for (int x = tid; x < min(tv, s); x += SK_WG) {
        const uint64_t v = tile[x];
        const int pos = x + upper_bound(best, nb, v);
        if (pos < s) nxt[pos] = v;
      }
      __syncthreads();
      uint64_t* t = best;
      best = nxt;
      nxt = t;
      nb = min(s, nb + tv);
    }
  }
  if (tid < 64) {  // deduplicate in order: one wave, a ballot per 64 entries
    const int lane = tid;
    const uint64_t below = (1ULL << lane) - 1;
    int base = 0;
    uint64_t* out = hashes + slot[i];
    for (int c = 0; c < nb; c += 64) {
      const int x = c + lane;
      const bool f = x < nb && (x == 0 || best[x] != best[x - 1]);
      const uint64_t mask = __ballot(f);
      if (f) out[base + __popcll(mask & below)] = best[x];
      base += __popcll(mask);
    }
    if (lane == 0) cnt[i] = (uint32_t)base;
  }
}

// |A n B| of sorted unique A (in LDS, na entries) and B (global, nb entries), summed over one wave
__device__ inline int wave_intersect(const uint64_t* A, int na, const uint64_t* __restrict__ B, int nb, int lane) {
  int c = 0;
  if (na > 0 && nb > 0) {
    const uint64_t lo = A[0], hi = A[na - 1];
    for (int x = lane; x < nb; x += 64) {
      const uint64_t v = B[x];
      if (v > hi) break;  // (B ascending: so is every later element of this lane)
      if (v < lo) continue;
      const int p = lower_bound(A, na, v);
      c += (p < na && A[p] == v) ? 1 : 0;
    }
  }
  for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m, 64);
  return c;
}

// rows row0 + blockIdx.x against columns [blockIdx.y * ROW_COLS, ...): out[(row - row0) * n + col]
__global__ __launch_bounds__(ROW_WG) void awp_rows_kernel(const uint64_t* __restrict__ ha, const uint64_t* __restrict__ sa,
                                                          const uint32_t* __restrict__ ca, const uint64_t* __restrict__ hb,
                                                          const uint64_t* __restrict__ sb, const uint32_t* __restrict__ cb, int row0,
                                                          int n, uint16_t* __restrict__ out) {
  extern __shared__ uint64_t A[];
  const int row = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int na = (int)ca[row];
  for (int x = tid; x < na; x += ROW_WG) A[x] = ha[sa[row] + x];
  __syncthreads();
  const int c1 = min(n, (int)(blockIdx.y + 1) * ROW_COLS);
  for (int j = blockIdx.y * ROW_COLS + wave; j < c1; j += ROW_WG / 64) {
    const int c = wave_intersect(A, na, hb + sb[j], (int)cb[j], lane);
    if (lane == 0) out[(size_t)blockIdx.x * n + j] = (uint16_t)c;
  }
}

// pairs grouped by their A sequence: segment g covers order[seg_first[g], seg_first[g + 1]), all with A = seg_a[g]
__global__ __launch_bounds__(ROW_WG) void awp_pair_counts_kernel(const uint64_t* __restrict__ ha, const uint64_t* __restrict__ sa,
                                                                 const uint32_t* __restrict__ ca, const uint64_t* __restrict__ hb,
                                                                 const uint64_t* __restrict__ sb, const uint32_t* __restrict__ cb,
                                                                 const int32_t* __restrict__ seg_a, const int64_t* __restrict__ seg_first,
                                                                 const int32_t* __restrict__ b_of, const uint32_t* __restrict__ order,
                                                                 uint16_t* __restrict__ out) {
  extern __shared__ uint64_t A[];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = seg_a[g];
  const int na = (int)ca[a];
  for (int x = tid; x < na; x += ROW_WG) A[x] = ha[sa[a] + x];
  __syncthreads();
  for (int64_t p = seg_first[g] + wave; p < seg_first[g + 1]; p += ROW_WG / 64) {
    const uint32_t idx = order[p];
    const int b = b_of[idx];
    const int c = wave_intersect(A, na, hb + sb[b], (int)cb[b], lane);
    if (lane == 0) out[idx] = (uint16_t)c;
  }
}

// ---- kNN -----------------------------------------------------------------------------------------------------------------
// A candidate column: Jaccard inter / uni (uni == 0 counts as 0 / 1).  Nearest first: larger Jaccard, then smaller j (the
// host's stable sort over j ascending); farthest first: smaller Jaccard, then smaller j.
struct Cand {
  uint32_t inter, uni;
  int32_t j;  // -1: none
};
__device__ inline bool ahead(const Cand& a, const Cand& b, bool farthest) {  // a strictly before b (both valid)
  const uint64_t l = (uint64_t)a.inter * b.uni, r = (uint64_t)b.inter * a.uni;
  if (l != r) return farthest ? l < r : l > r;
  return a.j < b.j;
}
__device__ inline Cand pick(Cand a, Cand b, bool farthest) {  // (selects field by field: no struct in scratch)
  const bool take_b = a.j < 0 || (b.j >= 0 && ahead(b, a, farthest));
  Cand r;
  r.inter = take_b ? b.inter : a.inter;
  r.uni = take_b ? b.uni : a.uni;
  r.j = take_b ? b.j : a.j;
  return r;
}

// the K best columns j != i of one row in order, found one at a time (each the best of those strictly behind the previous
// pick); -1 where fewer than K columns exist.  One wave; every lane ends with the same picks.
template <bool FARTHEST>
__device__ inline void knn_row(const uint16_t* __restrict__ row, const uint32_t* __restrict__ cnt, uint32_t si, int i, int n, int K,
                               int lane, int32_t* __restrict__ out) {
  Cand prev{0, 1, -1};
  for (int t = 0; t < K; ++t) {
    Cand best{0, 1, -1};
    for (int j = lane; j < n; j += 64) {
      if (j == i) continue;
      Cand c{row[j], 0, j};
      c.uni = si + cnt[j] - c.inter;
      if (c.uni == 0) { c.inter = 0; c.uni = 1; }
      if (prev.j >= 0 && !ahead(prev, c, FARTHEST)) continue;
      best = pick(best, c, FARTHEST);
    }
    for (int m = 32; m > 0; m >>= 1) {
      Cand o;
      o.inter = __shfl_xor(best.inter, m, 64);
      o.uni = __shfl_xor(best.uni, m, 64);
      o.j = __shfl_xor(best.j, m, 64);
      best = pick(best, o, FARTHEST);
    }
    if (lane == 0) out[t] = best.j;
    prev = best;
    if (best.j < 0) {  // (uniform across the wave after the butterfly)
      for (int u = t + 1 + lane; u < K; u += 64) out[u] = -1;
      return;
    }
  }
}

// one wave per row of the block: counts[r * n + j] = |S_i n S_j| for row i = row0 + r
__global__ __launch_bounds__(KNN_WG) void awp_knn_kernel(const uint16_t* __restrict__ counts, const uint32_t* __restrict__ cnt,
                                                         int row0, int nrows, int n, int kn, int kf, int32_t* __restrict__ near_out,
                                                         int32_t* __restrict__ far_out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (KNN_WG / 64) + (threadIdx.x >> 6);
  if (r >= nrows) return;  // (wave-uniform; no workgroup barrier below)
  const int i = row0 + r;
  const uint32_t si = cnt[i];
  const uint16_t* row = counts + (size_t)r * n;
  knn_row<false>(row, cnt, si, i, n, kn, lane, near_out + (size_t)i * kn);
  knn_row<true>(row, cnt, si, i, n, kf, lane, far_out + (size_t)i * kf);
}

// ---- hashed keep test ----------------------------------------------------------------------------------------------------
// <str as Hash> of "id_i:id_j" through DefaultHasher (the bytes, then 0xFF); bit (j & 31) of word gid = i * words + j / 32
// is set when the pair is kept: keep_all, or hash < threshold
__global__ __launch_bounds__(256) void awp_keep_kernel(const uint8_t* __restrict__ ids, const uint64_t* __restrict__ id_off, int n,
                                                       int words, uint64_t threshold, int keep_all, int include_diag,
                                                       uint32_t* __restrict__ bitmap) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)n * words) return;
  const int i = (int)(gid / words), w = (int)(gid % words);
  const uint8_t* a = ids + id_off[i];
  const int la = (int)(id_off[i + 1] - id_off[i]);
  uint32_t word = 0;
  for (int b = 0; b < 32; ++b) {
    const int j = 32 * w + b;
    if (j >= n) break;
    if (j == i && !include_diag) continue;
    bool keep = keep_all != 0;
    if (!keep) {
      const uint8_t* c = ids + id_off[j];
      const int lc = (int)(id_off[j + 1] - id_off[j]);
      const uint64_t h = sip_message(la + lc + 2, [&](int p) -> uint8_t {
        return p < la ? a[p] : p == la ? (uint8_t)':' : p < la + 1 + lc ? c[p - la - 1] : (uint8_t)0xFF;
      });
      keep = h < threshold;
    }
    if (keep) word |= 1u << b;
  }
  bitmap[gid] = word;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
using awvw::Buf;  // (wave_ops.hpp: the device buffer that only ever grows)

struct SketchSet {
  bool built = false;
  int k = 0, s = 0;
  std::vector<uint64_t> slot;  // n + 1
  std::vector<uint32_t> cnt;   // n
  Buf<uint64_t> d_hash, d_slot;
  Buf<uint32_t> d_cnt;
  void release() {
    d_hash.release();
    d_slot.release();
    d_cnt.release();
    built = false;
  }
};

struct PlanState {
  SketchSet sk[3];
  Buf<uint16_t> d_counts;
  Buf<int32_t> d_i32a, d_i32b, d_near, d_far;
  Buf<int64_t> d_i64;
  Buf<uint32_t> d_u32;
  Buf<uint8_t> d_bytes;
  Buf<uint64_t> d_u64;
  void release() {
    for (auto& s : sk) s.release();
    d_counts.release();
    d_i32a.release();
    d_i32b.release();
    d_near.release();
    d_far.release();
    d_i64.release();
    d_u32.release();
    d_bytes.release();
    d_u64.release();
  }
};

void plan_state_release(PlanState* p) {
  if (!p) return;
  p->release();
  delete p;
}

}  // namespace awp

using namespace awp;

namespace {

// the engine's view and plan state, the device made current
int open(awv_engine* e, EngineView& v, PlanState*& ps) {
  if (!e) return awv_internal_null_engine();
  if (int rc = awv_internal_view(e, &v)) return rc;
  AWV_TRY(hipSetDevice(v.device));
  PlanState*& slot = awv_internal_plan(e);
  if (!slot) slot = new PlanState();
  ps = slot;
  return AWV_OK;
}

int built_sketch(PlanState* ps, int kind, SketchSet*& out) {
  if (kind < AWV_SK_CANONICAL || kind > AWV_SK_REVCOMP) return awv_internal_fail(AWV_ERR_ARG, "sketch kind out of range");
  if (!ps->sk[kind].built) return awv_internal_fail(AWV_ERR_STATE, "no sketch of this kind: call awv_sketch first");
  out = &ps->sk[kind];
  return AWV_OK;
}

int sketch_core(awv_engine* e, int kind, int k, int s, uint32_t* sizes) {
  EngineView v;
  PlanState* ps = nullptr;
  if (int rc = open(e, v, ps)) return rc;
  if (kind < AWV_SK_CANONICAL || kind > AWV_SK_REVCOMP) return awv_internal_fail(AWV_ERR_ARG, "sketch kind out of range");
  if (k < 1 || k > AWV_PLAN_MAX_K) return awv_internal_fail(AWV_ERR_ARG, "sketch: k must be in [1, 64]");
  if (s < 1 || s > AWV_PLAN_MAX_S) return awv_internal_fail(AWV_ERR_ARG, "sketch: s must be in [1, 4096]");
  SketchSet& sk = ps->sk[kind];
  sk.built = false;
  const int n = v.n;
  sk.k = k;
  sk.s = s;
  sk.slot.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) sk.slot[i + 1] = sk.slot[i] + (uint64_t)std::min<int64_t>(s, std::max<int64_t>(0, (int64_t)v.len_host[i] - k + 1));
  sk.cnt.assign((size_t)n, 0);
  AWV_TRY(sk.d_hash.reserve(sk.slot[n]));
  AWV_TRY(sk.d_slot.reserve((size_t)n + 1));
  AWV_TRY(sk.d_cnt.reserve((size_t)n));
  AWV_TRY(hipMemcpyAsync(sk.d_slot.p, sk.slot.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, v.stream));
  const size_t lds = (size_t)(2 * s + SK_TILE) * 8 + SK_TILE + 64;
  AWV_TRY(hipFuncSetAttribute((const void*)awp_sketch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(awp_sketch_kernel, dim3(n), dim3(SK_WG), lds, v.stream, kind == AWV_SK_REVCOMP ? v.rc : v.fwd, v.off, v.len,
                     (const uint64_t*)sk.d_slot.p, k, s, kind == AWV_SK_CANONICAL ? 1 : 0, sk.d_hash.p, sk.d_cnt.p);
  AWV_TRY(hipGetLastError());
  AWV_TRY(hipMemcpyAsync(sk.cnt.data(), sk.d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  sk.built = true;
  if (sizes) std::memcpy(sizes, sk.cnt.data(), (size_t)n * 4);
  return AWV_OK;
}

int sketch_copy_core(awv_engine* e, int kind, uint64_t* offsets, uint64_t* hashes) {
  EngineView v;
  PlanState* ps = nullptr;
  SketchSet* sk = nullptr;
  if (int rc = open(e, v, ps)) return rc;
  if (int rc = built_sketch(ps, kind, sk)) return rc;
  const int n = v.n;
  std::vector<uint64_t> o((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) o[i + 1] = o[i] + sk->cnt[i];
  if (offsets) std::memcpy(offsets, o.data(), o.size() * 8);
  if (hashes) {
    for (int i = 0; i < n; ++i)
      if (sk->cnt[i]) AWV_TRY(hipMemcpyAsync(hashes + o[i], sk->d_hash.p + sk->slot[i], (size_t)sk->cnt[i] * 8, hipMemcpyDeviceToHost, v.stream));
    AWV_TRY(hipStreamSynchronize(v.stream));
  }
  return AWV_OK;
}

size_t max_cnt(const SketchSet& sk) {
  uint32_t m = 0;
  for (uint32_t c : sk.cnt) m = std::max(m, c);
  return m;
}

int rows_launch(const EngineView& v, const SketchSet& a, const SketchSet& b, int row0, int nrows, uint16_t* d_out) {
  const size_t lds = std::max<size_t>(max_cnt(a), 1) * 8;
  AWV_TRY(hipFuncSetAttribute((const void*)awp_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(awp_rows_kernel, dim3(nrows, (v.n + ROW_COLS - 1) / ROW_COLS), dim3(ROW_WG), lds, v.stream,
                     (const uint64_t*)a.d_hash.p, (const uint64_t*)a.d_slot.p, (const uint32_t*)a.d_cnt.p, (const uint64_t*)b.d_hash.p,
                     (const uint64_t*)b.d_slot.p, (const uint32_t*)b.d_cnt.p, row0, v.n, d_out);
  AWV_TRY(hipGetLastError());
  return AWV_OK;
}

int rows_core(awv_engine* e, int kind, int row0, int nrows, uint16_t* out) {
  EngineView v;
  PlanState* ps = nullptr;
  SketchSet* sk = nullptr;
  if (int rc = open(e, v, ps)) return rc;
  if (int rc = built_sketch(ps, kind, sk)) return rc;
  if (!out || row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > v.n) return awv_internal_fail(AWV_ERR_ARG, "sketch_rows: rows out of range");
  if (nrows == 0) return AWV_OK;
  AWV_TRY(ps->d_counts.reserve((size_t)nrows * v.n));
  if (int rc = rows_launch(v, *sk, *sk, row0, nrows, ps->d_counts.p)) return rc;
  AWV_TRY(hipMemcpyAsync(out, ps->d_counts.p, (size_t)nrows * v.n * 2, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

int pair_counts_core(awv_engine* e, int kind_a, int kind_b, const int32_t* a, const int32_t* b, int64_t npairs, uint16_t* out) {
  EngineView v;
  PlanState* ps = nullptr;
  SketchSet *sa = nullptr, *sb = nullptr;
  if (int rc = open(e, v, ps)) return rc;
  if (int rc = built_sketch(ps, kind_a, sa)) return rc;
  if (int rc = built_sketch(ps, kind_b, sb)) return rc;
  if (npairs < 0 || (npairs > 0 && (!a || !b || !out))) return awv_internal_fail(AWV_ERR_ARG, "sketch_pair_counts: null argument");
  if (npairs >= (int64_t)1 << 32) return awv_internal_fail(AWV_ERR_ARG, "sketch_pair_counts: more than 2^32 - 1 pairs");
  if (npairs == 0) return AWV_OK;
  const int n = v.n;
  for (int64_t p = 0; p < npairs; ++p)
    if (a[p] < 0 || a[p] >= n || b[p] < 0 || b[p] >= n) return awv_internal_fail(AWV_ERR_ARG, "sketch_pair_counts: sequence index out of range");
  // counting sort by A (stable), then segments of at most PAIR_SEG pairs with one A each
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int64_t p = 0; p < npairs; ++p) ++first[(size_t)a[p] + 1];
  for (int i = 0; i < n; ++i) first[i + 1] += first[i];
  std::vector<uint32_t> order((size_t)npairs);
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (int64_t p = 0; p < npairs; ++p) order[(size_t)at[(size_t)a[p]]++] = (uint32_t)p;
  }
  std::vector<int32_t> seg_a;
  std::vector<int64_t> seg_first;
  for (int i = 0; i < n; ++i)
    for (int64_t p = first[i]; p < first[i + 1]; p += PAIR_SEG) {
      seg_a.push_back(i);
      seg_first.push_back(p);
    }
  seg_first.push_back(npairs);
  const size_t nseg = seg_a.size();
  AWV_TRY(ps->d_i32a.reserve(nseg));
  AWV_TRY(ps->d_i64.reserve(nseg + 1));
  AWV_TRY(ps->d_i32b.reserve((size_t)npairs));
  AWV_TRY(ps->d_u32.reserve((size_t)npairs));
  AWV_TRY(ps->d_counts.reserve((size_t)npairs));
  AWV_TRY(hipMemcpyAsync(ps->d_i32a.p, seg_a.data(), nseg * 4, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(ps->d_i64.p, seg_first.data(), (nseg + 1) * 8, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(ps->d_i32b.p, b, (size_t)npairs * 4, hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(ps->d_u32.p, order.data(), (size_t)npairs * 4, hipMemcpyHostToDevice, v.stream));
  const size_t lds = std::max<size_t>(max_cnt(*sa), 1) * 8;
  AWV_TRY(hipFuncSetAttribute((const void*)awp_pair_counts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(awp_pair_counts_kernel, dim3((unsigned)nseg), dim3(ROW_WG), lds, v.stream, (const uint64_t*)sa->d_hash.p,
                     (const uint64_t*)sa->d_slot.p, (const uint32_t*)sa->d_cnt.p, (const uint64_t*)sb->d_hash.p,
                     (const uint64_t*)sb->d_slot.p, (const uint32_t*)sb->d_cnt.p, (const int32_t*)ps->d_i32a.p,
                     (const int64_t*)ps->d_i64.p, (const int32_t*)ps->d_i32b.p, (const uint32_t*)ps->d_u32.p, ps->d_counts.p);
  AWV_TRY(hipGetLastError());
  AWV_TRY(hipMemcpyAsync(out, ps->d_counts.p, (size_t)npairs * 2, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

int knn_core(awv_engine* e, int kind, int kn, int kf, int32_t* near_out, int32_t* far_out) {
  EngineView v;
  PlanState* ps = nullptr;
  SketchSet* sk = nullptr;
  if (int rc = open(e, v, ps)) return rc;
  if (int rc = built_sketch(ps, kind, sk)) return rc;
  if (kn < 0 || kf < 0 || kn > AWV_PLAN_MAX_KNN || kf > AWV_PLAN_MAX_KNN)
    return awv_internal_fail(AWV_ERR_ARG, "sketch_knn: k_nearest and k_farthest must be in [0, 64]");
  if ((kn > 0 && !near_out) || (kf > 0 && !far_out)) return awv_internal_fail(AWV_ERR_ARG, "sketch_knn: null output");
  const int n = v.n;
  if (kn + kf == 0 || n == 0) return AWV_OK;
  // rows in blocks whose counts take at most 128 MiB
  const int R = (int)std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)64 << 20) / n));
  AWV_TRY(ps->d_counts.reserve((size_t)R * n));
  AWV_TRY(ps->d_near.reserve((size_t)n * std::max(kn, 1)));
  AWV_TRY(ps->d_far.reserve((size_t)n * std::max(kf, 1)));
  for (int r0 = 0; r0 < n; r0 += R) {
    const int nr = std::min(R, n - r0);
    if (int rc = rows_launch(v, *sk, *sk, r0, nr, ps->d_counts.p)) return rc;
    hipLaunchKernelGGL(awp_knn_kernel, dim3((nr + KNN_WG / 64 - 1) / (KNN_WG / 64)), dim3(KNN_WG), 0, v.stream,
                       (const uint16_t*)ps->d_counts.p, (const uint32_t*)sk->d_cnt.p, r0, nr, n, kn, kf, ps->d_near.p, ps->d_far.p);
    AWV_TRY(hipGetLastError());
  }
  if (kn) AWV_TRY(hipMemcpyAsync(near_out, ps->d_near.p, (size_t)n * kn * 4, hipMemcpyDeviceToHost, v.stream));
  if (kf) AWV_TRY(hipMemcpyAsync(far_out, ps->d_far.p, (size_t)n * kf * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

int keep_core(awv_engine* e, int n, const uint8_t* id_bytes, const uint64_t* id_off, uint64_t threshold, int keep_all, int include_diag,
              uint32_t* bitmap) {
  if (!e) return awv_internal_null_engine();
  EngineView v;
  {
    const int rc = awv_internal_view(e, &v);  // (the keep test reads no sequence: an engine without a set will do)
    if (rc != AWV_OK && rc != AWV_ERR_STATE) return rc;
  }
  if (n < 0 || (n > 0 && (!id_off || !bitmap))) return awv_internal_fail(AWV_ERR_ARG, "keep_pairs: null argument");
  if (n == 0) return AWV_OK;
  for (int i = 0; i < n; ++i)
    if (id_off[i + 1] < id_off[i] || id_off[i + 1] - id_off[i] > (1u << 20)) return awv_internal_fail(AWV_ERR_ARG, "keep_pairs: bad id offsets");
  if (id_off[n] > 0 && !id_bytes) return awv_internal_fail(AWV_ERR_ARG, "keep_pairs: null id bytes");
  AWV_TRY(hipSetDevice(v.device));
  PlanState*& slot = awv_internal_plan(e);
  if (!slot) slot = new PlanState();
  PlanState* ps = slot;
  const int words = (n + 31) / 32;
  const size_t nw = (size_t)n * words;
  AWV_TRY(ps->d_bytes.reserve((size_t)id_off[n] - id_off[0] + 1));
  AWV_TRY(ps->d_u64.reserve((size_t)n + 1));
  AWV_TRY(ps->d_u32.reserve(nw));
  std::vector<uint64_t> off((size_t)n + 1);
  for (int i = 0; i <= n; ++i) off[i] = id_off[i] - id_off[0];
  if (off[n]) AWV_TRY(hipMemcpyAsync(ps->d_bytes.p, id_bytes + id_off[0], (size_t)off[n], hipMemcpyHostToDevice, v.stream));
  AWV_TRY(hipMemcpyAsync(ps->d_u64.p, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, v.stream));
  hipLaunchKernelGGL(awp_keep_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, v.stream, (const uint8_t*)ps->d_bytes.p,
                     (const uint64_t*)ps->d_u64.p, n, words, threshold, keep_all, include_diag, ps->d_u32.p);
  AWV_TRY(hipGetLastError());
  AWV_TRY(hipMemcpyAsync(bitmap, ps->d_u32.p, nw * 4, hipMemcpyDeviceToHost, v.stream));
  AWV_TRY(hipStreamSynchronize(v.stream));
  return AWV_OK;
}

}  // namespace

extern "C" {

int awv_sketch(awv_engine* e, int32_t kind, int32_t k, int32_t s, uint32_t* sizes) {
  AWV_GUARDED(return sketch_core(e, kind, k, s, sizes);)
}

int awv_sketch_copy(awv_engine* e, int32_t kind, uint64_t* offsets, uint64_t* hashes) {
  AWV_GUARDED(return sketch_copy_core(e, kind, offsets, hashes);)
}

int awv_sketch_pair_counts(awv_engine* e, int32_t kind_a, int32_t kind_b, const int32_t* a, const int32_t* b, int64_t npairs,
                           uint16_t* inter) {
  AWV_GUARDED(return pair_counts_core(e, kind_a, kind_b, a, b, npairs, inter);)
}

int awv_sketch_rows(awv_engine* e, int32_t kind, int32_t row0, int32_t nrows, uint16_t* inter) {
  AWV_GUARDED(return rows_core(e, kind, row0, nrows, inter);)
}

int awv_sketch_knn(awv_engine* e, int32_t kind, int32_t k_nearest, int32_t k_farthest, int32_t* nearest, int32_t* farthest) {
  AWV_GUARDED(return knn_core(e, kind, k_nearest, k_farthest, nearest, farthest);)
}

int awv_keep_pairs(awv_engine* e, int32_t n, const uint8_t* id_bytes, const uint64_t* id_offsets, uint64_t threshold, int32_t keep_all,
                   int32_t include_diag, uint32_t* bitmap) {
  AWV_GUARDED(return keep_core(e, n, id_bytes, id_offsets, threshold, keep_all, include_diag, bitmap);)
}

}  // extern "C"
