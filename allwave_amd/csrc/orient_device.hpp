// orient_device.hpp -- the WFA-orientation rule (include/allwave_hip.h, above awv_orient_pairs), once, for the host and the
// device: awv_orient_decide and the race's bookkeeping kernel (orient.hip) call these functions.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "allwave_hip.h"

struct awv_engine;

namespace awo {

// per edit column of an optimal CIGAR: at least cmin, at most cmax of the penalty
struct Rule {
  int cmin, cmax;
};

__host__ __device__ inline Rule make_rule(int x, int o1, int e1, int two_piece, int o2, int e2) {
  Rule r;
  r.cmin = x < e1 ? x : e1;
  int gap1 = o1 + e1;
  if (two_piece) {
    if (e2 < r.cmin) r.cmin = e2;
    if (o2 + e2 < gap1) gap1 = o2 + e2;
  }
  r.cmax = x > gap1 ? x : gap1;
  return r;
}

// the race cannot pay when the interval [ceil(P / cmax), floor(P / cmin)] is that wide
__host__ __device__ inline bool race_pays(const Rule& r) { return (long long)r.cmax < (long long)AWV_ORIENT_SKIP_RATIO * r.cmin; }

constexpr int HI_NONE = INT32_MAX;  // a strand bounded only from below

__host__ __device__ inline long long edits_max(const Rule& r, int hi) { return (long long)hi / r.cmin; }                 // E <= floor(P / cmin)
__host__ __device__ inline long long edits_min(const Rule& r, int lo) { return ((long long)lo + r.cmax - 1) / r.cmax; }  // E >= ceil(P / cmax)

// forward iff E_f <= E_r is certain, reverse iff E_r < E_f is certain; intervals with 0 <= lo <= hi
__host__ __device__ inline int decide(const Rule& r, int lo_f, int hi_f, int lo_r, int hi_r) {
  if (hi_f != HI_NONE && edits_max(r, hi_f) <= edits_min(r, lo_r)) return AWV_ORIENT_FORWARD;
  if (hi_r != HI_NONE && edits_max(r, hi_r) < edits_min(r, lo_f)) return AWV_ORIENT_REVERSE;
  return AWV_ORIENT_UNDECIDED;
}

// One strand's penalty P is known.  The smallest lower bound L of the other strand's penalty that settles the pair is
//   P forward:  ceil(L / cmax) >= floor(P / cmin) =: E      <=>  L >= cmax (E - 1) + 1      (E = 0: settled, any L)
//   P reverse:  ceil(L / cmax) >= E + 1                     <=>  L >= cmax E + 1
// and a search under bound B that ends "above" proves L = B + 1: the bound to search under is L - 1.  -1: settled already.
// Bounds the engine treats as none (>= 2^30) come back as INT32_MAX.
__host__ __device__ inline int settling_bound(const Rule& r, int known_is_reverse, int penalty) {
  const long long E = edits_max(r, penalty);
  long long B;
  if (known_is_reverse) B = (long long)r.cmax * E;
  else if (E == 0) return -1;
  else B = (long long)r.cmax * (E - 1);
  return B >= (1LL << 30) ? INT32_MAX : (int)B;
}

// the cheapest gap of d > 0 columns (0 for d = 0): what a length difference of d forces on every alignment
__host__ __device__ inline long long gap_cost(const awv_penalties& p, long long d) {
  if (d <= 0) return 0;
  long long g = p.gap_open1 + d * p.gap_ext1;
  if (p.two_piece && p.gap_open2 + d * p.gap_ext2 < g) g = p.gap_open2 + d * p.gap_ext2;
  return g;
}

// Is a strand's search worth starting?  The losing strand is an alignment of unrelated sequences: about every second of the
// shorter length's columns a mismatch on top of the forced gap G, W = G + x min(plen, tlen) / 2 (`wrong_estimate`).  A search
// under a bound above W is expected to complete rather than to prove "above" -- and two known penalties that far apart never
// satisfy `decide`.  So with `lo` a proved lower bound of the cheaper strand's penalty, the race goes on only while the bound
// that would settle the pair, settling_bound(lo), stays within W; otherwise the pair is handed to the full alignments at
// once.  This is a cost estimate, not part of the rule: a pair given up early is decided from edit counts, as before.
__host__ __device__ inline int wrong_estimate(const awv_penalties& p, int plen, int tlen) {
  const long long d = plen > tlen ? plen - tlen : tlen - plen, m = plen < tlen ? plen : tlen;
  const long long W = gap_cost(p, d) + (long long)p.mismatch * m / 2;
  return W >= (1LL << 30) ? INT32_MAX : (int)W;
}
__host__ __device__ inline bool worth_racing(const Rule& r, int lo, int west) { return settling_bound(r, 0, lo) <= west; }

// Round 0's bound of both strands: no alignment is cheaper than the forced gap G; on top of it a slack of 1/32 of the
// shorter length at cmax each (a pair below ~3 % divergence completes in round 0) and a small constant for short
// sequences.  While neither strand completes, the slack grows by GROWTH per round.
constexpr int GROWTH = 2;
__host__ __device__ inline int first_bound(const Rule& r, const awv_penalties& p, int plen, int tlen) {
  const long long d = plen > tlen ? plen - tlen : tlen - plen, m = plen < tlen ? plen : tlen;
  const long long B = gap_cost(p, d) + (long long)r.cmax * (m / 32) + 16;
  return B >= (1LL << 30) ? INT32_MAX : (int)B;
}
__host__ __device__ inline int grown_bound(int b, int base) {  // base: the pair's G
  if (b == INT32_MAX) return b;
  const long long B = base + (long long)(b - base) * GROWTH;
  return B >= (1LL << 30) ? INT32_MAX : (int)B;
}

}  // namespace awo

// engine.hip
void awv_internal_set_stats(awv_engine* e, const awv_stats* st);
