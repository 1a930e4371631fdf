/*
 * gotoh.c -- independent full-DP optimum for gap-affine / 2-piece gap-affine global alignment.
 *
 * TEST INFRASTRUCTURE ONLY (see biwfa_oracle.h).  This is the anchor that pins the oracle's
 * penalty: an exact WFA with no heuristic (alignment.rs:228 sets HeuristicStrategy::None)
 * returns the optimum, so WFA2-lib's penalty == this DP's by definition.
 * Gap of length L costs min(o1 + L*e1, o2 + L*e2); match = 0, mismatch = x.
 * O(plen * tlen) time, O(tlen) memory -- for cross-checks at <= a few kbp.  awo_gotoh_penalty_banded below runs the
 * same recurrences on the diagonals a path of cost <= bound can reach: exact up to that bound at 20-150 kbp.
 */
#include "biwfa_oracle.h"

#include <stdlib.h>

#define INF ((int64_t)1 << 50)
static inline int64_t min2(int64_t a, int64_t b) { return a < b ? a : b; }

int64_t awo_gotoh_penalty(const uint8_t* pattern, int plen, const uint8_t* text, int tlen,
                          const awo_penalties_t* pen) {
  const int64_t x = pen->mismatch, o1 = pen->gap_open1, e1 = pen->gap_ext1;
  const int64_t o2 = pen->two_piece ? pen->gap_open2 : INF, e2 = pen->two_piece ? pen->gap_ext2 : 0;
  const size_t n = (size_t)tlen + 1;
  /* rows over j (text); i (pattern) advances row by row */
  int64_t* M = (int64_t*)malloc(5 * n * sizeof(int64_t));
  if (!M) return -1;
  int64_t* I1 = M + n; /* gap consuming text (horizontal) */
  int64_t* I2 = I1 + n;
  int64_t* D1 = I2 + n; /* gap consuming pattern (vertical) */
  int64_t* D2 = D1 + n;
  M[0] = 0;
  I1[0] = I2[0] = D1[0] = D2[0] = INF;
  for (int j = 1; j <= tlen; ++j) {
    I1[j] = min2(M[j - 1] + o1 + e1, I1[j - 1] + e1);
    I2[j] = min2(M[j - 1] + o2 + e2, I2[j - 1] + e2);
    D1[j] = D2[j] = INF;
    M[j] = min2(I1[j], I2[j]);
  }
  for (int i = 1; i <= plen; ++i) {
    int64_t diag = M[0]; /* M[i-1][j-1] */
    D1[0] = min2(M[0] + o1 + e1, D1[0] + e1);
    D2[0] = min2(M[0] + o2 + e2, D2[0] + e2);
    I1[0] = I2[0] = INF;
    M[0] = min2(D1[0], D2[0]);
    const uint8_t pc = pattern[i - 1];
    for (int j = 1; j <= tlen; ++j) {
      const int64_t up = M[j]; /* M[i-1][j] */
      const int64_t d1 = min2(up + o1 + e1, D1[j] + e1);
      const int64_t d2 = min2(up + o2 + e2, D2[j] + e2);
      const int64_t i1 = min2(M[j - 1] + o1 + e1, I1[j - 1] + e1);
      const int64_t i2 = min2(M[j - 1] + o2 + e2, I2[j - 1] + e2);
      int64_t m = diag + (pc == text[j - 1] ? 0 : x);
      m = min2(m, min2(min2(d1, d2), min2(i1, i2)));
      diag = up;
      D1[j] = d1;
      D2[j] = d2;
      I1[j] = i1;
      I2[j] = i2;
      M[j] = m;
    }
  }
  const int64_t r = M[tlen];
  free(M);
  return r;
}

/* ---- banded exact DP --------------------------------------------------------------------------------------------
 * A path that visits diagonal k = j - i goes from diagonal 0 to k and on to dl = tlen - plen, so it holds at least
 * |k| + |k - dl| gap bases.  Since o >= 0 for both pieces, g(a) + g(b) >= g(a + b) for g(L) = min over pieces of
 * (o + L*e): splitting gap bases over several gaps never costs less than one gap of their total length.  So a path of
 * cost <= bound stays on diagonals k with g(|dl| + 2 * dist(k, [min(0, dl), max(0, dl)])) <= bound, and the DP restricted
 * to those diagonals finds every such path. */

/* the longest gap that costs at most bound (-1: none does) */
static int64_t longest_gap_within(const awo_penalties_t* pen, int64_t bound) {
  int64_t L = -1;
  if (pen->gap_open1 <= bound) L = (bound - pen->gap_open1) / pen->gap_ext1;
  if (pen->two_piece && pen->gap_open2 <= bound) {
    const int64_t L2 = (bound - pen->gap_open2) / pen->gap_ext2;
    if (L2 > L) L = L2;
  }
  return L;
}

int awo_gotoh_band(int plen, int tlen, const awo_penalties_t* pen, int64_t bound, int64_t* lo, int64_t* hi) {
  const int64_t dl = (int64_t)tlen - plen, adl = dl < 0 ? -dl : dl;
  if (bound < 0) return -1;
  const int64_t L = longest_gap_within(pen, bound);
  if (adl > 0 && L < adl) return -1; /* the forced gap alone costs more than bound */
  const int64_t m = L >= adl ? (L - adl) / 2 : 0;
  int64_t l = (dl < 0 ? dl : 0) - m, h = (dl > 0 ? dl : 0) + m;
  if (l < -(int64_t)plen) l = -(int64_t)plen;
  if (h > tlen) h = tlen;
  *lo = l;
  *hi = h;
  return 0;
}

int64_t awo_gotoh_penalty_band(const uint8_t* pattern, int plen, const uint8_t* text, int tlen,
                               const awo_penalties_t* pen, int64_t lo, int64_t hi) {
  const int64_t dl = (int64_t)tlen - plen;
  if (lo < -(int64_t)plen) lo = -(int64_t)plen;
  if (hi > tlen) hi = tlen;
  if (lo > 0 || hi < 0 || dl < lo || dl > hi) return INF; /* no path from (0, 0) to (plen, tlen) inside the band */
  const int64_t x = pen->mismatch, oe1 = (int64_t)pen->gap_open1 + pen->gap_ext1, e1 = pen->gap_ext1;
  const int64_t oe2 = pen->two_piece ? (int64_t)pen->gap_open2 + pen->gap_ext2 : INF;
  const int64_t e2 = pen->two_piece ? pen->gap_ext2 : 0;
  /* one slot per diagonal plus an INF slot at each end; row i is updated in place in ascending k: slot k + 1 still holds
   * row i - 1 (the cell above), slot k holds row i - 1 until written (the diagonal predecessor), slot k - 1 row i (left).
   * Slots of diagonals a row does not reach (j < 0 or j > tlen) are never written once they fall out of reach, so they
   * read INF. */
  const size_t w = (size_t)(hi - lo + 1) + 2;
  int64_t* buf = (int64_t*)malloc(5 * w * sizeof(int64_t));
  if (!buf) return -1;
  for (size_t s = 0; s < 5 * w; ++s) buf[s] = INF;
  int64_t* M = buf; /* M[z + k] for lo - 1 <= k <= hi + 1 */
  int64_t* I1 = M + w;
  int64_t* I2 = I1 + w;
  int64_t* D1 = I2 + w;
  int64_t* D2 = D1 + w;
  const int64_t z = 1 - lo;
  for (int64_t i = 0; i <= plen; ++i) {
    const int64_t kl = lo > -i ? lo : -i, kh = hi < tlen - i ? hi : tlen - i;
    const uint8_t pc = i > 0 ? pattern[i - 1] : 0;
    for (int64_t k = kl; k <= kh; ++k) {
      const int64_t j = i + k, c = z + k;
      const int64_t d1 = min2(M[c + 1] + oe1, D1[c + 1] + e1);
      const int64_t d2 = min2(M[c + 1] + oe2, D2[c + 1] + e2);
      const int64_t i1 = min2(M[c - 1] + oe1, I1[c - 1] + e1);
      const int64_t i2 = min2(M[c - 1] + oe2, I2[c - 1] + e2);
      int64_t m = (i > 0 && j > 0) ? M[c] + (pc == text[j - 1] ? 0 : x) : (i == 0 && j == 0 ? 0 : INF);
      m = min2(m, min2(min2(d1, d2), min2(i1, i2)));
      D1[c] = d1;
      D2[c] = d2;
      I1[c] = i1;
      I2[c] = i2;
      M[c] = m;
    }
  }
  const int64_t r = M[z + dl];
  free(buf);
  return r;
}

int64_t awo_gotoh_penalty_banded(const uint8_t* pattern, int plen, const uint8_t* text, int tlen,
                                 const awo_penalties_t* pen, int64_t bound) {
  /* I and D cost the same, so the penalty is symmetric: sweep rows over the shorter sequence */
  if (plen > tlen) {
    const uint8_t* s = pattern;
    pattern = text;
    text = s;
    const int n = plen;
    plen = tlen;
    tlen = n;
  }
  if (bound < 0) return bound + 1;
  /* every pair has an alignment of cost <= u (the shorter sequence base by base, then one gap): a larger bound only
   * widens the band */
  const int64_t dl = (int64_t)tlen - plen;
  int64_t u = (int64_t)plen * pen->mismatch;
  if (dl > 0) {
    int64_t g = (int64_t)pen->gap_open1 + dl * pen->gap_ext1;
    if (pen->two_piece) g = min2(g, (int64_t)pen->gap_open2 + dl * pen->gap_ext2);
    u += g;
  }
  const int64_t b = min2(bound, u);
  int64_t lo, hi;
  if (awo_gotoh_band(plen, tlen, pen, b, &lo, &hi) != 0) return bound + 1;
  const int64_t r = awo_gotoh_penalty_band(pattern, plen, text, tlen, pen, lo, hi);
  if (r < 0) return r;
  return r > bound ? bound + 1 : r;
}
