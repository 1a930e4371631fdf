// twin_base.hpp -- the mirror rule of a twin unit's base case.
//
// A twin unit aligns an entry (q, t) -- "A" -- and its swapped entry (t, q) -- "B".  B's wavefronts are A's mirrored: B's
// diagonal is A's negated, B's text offset is A's pattern offset, and an insertion of one is a deletion of the other.  So the
// history that A's base case keeps for its backtrace holds every cell that B's backtrace asks for.  This header maps a cell
// that B wants -- component, score, diagonal, all in B's frame -- onto the cell of A's history that holds it, and the value
// stored there back into B's frame.  Only the backtrace's tie order tells the two orientations apart, and that runs
// unchanged in B's frame on top of this mapping.
//
// Plain C++ with no HIP types, usable from host and device code, so that it can be built and tested on its own
// (tests/twin_base_driver.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWVB_HD __host__ __device__ inline
#else
#define AWVB_HD inline
#endif

namespace awvb {

// components as the kernels number them: 0 = M, 1 = I1, 2 = I2, 3 = D1, 4 = D2
AWVB_HD int twin_comp(int c) { return c == 0 ? 0 : (c <= 2 ? c + 2 : c - 2); }

// Where B's cell (comp_b, score, k_b) lies in A's history.  The score is the same.
struct Cell { int comp, k; };
AWVB_HD Cell cell_in_a(int comp_b, int k_b) { return Cell{twin_comp(comp_b), -k_b}; }

// The text offset B reads from the value h_a that A stored on its diagonal k_a: A's pattern offset there.  NULL (any negative
// value) before or after the translation: -1.  (A row's stored lo / hi are tested against k_a by the caller, as for A.)
AWVB_HD int offset_in_b(int h_a, int k_a) {
  if (h_a < 0) return -1;
  const int h_b = h_a - k_a;
  return h_b < 0 ? -1 : h_b;
}

// B's backtrace starts from A's end turned round: the end component's twin on diagonal -k_end at text offset plen (B's text
// is A's pattern), with plen and tlen swapped.
struct Start { int comp, k, offset, plen, tlen; };
AWVB_HD Start start_in_b(int ce_a, int plen_a, int tlen_a) { return Start{twin_comp(ce_a), plen_a - tlen_a, plen_a, tlen_a, plen_a}; }

}  // namespace awvb
