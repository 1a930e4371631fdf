// row_reuse.hpp -- the arithmetic of the row archive: a top-level breakpoint search keeps the rows of its
// far-apart passes, and the searches below it that run in its frame and share a corner with it -- the forward search of the
// left child, of that child's left child and so on; the reverse search of the right child and of its chain of right children --
// take them back instead of computing them again (take_dir).
//
// A child's search starts at the parent's origin over prefixes of the parent's sequences, so as long as a parent row lies
// inside the child's box (no cell beyond the child's pattern or text end) the child computes that very row, component by
// component.  This header holds what decides and addresses that: the layout of a workgroup's archive, the box test, which
// pass of the archive a pass of the child may take, and the column shift between the two searches' rows.
//
// Plain C++ with no HIP types, usable from host and device code, so that it can be built and tested on its own
// (tests/row_reuse_driver.cpp, tests/row_reuse_levels_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWVRR_HD __host__ __device__ inline
#else
#define AWVRR_HD inline
#endif

namespace awvrr {

constexpr int NCOMP = 5;
// the archive's header: 32-bit words at the start of a workgroup's slot
enum { H_NPASS = 0,   // passes archived by the running top-level search (both directions); 0 = void
       H_KMIN0 = 1,   // that search's column origins: column = k - kmin
       H_KMIN1 = 2,
       H_RCELLS = 4,  // words 4 and 5, one 64-bit count: cell-steps this workgroup took from its archive during the launch
       H_RSEARCH = 6, // searches that took some
       H_DCELLS = 8,  // words 8 and 9, one 64-bit count: the part of H_RCELLS that searches below level 1 took
       H_DMARK = 10,  // words 10 and 11: H_RCELLS as it stood when the running search below level 1 began
       H_DNOW = 12,   // 1 while such a search runs
       H_DSMARK = 13, // H_RSEARCH as it stood when it began
       H_DSEARCH = 14, // the part of H_RSEARCH that is searches below level 1
       H_WORDS = 16 };
// per pass and direction: 32-bit words of the pass table
enum { P_MAXAK = 0,   // the pass's maximum antidiagonal 2h - k
       P_CELLS = 1,   // its cell-steps (the sum of its rows' hull widths)
       P_BOXH = 2,    // running maximum over this pass and every earlier one of maxak + hi: twice the largest text offset
       P_BOXV = 3,    // ... of maxak - lo: twice the largest pattern offset
       P_WORDS = 4 };

// One workgroup's archive: `passes` passes of T scores per direction, every pass T rows of M and `nid` rows of I/D (the rows a
// pass leaves in memory: e1 scores of I1 and D1, e2 of I2 and D2), `cols` columns of 16 bits per row.  Linear in the pass
// index: pass p covers scores p T + 1 .. (p + 1) T.
struct Layout {
  int passes, T, nid, cols;
  AWVRR_HD int rows_per_pass() const { return T + nid; }
  AWVRR_HD int scores() const { return passes * T; }
  // a row at score s spans at most s diagonals either side of the origin (a hull grows by one diagonal per score at most)
  AWVRR_HD int reach() const { return scores(); }
  AWVRR_HD size_t table_off() const { return (size_t)H_WORDS * 4; }
  AWVRR_HD size_t table_index(int dir, int pass) const { return ((size_t)dir * passes + pass) * P_WORDS; }  // in words
  AWVRR_HD size_t meta_off() const { return table_off() + (size_t)2 * passes * P_WORDS * 4; }
  // hull of component c at score s (1 .. scores()): two 16-bit values lo, hi (empty: lo > hi), as one 32-bit word
  AWVRR_HD size_t meta_index(int dir, int s, int c) const { return ((size_t)dir * scores() + (s - 1)) * NCOMP + c; }  // in words
  AWVRR_HD size_t rows_off() const { return (meta_off() + (size_t)2 * scores() * NCOMP * 4 + 15) & ~(size_t)15; }
  // row r of pass p: r < T is the M row of score p T + 1 + r, r >= T the (r - T)-th I/D row
  AWVRR_HD size_t row_index(int dir, int pass, int r) const { return ((size_t)dir * passes + pass) * rows_per_pass() + r; }
  AWVRR_HD size_t row_off(int dir, int pass, int r) const { return rows_off() + row_index(dir, pass, r) * cols * 2; }
  AWVRR_HD size_t bytes() const { return (rows_off() + (size_t)2 * passes * rows_per_pass() * cols * 2 + 255) & ~(size_t)255; }
};

// columns of a row that holds every hull of the first `scores` scores as whole lane vectors of 4, whatever the origin (a multiple of 4)
AWVRR_HD int cols_for(int scores) { return (2 * (scores + 8) + 8 + 3) & ~3; }
AWVRR_HD Layout make_layout(int passes, int T, int nid) { return Layout{passes, T, nid, cols_for(passes * T)}; }

// the archive's first column in the recording search's column space (a multiple of 4, like every lane vector's first column)
AWVRR_HD int first_col(const Layout& l, int kmin) { return (-(l.reach() + 8) - kmin) & ~3; }
// a hull [lo, hi] that the archive's rows can hold
AWVRR_HD bool hull_fits(const Layout& l, int lo, int hi) { return lo > hi || (lo >= -l.reach() && hi <= l.reach()); }
// the M row of score s: which pass, which row of it
AWVRR_HD int pass_of(const Layout& l, int s) { return (s - 1) / l.T; }
AWVRR_HD int row_of(const Layout& l, int s) { return (s - 1) % l.T; }
// the I/D rows behind a pass's M rows, in the order I1 (e1 scores, ascending), D1, I2 (e2 scores), D2; components as the kernels
// number them (1 = I1, 2 = I2, 3 = D1, 4 = D2).  j counts back from the pass's last score: j = 0 is that score.
AWVRR_HD int id_row(const Layout& l, int e1, int e2, int comp, int j) {
  const int base = comp == 1 ? 0 : comp == 3 ? e1 : comp == 2 ? 2 * e1 : 2 * e1 + e2;
  const int e = (comp == 1 || comp == 3) ? e1 : e2;
  return l.T + base + (e - 1 - j);
}

// The box test.  boxh / boxv are a pass's P_BOXH / P_BOXV; the child's sequences are plen and tlen long.  Every cell of every
// row up to that pass then has h <= tlen and h - k <= plen.
AWVRR_HD bool box_ok(int boxh, int boxv, int plen, int tlen) { return boxh <= 2 * tlen && boxv <= 2 * plen; }

// Which archived pass a pass of the child may take: the child stands at score sc and has chosen a pass of Tc scores.  It must
// be the archive's own pass length and start on one of its boundaries, and the pass must be there.  -1: none.
AWVRR_HD int pass_for(const Layout& l, int npass, int sc, int Tc) {
  if (Tc != l.T || sc < 0 || sc % l.T != 0) return -1;
  const int p = sc / l.T;
  return p < npass && p < l.passes ? p : -1;
}

// Whose rows an archive holds, and who may take them.  A search's forward rows depend on its origin corner, its begin
// component and the sequences from that corner on, and on nothing else; its reverse rows on its end corner and its end
// component in the same way.  The top-level search runs from (0, 0) to (plen, tlen) with M at either end, so every task below
// it, in its frame, that begins at (0, 0) in M computes the archive's forward rows for as long as they lie inside its box (the
// left half, the left half's left half, ...), and every task that ends at (plen, tlen) in M its reverse rows.  Where the
// task's other end lies decides only which half it is: the level-1 rule asks for it, the general rule does not.
// Coordinates in the unit's frame; component 0 is M.
struct RootId { int plen, tlen, bv, bh, bcomp; };  // the recorded search: its lengths, its breakpoint's pattern / text offset and component
struct TaskId { int pb, pe, tb, te, cb, ce; };
constexpr int LV_ALL = 0, LV_ONE = 1;  // who takes: every task with the archive's corner and component / the two level-1 tasks only
// The frame rule.  A twin unit's shared search runs in A's frame and so do its shared tasks and A's own; B's own tasks (after a
// four-way split, or when B runs alone) have pattern and text swapped.  A task takes only from an archive recorded in its own
// frame: the same frame, or A's task under a shared top-level search.  (The kernel's TM_A / TM_B / TM_SHARED.)
constexpr int FR_A = 0, FR_B = 1, FR_SHARED = 2;
AWVRR_HD bool frame_ok(int root_frame, int task_frame) { return task_frame == root_frame || (root_frame == FR_SHARED && task_frame == FR_A); }
// the direction `t` takes from the root's archive (0 forward, 1 reverse; -1: none); *level1: it is one of the root's two halves
AWVRR_HD int take_dir(const RootId& r, const TaskId& t, int levels, bool* level1) {
  const bool fwd = t.pb == 0 && t.tb == 0 && t.cb == 0, rev = t.pe == r.plen && t.te == r.tlen && t.ce == 0;
  *level1 = true;
  if (fwd && t.pe == r.bv && t.te == r.bh && t.ce == r.bcomp) return 0;
  if (rev && t.pb == r.bv && t.tb == r.bh && t.cb == r.bcomp) return 1;
  *level1 = false;
  if (levels == LV_ONE) return -1;
  return fwd ? 0 : rev ? 1 : -1;
}

// ---- host side: how many passes a launch's archives hold ----------------------------------------------------------------
// The children's far-apart zones end near a quarter of the pair's score.  The score is not known before the launch; for the
// reads this is built for it is about one seventh of the summed lengths, so the cap is maxsum / 28 scores, at most 4096, in
// whole passes -- and fewer when `nslots` archives of that size would not fit `avail` bytes.  Fewer than 4 passes: none.
inline int plan_passes(int maxsum, int T, int nid, long long nslots, unsigned long long avail) {
  if (T < 2 || nslots <= 0) return 0;
  int passes = (maxsum / 28 < 4096 ? maxsum / 28 : 4096) / T;
  while (passes >= 4 && (unsigned long long)make_layout(passes, T, nid).bytes() * (unsigned long long)nslots > avail) passes = passes * 3 / 4;
  return passes >= 4 ? passes : 0;
}

}  // namespace awvrr
