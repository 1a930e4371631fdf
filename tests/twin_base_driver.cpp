// Stand-alone driver around allwave_amd/csrc/twin_base.hpp for tests/test_twin_base_cpu.py (built with the system compiler
// under -fsanitize=address,undefined): the proof on the CPU that a base case's history, kept for the pair (P, T), gives the
// swapped pair (T, P) its op string through the mirror rule.
//
// A scalar WFA with full history, gap-affine and 2-piece, as oracle/biwfa_oracle.c states it (limits, the M row's bounds
// check, trimmed ends, a row beyond its own ends reads as NULL), and the backtrace with the kernel's candidate table: nine
// candidates packed (offset << 4) | type, the largest wins.  The backtrace reads its cells through a function, so the same
// loop runs on a problem's own history and, through twin_base.hpp, on its twin's.
//
// stdin, per line:  x o1 e1 o2 e2 two_piece cb ce P T      (components as the kernels number them: M I1 I2 D1 D2)
// stdout, per line: penalty ops(P,T) ops(T,P) ops(T,P)-from-(P,T)'s-history
// Exit status 1 when the last two differ on some line, 2 on an alignment that fails.
#include <algorithm>
#include <array>
#include <cstdio>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "twin_base.hpp"

namespace {

constexpr int NUL = -(1 << 28);
constexpr int SCORE_CAP = 250;  // FALLBACK_MIN_SCORE: what a base case below a search can cost
enum { C_M = 0, C_I1 = 1, C_I2 = 2, C_D1 = 3, C_D2 = 4, NCOMP = 5 };
enum { BT_I1_OPEN = 1, BT_I1_EXT, BT_I2_OPEN, BT_I2_EXT, BT_D1_OPEN, BT_D1_EXT, BT_D2_OPEN, BT_D2_EXT, BT_M };

struct Pen { int x, o1, e1, o2, e2; bool p2; };

struct Row {
  bool present = false, null = true;
  int lo = 1, hi = -1, base = 0;
  std::vector<int> off;
  int at(int k) const { return (k < lo || k > hi) ? NUL : off[(size_t)(k - base)]; }
};

struct Wfa {
  Pen pn;
  std::string P, T;
  int plen, tlen, cb, ce, end_score = -1;
  std::vector<std::array<Row, NCOMP>> rows;
  Row none;

  const Row& fetch(int c, int s) const {
    if (s < 0 || s >= (int)rows.size() || !rows[(size_t)s][(size_t)c].present) return none;
    return rows[(size_t)s][(size_t)c];
  }
  // what a backtrace may read: NUL outside the row
  int at(int c, int s, int k) const { return fetch(c, s).at(k); }

  void trim(Row& w) const {
    int k;
    for (k = w.hi; k >= w.lo; --k) {
      const int o = w.off[(size_t)(k - w.base)];
      if ((unsigned)o <= (unsigned)tlen && (unsigned)(o - k) <= (unsigned)plen) break;
    }
    w.hi = k;
    for (k = w.lo; k <= w.hi; ++k) {
      const int o = w.off[(size_t)(k - w.base)];
      if ((unsigned)o <= (unsigned)tlen && (unsigned)(o - k) <= (unsigned)plen) break;
    }
    w.lo = k;
    w.null = w.lo > w.hi;
  }

  void compute(int s) {
    rows.emplace_back();
    const Row& mx = fetch(C_M, s - pn.x);
    const Row& mo1 = fetch(C_M, s - pn.o1 - pn.e1);
    const Row& i1 = fetch(C_I1, s - pn.e1);
    const Row& d1 = fetch(C_D1, s - pn.e1);
    const Row& mo2 = pn.p2 ? fetch(C_M, s - pn.o2 - pn.e2) : none;
    const Row& i2 = pn.p2 ? fetch(C_I2, s - pn.e2) : none;
    const Row& d2 = pn.p2 ? fetch(C_D2, s - pn.e2) : none;
    if (mx.null && mo1.null && i1.null && d1.null && mo2.null && i2.null && d2.null) return;  // a null step: no row
    int lo = mx.lo, hi = mx.hi;
    lo = std::min(lo, mo1.lo - 1); hi = std::max(hi, mo1.hi + 1);
    lo = std::min(lo, i1.lo + 1);  hi = std::max(hi, i1.hi + 1);
    lo = std::min(lo, d1.lo - 1);  hi = std::max(hi, d1.hi - 1);
    if (pn.p2) {
      lo = std::min(lo, mo2.lo - 1); hi = std::max(hi, mo2.hi + 1);
      lo = std::min(lo, i2.lo + 1);  hi = std::max(hi, i2.hi + 1);
      lo = std::min(lo, d2.lo - 1);  hi = std::max(hi, d2.hi - 1);
    }
    std::array<Row, NCOMP>& out = rows.back();
    for (int c = 0; c < NCOMP; ++c) {
      if (!pn.p2 && (c == C_I2 || c == C_D2)) continue;
      Row& w = out[(size_t)c];
      w.present = true;
      w.null = false;
      w.lo = lo; w.hi = hi; w.base = lo;
      w.off.assign((size_t)(hi - lo + 1), NUL);
    }
    for (int k = lo; k <= hi; ++k) {
      const size_t j = (size_t)(k - lo);
      const int ins1 = std::max(mo1.at(k - 1), i1.at(k - 1)) + 1;
      const int del1 = std::max(mo1.at(k + 1), d1.at(k + 1));
      out[C_I1].off[j] = ins1;
      out[C_D1].off[j] = del1;
      int best = std::max(del1, std::max(mx.at(k) + 1, ins1));
      if (pn.p2) {
        const int ins2 = std::max(mo2.at(k - 1), i2.at(k - 1)) + 1;
        const int del2 = std::max(mo2.at(k + 1), d2.at(k + 1));
        out[C_I2].off[j] = ins2;
        out[C_D2].off[j] = del2;
        best = std::max(best, std::max(ins2, del2));
      }
      if ((unsigned)best > (unsigned)tlen || (unsigned)(best - k) > (unsigned)plen) best = NUL;
      out[C_M].off[j] = best;
    }
    for (int c = 0; c < NCOMP; ++c)
      if (out[(size_t)c].present) trim(out[(size_t)c]);
  }

  // extends the M row of score s; whether the end component has reached (plen, tlen)
  bool extend(int s) {
    Row& m = rows[(size_t)s][C_M];
    if (!m.present) return false;
    for (int k = m.lo; k <= m.hi; ++k) {
      int& o = m.off[(size_t)(k - m.base)];
      if (o < 0) continue;
      while (o < tlen && o - k < plen && P[(size_t)(o - k)] == T[(size_t)o]) ++o;
    }
    const Row& w = rows[(size_t)s][(size_t)ce];
    const int k_end = tlen - plen;
    return w.present && w.lo <= k_end && k_end <= w.hi && w.at(k_end) >= tlen;
  }

  // 0, or 1 when the alignment costs more than SCORE_CAP
  int run() {
    rows.emplace_back();
    Row& w = rows[0][(size_t)cb];
    w.present = true;
    w.null = false;
    w.lo = w.hi = w.base = 0;
    w.off.assign(1, 0);
    for (int s = 0;; ) {
      if (extend(s)) { end_score = s; return 0; }
      if (++s > SCORE_CAP) return 1;
      compute(s);
    }
  }
};

// The kernel's backtrace (biwfa_device.hpp, base_align) in the frame the arguments name; `cell(comp, score, k)` is the text
// offset stored there, negative for none.  Returns false on an inconsistent history.
bool backtrace(const Pen& pn, int plen, int tlen, int ce, int score, const std::function<int(int, int, int)>& cell, std::string& ops) {
  (void)plen;
  std::string rev;
  int matrix = ce, sc = score, k = tlen - plen, offset = tlen;
  int h = offset, v = offset - k;
  long guard = 0;
  while (v > 0 && h > 0 && sc > 0) {
    if (++guard > 4L * (plen + tlen) + 16) return false;
    const int mismatch = sc - pn.x, gap_open1 = sc - pn.o1 - pn.e1, gap_extend1 = sc - pn.e1;
    const int gap_open2 = sc - pn.o2 - pn.e2, gap_extend2 = sc - pn.e2;
    int max_all = -1;
    for (int lane = 0; lane < 9; ++lane) {
      int ms;  // 0: M by a mismatch; 1 / 2: I1 opened / extended; 3 / 4: D1; 5 / 6: I2; 7 / 8: D2
      if (matrix == C_M) ms = lane <= (pn.p2 ? 8 : 4) ? lane : -1;
      else {
        const int ext = matrix == C_I1 ? 2 : matrix == C_D1 ? 4 : matrix == C_I2 ? 6 : 8;
        ms = lane == 0 ? ext : lane == 1 ? ext - 1 : -1;
      }
      if (ms < 0) continue;
      const bool open = (ms & 1) != 0, two = ms >= 5, ins = ms == 1 || ms == 2 || ms == 5 || ms == 6;
      const int comp = (ms == 0 || open) ? C_M : ms == 2 ? C_I1 : ms == 4 ? C_D1 : ms == 6 ? C_I2 : C_D2;
      const int cs = ms == 0 ? mismatch : sc - (two ? pn.e2 : pn.e1) - (open ? (two ? pn.o2 : pn.o1) : 0);
      const int ck = ms == 0 ? k : ins ? k - 1 : k + 1;
      const int add = (ms == 0 || ins) ? 1 : 0;
      const int type = ms == 0 ? BT_M : ms == 1 ? BT_I1_OPEN : ms == 2 ? BT_I1_EXT : ms == 3 ? BT_D1_OPEN : ms == 4 ? BT_D1_EXT
                     : ms == 5 ? BT_I2_OPEN : ms == 6 ? BT_I2_EXT : ms == 7 ? BT_D2_OPEN : BT_D2_EXT;
      const int val = cs >= 0 ? cell(comp, cs, ck) : -1;
      if (val >= 0) max_all = std::max(max_all, ((val + add) << 4) | type);
    }
    if (max_all < 0) return false;
    if (matrix == C_M) {
      const int max_offset = max_all >> 4;
      if (offset - max_offset < 0) return false;
      rev.append((size_t)(offset - max_offset), 'M');
      offset = max_offset;
      v = offset - k;
      h = offset;
      if (v <= 0 || h <= 0) break;
    }
    const int bt = max_all & 0xF;
    switch (bt) {
      case BT_M: sc = mismatch; matrix = C_M; break;
      case BT_I1_OPEN: sc = gap_open1; matrix = C_M; break;
      case BT_I1_EXT: sc = gap_extend1; matrix = C_I1; break;
      case BT_I2_OPEN: sc = gap_open2; matrix = C_M; break;
      case BT_I2_EXT: sc = gap_extend2; matrix = C_I2; break;
      case BT_D1_OPEN: sc = gap_open1; matrix = C_M; break;
      case BT_D1_EXT: sc = gap_extend1; matrix = C_D1; break;
      case BT_D2_OPEN: sc = gap_open2; matrix = C_M; break;
      default: sc = gap_extend2; matrix = C_D2; break;
    }
    if (bt == BT_M) { rev.push_back('X'); --offset; }
    else if (bt <= BT_I2_EXT) { rev.push_back('I'); --k; --offset; }
    else { rev.push_back('D'); ++k; }
    v = offset - k;
    h = offset;
  }
  if (matrix == C_M) {
    if (v > 0 && h > 0) {
      const int nm = std::min(v, h);
      rev.append((size_t)nm, 'M');
      v -= nm;
      h -= nm;
    }
    if (v > 0) rev.append((size_t)v, 'D');
    if (h > 0) rev.append((size_t)h, 'I');
  } else if (v != 0 || h != 0 || sc != 0) {
    return false;
  }
  ops.assign(rev.rbegin(), rev.rend());
  return true;
}

}  // namespace

int main() {
  std::string line;
  int differ = 0;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    ++n;
    std::istringstream in(line);
    Pen pn;
    int p2, cb, ce;
    std::string P, T;
    if (!(in >> pn.x >> pn.o1 >> pn.e1 >> pn.o2 >> pn.e2 >> p2 >> cb >> ce >> P >> T)) return 3;
    pn.p2 = p2 != 0;
    Wfa a, b;
    a.pn = b.pn = pn;
    a.P = P; a.T = T; a.plen = (int)P.size(); a.tlen = (int)T.size(); a.cb = cb; a.ce = ce;
    b.P = T; b.T = P; b.plen = a.tlen; b.tlen = a.plen; b.cb = awvb::twin_comp(cb); b.ce = awvb::twin_comp(ce);
    if (a.run() != 0 || b.run() != 0 || a.end_score != b.end_score) {
      std::fprintf(stderr, "line %ld: no alignment within %d (or two penalties: %d, %d)\n", n, SCORE_CAP, a.end_score, b.end_score);
      return 2;
    }
    std::string ops_a, ops_b, ops_m;
    const bool ok_a = backtrace(pn, a.plen, a.tlen, a.ce, a.end_score, [&](int c, int s, int k) { return a.at(c, s, k); }, ops_a);
    const bool ok_b = backtrace(pn, b.plen, b.tlen, b.ce, b.end_score, [&](int c, int s, int k) { return b.at(c, s, k); }, ops_b);
    // the swapped pair's backtrace on A's history: every cell through the mirror rule, the start from A's end turned round
    const awvb::Start st = awvb::start_in_b(a.ce, a.plen, a.tlen);
    if (st.k != st.tlen - st.plen || st.offset != st.tlen) return 4;
    const bool ok_m = backtrace(pn, st.plen, st.tlen, st.comp, a.end_score, [&](int c, int s, int k) {
      const awvb::Cell in_a = awvb::cell_in_a(c, k);
      return awvb::offset_in_b(a.at(in_a.comp, s, in_a.k), in_a.k);
    }, ops_m);
    if (!ok_a || !ok_b || !ok_m) {
      std::fprintf(stderr, "line %ld: a backtrace failed (%d %d %d)\n", n, (int)ok_a, (int)ok_b, (int)ok_m);
      return 2;
    }
    if (ops_b != ops_m) {
      ++differ;
      std::fprintf(stderr, "line %ld: the mirrored backtrace differs\n  direct %s\n  mirror %s\n", n, ops_b.c_str(), ops_m.c_str());
    }
    std::printf("%d %s %s %s\n", a.end_score, ops_a.c_str(), ops_b.c_str(), ops_m.c_str());
  }
  return differ ? 1 : 0;
}
