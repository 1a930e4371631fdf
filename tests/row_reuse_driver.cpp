// Stand-alone driver around allwave_amd/csrc/row_reuse.hpp for tests/test_row_reuse_cpu.py (built with the system compiler
// under -fsanitize=address,undefined).  One command per line on stdin, one answer line each on stdout:
//   layout P T NID               -> cols table_off meta_off rows_off bytes
//   roundtrip P T NID E1 E2 KMINP KMINC
//        fills an archive of exactly bytes() bytes the way a recording search does -- every row's hull as wide as a row can be
//        at its score, [-s, s], stored as whole lane vectors of 4 columns from the recording search's origin KMINP -- and reads
//        every cell back the way a taking search with origin KMINC does; -> "ok CELLS" or "bad ..." (the sanitizer sees any
//        access outside the buffer)
//   box BOXH BOXV PLEN TLEN      -> 0 | 1
//   pass P T NID NPASS SC TC     -> pass index or -1
//   plan MAXSUM T NID NSLOTS AVAIL -> passes
#include <cstdio>
#include <cstring>
#include <vector>

#include "row_reuse.hpp"

static short cell(int dir, int comp, int score, int k) { return (short)((dir * 7919 + comp * 104729 + score * 31 + k * 3) & 0x3fff); }

static long long roundtrip(const awvrr::Layout& l, int e1, int e2, int kminP, int kminC) {
  std::vector<unsigned char> buf(l.bytes());
  std::memset(buf.data(), 0xee, buf.size());
  const int fc = awvrr::first_col(l, kminP);
  if (fc & 3) return -1;
  auto comp_of = [&](int r, int& comp, int& back) {  // row r >= T of a pass: which component, how many scores before the pass's last
    int q = r - l.T;
    if (q < e1) { comp = 1; back = e1 - 1 - q; return; }
    q -= e1;
    if (q < e1) { comp = 3; back = e1 - 1 - q; return; }
    q -= e1;
    if (q < e2) { comp = 2; back = e2 - 1 - q; return; }
    q -= e2;
    comp = 4;
    back = e2 - 1 - q;
  };
  for (int d = 0; d < 2; ++d)
    for (int p = 0; p < l.passes; ++p)
      for (int r = 0; r < l.rows_per_pass(); ++r) {
        int comp = 0, score = p * l.T + 1 + r;
        if (r >= l.T) {
          int back;
          comp_of(r, comp, back);
          score = (p + 1) * l.T - back;
          if (awvrr::id_row(l, e1, e2, comp, back) != r) return -2;
        } else if (awvrr::pass_of(l, score) != p || awvrr::row_of(l, score) != r) return -3;
        const int lo = -score, hi = score;
        if (!awvrr::hull_fits(l, lo, hi)) return -4;
        short* row = reinterpret_cast<short*>(buf.data() + l.row_off(d, p, r));
        for (int c = (lo - kminP) & ~3; c <= ((hi - kminP) | 3); ++c) {
          if (c - fc < 0 || c - fc >= l.cols) return -5;
          row[c - fc] = cell(d, comp, score, c + kminP);
        }
        if (r < l.T) {
          int* meta = reinterpret_cast<int*>(buf.data() + l.meta_off());
          for (int c = 0; c < awvrr::NCOMP; ++c) meta[l.meta_index(d, score, c)] = (lo & 0xffff) | (hi << 16);
        }
      }
  for (int d = 0; d < 2; ++d)
    for (int p = 0; p < l.passes; ++p) {
      int* tab = reinterpret_cast<int*>(buf.data() + l.table_off()) + l.table_index(d, p);
      for (int w = 0; w < awvrr::P_WORDS; ++w) tab[w] = d * 1000 + p * 10 + w;
    }
  long long cells = 0;
  for (int d = 0; d < 2; ++d)
    for (int s = 1; s <= l.scores(); ++s) {
      const int w = reinterpret_cast<int*>(buf.data() + l.meta_off())[l.meta_index(d, s, 0)];
      const int lo = (short)(w & 0xffff), hi = (short)(w >> 16);
      if (lo != -s || hi != s) return -6;
      const short* row = reinterpret_cast<const short*>(buf.data() + l.row_off(d, awvrr::pass_of(l, s), awvrr::row_of(l, s)));
      for (int c = (lo - kminC) & ~3; c <= ((hi - kminC) | 3); ++c) {
        const int k = c + kminC;
        if (k < lo || k > hi) continue;
        if (row[k - kminP - fc] != cell(d, 0, s, k)) return -7;
        ++cells;
      }
    }
  return cells;
}

int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "layout")) {
      int P, T, nid;
      if (std::scanf("%d %d %d", &P, &T, &nid) != 3) return 2;
      const awvrr::Layout l = awvrr::make_layout(P, T, nid);
      std::printf("%d %zu %zu %zu %zu\n", l.cols, l.table_off(), l.meta_off(), l.rows_off(), l.bytes());
    } else if (!std::strcmp(cmd, "roundtrip")) {
      int P, T, nid, e1, e2, kp, kc;
      if (std::scanf("%d %d %d %d %d %d %d", &P, &T, &nid, &e1, &e2, &kp, &kc) != 7) return 2;
      const long long r = roundtrip(awvrr::make_layout(P, T, nid), e1, e2, kp, kc);
      if (r < 0) std::printf("bad %lld\n", r);
      else std::printf("ok %lld\n", r);
    } else if (!std::strcmp(cmd, "box")) {
      int a, b, p, t;
      if (std::scanf("%d %d %d %d", &a, &b, &p, &t) != 4) return 2;
      std::printf("%d\n", awvrr::box_ok(a, b, p, t) ? 1 : 0);
    } else if (!std::strcmp(cmd, "pass")) {
      int P, T, nid, np, sc, tc;
      if (std::scanf("%d %d %d %d %d %d", &P, &T, &nid, &np, &sc, &tc) != 6) return 2;
      std::printf("%d\n", awvrr::pass_for(awvrr::make_layout(P, T, nid), np, sc, tc));
    } else if (!std::strcmp(cmd, "plan")) {
      int maxsum, T, nid;
      long long nslots;
      unsigned long long avail;
      if (std::scanf("%d %d %d %lld %llu", &maxsum, &T, &nid, &nslots, &avail) != 5) return 2;
      std::printf("%d\n", awvrr::plan_passes(maxsum, T, nid, nslots, avail));
    } else {
      return 2;
    }
  }
  return 0;
}
