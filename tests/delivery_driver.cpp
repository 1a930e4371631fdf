// delivery_driver.cpp -- allwave_amd/csrc/host/delivery.hpp run on the CPU (tests/test_delivery_cpu.py builds this with the
// system C++ compiler under AddressSanitizer and UBSan).  Cases on stdin, one after the other, as numbers:
//   n bounded clipping splitting has_idx div min_score n_calls
//   n entries: status penalty cigar_off cigar_len M X I D   rev idx by_div
//              clip: code score col_beg col_end q_skip t_skip M X I D penalty
//              split: code count seg_first
//   n_slots, then n_slots segments: code score col_beg col_end q_skip t_skip M X I D penalty
//   n_calls sink calls: first cnt
// Every array the Delivery names is exactly as long as the mode makes it (none where the mode has none), so a read past one
// is the sanitizer's to find.  Per case, on stdout:
//   case <filters()>
//   per sink call: "call <kept>", then per kept entry its record (status penalty score cigar_off cigar_len M X I D q_end
//   t_end), rev, idx and, when the call delivered clips, the clip's eleven fields
//   stats: bounds (pairs above_penalty above_divergence), clips (pairs empty below_min_score), splits (pairs segments empty)
#include <cstdio>
#include <iostream>
#include <vector>

#include "delivery.hpp"

static bool read_clip(awv_clip_result& c) {
  c = awv_clip_result{};
  long long score;
  if (!(std::cin >> c.code >> score >> c.col_beg >> c.col_end >> c.q_skip >> c.t_skip >> c.num_matches >> c.num_mismatches >> c.num_ins >> c.num_del >> c.penalty)) return false;
  c.score = score;
  return true;
}

static void put_clip(const awv_clip_result& c) {
  std::printf(" %d %lld %u %u %d %d %d %d %d %d %d", c.code, (long long)c.score, c.col_beg, c.col_end, c.q_skip, c.t_skip, c.num_matches,
              c.num_mismatches, c.num_ins, c.num_del, c.penalty);
}

int main() {
  long long n, n_calls, min_score;
  int bounded, clipping, splitting, has_idx;
  double div;
  while (std::cin >> n >> bounded >> clipping >> splitting >> has_idx >> div >> min_score >> n_calls) {
    std::vector<awv_result> res((size_t)n);
    std::vector<uint8_t> rev((size_t)n), by_div(bounded ? (size_t)n : 0);
    std::vector<size_t> idx(has_idx ? (size_t)n : 0);
    std::vector<awv_clip_result> clip(clipping ? (size_t)n : 0);
    std::vector<awv_split_index> index(splitting ? (size_t)n : 0);
    std::vector<uint64_t> seg_first(splitting ? (size_t)n : 0);
    for (long long i = 0; i < n; ++i) {
      awv_result& r = res[(size_t)i];
      r = awv_result{};
      unsigned long long off, ix, sf;
      int rv, bd;
      awv_clip_result c;
      awv_split_index s{};
      if (!(std::cin >> r.status >> r.penalty >> off >> r.cigar_len >> r.num_matches >> r.num_mismatches >> r.num_ins >> r.num_del >> rv >> ix >> bd)) return 2;
      if (!read_clip(c) || !(std::cin >> s.code >> s.count >> sf)) return 2;
      r.score = -r.penalty;
      r.cigar_off = off;
      r.q_end = r.num_matches + r.num_mismatches + r.num_del;
      r.t_end = r.num_matches + r.num_mismatches + r.num_ins;
      rev[(size_t)i] = (uint8_t)rv;
      if (bounded) by_div[(size_t)i] = (uint8_t)bd;
      if (has_idx) idx[(size_t)i] = (size_t)ix;
      if (clipping) clip[(size_t)i] = c;
      s.column = -1;
      if (splitting) index[(size_t)i] = s;
      if (splitting) seg_first[(size_t)i] = sf;
    }
    long long n_slots;
    if (!(std::cin >> n_slots)) return 2;
    std::vector<awv_clip_result> seg(splitting ? (size_t)n_slots : 0);
    for (long long i = 0; i < n_slots; ++i) {
      awv_clip_result c;
      if (!read_clip(c)) return 2;
      if (splitting) seg[(size_t)i] = c;
    }
    allwave::BoundStats bst;
    allwave::ClipStats cst;
    allwave::SplitStats sst;
    allwave::Delivery d;
    d.rev = rev.data();
    d.idx = has_idx ? idx.data() : nullptr;
    if (bounded) {
      d.by_div = by_div.data();
      d.div = div;
      d.bounds = &bst;
    }
    if (clipping) {
      d.clip = clip.data();
      d.min_score = min_score;
      d.clips = &cst;
    }
    if (splitting) {
      d.seg_first = seg_first.data();
      d.index = index.data();
      d.seg = seg.data();
      d.splits = &sst;
    }
    std::printf("case %d\n", d.filters() ? 1 : 0);
    for (long long c = 0; c < n_calls; ++c) {
      long long first, cnt;
      if (!(std::cin >> first >> cnt)) return 2;
      if (first < 0 || cnt < 0 || first + cnt > n) return 3;
      // (the engine hands the sink a pointer to the call's own records: res + first, exactly cnt of them)
      const std::vector<awv_result> part(res.begin() + first, res.begin() + first + cnt);
      const allwave::Delivered k = allwave::deliver(d, first, cnt, part.data());
      if (k.rev.size() != k.res.size() || k.idx.size() != k.res.size() || (!k.clip.empty() && k.clip.size() != k.res.size())) return 4;
      std::printf("call %zu\n", k.res.size());
      for (size_t i = 0; i < k.res.size(); ++i) {
        const awv_result& r = k.res[i];
        std::printf("%d %d %d %llu %u %d %d %d %d %d %d %d %zu", r.status, r.penalty, r.score, (unsigned long long)r.cigar_off, r.cigar_len, r.num_matches,
                    r.num_mismatches, r.num_ins, r.num_del, r.q_end, r.t_end, (int)k.rev[i], k.idx[i]);
        if (!k.clip.empty()) put_clip(k.clip[i]);
        std::puts("");
      }
    }
    std::printf("stats %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)bst.pairs, (unsigned long long)bst.above_penalty,
                (unsigned long long)bst.above_divergence, (unsigned long long)cst.pairs, (unsigned long long)cst.empty, (unsigned long long)cst.below_min_score,
                (unsigned long long)sst.pairs, (unsigned long long)sst.segments, (unsigned long long)sst.empty);
  }
  return 0;
}
