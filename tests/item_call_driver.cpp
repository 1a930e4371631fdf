// item_call_driver.cpp -- a stand-alone program over allwave_amd/csrc/item_call.hpp for tests/test_item_call_cpu.py: it reads call
// descriptions from standard input and prints, per call, the refusal or the resolved pairs, rectangles and records, then the first
// record over the length limit.  Built with the system C++ compiler under AddressSanitizer and UBSan; every input array is a
// vector of exactly its size, so a read outside one is seen.
//
// A call:  nseq len[0 .. nseq)
//          form (0 pairs, 1 ranges)  n  arena_bytes  has_slices  max_columns
//          n lines  q t rc            (pairs)   or   q t rc q_beg q_end t_beg t_end   (ranges)
//          n lines  status cigar_off cigar_len
//          n lines  col_beg col_end q_skip t_skip   (with has_slices)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "allwave_hip.h"
#include "item_call.hpp"

int main() {
  long long nseq;
  while (std::cin >> nseq) {
    std::vector<int32_t> len((size_t)nseq);
    for (auto& l : len) std::cin >> l;
    long long form, n, has_slices, max_columns;
    unsigned long long arena_bytes;
    std::cin >> form >> n >> arena_bytes >> has_slices >> max_columns;
    std::vector<awv_pair> pairs(form == 0 ? (size_t)n : 0);
    std::vector<awv_range_pair> ranges(form == 1 ? (size_t)n : 0);
    for (auto& p : pairs) std::cin >> p.q_idx >> p.t_idx >> p.q_revcomp;
    for (auto& r : ranges) {
      r = awv_range_pair{};
      std::cin >> r.q_idx >> r.t_idx >> r.q_revcomp >> r.q_beg >> r.q_end >> r.t_beg >> r.t_end;
    }
    std::vector<awv_result> results((size_t)n);
    for (auto& r : results) {
      r = awv_result{};
      std::cin >> r.status >> r.cigar_off >> r.cigar_len;
    }
    std::vector<awv_cs_slice> slices(has_slices ? (size_t)n : 0);
    for (auto& s : slices) std::cin >> s.col_beg >> s.col_end >> s.q_skip >> s.t_skip;
    if (!std::cin) return 2;

    awvw::ItemCall call;
    static const awv_range_pair none{};  // (a range call without ranges still says that it is one: as the entry points do)
    const awvw::ItemCall::Refusal why = call.resolve(len.data(), (int32_t)nseq, form == 0 ? pairs.data() : nullptr, form == 1 ? (n > 0 ? ranges.data() : &none) : nullptr, n,
                                                     results.data(), arena_bytes, has_slices ? slices.data() : nullptr);
    if (why != awvw::ItemCall::NONE) {
      std::printf("refused %d %lld %s\n", (int)why, (long long)call.at, call.message("who").c_str());
      continue;
    }
    std::printf("ok %d\n", (int)(has_slices ? call.recs == call.sliced.data() : call.recs == results.data()));
    for (long long i = 0; i < n; ++i) {
      const awv_pair& p = call.pairs[i];
      const awvr::Span& sp = call.spans[(size_t)i];
      const awv_result& r = call.recs[i];
      std::printf("%d %d %d %d %d %d %d %d %llu %u\n", p.q_idx, p.t_idx, p.q_revcomp, sp.pb, sp.pe, sp.tb, sp.te, r.status, (unsigned long long)r.cigar_off, r.cigar_len);
    }
    std::printf("too_long %lld\n", (long long)awvw::first_too_long(call.recs, n, max_columns));
  }
  return 0;
}
