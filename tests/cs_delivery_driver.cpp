// cs_delivery_driver.cpp -- the cs records of allwave_amd/csrc/host/delivery.hpp on the CPU (tests/test_cs_cpu.py builds this
// with the system C++ compiler under AddressSanitizer and UBSan): in every filtering mode -- none, bounded, clipping, bounded and
// clipping, splitting, bounded and splitting -- the kept entries' awv_cs_text follow the kept records, one per kept record, and a
// Delivery without cs records delivers none.  The cases are made here, from a fixed generator; every array is exactly as long
// as the mode makes it.  stdout, per mode: "mode <bounded> <clipping> <splitting> kept <n> of <entries>"; exit status 1 on a
// record out of place.
#include <cstdio>
#include <vector>

#include "delivery.hpp"

static unsigned long long state = 88172645463325252ull;
static unsigned next(unsigned mod) {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (unsigned)(state % mod);
}

int main() {
  const int modes[6][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 1}, {1, 0, 1}};
  const size_t n = 200;
  for (const auto& m : modes) {
    const bool bounded = m[0], clipping = m[1], splitting = m[2];
    std::vector<awv_result> res(n);
    std::vector<uint8_t> rev(n), by_div(bounded ? n : 0);
    std::vector<awv_clip_result> clip(clipping ? n : 0), seg;
    std::vector<awv_split_index> index(splitting ? n : 0);
    std::vector<uint64_t> seg_first(splitting ? n : 0);
    std::vector<awv_cs_text> cs(n);
    for (size_t e = 0; e < n; ++e) {
      awv_result& r = res[e];
      r = awv_result{};
      const unsigned kind = next(10);
      r.status = kind == 0 ? AWV_ST_MAX_STEPS : kind == 1 && bounded ? AWV_ST_ABOVE_BOUND : AWV_ST_COMPLETED;
      r.num_matches = 50 + (int)next(50);
      r.num_mismatches = (int)next(30);
      r.cigar_len = (uint32_t)(r.num_matches + r.num_mismatches);
      rev[e] = (uint8_t)next(2);
      if (bounded) by_div[e] = (uint8_t)next(2);
      if (clipping) {
        clip[e] = awv_clip_result{};
        clip[e].code = next(5) == 0 ? AWV_CL_EMPTY : AWV_CL_OK;
        clip[e].score = (int64_t)next(40);
        clip[e].col_end = r.cigar_len;
      }
      if (splitting) {
        seg_first[e] = seg.size();
        const int count = (int)next(4);
        index[e] = awv_split_index{count ? AWV_CL_OK : AWV_CL_EMPTY, count, -1};
        for (int j = 0; j < count; ++j) {
          awv_clip_result c{};
          c.code = AWV_CL_OK;
          c.col_beg = (uint32_t)(10 * j);
          c.col_end = (uint32_t)(10 * j + 5);
          seg.push_back(c);
        }
      }
      cs[e].off = 1000 * e;
      cs[e].len = (uint32_t)e + 1;
      cs[e].code = (int32_t)next(4);
    }
    allwave::BoundStats bst;
    allwave::ClipStats cst;
    allwave::SplitStats sst;
    allwave::Delivery d;
    d.rev = rev.data();
    if (bounded) {
      d.by_div = by_div.data();
      d.div = 0.3;
      d.bounds = &bst;
    }
    if (clipping) {
      d.clip = clip.data();
      d.min_score = 10;
      d.clips = &cst;
    }
    if (splitting) {
      d.seg_first = seg_first.data();
      d.index = index.data();
      d.seg = seg.data();
      d.splits = &sst;
    }
    size_t kept = 0;
    for (int with_cs = 1; with_cs >= 0; --with_cs) {
      d.cs = with_cs ? cs.data() : nullptr;
      for (size_t first = 0; first < n; first += 70) {  // three sink calls
        const size_t cnt = first + 70 <= n ? 70 : n - first;
        const std::vector<awv_result> part(res.begin() + (long)first, res.begin() + (long)(first + cnt));
        const allwave::Delivered k = allwave::deliver(d, (int64_t)first, (int64_t)cnt, part.data());
        if (!with_cs) {
          if (!k.cs.empty()) return 1;
          continue;
        }
        if (k.cs.size() != k.res.size() || k.idx.size() != k.res.size()) return 1;
        for (size_t i = 0; i < k.res.size(); ++i) {  // (no idx array: an entry's index is its position in the call's pair array)
          const awv_cs_text& want = cs[k.idx[i]];
          if (k.idx[i] < first || k.idx[i] >= first + cnt || k.cs[i].off != want.off || k.cs[i].len != want.len || k.cs[i].code != want.code) return 1;
        }
        kept += k.res.size();
      }
    }
    std::printf("mode %d %d %d kept %zu of %zu\n", m[0], m[1], m[2], kept, n);
  }
  return 0;
}
