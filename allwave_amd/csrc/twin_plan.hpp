// twin_plan.hpp -- pairing of a launch group's entries into dispatch units.
//
// An all-pairs list holds every unordered pair twice, as (q, t) and as (t, q).  The two alignments share their breakpoint
// searches (the wavefronts of one are the other's mirrored), so the kernel takes such a pair of entries as one unit.
// This header decides which entries go together; it is plain C++ with no HIP types, so that it can be built and
// tested on its own.
//
// Rules: an entry (q, t, rc) is paired with an entry (t, q, rc') when rc == rc' == 0 and q != t; every entry belongs to
// exactly one unit; an entry is used at most once, so of two copies of (q, t) facing one (t, q) one copy gets it and
// the other stays single.  Units keep the order of their first entry; a twin is matched to the nearest unmatched
// earlier entry of the swapped kind.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace awvt {

struct TwinPlan {
  std::vector<int32_t> first;  // per unit: index of its (first) entry
  std::vector<int32_t> twin;   // per unit: index of the entry aligned along with it, or -1
};

// q, t, rc: the n entries of one launch, in dispatch order.
inline TwinPlan plan_twins(const int32_t* q, const int32_t* t, const int32_t* rc, size_t n) {
  TwinPlan p;
  p.first.reserve(n);
  p.twin.reserve(n);
  // (q, t) -> units still without a twin whose first entry is (q, t), most recent last
  std::unordered_map<uint64_t, std::vector<int32_t>> open;
  open.reserve(n);
  auto key = [](int32_t a, int32_t b) { return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b; };
  for (size_t i = 0; i < n; ++i) {
    const bool can = rc[i] == 0 && q[i] != t[i];
    if (can) {
      auto it = open.find(key(t[i], q[i]));
      if (it != open.end() && !it->second.empty()) {
        p.twin[(size_t)it->second.back()] = (int32_t)i;
        it->second.pop_back();
        continue;
      }
    }
    if (can) open[key(q[i], t[i])].push_back((int32_t)p.first.size());
    p.first.push_back((int32_t)i);
    p.twin.push_back(-1);
  }
  return p;
}

}  // namespace awvt
