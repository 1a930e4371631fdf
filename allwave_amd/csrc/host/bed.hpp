// bed.hpp -- the regions a BED file names, for --liftover (main.cpp): pure host code with no dependency but the ABI header, so a
// CPU program can run it (tests/lift_driver.cpp).
//
// A region line has three or more tab-separated columns: a sequence name, resolved against `names` (the first of equal names), and
// 0 <= beg < end <= the sequence's length; a non-empty fourth column is the region's label, else ".".  Empty lines and lines that
// begin with '#', "track" or "browser" are skipped.  Any other line gives no region and a class: "bad_line" (fewer than three
// columns, a number that does not parse, an interval that is empty or outside the sequence) or "unknown_name".
#pragma once

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "allwave_hip.h"

namespace allwave {

struct BedLine {
  size_t line = 0;  // 1-based line of the text
  std::string cls;  // "bad_line" or "unknown_name"
};
struct BedRegions {
  std::vector<awv_region> regions;  // of the good lines, in line order
  std::vector<std::string> labels;  // one per region
  std::vector<BedLine> bad;         // the lines that gave no region
};

inline BedRegions parse_bed_regions(const std::vector<std::string>& names, const std::vector<size_t>& lens, const std::string& text) {
  BedRegions out;
  std::map<std::string, size_t> by_name;
  for (size_t i = 0; i < names.size(); ++i) by_name.emplace(names[i], i);
  const auto number = [](const std::string& s, uint64_t& v) {
    if (s.empty() || s.size() > 18 || s.find_first_not_of("0123456789") != std::string::npos) return false;
    v = std::stoull(s);
    return true;
  };
  size_t pos = 0, line_no = 0;
  while (pos < text.size()) {
    size_t nl = text.find('\n', pos);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(pos, nl - pos);
    pos = nl + 1;
    ++line_no;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.find_first_not_of(" \t") == std::string::npos) continue;
    if (line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
    std::vector<std::string> f;
    for (size_t b = 0;;) {
      const size_t t = line.find('\t', b);
      f.push_back(line.substr(b, t == std::string::npos ? std::string::npos : t - b));
      if (t == std::string::npos) break;
      b = t + 1;
    }
    uint64_t beg = 0, end = 0;
    if (f.size() < 3) {
      out.bad.push_back(BedLine{line_no, "bad_line"});
      continue;
    }
    const auto it = by_name.find(f[0]);
    if (it == by_name.end()) {
      out.bad.push_back(BedLine{line_no, "unknown_name"});
      continue;
    }
    if (!number(f[1], beg) || !number(f[2], end) || beg >= end || end > lens[it->second] || end > (uint64_t)INT32_MAX) {
      out.bad.push_back(BedLine{line_no, "bad_line"});
      continue;
    }
    out.regions.push_back(awv_region{(int32_t)it->second, (int32_t)beg, (int32_t)end});
    out.labels.push_back(f.size() > 3 && !f[3].empty() ? f[3] : std::string("."));
  }
  return out;
}

}  // namespace allwave
