// coverage_driver.cpp -- the host side of csrc/coverage_device.hpp as a stand-alone program (tests/test_coverage_cpu.py builds it
// for the host only, under AddressSanitizer and UBSan): the slice rule of the cs text (slice_ok, apply_slice) and the serial
// walk (cov_one) on exact-size heap arrays, so that a read past an op string or an add past a sequence's last base is the
// sanitizer's to report.
//
// stdin, one case per line:  <roles> <q_revcomp> <qlen> <tlen> <pb> <pe> <tb> <te> <ops in hex, or -> <col_beg> <col_end> <q_skip> <t_skip>
// stdout, one line per case: <slice_ok> <code> <aligned_cols> <matched_cols> <boundaries> <sum q_aligned> <sum q_matched> <sum t_aligned>
//                            <sum t_matched> <fnv of the four tracks>
// The tracks are four fresh arrays of exactly qlen / tlen entries; the checksum is FNV-1a over their entries in that order.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "coverage_device.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string ho;
    long long roles = 0, rev = 0, qlen = 0, tlen = 0, pb = 0, pe = 0, tb = 0, te = 0, beg = 0, end = 0, q_skip = 0, t_skip = 0;
    in >> roles >> rev >> qlen >> tlen >> pb >> pe >> tb >> te >> ho >> beg >> end >> q_skip >> t_skip;
    const std::vector<uint8_t> ops = unhex(ho);
    awv_result rec{};
    rec.status = AWV_ST_COMPLETED;
    rec.cigar_len = (uint32_t)ops.size();
    const awv_cs_slice sl{(uint32_t)beg, (uint32_t)end, (int32_t)q_skip, (int32_t)t_skip};
    const bool ok = awvcov::roles_ok((int32_t)roles) && awvcs::slice_ok(rec, sl);
    awv_cov_item it = awvcov::make_item(AWV_CV_SKIPPED, 0, 0, 0);
    std::vector<uint32_t> qa((size_t)qlen, 0), qm((size_t)qlen, 0), ta((size_t)tlen, 0), tm((size_t)tlen, 0);
    if (ok) {
      awvcov::Span sp{(int32_t)pb, (int32_t)pe, (int32_t)tb, (int32_t)te};
      awvcs::apply_slice(rec, sp, sl);
      // an exact-size copy of what the record names; the rectangle begins behind the skips, as the kernel sees it
      const std::vector<uint8_t> c(ops.begin() + (long)rec.cigar_off, ops.begin() + (long)rec.cigar_off + rec.cigar_len);
      it = awvcov::cov_one((int32_t)roles, rev != 0, qlen, tlen, sp, c.data(), (int64_t)c.size(), 0, 0, qa.data(), qm.data(), ta.data(), tm.data());
    }
    unsigned long long sums[4] = {0, 0, 0, 0}, h = 1469598103934665603ull;
    const std::vector<uint32_t>* tracks[4] = {&qa, &qm, &ta, &tm};
    for (int k = 0; k < 4; ++k)
      for (uint32_t v : *tracks[k]) {
        sums[k] += v;
        h = (h ^ v) * 1099511628211ull;
      }
    std::printf("%d %d %u %u %u %llu %llu %llu %llu %llu\n", ok ? 1 : 0, it.code, it.aligned_cols, it.matched_cols, it.boundaries, sums[0], sums[1], sums[2],
                sums[3], h);
  }
  return 0;
}
