// lift_driver.cpp -- the host side of csrc/lift_device.hpp as a stand-alone program (tests/test_lift_cpu.py builds it for the host
// only, under AddressSanitizer and UBSan): the serial walk (lift_one) behind the slice rule of the cs text on an exact-size heap
// copy of the op bytes, so that a read past an op string is the sanitizer's to report; and the table's row order (row_less).
//
// stdin, one case per line:  L <from> <q_revcomp> <qlen> <pb> <pe> <tb> <te> <ops in hex, or -> <col_beg> <col_end> <q_skip> <t_skip> <beg> <end>
//                            R <twelve fields of a row>      (rows are collected, sorted and printed behind the last line)
// stdout, one line per L case: the thirteen fields of the result, awv_lift_result's order without `reserved`
// With the arguments `bed <len>:<name> ...` the program reads a BED text from stdin instead (csrc/host/bed.hpp's parser over those
// sequences) and prints `G <seq> <beg> <end> <label>` per region, then `B <line> <class>` per line that gave none.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "bed.hpp"
#include "lift_device.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

static int bed_main(int argc, char** argv) {
  std::vector<std::string> names;
  std::vector<size_t> lens;
  for (int k = 2; k < argc; ++k) {
    const std::string a = argv[k];
    const size_t c = a.find(':');
    lens.push_back((size_t)std::stoull(a.substr(0, c)));
    names.push_back(a.substr(c + 1));
  }
  std::stringstream ss;
  ss << std::cin.rdbuf();
  const allwave::BedRegions bed = allwave::parse_bed_regions(names, lens, ss.str());
  for (size_t k = 0; k < bed.regions.size(); ++k)
    std::printf("G %d %d %d %s\n", bed.regions[k].seq, bed.regions[k].beg, bed.regions[k].end, bed.labels[k].c_str());
  for (const allwave::BedLine& l : bed.bad) std::printf("B %zu %s\n", l.line, l.cls.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "bed") return bed_main(argc, argv);
  std::string line;
  std::vector<awv_lift_row> rows;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "R") {
      int32_t f[12];
      for (int k = 0; k < 12; ++k) in >> f[k];
      rows.push_back(awv_lift_row{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10], f[11]});
      continue;
    }
    std::string ho;
    long long from = 0, rev = 0, qlen = 0, pb = 0, pe = 0, tb = 0, te = 0, cb = 0, ce = 0, q_skip = 0, t_skip = 0, beg = 0, end = 0;
    in >> from >> rev >> qlen >> pb >> pe >> tb >> te >> ho >> cb >> ce >> q_skip >> t_skip >> beg >> end;
    const std::vector<uint8_t> ops = unhex(ho);
    awv_result rec{};
    rec.status = AWV_ST_COMPLETED;
    rec.cigar_len = (uint32_t)ops.size();
    const awv_cs_slice sl{(uint32_t)cb, (uint32_t)ce, (int32_t)q_skip, (int32_t)t_skip};
    awv_lift_result r = awvl::make_code(-1);
    if (awvl::from_ok((int32_t)from) && awvcs::slice_ok(rec, sl)) {
      awvl::Span sp{(int32_t)pb, (int32_t)pe, (int32_t)tb, (int32_t)te};
      awvcs::apply_slice(rec, sp, sl);
      const std::vector<uint8_t> c(ops.begin() + (long)rec.cigar_off, ops.begin() + (long)rec.cigar_off + rec.cigar_len);  // exactly the slice's bytes
      r = awvl::lift_one((int32_t)from, rev != 0, qlen, sp, c.data(), (int64_t)c.size(), sl, beg, end);
    }
    std::printf("%d %u %u %d %d %d %d %d %d %d %d %d %d\n", r.code, r.col_beg, r.col_end, r.q_skip, r.t_skip, r.src_beg, r.src_end, r.dst_beg, r.dst_end, r.num_matches,
                r.num_mismatches, r.num_ins, r.num_del);
  }
  std::sort(rows.begin(), rows.end(), awvl::row_less);
  for (const awv_lift_row& r : rows)
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", r.region, r.q_idx, r.t_idx, r.flags, r.src_beg, r.src_end, r.dst_beg, r.dst_end, r.num_matches, r.num_mismatches,
                r.num_ins, r.num_del);
  return 0;
}
