// encode_driver.cpp -- the host side of csrc/encode_device.hpp as a stand-alone program (tests/test_encode_cpu.py builds it for
// the host only, under AddressSanitizer and UBSan): the slice rule (slice_ok, apply_slice) and the serial walk (encode_one) on
// exact-size heap buffers, so that a read past a string or a write past a text is the sanitizer's to report.
//
// stdin, one case per line:  <ops in hex, or -> <status> <cigar_off> <col_beg> <col_end> <cap>
// stdout, one line per case: <slice_ok> <cigar_off> <cigar_len> <len> <runs> <written: 0 / 1> <text in hex, or ->
// The record names ops[0 .. n) at `cigar_off` of an arena that holds nothing else; the walk encodes the record's slice into a
// buffer of exactly `cap` bytes, pre-filled with 0xee: "written" says whether any of them changed.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "encode_device.hpp"

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
    std::string hex;
    long long status = 0, off = 0, beg = 0, end = 0, cap = 0;
    in >> hex >> status >> off >> beg >> end >> cap;
    const std::vector<uint8_t> ops = unhex(hex);
    std::vector<uint8_t> arena((size_t)off + ops.size());
    for (size_t i = 0; i < ops.size(); ++i) arena[(size_t)off + i] = ops[i];
    awv_result rec{};
    rec.status = (int32_t)status;
    rec.cigar_off = (uint64_t)off;
    rec.cigar_len = (uint32_t)ops.size();
    const bool ok = awve::slice_ok(rec, (uint32_t)beg, (uint32_t)end);
    awv_cigar_text t = awve::make_text(0, 0, 0);
    std::vector<uint8_t> text((size_t)cap, 0xee);
    if (ok) {
      awve::apply_slice(rec, (uint32_t)beg, (uint32_t)end);
      const int64_t n = rec.status == AWV_ST_COMPLETED ? (int64_t)rec.cigar_len : 0;
      t = awve::encode_one(n ? arena.data() + rec.cigar_off : nullptr, n, text.empty() ? nullptr : text.data(), (uint64_t)cap);
    }
    bool written = false;
    for (uint8_t b : text) written = written || b != 0xee;
    std::printf("%d %llu %u %u %u %d ", ok ? 1 : 0, (unsigned long long)rec.cigar_off, rec.cigar_len, t.len, t.runs, written ? 1 : 0);
    if (!written || t.len == 0) std::printf("-");
    else for (uint32_t i = 0; i < t.len; ++i) std::printf("%02x", text[i]);
    std::printf("\n");
  }
  return 0;
}
