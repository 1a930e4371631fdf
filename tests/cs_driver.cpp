// cs_driver.cpp -- the host side of csrc/cs_device.hpp as a stand-alone program (tests/test_cs_cpu.py builds it for the host
// only, under AddressSanitizer and UBSan): the slice rule (slice_ok, apply_slice) and the serial walk (cs_one) on exact-size heap
// buffers, so that a read past a sequence or an op string, or a write past a text, is the sanitizer's to report.
//
// stdin, one case per line:  <mode> <pattern in hex, or -> <text in hex, or -> <ops in hex, or -> <col_beg> <col_end> <q_skip> <t_skip> <cap>
// stdout, one line per case: <slice_ok> <code> <len> <written: 0 / 1> <cs text in hex, or ->
// The walk goes over the slice of the op string, with the sequences cut to the rectangle behind the skips as the kernels see
// them, into a buffer of exactly `cap` bytes, pre-filled with 0xee: "written" says whether any of them changed.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "cs_device.hpp"

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
    std::string hp, ht, ho;
    long long mode = 0, beg = 0, end = 0, q_skip = 0, t_skip = 0, cap = 0;
    in >> mode >> hp >> ht >> ho >> beg >> end >> q_skip >> t_skip >> cap;
    const std::vector<uint8_t> pattern = unhex(hp), text = unhex(ht), ops = unhex(ho);
    awv_result rec{};
    rec.status = AWV_ST_COMPLETED;
    rec.cigar_len = (uint32_t)ops.size();
    const awv_cs_slice sl{(uint32_t)beg, (uint32_t)end, (int32_t)q_skip, (int32_t)t_skip};
    const bool ok = awvcs::mode_ok((int32_t)mode) && awvcs::slice_ok(rec, sl);
    awv_cs_text t = awvcs::make_text(0, 0, AWV_CST_SKIPPED);
    std::vector<uint8_t> out((size_t)cap, 0xee);
    if (ok) {
      awvcs::Span sp{0, (int32_t)pattern.size(), 0, (int32_t)text.size()};
      awvcs::apply_slice(rec, sp, sl);
      // exact-size copies of what the record and the rectangle name (a rectangle of negative length names nothing)
      const std::vector<uint8_t> c(ops.begin() + (long)rec.cigar_off, ops.begin() + (long)rec.cigar_off + rec.cigar_len);
      const int plen = sp.pe - sp.pb, tlen = sp.te - sp.tb;
      const std::vector<uint8_t> p(pattern.begin() + (plen > 0 ? sp.pb : 0), pattern.begin() + (plen > 0 ? sp.pe : 0));
      const std::vector<uint8_t> x(text.begin() + (tlen > 0 ? sp.tb : 0), text.begin() + (tlen > 0 ? sp.te : 0));
      t = awvcs::cs_one((int32_t)mode, p.data(), plen, x.data(), tlen, c.data(), (int64_t)c.size(), 0, 0, out.empty() ? nullptr : out.data(), (uint64_t)cap);
    }
    bool written = false;
    for (uint8_t b : out) written = written || b != 0xee;
    std::printf("%d %d %u %d ", ok ? 1 : 0, t.code, t.len, written ? 1 : 0);
    if (!written || t.len == 0) std::printf("-");
    else for (uint32_t i = 0; i < t.len; ++i) std::printf("%02x", out[i]);
    std::printf("\n");
  }
  return 0;
}
