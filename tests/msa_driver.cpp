// msa_driver.cpp -- the host side of csrc/msa_device.hpp as a stand-alone program (tests/test_msa_cpu.py builds it for the host
// only, under AddressSanitizer and UBSan): one target's items through msa_target, behind the slice rule of the cs text, on
// exact-size heap copies of the sequences, of the slices' op bytes, of the slots and of the block, so that a read or a store past
// any of them is the sanitizer's to report.
//
// stdin:  T <text in hex, or ->                                                    opens a target
//         I <pattern in hex, or -> <pb> <pe> <tb> <te> <ops in hex, - for none, ! for a record that is not completed>
//           <col_beg> <col_end> <q_skip> <t_skip>                                  adds an item
//         E                                                                        closes it
// stdout, per target:  W <width> <rows>, C <the items' codes>, N <the len + 1 widths>, then the block's rows as text
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "msa_device.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-" || s == "!") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

// an exact-size heap copy (also of nothing)
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> c(new uint8_t[n]);
  if (n) std::memcpy(c.get(), p, n);
  return c;
}

int main() {
  std::string line;
  std::unique_ptr<uint8_t[]> text;
  int64_t tlen = 0;
  std::vector<std::unique_ptr<uint8_t[]>> keep;
  std::vector<awvmsa::HostItem> items;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "T") {
      std::string h;
      in >> h;
      const std::vector<uint8_t> t = unhex(h);
      text = exact(t.data(), t.size());
      tlen = (int64_t)t.size();
      keep.clear();
      items.clear();
    } else if (kind == "I") {
      std::string hp, ho;
      long long pb = 0, pe = 0, tb = 0, te = 0, cb = 0, ce = 0, q_skip = 0, t_skip = 0;
      in >> hp >> pb >> pe >> tb >> te >> ho >> cb >> ce >> q_skip >> t_skip;
      const std::vector<uint8_t> p = unhex(hp), ops = unhex(ho);
      awv_result rec{};
      rec.status = ho == "!" ? AWV_ST_CAPACITY : AWV_ST_COMPLETED;
      rec.cigar_len = (uint32_t)ops.size();
      const awv_cs_slice sl{(uint32_t)cb, (uint32_t)ce, (int32_t)q_skip, (int32_t)t_skip};
      if (!awvcs::slice_ok(rec, sl)) return 3;
      awvmsa::Span sp{(int32_t)pb, (int32_t)pe, (int32_t)tb, (int32_t)te}, moved = sp;
      awvcs::apply_slice(rec, moved, sl);  // (the record names the slice's bytes; msa_target takes the rectangle and the skips apart)
      keep.push_back(exact(p.data(), p.size()));
      const uint8_t* const pattern = keep.back().get();
      keep.push_back(exact(ops.data() + (rec.status == AWV_ST_COMPLETED ? rec.cigar_off : 0), rec.status == AWV_ST_COMPLETED ? rec.cigar_len : 0));
      items.push_back(awvmsa::HostItem{pattern, (int64_t)p.size(), sp, keep.back().get(), rec.status == AWV_ST_COMPLETED ? (int64_t)rec.cigar_len : -1, q_skip, t_skip});
    } else if (kind == "E") {
      const int64_t n = (int64_t)items.size();
      std::unique_ptr<uint32_t[]> ins(new uint32_t[(size_t)tlen + 1]);
      std::unique_ptr<int32_t[]> codes(new int32_t[(size_t)n]);
      int64_t width = 0;
      uint64_t bytes = 0;
      awvmsa::msa_target(text.get(), tlen, items.data(), n, ins.get(), &width, codes.get(), nullptr, 0, &bytes);
      std::unique_ptr<uint8_t[]> block(new uint8_t[(size_t)bytes]);
      awvmsa::msa_target(text.get(), tlen, items.data(), n, ins.get(), &width, codes.get(), block.get(), bytes, &bytes);
      const int64_t rows = width ? (int64_t)(bytes / (uint64_t)width) : 0;
      std::printf("W %lld %lld\nC", (long long)width, (long long)rows);
      for (int64_t i = 0; i < n; ++i) std::printf(" %d", codes[(size_t)i]);
      std::printf("\nN");
      for (int64_t p = 0; p <= tlen; ++p) std::printf(" %u", ins[(size_t)p]);
      std::printf("\n");
      for (int64_t r = 0; r < rows; ++r) {
        std::fwrite(block.get() + r * width, 1, (size_t)width, stdout);
        std::printf("\n");
      }
    }
  }
  return 0;
}
