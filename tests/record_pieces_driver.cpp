// record_pieces_driver.cpp -- allwave_amd/csrc/record_pieces.hpp run on the CPU (tests/test_record_pieces_cpu.py builds this
// with the system C++ compiler under AddressSanitizer and UBSan).  Cases on stdin, one after the other:
//   n_all arena_bytes max_arena max_records keep_residue      (max_records 0: the header's default)
//   the caller's arena as hex ("-": empty)
//   n_all lines: status cigar_off cigar_len code      (code: the awv_norm_result code the "device" returns for the record)
// Every case is cut into pieces as an awv_*_cigars call cuts it.  Per piece, on stdout:
//   piece first n bytes
//   the n staged cigar_off values
//   the staging buffer as hex ("-": empty)
// then the piece plays the device's part -- every staged byte, padding included, is XORed with 0xA5 -- and goes through
// scatter_back.  After the last piece: "arena" and the caller's arena as hex.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "allwave_hip.h"
#include "record_pieces.hpp"

static void put_hex(const std::vector<uint8_t>& b) {
  if (b.empty()) {
    std::puts("-");
    return;
  }
  std::string s;
  for (uint8_t x : b) {
    s += "0123456789abcdef"[x >> 4];
    s += "0123456789abcdef"[x & 15];
  }
  std::puts(s.c_str());
}

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main() {
  long long n_all;
  unsigned long long arena_bytes, max_arena;
  long long max_records;
  int keep;
  while (std::cin >> n_all >> arena_bytes >> max_arena >> max_records >> keep) {
    std::string hex;
    std::cin >> hex;
    std::vector<uint8_t> arena;  // exactly arena_bytes long: a read or write past the caller's arena is the sanitizer's to find
    if (hex != "-")
      for (size_t i = 0; i + 1 < hex.size(); i += 2) arena.push_back((uint8_t)(nibble(hex[i]) * 16 + nibble(hex[i + 1])));
    if (arena.size() != arena_bytes) return 2;
    std::vector<awv_result> results((size_t)n_all);
    std::vector<awv_norm_result> codes((size_t)n_all);
    for (long long i = 0; i < n_all; ++i) {
      long long status, len, code;
      unsigned long long off;
      if (!(std::cin >> status >> off >> len >> code)) return 2;
      results[(size_t)i] = awv_result{};
      results[(size_t)i].status = (int32_t)status;
      results[(size_t)i].cigar_off = off;
      results[(size_t)i].cigar_len = (uint32_t)len;
      codes[(size_t)i] = awv_norm_result{};
      codes[(size_t)i].code = (int32_t)code;
      if (awvw::outside(results[(size_t)i], arena_bytes)) return 3;  // (the entry points refuse such a call before a piece is cut)
    }
    std::vector<uint8_t> stage;
    std::vector<awv_result> recs;
    for (long long first = 0; first < n_all;) {
      const awvw::Piece pc = max_records > 0 ? awvw::pack_piece(results.data(), n_all, first, arena.data(), max_arena, keep != 0, recs, stage, max_records)
                                             : awvw::pack_piece(results.data(), n_all, first, arena.data(), max_arena, keep != 0, recs, stage);
      if (pc.n < 1 || (size_t)pc.n != recs.size() || pc.bytes != stage.size()) return 4;
      std::printf("piece %lld %lld %llu\n", first, (long long)pc.n, (unsigned long long)pc.bytes);
      for (long long i = 0; i < pc.n; ++i) std::printf("%llu%c", (unsigned long long)recs[(size_t)i].cigar_off, i + 1 < pc.n ? ' ' : '\n');
      put_hex(stage);
      for (uint8_t& b : stage) b ^= 0xA5;
      awvw::scatter_back(results.data() + first, codes.data() + first, pc.n, recs, stage, arena.data());
      first += pc.n;
    }
    std::puts("arena");
    put_hex(arena);
  }
  return 0;
}
