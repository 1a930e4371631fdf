// variants_driver.cpp -- the host side of csrc/variants_device.hpp as a stand-alone program (tests/test_variants_cpu.py builds it
// for the host only, under AddressSanitizer and UBSan): the allele hash and its combine, the slice rule of the cs text (slice_ok,
// apply_slice), the serial walk (var_one) and the fold (fold_rows) on exact-size heap arrays, so that a read past an op string or
// past the pattern's last base, or a write past the events, is the sanitizer's to report.
//
// stdin, one case per line:
//   V <q_idx> <t_idx> <q_revcomp> <tlen> <pb> <pe> <tb> <te> <pattern in hex, or -> <ops in hex, or -> <col_beg> <col_end> <q_skip> <t_skip>
//   H <a in hex, or -> <b in hex, or ->
// stdout, one line per case:
//   V: <slice_ok> <code> <snv> <ins> <del> <events> <fnv of the events in column order> <rows after the fold> <fnv of the rows>
//   H: <h(a)> <h(b)> <h(a.b)> <hash_combine(h(a), h(b), B^|b|)>
// The events go into an array of exactly snv + ins + del entries; the checksum is FNV-1a over every event's t_idx, pos, type, len,
// hash, rep and count.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "variants_device.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

static unsigned long long fnv(const awv_variant* rows, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) {
    const awv_variant& r = rows[i];
    const unsigned long long f[7] = {(unsigned long long)(uint32_t)r.t_idx, (unsigned long long)(uint32_t)r.pos, (unsigned long long)(uint32_t)r.type,
                                     (unsigned long long)(uint32_t)r.len, r.hash, r.rep, r.count};
    for (unsigned long long v : f) h = (h ^ v) * 1099511628211ull;
  }
  return h;
}

static uint64_t hash_all(const std::vector<uint8_t>& s) {
  uint64_t h = 0;
  for (uint8_t c : s) h = awvvar::hash_push(h, c);
  return h;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "H") {
      std::string ha, hb;
      in >> ha >> hb;
      const std::vector<uint8_t> a = unhex(ha), b = unhex(hb);
      std::vector<uint8_t> ab(a);
      ab.insert(ab.end(), b.begin(), b.end());
      std::printf("%llu %llu %llu %llu\n", (unsigned long long)hash_all(a), (unsigned long long)hash_all(b), (unsigned long long)hash_all(ab),
                  (unsigned long long)awvvar::hash_combine(hash_all(a), hash_all(b), awvvar::hash_pow(b.size())));
      continue;
    }
    std::string hp, ho;
    long long q = 0, t = 0, rev = 0, tlen = 0, pb = 0, pe = 0, tb = 0, te = 0, beg = 0, end = 0, q_skip = 0, t_skip = 0;
    in >> q >> t >> rev >> tlen >> pb >> pe >> tb >> te >> hp >> ho >> beg >> end >> q_skip >> t_skip;
    const std::vector<uint8_t> pattern = unhex(hp), ops = unhex(ho);
    awv_result rec{};
    rec.status = AWV_ST_COMPLETED;
    rec.cigar_len = (uint32_t)ops.size();
    const awv_cs_slice sl{(uint32_t)beg, (uint32_t)end, (int32_t)q_skip, (int32_t)t_skip};
    const bool ok = awvcs::slice_ok(rec, sl);
    awv_var_item it = awvvar::make_item(AWV_VR_SKIPPED, 0, 0, 0);
    std::vector<awv_variant> events;
    uint64_t n_events = 0, n_rows = 0;
    unsigned long long h_events = fnv(nullptr, 0), h_rows = fnv(nullptr, 0);
    if (ok) {
      awvvar::Span sp{(int32_t)pb, (int32_t)pe, (int32_t)tb, (int32_t)te};
      awvcs::apply_slice(rec, sp, sl);
      // an exact-size copy of what the record names; the rectangle begins behind the skips, as the kernel sees it
      const std::vector<uint8_t> c(ops.begin() + (long)rec.cigar_off, ops.begin() + (long)rec.cigar_off + rec.cigar_len);
      it = awvvar::var_one((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, c.data(), (int64_t)c.size(), 0, 0, nullptr, 0, &n_events);  // counts only
      events.resize((size_t)n_events);
      it = awvvar::var_one((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, c.data(), (int64_t)c.size(), 0, 0, events.data(), events.size(), &n_events);
      h_events = fnv(events.data(), events.size());
      std::vector<awv_variant> twice(events);  // every event twice: the fold leaves one row each with count 2
      twice.insert(twice.end(), events.rbegin(), events.rend());
      n_rows = awvvar::fold_rows(twice.data(), twice.size());
      h_rows = fnv(twice.data(), (size_t)n_rows);
    }
    std::printf("%d %d %u %u %u %llu %llu %llu %llu\n", ok ? 1 : 0, it.code, it.snv, it.ins, it.del, (unsigned long long)n_events, h_events,
                (unsigned long long)n_rows, h_rows);
  }
  return 0;
}
