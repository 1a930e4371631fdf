// variants_walk_driver.cpp -- the walk of csrc/variants.hip's kernel, emulated serially, as a stand-alone program
// (tests/test_variants_walk_cpu.py builds it for the host only, under AddressSanitizer and UBSan).  The decomposition is the
// kernel's: a string at a residue modulo 16 inside an aligned frame, chunks of 1,024 bytes, lanes of 16, a break owns the run that ends
// there, the packed position sums, the lanes' event offsets, the segmented hash scan as a left fold in lane order, and the
// carries from chunk to chunk -- and the parts that are new relative to the cs walk are the very functions the kernel calls
// (variants_device.hpp: lane_seg, seg_combine, seg_behind, lane_events, lane_event_count, gap_event).  Every item must come out as
// var_one says, byte for byte; the pattern and the events live in exact-size heap arrays, so a read or a write past them is the
// sanitizer's to report.
//
// stdin, one case per line:
//   W <residue> <q_idx> <t_idx> <q_revcomp> <tlen> <pb> <pe> <tb> <te> <pattern in hex, or -> <ops in hex, or -> <col_beg> <col_end> <q_skip> <t_skip>
//   A <count> <seed>
// stdout, one line per case:
//   W: <1: the emulation's item and events equal var_one's> <code> <snv> <ins> <del> <events> <fnv of the emulation's events>
//   A: <1: seg_combine is associative and seg_identity() neutral on <count> random triples>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "variants_device.hpp"

using awvvar::HashSeg;
using awvvar::LaneCols;

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

constexpr int LANES = 64, LANE_BYTES = 16, CHUNK = LANES * LANE_BYTES;

struct Lane {  // text_pass.hpp's LaneRuns and the masks on top of it
  long long b0 = 0, rs0 = 0;
  int jlo = 0, jhi = 0, kin = -1;
  unsigned prev = 0, last = 0;
  LaneCols c{};
  bool bad = false;
};

// The item the way the kernel walks it: ops[sh + k] is column k, the frame readable up to the 16-byte boundary behind the string.
// measure (events == nullptr) only counts; emit stores at most `room` events.
static awv_var_item walk(int32_t q_idx, int32_t t_idx, bool revcomp, const uint8_t* pattern, const awvvar::Span& sp, const std::vector<uint8_t>& frame, int sh,
                         long long n, awv_variant* events, uint64_t room, uint64_t* n_events) {
  const long long span = sh + n;
  long long cq = 0, ct = 0, start = 0;
  unsigned carry_prev = 0;
  uint64_t hcarry = 0, c_ev = 0;
  uint32_t snv = 0, ins = 0, del = 0;
  bool bad = false;
  const auto put = [&](uint64_t& at, const awv_variant& ev) {
    if (events && at < room) events[at] = ev;
    ++at;
  };
  for (long long base = 0; base < span; base += CHUNK) {
    Lane L[LANES];
    int run_max = -1;
    for (int lane = 0; lane < LANES; ++lane) {  // lane_runs
      Lane& r = L[lane];
      r.b0 = base + (long long)lane * LANE_BYTES;
      r.jlo = (int)std::min<long long>(std::max<long long>((long long)sh - r.b0, 0), LANE_BYTES);
      r.jhi = (int)std::min<long long>(std::max<long long>(span - r.b0, 0), LANE_BYTES);
      r.prev = lane == 0 ? carry_prev : (L[lane - 1].b0 < span ? frame[(size_t)(L[lane - 1].b0 + 15)] : 0u);
      r.last = r.prev;
      for (int j = r.jlo; j < r.jhi; ++j) {
        const unsigned op = frame[(size_t)(r.b0 + j)];
        if (op != r.last && r.b0 + j > sh) r.c.brk |= 1u << j;
        r.last = op;
        r.c.valid |= 1u << j;
        r.c.x |= (unsigned)(op == 'X') << j;
        r.c.i |= (unsigned)(op == 'I') << j;
        r.c.d |= (unsigned)(op == 'D') << j;
        r.bad = r.bad || !awvcs::is_op(op);
      }
      r.c.prev_i = r.prev == 'I';
      r.c.prev_d = r.prev == 'D';
      r.rs0 = run_max >= 0 ? base + run_max - sh : start;  // the exclusive max-scan of the lanes' last breaks
      if (r.c.brk != 0) run_max = lane * LANE_BYTES + awvvar::top_bit(r.c.brk);
      r.kin = run_max;
    }
    // the scans as left folds in lane order
    long long ex_p = 0, ex_t = 0;
    uint64_t ex_ev = 0;
    HashSeg ex = awvvar::seg_identity();
    for (int lane = 0; lane < LANES; ++lane) {
      const Lane& r = L[lane];
      const LaneCols& c = r.c;
      const long long x0 = (long long)sp.pb + cq + ex_p, y0 = (long long)sp.tb + ct + ex_t;
      const auto byte = [&](int k) { return (uint32_t)pattern[x0 + k]; };
      bad = bad || r.bad;
      snv += (uint32_t)awvvar::popc32(c.x);
      ins += (uint32_t)awvvar::popc32(awvvar::ends_d(c));
      del += (uint32_t)awvvar::popc32(awvvar::ends_i(c));
      const uint32_t cnt = awvvar::lane_event_count(c);
      if (events) {
        uint64_t at = c_ev + ex_ev;
        awvvar::lane_events(c, q_idx, t_idx, revcomp, r.b0 - sh, r.rs0, x0, y0, awvvar::seg_behind(hcarry, ex), byte, [&](const awv_variant& ev) { put(at, ev); });
        if (at != c_ev + ex_ev + cnt) return awvvar::make_item(-1, 0, 0, 0);  // the count and the walk disagree
        ex = awvvar::seg_combine(ex, awvvar::lane_seg(c, byte));
      }
      ex_p += awvvar::popc32(c.valid & ~c.i);
      ex_t += awvvar::popc32(c.valid & ~c.d);
      ex_ev += cnt;
    }
    // carry_on and the chunk's totals
    const int last_lane = (int)std::min<long long>(63, (span - 1 - base) >> 4);
    carry_prev = L[last_lane].last;
    if (L[LANES - 1].kin >= 0) start = base + L[LANES - 1].kin - sh;
    cq += ex_p;
    ct += ex_t;
    c_ev += ex_ev;
    hcarry = awvvar::seg_behind(hcarry, ex);
  }
  // the string's last run has no break behind it: closed behind the chunks
  const bool last_gap = n > 0 && (carry_prev == 'I' || carry_prev == 'D');
  ins += last_gap && carry_prev == 'D';
  del += last_gap && carry_prev == 'I';
  if (events && last_gap)
    put(c_ev, awvvar::gap_event(q_idx, t_idx, revcomp, carry_prev == 'D', (long long)sp.pb + cq, (long long)sp.tb + ct, n - start, hcarry));
  else if (last_gap)
    ++c_ev;
  if (!events) c_ev = (uint64_t)snv + ins + del;
  *n_events = c_ev;
  return awvvar::make_item(awvvar::whole_code(bad, cq, ct, (int64_t)sp.pe - sp.pb, (int64_t)sp.te - sp.tb), snv, ins, del);
}

static uint64_t next(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s ^ (s >> 29);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "A") {
      long long count = 0;
      uint64_t seed = 0;
      in >> count >> seed;
      bool ok = true;
      const auto same = [](const HashSeg& a, const HashSeg& b) { return a.h == b.h && a.pw == b.pw && a.reset == b.reset; };
      const auto rnd = [&]() {
        const uint64_t len = next(seed) % 40;  // short lengths often: powers that really are B^len, and arbitrary residues too
        const bool free_pw = next(seed) % 3 == 0;
        return HashSeg{next(seed) % awvvar::MOD61, free_pw ? next(seed) % awvvar::MOD61 : awvvar::hash_pow(len), (uint32_t)(next(seed) % 3 == 0)};
      };
      for (long long k = 0; k < count; ++k) {
        const HashSeg a = rnd(), b = rnd(), c = rnd(), id = awvvar::seg_identity();
        ok = ok && same(awvvar::seg_combine(awvvar::seg_combine(a, b), c), awvvar::seg_combine(a, awvvar::seg_combine(b, c)));
        ok = ok && same(awvvar::seg_combine(id, a), a) && same(awvvar::seg_combine(a, id), a);
        const uint64_t carry = next(seed) % awvvar::MOD61;  // the carry is one more element on the left
        ok = ok && awvvar::seg_behind(awvvar::seg_behind(carry, a), b) == awvvar::seg_behind(carry, awvvar::seg_combine(a, b));
      }
      std::printf("%d\n", ok ? 1 : 0);
      continue;
    }
    std::string hp, ho;
    long long sh = 0, q = 0, t = 0, rev = 0, tlen = 0, pb = 0, pe = 0, tb = 0, te = 0, beg = 0, end = 0, q_skip = 0, t_skip = 0;
    in >> sh >> q >> t >> rev >> tlen >> pb >> pe >> tb >> te >> hp >> ho >> beg >> end >> q_skip >> t_skip;
    const std::vector<uint8_t> pattern = unhex(hp), ops = unhex(ho);
    awv_result rec{};
    rec.status = AWV_ST_COMPLETED;
    rec.cigar_len = (uint32_t)ops.size();
    awvvar::Span sp{(int32_t)pb, (int32_t)pe, (int32_t)tb, (int32_t)te};
    awvcs::apply_slice(rec, sp, awv_cs_slice{(uint32_t)beg, (uint32_t)end, (int32_t)q_skip, (int32_t)t_skip});
    const long long n = rec.cigar_len;
    const std::vector<uint8_t> c(ops.begin() + (long)rec.cigar_off, ops.begin() + (long)rec.cigar_off + n);
    // the yardstick
    uint64_t want_n = 0, got_n = 0;
    awv_var_item want = awvvar::var_one((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, c.data(), n, 0, 0, nullptr, 0, &want_n);
    std::vector<awv_variant> want_ev((size_t)want_n);
    want = awvvar::var_one((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, c.data(), n, 0, 0, want_ev.data(), want_ev.size(), &want_n);
    // the emulation: the slice's bytes at the residue, other bytes before them, zeros behind up to the 16-byte boundary
    std::vector<uint8_t> frame((size_t)((sh + n + 15) & ~15ll), 0);
    for (long long k = 0; k < sh; ++k) frame[(size_t)k] = (uint8_t)"DIXM"[k & 3];
    if (n) std::memcpy(frame.data() + sh, c.data(), (size_t)n);
    awv_var_item got = walk((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, frame, (int)sh, n, nullptr, 0, &got_n);  // measure
    std::vector<awv_variant> got_ev((size_t)(got.code == AWV_VR_OK ? got_n : 0));
    if (got.code == AWV_VR_OK) {  // emit: a sound item only, into exactly the rows measure counted
      uint64_t again = 0;
      const awv_var_item second = walk((int32_t)q, (int32_t)t, rev != 0, pattern.data(), sp, frame, (int)sh, n, got_ev.data(), got_ev.size(), &again);
      if (again != got_n || std::memcmp(&second, &got, sizeof got) != 0) got.code = -1;
    } else {
      got_n = 0;
    }
    const bool same = std::memcmp(&got, &want, sizeof got) == 0 && got_n == want_n &&
                      (got_ev.empty() || std::memcmp(got_ev.data(), want_ev.data(), got_ev.size() * sizeof(awv_variant)) == 0);
    std::printf("%d %d %u %u %u %llu %llu\n", same ? 1 : 0, got.code, got.snv, got.ins, got.del, (unsigned long long)got_n, fnv(got_ev.data(), got_ev.size()));
  }
  return 0;
}
