// batch_plan_driver.cpp -- stand-alone driver of allwave_amd/csrc/batch_plan.hpp for tests/test_batch_plan_cpu.py.
// Reads one case per line from stdin and prints the plan the header makes of it; the first line sets the Limits.
//   limits  tmax tmax32 chain_max max_ring max_scope ncomp col_pad fb_score fb_length waves_per_simd static_lds ev_stack ev_twin meta meta16 bp
//   pen     flags match x o1 e1 o2 e2 two_piece
//   carve   max_batch max_arena score_only n  (ql tl)*n
//   order   n  (ql tl)*n
//   groups  flags num_cus skewed n  (ql tl)*n                      -- the pairs in dispatch order
//   rows    flags num_cus workgroups max_scratch first_row_cols twin_ok waves width  flags_pen match x o1 e1 o2 e2 two_piece  n  (ql tl)*n
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "batch_plan.hpp"

using namespace awvb;

static std::vector<Entry> read_entries(std::istream& in) {
  long long n = 0;
  in >> n;
  std::vector<Entry> en((size_t)n);
  for (long long i = 0; i < n; ++i) {
    en[(size_t)i] = Entry{};
    in >> en[(size_t)i].ql >> en[(size_t)i].tl;
    en[(size_t)i].batch_index = i;
  }
  return en;
}

static PenaltyPlan read_pen(const Limits& L, std::istream& in) {
  int flags;
  awv_penalties p{};
  int two;
  in >> flags >> p.match >> p.mismatch >> p.gap_open1 >> p.gap_ext1 >> p.gap_open2 >> p.gap_ext2 >> two;
  p.two_piece = two;
  return plan_penalties(L, &p, flags);
}

int main() {
  Limits L{};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "limits") {
      in >> L.tmax >> L.tmax32 >> L.chain_max >> L.max_ring >> L.max_scope >> L.ncomp >> L.col_pad >> L.fallback_min_score >>
          L.fallback_min_length >> L.waves_per_simd >> L.static_lds_reserve >> L.ev_stack_words >> L.ev_twin_words >> L.row_meta >>
          L.row_meta16 >> L.breakpoint;
    } else if (what == "pen") {
      const PenaltyPlan d = read_pen(L, in);
      printf("pen %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", d.code, d.late ? 1 : 0, d.two_piece, d.x, d.o1, d.e1, d.o2, d.e2, d.scope, d.multi_T,
             d.chain_max, d.ring, d.sb_cap, d.wb_cap, d.message.empty() ? "-" : d.message.c_str());
    } else if (what == "carve") {
      long long max_batch, score_only;
      unsigned long long max_arena;
      in >> max_batch >> max_arena >> score_only;
      const std::vector<Entry> all = read_entries(in);
      std::vector<Entry> en;
      for (int64_t first = 0; first < (int64_t)all.size();) {
        const Carve c = carve_batch([&](int64_t i, int32_t& ql, int32_t& tl) { ql = all[(size_t)i].ql; tl = all[(size_t)i].tl; }, first,
                                    (int64_t)all.size(), max_batch, max_arena, score_only != 0, en);
        printf("batch %lld %lld %llu", (long long)first, (long long)c.n, (unsigned long long)c.arena);
        for (const Entry& e : en) printf(" %llu:%lld:%d:%d", (unsigned long long)e.off, (long long)e.batch_index, e.ql, e.tl);
        printf("\n");
        if (c.n <= 0) return 2;
        first += c.n;
      }
      printf("end\n");
    } else if (what == "order") {
      std::vector<Entry> en = read_entries(in);
      const bool skewed = order_by_cost(en);
      printf("order %d", skewed ? 1 : 0);
      for (const Entry& e : en) printf(" %lld", (long long)e.batch_index);
      printf("\n");
    } else if (what == "groups") {
      Config cfg;
      int skewed;
      in >> cfg.flags >> cfg.num_cus >> skewed;
      const std::vector<Entry> en = read_entries(in);
      const GroupPlan gp = assign_groups(L, cfg, en, skewed != 0, INT_MAX);
      printf("groups");
      for (uint8_t g : gp.group) printf(" %d", (int)g);
      printf(" | ");
      for (int k = 0; k < NG; ++k) printf(" %d", gp.demand_order[k]);
      printf(" | ");
      for (int g = 0; g < NG; ++g) printf(" %zu:%d", gp.count[g], gp.maxsum[g]);
      printf("\n");
    } else if (what == "rows") {
      Config cfg;
      long long max_scratch;
      int twin_ok, waves, width;
      in >> cfg.flags >> cfg.num_cus >> cfg.workgroups >> max_scratch >> cfg.first_row_cols >> twin_ok >> waves >> width;
      cfg.max_scratch_bytes = max_scratch;
      const PenaltyPlan pp = read_pen(L, in);
      if (pp.code != AWV_OK) return 3;
      const std::vector<Entry> all = read_entries(in);
      const int w2g = wc_2g(L, pp.ring, width);
      const long long span = capacity_span(L, w2g);
      std::vector<Entry> en;
      printf("rows %d %lld ", w2g, span);
      for (const Entry& e : all) {
        const bool out = beyond_span(e.ql, e.tl, span);
        printf("%d", out ? 1 : 0);
        if (!out) en.push_back(e);
      }
      const RowPlan r = plan_rows(L, cfg, pp, en, waves, width, twin_ok != 0);
      printf(" %d %d %zu %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu |", r.waves, r.wg, r.esz, r.wc_2g, r.nslots_g, r.wcap_full, r.wcap, r.wc_last,
             r.twin_here ? 1 : 0, r.ev_extra, r.lds_meta, r.lds_seq, r.dyn_lds, r.lds_budget, r.hist_rows, r.hist_stride, r.budget);
      for (int wc = r.wcap;; wc = r.next_wc(wc)) {  // the attempts of a group all of whose pairs outgrow every row
        printf(" %d:%d:%zu:%zu:%zu", wc, r.slots(wc, (int64_t)en.size()), r.per_slot(wc), r.ring_stride(wc), r.ev_stride(wc));
        if (wc >= r.wc_last) break;
      }
      printf("\n");
    } else {
      fprintf(stderr, "unknown case: %s\n", what.c_str());
      return 1;
    }
  }
  return 0;
}
