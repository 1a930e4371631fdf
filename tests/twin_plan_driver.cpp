// Stand-alone driver around allwave_amd/csrc/twin_plan.hpp for tests/test_twin_plan_cpu.py (built with the system compiler
// under -fsanitize=address,undefined).  stdin: "q t rc" per line; stdout: "first twin" per unit.
#include <cstdio>
#include <vector>

#include "twin_plan.hpp"

int main() {
  std::vector<int32_t> q, t, rc;
  int a, b, c;
  while (std::scanf("%d %d %d", &a, &b, &c) == 3) {
    q.push_back(a);
    t.push_back(b);
    rc.push_back(c);
  }
  const awvt::TwinPlan p = awvt::plan_twins(q.data(), t.data(), rc.data(), q.size());
  if (p.first.size() != p.twin.size()) return 3;
  for (size_t u = 0; u < p.first.size(); ++u) std::printf("%d %d\n", p.first[u], p.twin[u]);
  return 0;
}
