// Stand-alone driver around awvrr::take_dir (allwave_amd/csrc/row_reuse.hpp) for tests/test_row_reuse_levels_cpu.py, built
// with the system compiler under -fsanitize=address,undefined.  One command per line on stdin, one answer line each:
//   take PLEN TLEN BV BH BCOMP  PB PE TB TE CB CE  LEVELS   -> DIR LEVEL1
//        the top-level search over (0, 0) .. (PLEN, TLEN) broke at pattern offset BV, text offset BH in component BCOMP;
//        DIR: the direction the task takes from its archive (0 forward, 1 reverse, -1 none) under LEVELS (0 all, 1 level 1
//        only), LEVEL1: 1 when the task is one of the top-level search's two halves
//   frame ROOT TASK   -> 0 | 1: whether a task of frame TASK (0 A, 1 B, 2 shared) may take from an archive recorded in frame ROOT
#include <cstdio>
#include <cstring>

#include "row_reuse.hpp"

int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "take")) {
      int v[12];
      for (int& x : v)
        if (std::scanf("%d", &x) != 1) return 2;
      bool level1 = false;
      const int dir = awvrr::take_dir(awvrr::RootId{v[0], v[1], v[2], v[3], v[4]}, awvrr::TaskId{v[5], v[6], v[7], v[8], v[9], v[10]}, v[11], &level1);
      std::printf("%d %d\n", dir, level1 ? 1 : 0);
    } else if (!std::strcmp(cmd, "frame")) {
      int r, t;
      if (std::scanf("%d %d", &r, &t) != 2) return 2;
      std::printf("%d\n", awvrr::frame_ok(r, t) ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
