// CPU test (tests/test_msm_plan_cpu.py): the MSM's host-side planning (csrc/msm_plan.hpp) on cases
// read from a file, one line of decimal numbers out per line in.  No arithmetic of its own.
//   consts                                    -> BS_BLOCK BS_MAXBITS BS_TILE SCAN_SMALL KF_U32 KF_U16 shapes (c W spt)...
//   table n                                   -> c W of the window table over n points
//   plan n bits tn tc tW fb_off tables        -> c W shared bucket_bits stride Wr half nb
//   geom n c W shared bucket_bits stride      -> wb keybits npass pk vo ibits ct spb T1 nb shift max_seg
//                                                max_tiles cnt_len, then bits[8] kf[8] tile[8] one_launch[8]
#include <cstdio>
#include <cstring>

#include "msm_plan.hpp"
using namespace tns;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[16];
  while (std::fscanf(f, "%15s", op) == 1) {
    unsigned long long n, tn, off, stride;
    int bits, tc, tW, tables, c, W, shared, bb;
    if (!std::strcmp(op, "consts")) {
      std::printf("%d %d %d %zu %d %d", BS_BLOCK, BS_MAXBITS, BS_TILE, SCAN_SMALL, (int)KF_U32, (int)KF_U16);
      for (const Pass1Shape &s : kPass1Shapes) std::printf(" %d %d %d", s.c, s.W, s.spt);
    } else if (!std::strcmp(op, "table") && std::fscanf(f, "%llu", &n) == 1) {
      const int tw = table_window(n);
      std::printf("%d %d", tw, windows_for(254, tw));
    } else if (!std::strcmp(op, "plan") &&
               std::fscanf(f, "%llu %d %llu %d %d %llu %d", &n, &bits, &tn, &tc, &tW, &off, &tables) == 7) {
      const MsmPlan P = plan_msm(n, bits, TableShape{(size_t)tn, tc, tW}, off, tables != 0);
      std::printf("%d %d %d %d %u %d %zu %zu", P.c, P.W, (int)P.shared, P.bucket_bits, P.stride, P.Wr, P.half, P.nb);
    } else if (!std::strcmp(op, "geom") &&
               std::fscanf(f, "%llu %d %d %d %d %llu", &n, &c, &W, &shared, &bb, &stride) == 6) {
      const SortGeom g = sort_geom(n, WindowPlan{c, W, shared != 0, bb, (uint32_t)stride});
      std::printf("%d %d %d %d %d %d %d %zu %zu %d %d %zu %zu %zu", g.wb, g.keybits, g.npass, (int)g.pk, (int)g.vo, g.ibits,
                  g.ct, g.spb, g.T1, g.nb, g.shift, g.max_seg, g.max_tiles, g.cnt_len);
      for (int p = 0; p < 8; p++) std::printf(" %d", g.bits[p]);
      for (int p = 0; p < 8; p++) std::printf(" %d", g.kf[p]);
      for (int p = 0; p < 8; p++) std::printf(" %d", g.tile[p]);
      for (int p = 0; p < 8; p++) std::printf(" %d", (int)g.one_launch[p]);
    } else {
      std::fprintf(stderr, "bad line: %s\n", op);
      return 1;
    }
    std::putchar('\n');
  }
  std::fclose(f);
  return 0;
}
