// Host program around the planning block of agile3d_amd/csrc/wgrad.hip (test_wgrad_plan_host.py cuts the block out by its two
// marker lines into wgrad_planning_block.inc and compiles this file next to it; no HIP header is involved).
// stdin:  one question per line
//           plan cin cout K ngroups seg has_counts  then, with has_counts = 1, the 27 per-offset group counts
//             seg is the value of A3D_WGRAD_SEG (0: the model chooses), has_counts = 0 a map in which every group has every offset
//           maps                                      the scene's map table
// stdout: one line each
//           plan: 1 cx cy nblocks seg_len slots grid_items part_bytes  then cnt[27] base[28] xbase[8][28] seg_lo[27][9], row-major;
//                 a refusal is the line "0 <reason>"
//           maps: per map  list_kind level K pos_above jobs_before,  then the job count
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "agile3d_hip.h"   // A3D_NUM_LEVELS, the A3D_OP_* codes

static int env_int(const char* name, int dflt) {   // common.h's
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

#include "wgrad_planning_block.inc"

int main() {
  char what[16];
  while (scanf("%15s", what) == 1) {
    if (!strcmp(what, "maps")) {
      for (int m = 0; m < kListMaps; ++m)
        printf("%d %d %d %d %d ", kWgradMaps[m].list_kind, kWgradMaps[m].level, kWgradMaps[m].K, (int)kWgradMaps[m].pos_above, wgrad_jobs_before(m));
      printf("%d\n", kListJobs);
      continue;
    }
    int cin, cout, K, ngroups, seg, has_counts, counts[27] = {};
    if (strcmp(what, "plan") || scanf("%d %d %d %d %d %d", &cin, &cout, &K, &ngroups, &seg, &has_counts) != 6) return 1;
    if (has_counts)
      for (int k = 0; k < 27; ++k)
        if (scanf("%d", &counts[k]) != 1) return 1;
    WgradPlan p;
    memset(&p, 0, sizeof(p));
    if (const char* why = wgrad_plan(ngroups, K, has_counts ? counts : nullptr, cin, cout, make_wgrad_switches(seg, 0), p)) {
      printf("0 %s\n", why);
      continue;
    }
    printf("1 %d %d %d %d %d %d %zu", p.cx, p.cy, p.nblocks, p.cut.seg_len, p.slots, p.grid_items, p.part_bytes);
    for (int k = 0; k < 27; ++k) printf(" %d", p.cut.cnt[k]);
    for (int k = 0; k < 28; ++k) printf(" %d", p.cut.base[k]);
    for (int x = 0; x < 8; ++x)
      for (int k = 0; k < 28; ++k) printf(" %d", p.cut.xbase[x][k]);
    for (int k = 0; k < 27; ++k)
      for (int x = 0; x < 9; ++x) printf(" %d", p.cut.seg_lo[k][x]);
    printf("\n");
  }
  return 0;
}
