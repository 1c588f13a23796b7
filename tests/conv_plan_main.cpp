// Host program around the planning block of agile3d_amd/csrc/spconv.hip (test_conv_plan_classes.py cuts the block out by its
// two marker lines into conv_planning_block.inc and compiles this file next to it; no HIP header is involved).
// stdin:  one op per line   n_out K cin cout cin2 head_cout up mode [stats]
//         (stats: ConvShape.stats as the training path sets it -- 0 none (the default), 1 the BatchNorm partials of
//          a3d_conv_bn_train_forward, 2 the backward sums of a3d_conv_dgrad_bn)
// stdout: one plan per line family K bn ch pair handoff gcap pass2 D P G fused_ok head_ok ntile n_cblk
//         (family: wl / deep / sk; gcap: G sits at the resident-workgroup cap of the build; pass2: a cout that is a
//          multiple of 128 run with 64 columns).  The planner is asked as the library asks it: zeroed hand-off state at
//          hand, the slab the library would size for the shape, the op's tables bound.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int env_int(const char* name, int dflt) {   // common.h's
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

#include "conv_planning_block.inc"

int main() {
  int n_out, K, cin, cout, cin2, head, up, mode;
  char line[256];
  while (fgets(line, sizeof(line), stdin)) {
    int stats = 0;
    if (sscanf(line, "%d %d %d %d %d %d %d %d %d", &n_out, &K, &cin, &cout, &cin2, &head, &up, &mode, &stats) < 8) break;
    g_deep_mode = mode;
    ConvShape s;
    memset(&s, 0, sizeof(s));
    s.n_out = n_out, s.K = K, s.cin = cin, s.cout = cout, s.cin2 = cin2, s.head_cout = head;
    s.stats = stats;
    s.up = up != 0, s.tables = K > 1, s.proj_in_ok = cin2 > 0, s.has_state = true;
    s.slab_floats = max_slab_floats(n_out, K, cin, cout, cin2, up != 0);
    const ConvPlan p = plan_conv(s);
    const char* fam = p.family == kConvWl ? "wl" : p.family == kConvDeep ? "deep" : "sk";
    int gcap = 0, pass2 = 0;
    if (p.family == kConvSk) {
      int cap = 256 * sk_wgs_per_cu(p.bn, p.ch, p.pair, p.lds);
      if (cap > kSkMaxG) cap = kSkMaxG;
      gcap = p.G == cap;
      pass2 = cout % 128 == 0 && p.bn == 64;
    }
    printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", fam, K, p.bn, p.ch, p.pair, (int)p.handoff, gcap, pass2, p.D, p.P, p.G,
           (int)p.fused_ok, (int)p.head_ok, p.ntile, p.n_cblk);
  }
  return 0;
}
