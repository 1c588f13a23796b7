// Host program around the planning block of agile3d_amd/csrc/decoder.hip (decoder_edge_cases.py cuts the block out by its two
// marker lines into decoder_planning_block.inc and compiles this file next to it; no HIP header is involved).
// stdin:  one question per line.  A launch-group candidate:
//           plan fused_c2s fused_wide fused_s2o fused_s2c wide_from n_bg ns  then ns x (nq n_objects kv0_state)
//         the switches are the values of A3D_FUSED_C2S, A3D_FUSED_WIDE, A3D_FUSED_S2O, A3D_FUSED_S2C and A3D_WIDE_FROM.
// stdout: one line each
//           rc grouped wide qt nblk leftover fuse_c2s fuse_s2c fuse_out fuse_all s2c_kg fits12 cached0 fill0
//           then six builds, name and LDS bytes each: click-to-scene, scene-to-click and output half of the first layer, then
//           of the other layers ("-" 0: the phase before it does the work)
//         rc: A3D_OK, or A3D_ERR_UNSUPPORTED from the sample check of prepare_sample or from the plan;
//         grouped: a3d_decoder_forward_batch would keep these consecutive samples in ONE launch group (the plan is the plan of
//         that group; with grouped = 0 it is not one the library ever makes).
// The workgroup shares of a launch group (dec_wg_shares):
//           shares wg_per_group ns  then ns x points      ->   grid  then ns x (wg_begin wg_end)
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "agile3d_hip.h"   // A3D_MAX_QUERIES, the A3D_* codes

static int env_int(const char* name, int dflt) {   // common.h's
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// decoder.hip's and decoder_wide.h's; the block's static_assert holds both sides to them
constexpr int D = 128, H = 8, kWTile = 16 * 136;

#include "decoder_planning_block.inc"

static std::string build_name(const DecPhase& ph) {
  char b[96];
  const int q = ph.qt;
  switch (ph.kernel) {
    case kDkNone: return "-";
    case kDkC2sAttn: snprintf(b, sizeof b, "k_c2s_attn<%d>", q); break;
    case kDkC2sAttnB: snprintf(b, sizeof b, "k_c2s_attn_b<%d>", q); break;
    case kDkKvC2s: snprintf(b, sizeof b, "k_kv_c2s<%d%s>", q, ph.lo ? ",LO" : ""); break;
    case kDkC2sW: snprintf(b, sizeof b, "k_c2s_w<%d>", q); break;
    case kDkS2cOut: snprintf(b, sizeof b, "k_s2c_out<%d,%d%s%s%s>", q, ph.waves, ph.kg ? ",KG" : "", ph.qc ? ",QC" : "", ph.lo ? ",LO" : ""); break;
    case kDkQS2c: snprintf(b, sizeof b, "k_q_s2c<%d%s>", q, ph.qc ? ",QC" : ""); break;
    case kDkS2cAttnWide: snprintf(b, sizeof b, "k_s2c_attn_wide<%d>%s", q, ph.qc ? "+cachedQ" : ""); break;
    case kDkS2oW: snprintf(b, sizeof b, "k_s2o_w<%d%s>", q, ph.qc ? ",QC" : ""); break;
    case kDkS2cW: snprintf(b, sizeof b, "k_s2c_w<%d%s>", q, ph.qc ? ",QC" : ""); break;
    case kDkOutLnMask: snprintf(b, sizeof b, "k_out_ln_mask<%d>", q); break;
    case kDkLnMask: snprintf(b, sizeof b, "k_ln_mask<%d>", q); break;
    case kDkOutW: snprintf(b, sizeof b, "k_out_w<%d>", q); break;
  }
  return b;
}

int main() {
  int c2s, wide, s2o, s2c, wide_from, n_bg, ns;
  char what[16];
  while (scanf("%15s", what) == 1) {
    if (!strcmp(what, "shares")) {
      int per_group;
      if (scanf("%d %d", &per_group, &ns) != 2 || ns < 1) return 1;
      std::vector<int> n((size_t)ns), b((size_t)ns), e((size_t)ns);
      for (int i = 0; i < ns; ++i)
        if (scanf("%d", &n[i]) != 1) return 1;
      printf("%d", dec_wg_shares(n.data(), ns, per_group != 0, b.data(), e.data()));
      for (int i = 0; i < ns; ++i) printf(" %d %d", b[i], e[i]);
      printf("\n");
      continue;
    }
    if (strcmp(what, "plan") || scanf("%d %d %d %d %d %d %d", &c2s, &wide, &s2o, &s2c, &wide_from, &n_bg, &ns) != 7) return 1;
    const DecSwitches sw = make_dec_switches(c2s, wide, s2o, s2c, wide_from);
    std::vector<DecSampleShape> s((size_t)ns);
    bool unsupported = false, grouped = true;
    for (int i = 0; i < ns; ++i) {
      if (scanf("%d %d %d", &s[i].nq, &s[i].K, &s[i].kv0_state) != 3) return 1;
      unsupported = unsupported || dec_sample_unsupported(s[i].nq, s[i].K, s[i].nq - n_bg);
      s[i].qtw = unsupported ? 0 : dec_sample_qtw(s[i].nq, sw);
    }
    if (unsupported) {
      printf("%d 0 0 0 0 0 0 0 0 0 0 0 0 0 - 0 - 0 - 0 - 0 - 0 - 0\n", A3D_ERR_UNSUPPORTED);
      continue;
    }
    // the library puts the wide tier's samples first, then walks the list
    std::stable_partition(s.begin(), s.end(), [](const DecSampleShape& a) { return a.qtw > 0; });
    for (int i = 1; i < ns; ++i) grouped = grouped && dec_same_group(s[0].qtw, round_qp(s[0].nq), s[i].qtw, round_qp(s[i].nq));
    const DecPlan p = plan_decoder(s.data(), ns, sw);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", p.rc, (int)grouped, (int)p.wide, p.qt, p.nblk, (int)p.leftover, (int)p.fuse_c2s,
           (int)p.fuse_s2c, (int)p.fuse_out, (int)p.fuse_all, (int)p.s2c_kg, (int)p.fits12, (int)p.cached0, (int)p.fill0);
    for (int f = 0; f < 2; ++f)
      for (const DecPhase* ph : {&p.c2s[f], &p.s2c[f], &p.out[f]}) printf(" %s %zu", build_name(*ph).c_str(), ph->lds);
    printf("\n");
  }
  return 0;
}
