// Launch selection of the factor sweep and the solves (device_plan.hpp LaunchForm): host only.
#include "device_plan.hpp"
#include "fgo_internal.hpp"

namespace fgo {

// ---- launch selection (device_plan.hpp): every threshold of the factor / solve launchers, as pure functions of the schedule.
// The height cuts of the generic kernels choose how many waves share a column or a row, never what a kernel can hold: k_chol_fact
// takes the blocks beyond MAXP * NW * 10 in overflow passes and the solve kernels stride over a list of any length, so a forced
// cut-off needs no clamp -- every instantiation is correct (only slower) at every height.
const char *launch_form_name(int form) {
  static const char *const names[LF_COUNT] = {
    "k_chol_acc<8>", "k_chol_acc<4>", "k_chol_acc<2>", "k_chol_acc<1>", "k_chol_acc2<8>", "k_chol_acc2<4>", "k_chol_acc2<1>", "k_fwd_combine",
    "k_panel_tri<16>", "k_panel_tri<8>", "k_panel_tri1", "k_panel_rows", "k_panel_rows_byc", "k_chol_leaf<4>",
    "k_chol_fact<1,2>", "k_chol_fact<1,3>", "k_chol_fact<4,3>", "k_chol_fact<8,3>", "k_chol_fact<16,2>",
    "k_solve_fwd<1>", "k_solve_fwd<4>", "k_solve_fwd<16>", "k_fwd_ext", "k_fwd_tri",
    "k_bwd_chain", "k_bwd_fused", "k_bwd_ext", "k_bwd_tri", "k_solve_bwd<1>", "k_solve_bwd<4>", "k_solve_bwd<8>"};
  return form >= 0 && form < LF_COUNT ? names[form] : "?";
}
LaunchForm select_acc(const HostSchedule &H, int l) {
  const int n_g2_full = H.g2_lvl.empty() ? 0 : (int)(H.g2_lvl[l + 1] - H.g2_lvl[l]);
  if (n_g2_full > 0) {      // (the symbolic phase builds these lists for the very wide levels only: FGO_ACC2_MIN)
    // column-group form (scalar B operand).  Split the entry lists where there are few groups (short chains at the top)
    static const int g2_narrow = (int)tune("acc2_narrow", 400);
    static const int g2_mid = (int)tune("acc2_mid", 6000);
    return n_g2_full <= g2_narrow ? LF_ACC2_8 : n_g2_full <= g2_mid ? LF_ACC2_4 : LF_ACC2_1;   // (by the level's FULL list, partial sweep or not)
  }
  const int64_t n = H.acc_ptr[l + 1] - H.acc_ptr[l];
  // few targets (the skinny top of the tree): split every source list 8 ways to shorten the dependent chain
  static const int64_t narrow_max = (int64_t)tune("acc_narrow", 4000);
  // very many targets (the lowest panel levels: short lists, 10^5 .. 10^6 targets): one wave per 10 targets, no
  // split-K and no LDS combine -- the launch is bound by how many independent waves are in flight, not by the
  // length of a list (cfg 2: factor sweep 5.98 -> 5.73 ms, cfg 5: 35.9 -> 33.0 ms)
  static const int64_t acc_wide2 = (int64_t)tune("acc_wide2", 60000);
  static const int64_t acc_mid2 = (int64_t)tune("acc_mid2", 15000);   // in between: split two ways (3.78 -> 3.74 ms)
  static const int acc_wide_split = (int)tune("acc_wide_split", 1);
  if (n <= narrow_max) return LF_ACC8;
  if (n > acc_wide2) return acc_wide_split == 1 ? LF_ACC1 : LF_ACC2;
  return n > acc_mid2 ? LF_ACC2 : LF_ACC4;
}
LaunchForm select_tri(const HostSchedule &H, int l) {
  const int ntf = H.level_ptr[l + 1] - H.level_ptr[l];         // the whole level (kernel choices go by it)
  // 16 waves hold a panel's trailing matrix with the fewest tiles per wave, but their registers allow one workgroup
  // per CU; levels with more panels than CUs run the 8-wave instantiation, two workgroups per CU
  const int tri_wide = tri_wide_panels(H.cus);
  // (a 4-wave instantiation with four workgroups per CU for the very wide levels -- twice the pivot chains in flight --
  //  was measured slower: cfg 2 factor sweep 3.27 -> 3.34 ms, cfg 5 21.5 -> 22.3 ms)
  // wide levels: the throughput form, one wave per panel (FGO_TRI1=0: the 8-wave latency form, two workgroups per CU)
  static const int tri1_on = (int)tune("tri1", 1);
  // (one wave per panel holds 4 panels per CU: it beats two 8-wave workgroups per CU once there are >= 3 rounds of those)
  const int tri1_min = (int)tune("tri1_min", 3 * H.cus);
  if (tri1_on && ntf > tri_wide && ntf >= tri1_min) return LF_TRI1;
  return ntf > tri_wide ? LF_TRI8 : LF_TRI16;
}
LaunchForm select_rows(const HostSchedule &H, int l) { return l >= H.rows_byc_level ? LF_ROWS_BYC : LF_ROWS; }
LaunchForm select_fact(const HostSchedule &H, int l) {
  if (!H.level_leaf.empty() && H.level_leaf[l]) return LF_LEAF4;
  // single-column tasks (the landmarks of a bundle adjustment): one wave per task instead of four; columns of <= 20
  // blocks keep two register passes instead of three (fewer VGPRs, more waves per SIMD)
  static const int h1_2 = (int)tune("fact_h1_2", 20), h1_3 = (int)tune("fact_h1_3", 30), h4 = (int)tune("fact_h4", 120), h8 = (int)tune("fact_h8", 240);
  const bool single = H.level_maxtaskcols[l] == 1;
  const int h = H.level_maxcol[l];
  if (single && h <= h1_2) return LF_FACT_1_2;
  if (single && h <= h1_3) return LF_FACT_1_3;
  return h <= h4 ? LF_FACT_4_3 : h <= h8 ? LF_FACT_8_3 : LF_FACT_16_2;
}
LaunchForm select_fwd(const HostSchedule &H, int l) {
  static const int h1 = (int)tune("fwd_h1", 40), h4 = (int)tune("fwd_h4", 160);
  if (H.level_maxtaskcols[l] == 1 && H.level_maxrow[l] <= h1) return LF_FWD1;
  return H.level_maxrow[l] <= h4 ? LF_FWD4 : LF_FWD16;
}
LaunchForm select_bwd(const HostSchedule &H, int l) {
  if (H.level_panel[l]) {
    // few panels (the top of the tree): one fused launch per level, a 16-wave workgroup per panel
    static const int bwd_fused_max = (int)tune("bwd_fused", 256);   // swept 0 / 32 / 128 / 256 / 512 / 4096 on cfg 2: 137.3 / 138.4 / 138.9 / 139.0 / 139.0 / 132.6 it/s
    return H.level_ptr[l + 1] - H.level_ptr[l] <= bwd_fused_max ? LF_BWD_FUSED : LF_BWD_EXT;
  }
  static const int h1 = (int)tune("bwd_h1", 20), h4 = (int)tune("bwd_h4", 80);
  if (H.level_maxtaskcols[l] == 1 && H.level_maxcol[l] <= h1) return LF_BWD1;
  return H.level_maxcol[l] <= h4 ? LF_BWD4 : LF_BWD8;
}

}  // namespace fgo
