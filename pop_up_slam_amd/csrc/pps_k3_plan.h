// pps_k3_plan.h -- the launch schedule of K3 (pps_k3.hip), decided once per analysis.  Host only: no HIP header, any C++17 compiler
// (tests/cpp/k3_plan_host.cpp).  plan_k3 turns the band schedule of an Analysis into a K3Plan -- kernels, grids, waves, dynamic LDS --; run_analysis
// keeps it in the handle, the launchers of pps_k3.hip launch by it, and plan_chunks (pps_multi.cpp) sizes a batch with the same functions.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace pps {

constexpr int kBandMaxRows = 128;        // rows per front of the band kernels, including the rhs row
// pps_regtile.h (a device header) owns these three as kRegRows / kRegRowsMax / kP8Stride; pps_k3.hip asserts that the copies are equal
constexpr int kPlanRegRows = 64, kPlanRegRowsMax = 80, kPlanP8Stride = 9;
constexpr int kDenseMaxPivots = 64;      // pivots per front of the dense-front kernels (pps_dense.hip asserts it)

// Two LDS ceilings, not one.  Unifying them would change launches; DESIGN.md (K3, "where the schedule is decided") names the asymmetry.
//   kLdsPlanBudgetBytes    what a workgroup is PLANNED into: the factor and barrier-solve wave counts of a stage, the test that takes a graph
//                          off the band kernels (a group's solution vectors + one wave do not fit), the factor side of the whole-tree rule, and
//                          everything plan_chunks sizes for a batch -- the data-flow waves of a batch stage included.
//   kLdsLaunchCeilingBytes what a launch may ASK for (the dynamic-LDS attribute of every K3 kernel): the data-flow waves of a single handle's
//                          stage, of its fused root and of its whole-tree back-substitution, and the level-per-launch fall-back's front.
constexpr size_t kLdsPlanBudgetBytes = 150 * 1024;
constexpr int kLdsLaunchCeilingBytes = 160 * 1024 - 1024;
// waves per workgroup: the factor kernels hold two waves per SIMD, the data-flow back-substitution three, the fused root launch is a factor kernel
constexpr int kFactorWaveCap = 8, kFlowWaveCap = 12, kRootFlowWaveCap = 8;

constexpr int band_front_limit() { return kBandMaxRows - 1; }      // largest front (scalars, without the rhs row) of the band kernels
constexpr int band_reg_rows() { return kPlanRegRows; }             // fronts up to this many rows (incl. rhs) take the register-resident path

// LDS of one wave in the factor kernels.  Register-only kernels (every front of the stage <= 64 rows; the level kernels): the packed
// triangle, whose first 64 x kP8Stride doubles double as the panel buffer once the tiles are loaded (the triangle is dead from then
// on), and one spare double at the end (where masked-off items of a scatter-add land).  The other kernels (LDS strip, fifth tile
// row, LDS-tile path): triangle | spare | panel buffer of 80 rows.
inline size_t band_lds_bytes(int max_front, bool reg_only_kernel = false) {
  const size_t fa = (size_t)max_front + 1, ntri = fa * (fa + 1) / 2;
  const size_t n = reg_only_kernel ? std::max<size_t>(ntri, (size_t)kPlanRegRows * kPlanP8Stride) + 1 : ntri + 1 + (size_t)kPlanRegRowsMax * kPlanP8Stride;
  return ((n + 1) & ~size_t(1)) * sizeof(double);      // (an even number of doubles: every wave's triangle starts 16-byte aligned)
}
// ... and in the back-substitution: xb + the factor panel (max_panel = largest (f+1)*p of the stage)
inline size_t band_solve_lds_bytes(int max_panel) { return (size_t)(kBandMaxRows + max_panel) * sizeof(double); }
// level-per-launch kernels: the packed triangle of a front of <= 16 nt rows (+ rhs), whose head doubles as the 8-column panel buffer, + the spare double
inline int level_lds_doubles(int nt) {
  const size_t fa = (size_t)16 * nt + 1, n = std::max<size_t>(fa * (fa + 1) / 2, (size_t)kPlanRegRows * kPlanP8Stride) + 1;
  return (int)((n + 1) & ~size_t(1));
}

// The data-flow back-substitution: per workgroup one local solution vector per front of the group + a hand-over flag (an int) per front ...
inline size_t band_flow_fixed_bytes(int mg) { return ((size_t)mg * kBandMaxRows + (size_t)(mg + 1) / 2) * sizeof(double); }
// ... and its waves: as many as the group has fronts, at most `cap`, and what `ceiling` holds next to the fixed part (0: not even one)
inline int band_flow_waves(size_t per_wave_bytes, int mg, int cap, size_t ceiling) {
  const size_t fixed = band_flow_fixed_bytes(mg);
  const size_t room = ceiling > fixed ? (ceiling - fixed) / per_wave_bytes : 0;
  return (int)std::min<size_t>(std::min<size_t>((size_t)cap, (size_t)mg), room);
}

// What the planner reads of an Analysis (one line per field to fill, k3_tree_view in pps_graph.h)
struct BandTreeView {
  int n_stages = 0, n_groups = 0, n_levels = 0, n_fronts = 0;
  int band_levels = 1;
  const int *stage_grp_off = nullptr, *grp_lvl_off = nullptr, *glvl_front_off = nullptr, *glvl_fronts = nullptr;
  const int *stage_max_front = nullptr, *stage_max_width = nullptr;
  const int *f_p = nullptr, *f_b = nullptr, *f_level = nullptr;
  const int *level_off = nullptr, *level_fronts = nullptr, *f_el_off = nullptr;
};
// ... and of the handle's Switches
struct K3Switches { bool no_preassemble = false, no_solve_flow = false, no_root_fuse = false, no_strip = false; int trace = 0; };

// k_band_factor_pre walks every level of a group in one round of the stage's nw waves: either the whole group on waves of its own (shape B:
// 4 + 2 + 1 on eight waves) or three to four local levels with the fronts of local levels 2 and up on waves that idle from level 1 on
// (shape A: 8 + 4 + 2 + 1 on eight waves, 4 + 2 + 1 <= 8) -- body_band_factor_pre tells the two apart the same way
inline bool band_group_fits_pre(const BandTreeView& v, int group, int nw) {
  const int l0 = v.grp_lvl_off[group], nl = v.grp_lvl_off[group + 1] - l0;
  if (nl < 1 || nl > 4) return false;
  int upper = 0, c0 = 0;
  for (int k = 0; k < nl; k++) {
    const int c = v.glvl_front_off[l0 + k + 1] - v.glvl_front_off[l0 + k];
    if (k == 0) c0 = c; else upper += c;
  }
  return c0 + upper <= nw || (nl >= 3 && c0 <= nw && upper <= nw);
}

// One band stage: its groups, and the geometry of every kernel that may run it.  Doubles per wave are kernel arguments, bytes the dynamic LDS.
struct K3StagePlan {
  int grp_begin = 0, grp_count = 0;
  int max_front = 0, max_piv = 1, max_panel = 1, max_grp_fronts = 1;   // maxima over the stage: front scalars, pivots, (f+1) p, fronts of a group
  // pre: every group fits the pre-assembling walk (band_group_fits_pre at nw_factor); reg_only: every front <= 64 rows, the register-only
  // kernels; r5_ok: fronts of 65 .. 80 rows, all of them in registers on at most four waves (k_band_factor_r5)
  bool pre = false, reg_only = false, r5_ok = false;
  // factorisation: the register-only family (k_band_factor<true>, _pre, _lean_trace; 0 where !reg_only), the general kernel, and _r5
  int nw_factor = 1, nw_factor_r5 = 1, pw_factor_reg = 0, pw_factor_gen = 0;
  size_t lds_factor_reg = 0, lds_factor_gen = 0, lds_factor_r5 = 0;
  // back-substitution: the barrier form, and the data-flow form (nw_flow == 0: none)
  int nw_solve = 1, pw_solve = 0, nw_flow = 0;
  size_t lds_solve = 0, lds_flow = 0;
};
// the root stage factored and solved by one launch (k_band_root)
struct K3RootPlan { bool fusable = false, pre = false, flow = false; int nw = 0, pw_factor = 0, pw_solve = 0, max_grp_fronts = 0; size_t lds = 0; };
// the whole tree in one factor launch + one back-substitution launch (k_band_factor_all / k_band_solve_all)
struct K3AllPlan { int n_groups = 0, nw_factor = 0, nw_solve = 0, pw_factor = 0, pw_solve = 0, max_grp_fronts = 0; size_t lds_factor = 0, lds_solve = 0; };
enum class K3Form { BandStages, BandAll, Dense, Levels };      // a launch per band stage | the whole tree in two | dense fronts (pps_dense.hip) | a launch per level
struct K3Plan {
  K3Form form = K3Form::Levels;
  std::vector<K3StagePlan> stages;
  K3RootPlan root;
  K3AllPlan all;                                   // (read where form == BandAll)
  std::vector<int> level_max_front, level_max_b;   // per tree level: widest front, widest boundary
  int max_el_per_front = 0;
  // dense-front work lists: per level a prefix sum over its fronts (count + 1 entries at level_off[l] + l) of the 32x32 assembly tiles, the
  // 256-row panel slabs and the 64x64 update tiles
  std::vector<int> dw_asm, dw_pan, dw_trl;
  bool band() const { return form == K3Form::BandStages || form == K3Form::BandAll; }
};

inline K3Plan plan_k3(const BandTreeView& A, const K3Switches& sw) {
  K3Plan P;
  const int Bn = std::max(1, A.band_levels);
  P.stages.assign(A.n_stages, K3StagePlan{});
  P.level_max_front.assign(A.n_levels, 0); P.level_max_b.assign(A.n_levels, 0);
  int max_front = 0, max_piv = 0;
  for (int s = 0; s < A.n_fronts; s++) {
    const int p = A.f_p[s], b = A.f_b[s], l = A.f_level[s];
    K3StagePlan& sp = P.stages[l / Bn];
    sp.max_piv = std::max(sp.max_piv, p); sp.max_panel = std::max(sp.max_panel, (p + b + 1) * p);
    P.level_max_front[l] = std::max(P.level_max_front[l], p + b); P.level_max_b[l] = std::max(P.level_max_b[l], b);
    P.max_el_per_front = std::max(P.max_el_per_front, A.f_el_off[s + 1] - A.f_el_off[s]);
    max_front = std::max(max_front, p + b);
  }
  for (const K3StagePlan& sp : P.stages) max_piv = std::max(max_piv, sp.max_piv);
  bool use_band = max_front <= band_front_limit() && max_piv <= 64;
  // the dense-front solve keeps a front's boundary values in LDS: 15 000 scalars is the ceiling (2-D loop-closure
  // meshes such as torus10000 reach 24 540 under this chain-based dissection and are refused by run_analysis)
  const bool use_dense = !use_band && max_piv <= kDenseMaxPivots && max_front <= 15000;
  if (use_dense)
    for (int l = 0; l < A.n_levels; l++) {
      int a = 0, pn = 0, t = 0;
      P.dw_asm.push_back(0); P.dw_pan.push_back(0); P.dw_trl.push_back(0);
      for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) {
        const int s = A.level_fronts[k];
        const int fa = A.f_p[s] + A.f_b[s] + 1, b1 = A.f_b[s] + 1;
        const int T32 = (fa + 31) / 32, T64 = (b1 + 63) / 64;
        a += T32 * ((A.f_p[s] + 31) / 32); pn += (fa - A.f_p[s] + 255) / 256; t += T64 * (T64 + 1) / 2;
        P.dw_asm.push_back(a); P.dw_pan.push_back(pn); P.dw_trl.push_back(t);
      }
    }
  for (int st = 0; st < A.n_stages; st++) {
    K3StagePlan& sp = P.stages[st];
    sp.grp_begin = A.stage_grp_off[st]; sp.grp_count = A.stage_grp_off[st + 1] - sp.grp_begin; sp.max_front = A.stage_max_front[st];
    int mg = 1;
    for (int gi = sp.grp_begin; gi < sp.grp_begin + sp.grp_count; gi++)
      mg = std::max(mg, A.glvl_front_off[A.grp_lvl_off[gi + 1]] - A.glvl_front_off[A.grp_lvl_off[gi]]);
    sp.max_grp_fronts = mg;
    sp.reg_only = sp.max_front + 1 <= kPlanRegRows;
    sp.r5_ok = !sp.reg_only && sp.max_front + 1 <= kPlanRegRowsMax && sw.trace == 0 && !sw.no_strip;
    // waves per group: one per front of its widest level -- or, when the whole group fits (4 + 2 + 1 on eight waves), one per front
    // of the group: every upper front is then assembled ahead of its level by a wave of its own (body_band_factor_pre, shape B)
    const bool reg_stage = sp.reg_only && sw.trace == 0;
    const int want = std::max(1, std::min(kFactorWaveCap, reg_stage && mg <= kFactorWaveCap && !sw.no_preassemble ? mg : A.stage_max_width[st]));
    sp.nw_factor = (int)std::max<size_t>(1, std::min<size_t>(want, kLdsPlanBudgetBytes / band_lds_bytes(sp.max_front, reg_stage)));
    sp.nw_factor_r5 = std::min(sp.nw_factor, 4);             // (one wave per SIMD: see k_band_factor_r5)
    sp.pw_factor_reg = sp.reg_only ? (int)(band_lds_bytes(sp.max_front, true) / sizeof(double)) : 0;
    sp.pw_factor_gen = (int)(band_lds_bytes(sp.max_front, false) / sizeof(double));
    sp.lds_factor_reg = (size_t)sp.pw_factor_reg * sp.nw_factor * sizeof(double); sp.lds_factor_gen = (size_t)sp.pw_factor_gen * sp.nw_factor * sizeof(double);
    sp.lds_factor_r5 = (size_t)sp.pw_factor_gen * sp.nw_factor_r5 * sizeof(double);
    // per workgroup: one local solution vector per front of a group + per wave xb and the factor panel.  A group that does
    // not fit (very wide elimination trees: hundreds of fronts in one band group) takes the graph off the band kernels
    // (such a graph then runs on the level-per-launch kernels: its fronts are <= 127 rows by the use_band test above)
    const size_t xbytes = (size_t)mg * kBandMaxRows * sizeof(double);
    const size_t per_wave = band_solve_lds_bytes(sp.max_panel);
    sp.pw_solve = (int)(per_wave / sizeof(double));
    if (xbytes + per_wave > kLdsPlanBudgetBytes) { use_band = false; sp.nw_solve = 1; continue; }
    sp.nw_solve = (int)std::max<size_t>(1, std::min<size_t>(want, (kLdsPlanBudgetBytes - xbytes) / per_wave));
    sp.lds_solve = (size_t)sp.pw_solve * sp.nw_solve * sizeof(double) + xbytes;
    // data-flow form: up to twelve waves (three per SIMD), as many as the group has fronts and the LDS holds
    if (!sw.no_solve_flow && mg > 1) sp.nw_flow = band_flow_waves(per_wave, mg, kFlowWaveCap, (size_t)kLdsLaunchCeilingBytes);
    if (sp.nw_flow > 0) sp.lds_flow = (size_t)sp.pw_solve * sp.nw_flow * sizeof(double) + band_flow_fixed_bytes(mg);
  }
  if (!sw.no_preassemble)
    for (K3StagePlan& sp : P.stages) {
      bool ok = sp.grp_count > 0 && sp.reg_only;
      for (int gi = sp.grp_begin; ok && gi < sp.grp_begin + sp.grp_count; gi++) ok = band_group_fits_pre(A, gi, sp.nw_factor);
      sp.pre = ok;
    }
  P.form = use_band ? K3Form::BandStages : use_dense ? K3Form::Dense : K3Form::Levels;
  if (!use_band) return P;
  // The root stage as one launch: one group, every front register-resident, no trace.  The walk back down runs as a data flow when the group
  // has more than one front and the LDS holds a wave per front (at most eight here), else behind barriers on the wider of the two wave counts.
  if (A.n_stages > 0) {
    const K3StagePlan& top = P.stages[A.n_stages - 1];
    K3RootPlan& r = P.root;
    r.fusable = !sw.no_root_fuse && top.grp_count == 1 && top.reg_only && sw.trace == 0;
    if (r.fusable) {
      const int mg = top.max_grp_fronts;
      r.pre = top.pre; r.pw_factor = top.pw_factor_reg; r.pw_solve = top.pw_solve; r.max_grp_fronts = mg;
      r.nw = std::max(top.nw_factor, top.nw_solve); r.flow = !sw.no_solve_flow && mg > 1;
      if (r.flow) {
        const int want = std::max(top.nw_factor, std::min(mg, kRootFlowWaveCap));
        if ((size_t)r.pw_solve * want * sizeof(double) + band_flow_fixed_bytes(mg) <= (size_t)kLdsLaunchCeilingBytes) r.nw = want; else r.flow = false;
      }
      const size_t bf = (size_t)r.pw_factor * r.nw * sizeof(double);
      const size_t bs = (size_t)r.pw_solve * r.nw * sizeof(double) + (r.flow ? band_flow_fixed_bytes(mg) : (size_t)mg * kBandMaxRows * sizeof(double));
      r.lds = std::max(bf, bs);
    }
  }
  // The whole tree in one factor launch + one back-substitution launch (k_band_factor_all / k_band_solve_all, round 6): every stage takes the
  // pre-assembling walk on register-resident fronts, the data-flow back-substitution holds a group of any stage, and the groups fit the chip
  // a few times over -- a graph of thousands of groups (C3) keeps a launch per stage: its upper workgroups would sit on wave slots its leaves
  // need.  Measured over corridor graphs of 500 .. 3 500 poses (tools/size_probe.py, same box, us per LM iteration, whole tree | a launch per
  // band): 75 groups and fewer (up to 1 250 poses; C2 and every frame of C5: 73) 52.2 | 55.9, 56.5 | 57.3, 82.0 | 88.3; 127 groups and
  // more 87.7 | 77.0, 81.4 | 71.0, 85.5 | 74.9, 140.8 | 110.2 (every group's top front releases at agent scope, every waiting group acquires:
  // hundreds of L2 write-backs and invalidations inside one launch instead of one per band): at most 100 groups (it was 512).
  if (A.n_stages >= 2 && sw.trace == 0 && !sw.no_preassemble && !sw.no_solve_flow && !sw.no_root_fuse && A.n_groups <= 100) {
    bool ok = true;
    int nwf = 1, mf = 0, mp = 1, mg = 1;
    for (const K3StagePlan& sp : P.stages) {
      ok = ok && sp.pre && sp.reg_only;
      nwf = std::max(nwf, sp.nw_factor); mf = std::max(mf, sp.max_front);
      mp = std::max(mp, sp.max_panel); mg = std::max(mg, sp.max_grp_fronts);
    }
    const int nws = ok ? band_flow_waves(band_solve_lds_bytes(mp), mg, kFlowWaveCap, (size_t)kLdsLaunchCeilingBytes) : 0;
    ok = ok && mg > 1 && nws >= std::min(8, mg) && band_lds_bytes(mf, true) * (size_t)nwf <= kLdsPlanBudgetBytes;
    if (ok) {
      K3AllPlan& a = P.all;
      P.form = K3Form::BandAll;
      a.n_groups = A.n_groups; a.nw_factor = nwf; a.nw_solve = nws; a.max_grp_fronts = mg;
      a.pw_factor = (int)(band_lds_bytes(mf, true) / sizeof(double)); a.pw_solve = (int)(band_solve_lds_bytes(mp) / sizeof(double));
      a.lds_factor = (size_t)a.pw_factor * nwf * sizeof(double); a.lds_solve = (size_t)a.pw_solve * nws * sizeof(double) + band_flow_fixed_bytes(mg);
    }
  }
  return P;
}

}  // namespace pps
