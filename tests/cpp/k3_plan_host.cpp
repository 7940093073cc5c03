// k3_plan_host.cpp -- csrc/pps_k3_plan.h behind a C interface for tests/test_host_k3_plan.py: a plain C++ translation unit, no HIP.
// The plan leaves as JSON text (every field of K3Plan, so the test compares the whole value with tests/golden/k3_plan.json).
#include <cstdio>
#include <cstring>
#include <string>

#include "pps_k3_plan.h"

using namespace pps;

namespace {
struct Json {
  std::string s;
  bool first = true;
  void key(const char* k) { if (!first) s += ", "; first = false; s += '"'; s += k; s += "\": "; }
  void num(const char* k, long long v) { key(k); s += std::to_string(v); }
  void flag(const char* k, bool v) { key(k); s += v ? "true" : "false"; }
  void vec(const char* k, const std::vector<int>& v) {
    key(k); s += '[';
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ", "; s += std::to_string(v[i]); }
    s += ']';
  }
  void open(const char* k, char c) { key(k); s += c; first = true; }
  void close(char c) { s += c; first = false; }
};

std::string to_json(const K3Plan& P) {
  static const char* const forms[] = {"band_stages", "band_all", "dense", "levels"};
  Json j;
  j.s = "{";
  j.key("form"); j.s += '"'; j.s += forms[(int)P.form]; j.s += '"';
  j.open("stages", '[');
  for (const K3StagePlan& sp : P.stages) {
    if (!j.first) j.s += ", ";
    j.s += '{'; j.first = true;
    j.num("grp_begin", sp.grp_begin); j.num("grp_count", sp.grp_count);
    j.num("max_front", sp.max_front); j.num("max_piv", sp.max_piv); j.num("max_panel", sp.max_panel); j.num("max_grp_fronts", sp.max_grp_fronts);
    j.flag("pre", sp.pre); j.flag("reg_only", sp.reg_only); j.flag("r5_ok", sp.r5_ok);
    j.num("nw_factor", sp.nw_factor); j.num("nw_factor_r5", sp.nw_factor_r5);
    j.num("pw_factor_reg", sp.pw_factor_reg); j.num("pw_factor_gen", sp.pw_factor_gen);
    j.num("lds_factor_reg", (long long)sp.lds_factor_reg); j.num("lds_factor_gen", (long long)sp.lds_factor_gen); j.num("lds_factor_r5", (long long)sp.lds_factor_r5);
    j.num("nw_solve", sp.nw_solve); j.num("pw_solve", sp.pw_solve); j.num("nw_flow", sp.nw_flow);
    j.num("lds_solve", (long long)sp.lds_solve); j.num("lds_flow", (long long)sp.lds_flow);
    j.close('}');
  }
  j.close(']');
  j.open("root", '{');
  j.flag("fusable", P.root.fusable); j.flag("pre", P.root.pre); j.flag("flow", P.root.flow);
  j.num("nw", P.root.nw); j.num("pw_factor", P.root.pw_factor); j.num("pw_solve", P.root.pw_solve); j.num("max_grp_fronts", P.root.max_grp_fronts);
  j.num("lds", (long long)P.root.lds);
  j.close('}');
  j.open("all", '{');
  j.num("n_groups", P.all.n_groups); j.num("nw_factor", P.all.nw_factor); j.num("nw_solve", P.all.nw_solve);
  j.num("pw_factor", P.all.pw_factor); j.num("pw_solve", P.all.pw_solve); j.num("max_grp_fronts", P.all.max_grp_fronts);
  j.num("lds_factor", (long long)P.all.lds_factor); j.num("lds_solve", (long long)P.all.lds_solve);
  j.close('}');
  j.vec("level_max_front", P.level_max_front); j.vec("level_max_b", P.level_max_b);
  j.num("max_el_per_front", P.max_el_per_front);
  j.vec("dw_asm", P.dw_asm); j.vec("dw_pan", P.dw_pan); j.vec("dw_trl", P.dw_trl);
  j.s += "}";
  return j.s;
}
}  // namespace

extern "C" {

// counts: n_stages, n_groups, n_levels, n_fronts, band_levels; sw: no_preassemble, no_solve_flow, no_root_fuse, no_strip, trace.
// Returns the length of the JSON text (written when it fits cap, NUL included).
int k3_plan_json(const int* counts, const int* stage_grp_off, const int* grp_lvl_off, const int* glvl_front_off, const int* glvl_fronts,
                 const int* stage_max_front, const int* stage_max_width, const int* f_p, const int* f_b, const int* f_level, const int* level_off,
                 const int* level_fronts, const int* f_el_off, const int* sw, char* out, int cap) {
  BandTreeView v;
  v.n_stages = counts[0]; v.n_groups = counts[1]; v.n_levels = counts[2]; v.n_fronts = counts[3]; v.band_levels = counts[4];
  v.stage_grp_off = stage_grp_off; v.grp_lvl_off = grp_lvl_off; v.glvl_front_off = glvl_front_off; v.glvl_fronts = glvl_fronts;
  v.stage_max_front = stage_max_front; v.stage_max_width = stage_max_width;
  v.f_p = f_p; v.f_b = f_b; v.f_level = f_level;
  v.level_off = level_off; v.level_fronts = level_fronts; v.f_el_off = f_el_off;
  K3Switches ks;
  ks.no_preassemble = sw[0] != 0; ks.no_solve_flow = sw[1] != 0; ks.no_root_fuse = sw[2] != 0; ks.no_strip = sw[3] != 0; ks.trace = sw[4];
  const std::string s = to_json(plan_k3(v, ks));
  if ((int)s.size() + 1 <= cap) memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

int k3_flow_waves(long long per_wave_bytes, int mg, int cap, long long ceiling) { return band_flow_waves((size_t)per_wave_bytes, mg, cap, (size_t)ceiling); }
long long k3_flow_fixed_bytes(int mg) { return (long long)band_flow_fixed_bytes(mg); }
long long k3_solve_lds_bytes(int max_panel) { return (long long)band_solve_lds_bytes(max_panel); }

// group `group` of a tree given by its two offset arrays (a hand-made group: grp_lvl_off = {0, nl}, glvl_front_off = prefix sums of its level counts)
int k3_group_fits_pre(const int* grp_lvl_off, const int* glvl_front_off, int group, int nw) {
  BandTreeView v;
  v.grp_lvl_off = grp_lvl_off; v.glvl_front_off = glvl_front_off;
  return band_group_fits_pre(v, group, nw) ? 1 : 0;
}

// 0 planning budget, 1 launch ceiling, 2 / 3 / 4 wave caps (factor, data flow, fused root), 5 rows of a band front
long long k3_const(int which) {
  switch (which) {
    case 0: return (long long)kLdsPlanBudgetBytes;
    case 1: return kLdsLaunchCeilingBytes;
    case 2: return kFactorWaveCap;
    case 3: return kFlowWaveCap;
    case 4: return kRootFlowWaveCap;
    case 5: return kBandMaxRows;
  }
  return -1;
}
}
