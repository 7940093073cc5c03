// mp_geom_host.cpp -- csrc/pps_lin.h / pps_geom.h / pps_cost.h on the host (test infrastructure, tests/test_host_mp_geometry.py): one
// factor's record in either Jacobian mode, plain or robust, and the two retractions, for the arbitrary-precision fixture
// tests/golden/mp_geometry_cases.json.  Planes and 4-vector measurements are normalised first, as pps_add_plane / add_factor do.
// A re-popping plane observation has no lin_* form: its 19 evaluations are the loop of body_linearize_repop (csrc/pps_k1_body.h).
#include <cstring>

#include "pps_lin.h"

using namespace pps;

template <bool ROBUST>
static void lin_repop(const double* pz, const double* pl, const double* ray, const double* w, double* out, const CostFn& cost) {
  const double inv2e = 1.0 / (kNumDiffEps + kNumDiffEps);
  double e[3], r[3];
  res_plane_obs2(pz, pl, ray, e);
  whiten<3>(w, e, r); if (ROBUST) robustify<3>(cost, r);
  for (int j = 0; j < 6; j++) {
    double dl[6] = {0, 0, 0, 0, 0, 0}, pp[7], yp[3], ym[3];
    dl[j] = kNumDiffEps;
    pose_exmap(pz, dl, pp); res_plane_obs2(pp, pl, ray, e); whiten<3>(w, e, yp); if (ROBUST) robustify<3>(cost, yp);
    dl[j] = -kNumDiffEps;
    pose_exmap(pz, dl, pp); res_plane_obs2(pp, pl, ray, e); whiten<3>(w, e, ym); if (ROBUST) robustify<3>(cost, ym);
    for (int q = 0; q < 3; q++) out[q * 6 + j] = (yp[q] - ym[q]) * inv2e;
  }
  for (int j = 0; j < 3; j++) {
    double dl[3] = {0, 0, 0}, pp[4], yp[3], ym[3];
    dl[j] = kNumDiffEps;
    plane_exmap(pl, dl, pp); res_plane_obs2(pz, pp, ray, e); whiten<3>(w, e, yp); if (ROBUST) robustify<3>(cost, yp);
    dl[j] = -kNumDiffEps;
    plane_exmap(pl, dl, pp); res_plane_obs2(pz, pp, ray, e); whiten<3>(w, e, ym); if (ROBUST) robustify<3>(cost, ym);
    for (int q = 0; q < 3; q++) out[18 + q * 3 + j] = (yp[q] - ym[q]) * inv2e;
  }
  for (int q = 0; q < 3; q++) out[27 + q] = r[q];
}

template <int MODE, bool ROBUST>
static void eval(int kind, const double* a, const double* b, const double* ms, const double* w, const double* ray, double* out,
                 const CostFn& cost) {
  double pa[4], pb[4], m4[4];
  if (kind == 0 || kind == 4) {                      // plane observation / re-popping plane observation: a pose, b plane
    memcpy(pb, b, sizeof pb); normalize4(pb);
    if (kind == 4) { lin_repop<ROBUST>(a, pb, ray, w, out, cost); return; }
    memcpy(m4, ms, sizeof m4); normalize4(m4);
    lin_plane_obs<MODE, ROBUST>(a, pb, m4, w, out, cost);
  } else if (kind == 1) {
    lin_odometry<MODE, ROBUST>(a, b, ms, w, out, cost);
  } else if (kind == 2) {
    lin_pose_prior<MODE, ROBUST>(a, ms, w, out, cost);
  } else {                                           // 3: plane prior, a plane
    memcpy(pa, a, sizeof pa); normalize4(pa);
    memcpy(m4, ms, sizeof m4); normalize4(m4);
    lin_plane_prior<MODE, ROBUST>(pa, m4, w, out, cost);
  }
}

// records as K1 writes them: plane observation 30 = Jp 3x6 | Jl 3x3 | r; odometry 78 = J1 6x6 | J2 6x6 | r; pose prior 42; plane prior 12
extern "C" void mp_geom_eval(int kind, int mode, int cost_kind, double cost_b, const double* a, const double* b, const double* ms,
                             const double* w, const double* ray, double* out) {
  const CostFn cost = cost_kind == COST_NONE ? CostFn{} : make_cost(cost_kind, cost_b);
  if (cost_kind == COST_NONE) {
    if (mode == 1) eval<1, false>(kind, a, b, ms, w, ray, out, cost); else eval<0, false>(kind, a, b, ms, w, ray, out, cost);
  } else {
    if (mode == 1) eval<1, true>(kind, a, b, ms, w, ray, out, cost); else eval<0, true>(kind, a, b, ms, w, ray, out, cost);
  }
}

extern "C" void mp_geom_exmap(int kind, const double* x, const double* d, double* out) {
  if (kind == 0) { pose_exmap(x, d, out); return; }
  double pl[4];
  memcpy(pl, x, sizeof pl); normalize4(pl);
  plane_exmap(pl, d, out);
}

extern "C" void mp_geom_repop_wall_plane(const double* pose, const double* ray, double* out) { repop_wall_plane(pose, ray, out); }
