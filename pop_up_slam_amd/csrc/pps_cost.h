// pps_cost.h -- robust cost functions (Slam::set_cost_function).  Host + device, no HIP needed: tests/cpp/cost_host.cpp compiles it with g++.
//   reference: Factor::error (isam/Factor.h:67-77) -- after whitening every component becomes r_i <- sign(r_i) sqrt(rho(r_i)), sign(0) = +1,
//   in EVERY evaluation of the error: the 2 n + 1 evaluations of the central differences (the numeric Jacobian differentiates through rho),
//   weighted_errors, and chi2 = sum rho(r_i).  The cost functions restate isam/robust.h.
// A function pointer cannot cross to the device: a cost is an enumerated kind (include/pps.h: PPS_COST_*) and one parameter b.
//   HUBER         rho = d^2 for |d| < b, else 2 b |d| - b^2
//   PSEUDO_HUBER  rho = 2 b^2 (sqrt(1 + d^2 / b^2) - 1), evaluated as 2 d^2 / (sqrt(1 + d^2 / b^2) + 1): the same function without the
//                 cancellation at |d| << b (the numerical differences evaluate it 1e-4 away from zero residuals)
//   CAUCHY        rho = log(pi / b) * log(1 + d^2 / b^2) -- a PRODUCT of two logarithms, as the reference writes it.  That is a quirk (the
//                 textbook form is b^2 log(1 + d^2 / b^2)); it is kept because the reference is the yardstick.  rho > 0 needs b < pi: the C ABI
//                 refuses b >= pi.  The second logarithm is taken as log1p.
// Kinds of isam/robust.h that are left out, and why:
//   Blake-Zisserman     rho(0) = -log(1 + e) < 0: sqrt(rho) is NaN at every small residual
//   corrupted Gaussian  rho(0) > 0: sign * sqrt(rho) jumps from -sqrt(rho(0)) to +sqrt(rho(0)) at 0, no Jacobian there
//   L1                  rho = 2 b |d|: phi = sqrt(2 b |d|) has infinite slope at 0, so JAC_ANALYTIC has no form
// JAC_ANALYTIC uses the chain rule: row i of the whitened J is scaled by phi'(r_i) = rho'(r_i) / (2 sqrt(rho(r_i))) (taken with the sign of
// r_i, i.e. >= 0); at r_i = 0 the limit: 1 for Huber and pseudo-Huber, sqrt(log(pi / b)) / b for Cauchy.
#pragma once
#include "pps_geom.h"

namespace pps {

enum { COST_NONE = 0, COST_HUBER = 1, COST_PSEUDO_HUBER = 2, COST_CAUCHY = 3 };      // == PPS_COST_* (include/pps.h)

// a kernel argument of the robust kernels (pps_robust.hip) -- not a member of DevGraph
struct CostFn {
  int kind = COST_NONE;
  double b = 1.0;
  double k = 0.0;      // CAUCHY: log(pi / b), evaluated once on the host (make_cost)
};

inline CostFn make_cost(int kind, double b) {
  CostFn c;
  c.kind = kind; c.b = b;
  c.k = kind == COST_CAUCHY ? log(kPi / b) : 0.0;
  return c;
}

PPS_HD double cost_rho(const CostFn& c, double d) {
  const double ad = fabs(d), d2 = d * d, b2 = c.b * c.b;
  if (c.kind == COST_HUBER) return ad < c.b ? d2 : 2.0 * c.b * ad - b2;
  if (c.kind == COST_PSEUDO_HUBER) return 2.0 * d2 / (sqrt(1.0 + d2 / b2) + 1.0);
  if (c.kind == COST_CAUCHY) return c.k * log1p(d2 / b2);
  return d2;
}

// phi = sign(d) sqrt(rho(d)), sign(0) = sign(-0.0) = +1
PPS_HD double cost_phi(const CostFn& c, double d) {
  const double s = sqrt(cost_rho(c, d));
  return d < 0.0 ? -s : s;
}

// phi'(d) >= 0; where rho rounds to 0 (d = 0, or d^2 underflows) the limit at 0
PPS_HD double cost_dphi(const CostFn& c, double d) {
  const double ad = fabs(d), b2 = c.b * c.b, rho = cost_rho(c, d);
  if (c.kind == COST_HUBER) return ad < c.b ? 1.0 : c.b / sqrt(rho);
  if (c.kind == COST_PSEUDO_HUBER) return rho > 0.0 ? ad / (sqrt(1.0 + d * d / b2) * sqrt(rho)) : 1.0;
  if (c.kind == COST_CAUCHY) return rho > 0.0 ? c.k * ad / ((b2 + d * d) * sqrt(rho)) : sqrt(c.k) / c.b;
  return 1.0;
}

// r_i <- phi(r_i), in place: what follows every whiten<M> of a robust evaluation
template <int M>
PPS_HD void robustify(const CostFn& c, double r[M]) {
#pragma unroll
  for (int i = 0; i < M; i++) r[i] = cost_phi(c, r[i]);
}

// the analytic mode: rows of the whitened J (COLS columns each, row-major) scaled by phi'(r_i); r is the whitened residual BEFORE robustify
template <int M, int COLS>
PPS_HD void robustify_rows(const CostFn& c, const double r[M], double* J) {
#pragma unroll
  for (int i = 0; i < M; i++) {
    const double s = cost_dphi(c, r[i]);
#pragma unroll
    for (int j = 0; j < COLS; j++) J[i * COLS + j] *= s;
  }
}

}  // namespace pps
