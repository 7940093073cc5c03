// pps_gate_dev.h -- what the Mahalanobis gate kernels share on the device (pps_gate.hip, pps_merge.hip, pps_fgate.hip, pps_loop.hip): the lane
// evaluations of a central difference, the strip products J Sigma J' from end-aligned strips, the small Cholesky solve behind d2, and the
// best-candidate scan, the common-ancestor walk.  The calls must agree bit for bit with pps_eval_factor and with each other, so every function states the
// order of operations it promises; tests/test_host_gate_dev.py and tests/test_host_gate_dev_m6.py pin those orders on the host.  Compile the including file without
// contraction (the Makefile does), like pps_k1_lanes.hip.
#pragma once
#include "pps_k1_body.h"
#include "pps_status.h"

namespace pps {

// ---- one lane's evaluation of a central difference: state, step of column q with sign sgn, residual, whiten ----
// The single copy for the gate kernels of the four chains of body_linearize_lanes (pps_k1_body.h: plane observation at "every lane takes
// the same path", odometry, pose prior and plane prior behind it), statement for statement: K1 keeps its own, because every kernel that
// sweeps in the lane form must inline the same source (see state_pose there).  A column index out of range is the zero step, which is the
// exact identity for a pose; a plane keeps its stored value unless it is the stepped node.  The callers load state, measurement and
// weights and pass DevGraph::step_ac: nothing here indexes anything.  (k_factor_gate keeps the plane-observation chain written out: see there.)
// plane observation: q in 0 .. 5 steps the pose, 6 .. 8 the plane
__device__ __forceinline__ void eval_plane_obs(const double pz[7], const double pl[4], const double ms[4], const double sw[6], int q, double sgn,
                                               const double step_ac[4], double y[3]) {
  double pp[7], lp[4], e[3];
  perturb6(pz, q, sgn, step_ac, pp);
  perturb3(pl, q - 6, sgn, step_ac, lp);
  const bool pert_plane = q >= 6 && q < 9;
#pragma unroll
  for (int k = 0; k < 4; k++) lp[k] = pert_plane ? lp[k] : pl[k];
  res_plane_obs(pp, lp, ms, e);
  whiten<3>(sw, e, y);
}
// plane prior: q in 0 .. 2
__device__ __forceinline__ void eval_plane_prior(const double pl[4], const double ms[4], const double sw[6], int q, double sgn, const double step_ac[4],
                                                 double y[3]) {
  double lp[4], e[3];
  perturb3(pl, q, sgn, step_ac, lp);
#pragma unroll
  for (int k = 0; k < 4; k++) lp[k] = q < 3 ? lp[k] : pl[k];
  res_plane_prior(lp, ms, e);
  whiten<3>(sw, e, y);
}
// odometry: q in 0 .. 5 steps the first pose, 6 .. 11 the second
__device__ __forceinline__ void eval_odometry(const double p1[7], const double p2[7], const double ms[6], const double sw[21], int q, double sgn,
                                              const double step_ac[4], double y[6]) {
  double pa[7], pb[7], e[6];
  perturb6(p1, q, sgn, step_ac, pa);
  perturb6(p2, q - 6, sgn, step_ac, pb);
  res_odometry(pa, pb, ms, e);
  whiten<6>(sw, e, y);
}
// pose prior: q in 0 .. 5
__device__ __forceinline__ void eval_pose_prior(const double pz[7], const double ms[6], const double sw[21], int q, double sgn, const double step_ac[4],
                                                double y[6]) {
  double pp[7], e[6];
  perturb6(pz, q, sgn, step_ac, pp);
  res_pose_prior(pp, ms, e);
  whiten<6>(sw, e, y);
}

// ---- one lane's share of the six distinct entries of S = Ja Sigma_aa Ja' + Jb Sigma_bb Jb' + Ja Sigma_ab Jb' + Jb Sigma_ba Ja' ----
// Ja (3 x DA), Jb (3 x DB) row-major; Ya (K x DA), Yb (K x DB) the strips of k_cov_path (pps_cov.h), filled from their END: rows
// K - len .. K - 1 are valid, the rows ahead of them are never read.  Lane `lane` takes the rows K - 1 - j, j = lane, lane + 64, ...
// below max(len_a, len_b): the products of a lane and the order they are added in depend on the two nodes alone, not on K -- not on
// what else is in the call.  Per row z_a = Ja y_a, z_b = Jb y_b (columns ascending, from 0.0; zero where the strip has no such row),
// then s[e] += ... for e = (0,0) (1,0) (1,1) (2,0) (2,1) (2,2).
// A row of a front both paths pass through (j < common) carries all four products z_a z_a' + z_b z_b' + z_a z_b' + z_b z_a' =
// (z_a + z_b)(z_a + z_b)': the two are added BEFORE they are multiplied.  A pose and a landmark it sees -- or two estimates of one wall
// -- share most of their uncertainty, z_a is close to -z_b on those rows and S is what is left of the difference: summed first, rounding
// is relative to |z_a|, multiplied out it would be relative to |z_a|^2 against a result of the size |z_a + z_b|^2.  Rows of fronts the
// paths do not share keep their two squares apart: no cross term exists there, whatever sits at the same strip index -- which is also
// why the strips are NOT added row by row ahead of the product (end-aligned strips put rows of two different fronts at one index).
// strip_gram<M, DA, DB> is that operation for M rows of J, with the M (M + 1) / 2 entries in the same row-major lower-triangle order
// ((0,0) (1,0) (1,1) (2,0) ...) and the rows of Ja / Jb lda / ldb doubles apart (two halves of one wider J: pps_loop.hip reads its
// 6 x 12 Jacobian from LDS, the same address in every lane).  strip_gram3 is its M = 3 case on packed Jacobians: the same statements.
template <int M, int DA, int DB>
__device__ __forceinline__ void strip_gram(const double* Ja, int lda, const double* Jb, int ldb, const double* __restrict__ Ya, const double* __restrict__ Yb,
                                           int len_a, int len_b, int common, int K, int lane, double s[M * (M + 1) / 2]) {
  const int len = len_a > len_b ? len_a : len_b;
  for (int j = lane; j < len; j += 64) {
    const size_t k = (size_t)(K - 1 - j);
    double za[M], zb[M], z[M];
#pragma unroll
    for (int i = 0; i < M; i++) za[i] = zb[i] = 0.0;
    if (j < len_a) {
      double y[DA];
#pragma unroll
      for (int q = 0; q < DA; q++) y[q] = Ya[k * DA + q];
#pragma unroll
      for (int i = 0; i < M; i++) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < DA; q++) t += Ja[i * lda + q] * y[q];
        za[i] = t;
      }
    }
    if (j < len_b) {
      double y[DB];
#pragma unroll
      for (int q = 0; q < DB; q++) y[q] = Yb[k * DB + q];
#pragma unroll
      for (int i = 0; i < M; i++) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < DB; q++) t += Jb[i * ldb + q] * y[q];
        zb[i] = t;
      }
    }
    const bool cross = j < common;
#pragma unroll
    for (int i = 0; i < M; i++) z[i] = za[i] + zb[i];
    int e = 0;
#pragma unroll
    for (int i = 0; i < M; i++)
#pragma unroll
      for (int jj = 0; jj <= i; jj++, e++) s[e] += cross ? z[i] * z[jj] : za[i] * za[jj] + zb[i] * zb[jj];
  }
}
template <int DA, int DB>
__device__ __forceinline__ void strip_gram3(const double* Ja, const double* Jb, const double* __restrict__ Ya, const double* __restrict__ Yb, int len_a,
                                            int len_b, int common, int K, int lane, double s[6]) {
  strip_gram<3, DA, DB>(Ja, DA, Jb, DB, Ya, Yb, len_a, len_b, common, K, lane, s);
}
// the 64 partial sums of one entry, added in lane order from 0.0 by ONE lane: one fixed order of additions
__device__ __forceinline__ double lane_order_sum(const double* part) {
  double t = 0.0;
  for (int k = 0; k < 64; k++) t += part[k];
  return t;
}

// ---- the pivots two root paths have in common (pps_merge.hip, pps_loop.hip) ----
// parent: the parent front of every front (-1: a root); rootlen: per front the pivots of the front and of all its ancestors, which fall
// strictly on the way up -- so the front with the longer path cannot be the meeting point and steps to its parent until the two meet (the
// same front; one an ancestor of the other; disjoint subtrees) or both have left the tree (no common root: 0).  Every front the walk
// reaches is checked against n_fronts and the hops are counted: false = an index outside the tables (common is then 0).
__device__ __forceinline__ bool common_root_pivots(const int* __restrict__ parent, const int* __restrict__ rootlen, int n_fronts, int fa, int fb, int& common) {
  common = 0;
  int hops = 0;
  while (fa != fb && fa >= 0 && fb >= 0) {
    const int la = rootlen[fa], lb = rootlen[fb];
    int na = fa, nb = fb;
    if (la >= lb) na = parent[fa];
    if (lb >= la) nb = parent[fb];
    fa = na; fb = nb;
    if (fa < -1 || fa >= n_fronts || fb < -1 || fb >= n_fronts || ++hops > 2 * n_fronts) return false;
  }
  common = (fa == fb && fa >= 0) ? rootlen[fa] : 0;
  return true;
}

// ---- d2 = r' A^-1 r by the Cholesky factor of a symmetric M x M matrix ----
// A row-major with leading dimension M, read on and below the diagonal only.  Column by column, j ascending: the pivot
// p_j = A_jj - sum_k l_jk^2 and t_j = r_j - sum_k l_jk y_k (k ascending, both subtracted term by term), l_jj = sqrt(p_j), y_j = t_j / l_jj,
// then l_ij = (A_ij - sum_k l_ik l_jk) / l_jj for i > j (k ascending); d2 = sum_j y_j^2 from 0.0, j ascending.  Returns false with
// d2 = NaN at the first pivot that is not above pivot_min or not finite (NaN included); nothing behind that pivot is evaluated.
template <int M>
__device__ __forceinline__ bool chol_d2(const double* A, const double* r, double pivot_min, double& d2) {
  double l[M * M], y[M], acc = 0.0;
  d2 = __builtin_nan("");
#pragma unroll
  for (int j = 0; j < M; j++) {
    double p = A[j * M + j], t = r[j];
#pragma unroll
    for (int k = 0; k < j; k++) { p -= l[j * M + k] * l[j * M + k]; t -= l[j * M + k] * y[k]; }
    if (!(p > pivot_min && p <= kDblMax)) return false;
    const double ljj = sqrt(p);
    y[j] = t / ljj;
    acc += y[j] * y[j];
#pragma unroll
    for (int i = j + 1; i < M; i++) {
      double u = A[i * M + j];
#pragma unroll
      for (int k = 0; k < j; k++) u -= l[i * M + k] * l[j * M + k];
      l[i * M + j] = u / ljj;
    }
  }
  d2 = acc;
  return true;
}

// ---- the best candidate of a row of d2: the smallest finite value, the first index on ties; a NaN or an infinity never wins ----
// thread t of nt: the candidates t, t + nt, ... below n in ascending order with strict <, index `skip` left out (-1: none).  bi = -1: none.
__device__ __forceinline__ void best_scan_thread(const double* row, int n, int skip, int t, int nt, int& bi, double& bv) {
  bi = -1; bv = 0.0;
  for (int k = t; k < n; k += nt) {
    if (k == skip) continue;
    const double v = __hip_atomic_load(&row[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (is_finite(v) && (bi < 0 || v < bv)) { bi = k; bv = v; }
  }
}
// one thread, starting from its own candidate (bi, bv), takes the candidates of threads 1 .. nt - 1 in thread order; returns the index
__device__ __forceinline__ int best_scan_final(const double* cv, const int* ci, int nt, int bi, double bv) {
  for (int k = 1; k < nt; k++) {
    const int ki = ci[k];
    const double kv = cv[k];
    if (ki >= 0 && (bi < 0 || kv < bv || (kv == bv && ki < bi))) { bi = ki; bv = kv; }
  }
  return bi;
}

}  // namespace pps
