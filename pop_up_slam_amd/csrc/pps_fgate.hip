// pps_fgate.hip -- the leave-one-out chi-square test of the graph's own factors (pps_factor_gate): d2 = r' (I - P)^-1 r and
// lev = trace(P), P = J Sigma_ff J', of every listed factor, from the selected inverse a recovery left in the panel layout of L.
// pps_fgate.h has the algebra.
//
// One wave per list entry, kFgateWaves entries per workgroup, ONE launch; an entry reads the table record of its factor, the state and the
// three blocks of Sigma_ff, and writes its own d2, lev, status and record: no entry waits for another, nothing is accumulated across
// entries, so an entry's answer does not depend on what else is in the list.
//   1. r and J at the estimate by the device functions K1 runs for the factor's type.  Numeric mode: the 2 c + 1 evaluations of the lane
//      form side by side on lanes (eval_odometry / eval_pose_prior / eval_plane_prior of pps_gate_dev.h, the gate kernels' copy of
//      body_linearize_lanes; the plane observation's chain is written out next to its contracted sibling, see there), the column
//      differences through LDS.  Analytic mode: the closed form of pps_lin.h in one lane.  This file is compiled without contraction
//      like pps_k1_lanes.hip, pps_gate.hip and pps_merge.hip.  A re-popping plane observation (Pose3d_Plane3d_Factor2) takes the 19 evaluations of body_linearize_repop in both modes: the steps by pose_exmap / plane_exmap,
//      the residual by fgate_repop_eval below, which carries the contraction of the one kernel pps_eval_factor has for such a factor.
//   2. the record [J m x c row-major | r m]: columns of node a, then of node b -- the order of pps_eval_factor.
//   3. Sigma_ff (c x c) straight from the selected inverse into LDS: lanes over its entries, each through the block descriptor of its
//      quadrant (source offset, leading dimension, transpose flag; the lower-left quadrant is the transposed upper-right one).
//   4. T = J Sigma_ff (m x c) and P = T J' (m x m), lanes over the entries, the inner sums in ascending order.
//   5. one lane: lev, I - P in place, then chol_d2<3> or <6> (pps_gate_dev.h) on the wave-uniform m with pivot floor kFgatePivotMin.
// LDS per wave: Sigma 144 | T 72 | record 78 doubles (2 352 bytes); the evaluations of step 1 use the first two areas before Sigma arrives,
// P takes Sigma's place once T is complete.  Plain fp64 multiply-add loops: 6 x 12 against 12 x 12 is no MFMA shape.
#include <hip/hip_runtime.h>

#include "pps_fgate.h"
#include "pps_gate_dev.h"
#include "pps_symbolic.h"

namespace pps {

namespace {

constexpr int kFgateThreads = 64 * kFgateWaves;
// dynamic LDS per wave, in doubles
constexpr int kFgateLdsS = 0, kFgateLdsT = kFgateLdsS + 144, kFgateLdsJ = kFgateLdsT + 72, kFgateLdsWave = kFgateLdsJ + kFgateRecord;
constexpr int kFgateEvalStride = 6;              // doubles per evaluation (m <= 6), 25 evaluations at most
static_assert(25 * kFgateEvalStride <= kFgateLdsJ, "the evaluations use the Sigma and T areas");
static_assert((kFgateLdsWave * sizeof(double)) % 16 == 0, "every wave's area starts at a multiple of 16 bytes");

// ---- one whitened evaluation of a re-popping plane observation, contracted as K1 contracts it ----
// pps_eval_factor takes a Pose3d_Plane3d_Factor2 through k_linearize_repop (pps_k1.hip), the one K1 kernel that has no lane form and is
// built WITH contraction.  Its record is met bit for bit only by the same expressions under the same contraction: the few functions of
// pps_geom.h on that path that are not contraction-exact by themselves are written out here once more, between the two pragmas.  (The
// steps -- pose_exmap, plane_exmap -- and normalize4 / normalize4_r / quat_mul / rsqrt_acc are exact wherever they are compiled.)
#pragma clang fp contract(fast)
__device__ __forceinline__ void fgate_quat_to_R(const double q[4], double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
__device__ __forceinline__ void fgate_repop_eval(const double pose[7], const double plane[4], const double ray[6], const double w[6], double y[3]) {
  double R[9];
  fgate_quat_to_R(pose + 3, R);
  // repop_wall_plane
  double gs[4], ms[4];
  gs[0] = R[0] * 0.0 + R[3] * 0.0 + R[6] * -1.0 + 0.0 * 0.0;
  gs[1] = R[1] * 0.0 + R[4] * 0.0 + R[7] * -1.0 + 0.0 * 0.0;
  gs[2] = R[2] * 0.0 + R[5] * 0.0 + R[8] * -1.0 + 0.0 * 0.0;
  gs[3] = pose[0] * 0.0 + pose[1] * 0.0 + pose[2] * -1.0 + 1.0 * 0.0;
  double Pt[2][3];
  for (int j = 0; j < 2; j++) {
    const double* r = ray + 3 * j;
    const double frac = -gs[3] / (gs[0] * r[0] + gs[1] * r[1] + gs[2] * r[2]);
    Pt[j][0] = frac * r[0]; Pt[j][1] = frac * r[1]; Pt[j][2] = frac * r[2];
  }
  const double t1[3] = {Pt[1][0] - Pt[0][0], Pt[1][1] - Pt[0][1], Pt[1][2] - Pt[0][2]};
  const double n[3] = {t1[1] * gs[2] - t1[2] * gs[1], t1[2] * gs[0] - t1[0] * gs[2], t1[0] * gs[1] - t1[1] * gs[0]};
  ms[0] = n[0]; ms[1] = n[1]; ms[2] = n[2];
  ms[3] = -(n[0] * Pt[0][0] + n[1] * Pt[0][1] + n[2] * Pt[0][2]);
  normalize4(ms);
  // res_plane_obs: quat_to_R once more, as K1's inlined copy has it
  double R2[9], u[4], dq[4], e[3];
  fgate_quat_to_R(pose + 3, R2);
  u[0] = R2[0] * plane[0] + R2[3] * plane[1] + R2[6] * plane[2];
  u[1] = R2[1] * plane[0] + R2[4] * plane[1] + R2[7] * plane[2];
  u[2] = R2[2] * plane[0] + R2[5] * plane[1] + R2[8] * plane[2];
  u[3] = pose[0] * plane[0] + pose[1] * plane[1] + pose[2] * plane[2] + plane[3];
  normalize4_r(u);
  // log_diff
  const double cj[4] = {-ms[0], -ms[1], -ms[2], ms[3]};
  quat_mul(u, cj, dq);
  const double nn = dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2];
  if (nn != 0.0) {
    const double ri = rsqrt_acc(nn);
    const double angle = 2.0 * atan2(nn * ri, fabs(dq[3]));
    const double s = dq[3] < 0 ? -(angle * ri) : angle * ri;
    e[0] = dq[0] * s; e[1] = dq[1] * s; e[2] = dq[2] * s;
  } else {
    e[0] = e[1] = e[2] = 0.0;
  }
  // whiten<3>
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double s = 0;
#pragma unroll
    for (int j = i; j < 3; j++) s += w[k++] * e[j];
    y[i] = s;
  }
}
#pragma clang fp contract(off)

// where block (dr x dc) of descriptor k ends in S
__device__ __forceinline__ bool fgate_block_ok(const FgateFactor& f, int k, int dr, int dc, long long n_S) {
  if (f.src[k] < 0 || f.ld[k] < 1) return false;
  const bool tr = k == 2 && f.tr != 0;
  const long long last = f.src[k] + (long long)((tr ? dc : dr) - 1) * f.ld[k] + ((tr ? dr : dc) - 1);
  return last < n_S;
}

__global__ __launch_bounds__(kFgateThreads) void k_factor_gate(DevGraph d, FgateArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fgate_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int e = blockIdx.x * kFgateWaves + w;
  double* Sg = fgate_lds + w * kFgateLdsWave + kFgateLdsS;               // (the areas are re-used under other names: no __restrict__)
  double* T = fgate_lds + w * kFgateLdsWave + kFgateLdsT;
  double* J = fgate_lds + w * kFgateLdsWave + kFgateLdsJ;
  double* yb = Sg;                                                       // step 1 only
  // (every test below is the same in all lanes of a wave; a wave without an entry still takes part in the barriers)
  bool valid = e < a.n;
  FgateFactor f = {{0, 0, 0}, {1, 1, 1}, 0, -1, 0};
  int ia = 0, ib = -1, da = 0, db = 0, m = 0;
  bool repop = false;
  if (valid) {
    const int fid = a.list[e];
    bool ok = fid >= 0 && fid < a.n_factors;
    if (ok) {
      f = a.factors[fid];
      ok = f.slot >= 0 && ((f.type == F_POSE_PRIOR && f.slot < d.n_pp) || (f.type == F_ODOMETRY && f.slot < d.n_odo) ||
                           (f.type == F_PLANE_OBS && f.slot < d.n_obs) || (f.type == F_PLANE_PRIOR && f.slot < d.n_lp));
    }
    if (ok) {
      if (f.type == F_POSE_PRIOR) { ia = d.pp_pose[f.slot]; da = 6; m = 6; }
      else if (f.type == F_ODOMETRY) { ia = d.odo_a[f.slot]; ib = d.odo_b[f.slot]; da = db = 6; m = 6; }
      else if (f.type == F_PLANE_OBS) { ia = d.obs_pose[f.slot]; ib = d.obs_plane[f.slot]; da = 6; db = 3; m = 3; repop = f.slot >= d.n_obs_fixed; }
      else { ia = d.lp_plane[f.slot]; da = 3; m = 3; }
      ok = ia >= 0 && ia < (da == 6 ? d.n_pose : d.n_plane) && (db == 0 || (ib >= 0 && ib < (db == 6 ? d.n_pose : d.n_plane))) &&
           (!repop || d.obs_ray != nullptr) && fgate_block_ok(f, 0, da, da, a.n_S) &&
           (db == 0 || (fgate_block_ok(f, 1, db, db, a.n_S) && fgate_block_ok(f, 2, da, db, a.n_S)));
    }
    if (lane == 0) a.status[e] = ok ? 0 : 1;
    valid = ok;
  }
  const int c = da + db;
  const bool analytic = a.mode == 1 && !repop;
  // ---- 1. whitened residual and Jacobian at the estimate ----
  if (valid && analytic) {
    if (lane == 0) {                                                     // K1's record [J_a | J_b | r] into the evaluation area
      if (f.type == F_PLANE_OBS) {
        double pz[7], pl[4], ms[4], sw[6];
        load_pose(d.pose_est, d.pose_ld, ia, pz); load_plane(d.plane_est, d.plane_ld, ib, pl);
        load_soa<4>(d.obs_meas, d.obs_ld, f.slot, ms); load_soa<6>(d.obs_w, d.obs_ld, f.slot, sw);
        lin_plane_obs<1>(pz, pl, ms, sw, yb);
      } else if (f.type == F_ODOMETRY) {
        double p1[7], p2[7], ms[6], sw[21];
        load_pose(d.pose_est, d.pose_ld, ia, p1); load_pose(d.pose_est, d.pose_ld, ib, p2);
        load_soa<6>(d.odo_meas, d.odo_ld, f.slot, ms); load_soa<21>(d.odo_w, d.odo_ld, f.slot, sw);
        lin_odometry<1>(p1, p2, ms, sw, yb);
      } else if (f.type == F_POSE_PRIOR) {
        double pz[7], ms[6], sw[21];
        load_pose(d.pose_est, d.pose_ld, ia, pz);
        load_soa<6>(d.pp_meas, d.pp_ld, f.slot, ms); load_soa<21>(d.pp_w, d.pp_ld, f.slot, sw);
        lin_pose_prior<1>(pz, ms, sw, yb);
      } else {
        double pl[4], ms[4], sw[6];
        load_plane(d.plane_est, d.plane_ld, ia, pl);
        load_soa<4>(d.lp_meas, d.lp_ld, f.slot, ms); load_soa<6>(d.lp_w, d.lp_ld, f.slot, sw);
        lin_plane_prior<1>(pl, ms, sw, yb);
      }
    }
  } else if (valid && lane < 2 * c + 1) {
    // one evaluation per lane, in the lane numbering of body_linearize_lanes: a plane observation has the nominal residual in lane 0 and
    // column q at x (+) / (-) eps e_q in lanes 2q + 1 / 2q + 2; the other types have column q in lanes 2q / 2q + 1 and the nominal residual
    // in lane 2c (a column index out of range is the zero step)
    double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (f.type == F_PLANE_OBS) {
      const int q3 = lane > 0 ? (lane - 1) >> 1 : 9;
      const double s3 = (lane & 1) ? 1.0 : -1.0;
      double pz[7], pl[4], sw[6];
      load_pose(d.pose_est, d.pose_ld, ia, pz); load_plane(d.plane_est, d.plane_ld, ib, pl);
      load_soa<6>(d.obs_w, d.obs_ld, f.slot, sw);
      if (!repop) {
        // eval_plane_obs (pps_gate_dev.h), statement for statement, written out HERE: this arm ends in the same whiten as the contracted
        // arm below, and the compiler merges part of the two tails.  With the shared function in this place the merge came out another
        // way and the nominal residual of re-popping observations left pps_eval_factor's bits (1e-13 relative on the mixed graph of
        // tests/test_gpu_factor_gate.py, measured on the device), although the function's arithmetic is the same.
        double ms[4], pp[7], lp[4], ev[3];
        load_soa<4>(d.obs_meas, d.obs_ld, f.slot, ms);
        perturb6(pz, q3, s3, d.step_ac, pp);
        perturb3(pl, q3 - 6, s3, d.step_ac, lp);
        const bool pert_plane = q3 >= 6 && q3 < 9;
#pragma unroll
        for (int k = 0; k < 4; k++) lp[k] = pert_plane ? lp[k] : pl[k];
        res_plane_obs(pp, lp, ms, ev);
        whiten<3>(sw, ev, y);
      } else {
        // body_linearize_repop: the steps go through pose_exmap / plane_exmap, the measurement is re-popped at the stepped pose
        const int n2 = d.n_obs - d.n_obs_fixed;
        double ray[6];
        load_soa<6>(d.obs_ray, n2, f.slot - d.n_obs_fixed, ray);
        const double step = s3 * kNumDiffEps;
        if (q3 < 6) {
          double dl[6], pp[7];
#pragma unroll
          for (int k = 0; k < 6; k++) dl[k] = k == q3 ? step : 0.0;
          pose_exmap(pz, dl, pp);
          fgate_repop_eval(pp, pl, ray, sw, y);
        } else if (q3 < 9) {
          double dl[3], lp[4];
#pragma unroll
          for (int k = 0; k < 3; k++) dl[k] = k == q3 - 6 ? step : 0.0;
          plane_exmap(pl, dl, lp);
          fgate_repop_eval(pz, lp, ray, sw, y);
        } else fgate_repop_eval(pz, pl, ray, sw, y);
      }
    } else {
      const int q = lane >> 1;
      const double sgn = (lane & 1) ? -1.0 : 1.0;
      if (f.type == F_ODOMETRY) {
        double p1[7], p2[7], ms[6], sw[21];
        load_pose(d.pose_est, d.pose_ld, ia, p1); load_pose(d.pose_est, d.pose_ld, ib, p2);
        load_soa<6>(d.odo_meas, d.odo_ld, f.slot, ms); load_soa<21>(d.odo_w, d.odo_ld, f.slot, sw);
        eval_odometry(p1, p2, ms, sw, q, sgn, d.step_ac, y);
      } else if (f.type == F_POSE_PRIOR) {
        double pz[7], ms[6], sw[21];
        load_pose(d.pose_est, d.pose_ld, ia, pz);
        load_soa<6>(d.pp_meas, d.pp_ld, f.slot, ms); load_soa<21>(d.pp_w, d.pp_ld, f.slot, sw);
        eval_pose_prior(pz, ms, sw, q, sgn, d.step_ac, y);
      } else {
        double pl[4], ms[4], sw[6];
        load_plane(d.plane_est, d.plane_ld, ia, pl);
        load_soa<4>(d.lp_meas, d.lp_ld, f.slot, ms); load_soa<6>(d.lp_w, d.lp_ld, f.slot, sw);
        eval_plane_prior(pl, ms, sw, q, sgn, d.step_ac, y);
      }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) yb[lane * kFgateEvalStride + r] = y[r];
  }
  __syncthreads();
  // ---- 2. the record [J m x c | r m], columns of a then of b ----
  double jr[2] = {0.0, 0.0};                                             // entries lane and lane + 64 of the record
  if (valid) {
    const int n_rec = m * c + m;
    const bool obs = f.type == F_PLANE_OBS;
    const double inv2e = 1.0 / (kNumDiffEps + kNumDiffEps);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = lane + 64 * h;
      if (k >= n_rec) continue;
      const bool res = k >= m * c;
      const int i = res ? k - m * c : k / c, j = res ? 0 : k - i * c;
      if (analytic) jr[h] = res ? yb[m * c + i] : (j < da ? yb[i * da + j] : yb[m * da + i * db + (j - da)]);
      else if (res) jr[h] = yb[(obs ? 0 : 2 * c) * kFgateEvalStride + i];
      else {
        const int plus = (obs ? 1 : 0) + 2 * j;
        jr[h] = (yb[plus * kFgateEvalStride + i] - yb[(plus + 1) * kFgateEvalStride + i]) * inv2e;
      }
    }
  }
  __syncthreads();                                                       // (the evaluations have been read: Sigma may arrive)
  if (valid) {
    const int n_rec = m * c + m;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = lane + 64 * h;
      if (k >= n_rec) continue;
      J[k] = jr[h];
      if (a.rec) a.rec[(size_t)e * kFgateRecord + k] = jr[h];            // (what pps_debug_factor_gate_records reads)
    }
    // ---- 3. Sigma_ff ----
    for (int k = lane; k < c * c; k += 64) {
      const int i = k / c, j = k - i * c;
      double v;
      if (i < da && j < da) v = a.S[f.src[0] + (long long)i * f.ld[0] + j];
      else if (i >= da && j >= da) v = a.S[f.src[1] + (long long)(i - da) * f.ld[1] + (j - da)];
      else {
        const int ra = i < da ? i : j, cb = (i < da ? j : i) - da;      // entry (ra, cb) of Sigma_ab
        v = f.tr ? a.S[f.src[2] + (long long)cb * f.ld[2] + ra] : a.S[f.src[2] + (long long)ra * f.ld[2] + cb];
      }
      Sg[k] = v;
    }
  }
  __syncthreads();
  // ---- 4. T = J Sigma_ff, P = T J' ----
  if (valid)
    for (int k = lane; k < m * c; k += 64) {
      const int i = k / c, j = k - i * c;
      double t = 0.0;
      for (int q = 0; q < c; q++) t += J[i * c + q] * Sg[q * c + j];
      T[k] = t;
    }
  __syncthreads();
  double* Pm = Sg;                                         // (every lane is done with Sigma)
  if (valid && lane < m * m) {
    const int i = lane / m, j = lane - i * m;
    double t = 0.0;
    for (int q = 0; q < c; q++) t += T[i * c + q] * J[j * c + q];
    Pm[lane] = t;
  }
  __syncthreads();
  // ---- 5. lev, I - P on and below the diagonal, d2 = r' (I - P)^-1 r ----
  if (valid && lane == 0) {
    double lev = 0.0, d2;
    for (int i = 0; i < m; i++) lev += Pm[i * m + i];
    for (int i = 0; i < m; i++)
      for (int j = 0; j <= i; j++) Pm[i * m + j] = (i == j ? 1.0 : 0.0) - Pm[i * m + j];
    if (m == 3) chol_d2<3>(Pm, J + m * c, kFgatePivotMin, d2);           // (d2 = NaN at a pivot that fails)
    else chol_d2<6>(Pm, J + m * c, kFgatePivotMin, d2);
    a.d2[e] = d2;
    a.lev[e] = lev;
  }
}

}  // namespace

hipError_t launch_factor_gate(const DevGraph& d, const FgateArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  PPS_LAUNCH(k_factor_gate, dim3((a.n + kFgateWaves - 1) / kFgateWaves), dim3(kFgateThreads), kFgateWaves * kFgateLdsWave * sizeof(double), st, d, a);
  return hipGetLastError();
}

}  // namespace pps
