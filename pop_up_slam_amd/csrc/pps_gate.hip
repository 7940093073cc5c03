// pps_gate.hip -- the Mahalanobis gate of plane association (pps_assoc_gate): all n_meas x n_planes squared distances
// d2 = r' (I + Jw Sigma Jw')^-1 r of one pose's measurements against candidate landmarks, and the best candidate per measurement, from the
// strips k_cov_path (pps_cov.hip) has just written for the pose and the candidates.  pps_gate.h has the algebra.
//
// One wave per candidate, kGateWaves candidates of one measurement per workgroup:
//   1. r and Jw by the device functions K1 runs for a plane observation -- numeric mode: the 19 evaluations of the lane form
//      (body_linearize_lanes, pps_k1_body.h: perturb6 / perturb3 with the device's step quaternions, res_plane_obs, whiten), one per lane,
//      the column differences through LDS; analytic mode: lin_plane_obs<1> (pps_lin.h) in one lane.  This file is compiled without
//      contraction like pps_k1_lanes.hip, so in numeric mode the bits are those of pps_eval_factor's lane form.
//   2. lanes over the strip rows, counted from the strips' END (row K - 1 - j in lane j % 64, j ascending): the products of a lane and
//      the order they are added in depend on the candidate alone, not on K -- not on which other candidates are in the call.  Each row
//      gives z_x = Jp y_x, z_l = Jl y_l (3 each) and its contribution to the six distinct entries of S.
//   3. the 64 partial sums of an entry are added in lane order by one lane, then one lane factors the 3 x 3 S and solves.
//   4. the workgroup that draws a measurement's last ticket scans the measurement's row of d2 for the smallest finite value.
// Plain fp64 multiply-add loops: a candidate is 9 + 3 columns against 3 rows of Jw over a few hundred strip rows (DESIGN.md section 5b
// on why such shapes stay off the MFMA unit); the call's time is its two launches and the strips' latency.
#include <hip/hip_runtime.h>

#include "pps_gate.h"
#include "pps_k1_body.h"

namespace pps {

namespace {

constexpr int kGateThreads = 64 * kGateWaves;
constexpr double kGateStatusInternal = 64.0;     // = kStatusInternal
constexpr double kGateDblMax = 1.79769313486231570e308;
// dynamic LDS, in doubles: Jacobian records | the 19 whitened evaluations per wave | partial sums [wave][entry][lane] | S entries | d2 | flag
constexpr int kGateLdsJ = 0, kGateLdsY = kGateLdsJ + kGateWaves * 30, kGateLdsRed = kGateLdsY + kGateWaves * 3 * kObsLanes,
              kGateLdsS = kGateLdsRed + kGateWaves * 6 * 64, kGateLdsD = kGateLdsS + kGateWaves * 8, kGateLdsFlag = kGateLdsD + kGateWaves,
              kGateLdsDoubles = kGateLdsFlag + 2;
static_assert(kGateWaves * 6 * 64 >= kGateThreads + kGateThreads / 2 + 1, "the best-candidate scan re-uses the partial-sum area");

__device__ __forceinline__ void gate_raise(double* w, double v) {      // the status word is raised, never overwritten (pps_cov.hip)
  atomicMax(reinterpret_cast<unsigned long long*>(w), (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ bool gate_pivot_ok(double p) { return p > 0.0 && p <= kGateDblMax; }      // positive and finite (false for NaN)

__global__ __launch_bounds__(kGateThreads) void k_assoc_gate(DevGraph d, GateArgs a) {
  extern __shared__ __attribute__((aligned(16))) double gate_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int m = blockIdx.y, l = blockIdx.x * kGateWaves + w;
  double* __restrict__ J = gate_lds + kGateLdsJ + w * 30;              // [Jp 3 x 6 | Jl 3 x 3 | r 3]: the record of K1
  double* __restrict__ yb = gate_lds + kGateLdsY + w * 3 * kObsLanes;
  double* __restrict__ red = gate_lds + kGateLdsRed;
  double* __restrict__ d2_out = a.out + 1;
  // (every test below is the same in all lanes of a wave; a wave without a candidate still takes part in the barriers)
  bool valid = l < a.n_planes;
  GatePlane c = {0, 0, 0, 0, 0};
  if (valid) {
    c = a.planes[l];
    const int lo = a.rootlen_x < c.rootlen ? a.rootlen_x : c.rootlen;
    const bool ok = a.pose_slot >= 0 && a.pose_slot < d.n_pose && c.slot >= 0 && c.slot < d.n_plane && a.K >= 1 && a.rootlen_x >= 6 &&
                    a.rootlen_x <= a.K && c.rootlen >= 3 && c.rootlen <= a.K && c.common >= 0 && c.common <= lo && a.strip_x >= 0 &&
                    a.strip_x + (long long)a.K * 6 <= a.n_strip && c.strip >= 0 && c.strip + (long long)a.K * 3 <= a.n_strip;
    if (!ok) { if (lane == 0) gate_raise(&a.out[0], kGateStatusInternal); valid = false; }
  }
  // ---- 1. whitened residual and Jacobian at the estimate ----
  if (valid && (a.mode == 1 ? lane == 0 : lane < kObsLanes)) {
    double pz[7], pl[4], ms[4], sw[6];
    load_pose(d.pose_est, d.pose_ld, a.pose_slot, pz);
    load_plane(d.plane_est, d.plane_ld, c.slot, pl);
#pragma unroll
    for (int k = 0; k < 4; k++) ms[k] = a.meas[(size_t)m * 10 + k];
#pragma unroll
    for (int k = 0; k < 6; k++) sw[k] = a.meas[(size_t)m * 10 + 4 + k];
    if (a.mode == 1) {
      double rec[30];
      lin_plane_obs<1>(pz, pl, ms, sw, rec);
#pragma unroll
      for (int k = 0; k < 30; k++) J[k] = rec[k];
    } else {
      // lane 0: the nominal residual; lanes 2q + 1 / 2q + 2: the residual at x (+) / (-) eps e_q, as in body_linearize_lanes
      const int q3 = lane > 0 ? (lane - 1) >> 1 : 9;
      const double s3 = (lane & 1) ? 1.0 : -1.0;
      double pp[7], lp[4], e[3], y[3];
      perturb6(pz, q3, s3, d.step_ac, pp);
      perturb3(pl, q3 - 6, s3, d.step_ac, lp);
      const bool pert_plane = q3 >= 6 && q3 < 9;
#pragma unroll
      for (int k = 0; k < 4; k++) lp[k] = pert_plane ? lp[k] : pl[k];
      res_plane_obs(pp, lp, ms, e);
      whiten<3>(sw, e, y);
#pragma unroll
      for (int r = 0; r < 3; r++) yb[lane * 3 + r] = y[r];
    }
  }
  __syncthreads();
  if (valid && a.mode != 1 && lane < 10) {
    const double inv2e = 1.0 / (kNumDiffEps + kNumDiffEps);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (lane < 9) {
        const double v = (yb[(2 * lane + 1) * 3 + r] - yb[(2 * lane + 2) * 3 + r]) * inv2e;
        if (lane < 6) J[r * 6 + lane] = v;
        else J[18 + r * 3 + (lane - 6)] = v;
      } else J[27 + r] = yb[r];
    }
  }
  __syncthreads();
  if (valid && a.rec && lane < 30) a.rec[((size_t)m * a.n_planes + l) * 30 + lane] = J[lane];      // (what pps_debug_assoc_gate_records reads)
  // ---- 2. the six distinct entries of Jw Sigma Jw', lanes over strip rows ----
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                        // (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
  if (valid) {
    double Jp[18], Jl[9];
#pragma unroll
    for (int k = 0; k < 18; k++) Jp[k] = J[k];
#pragma unroll
    for (int k = 0; k < 9; k++) Jl[k] = J[18 + k];
    const double* __restrict__ Yx = a.Y + a.strip_x;
    const double* __restrict__ Yl = a.Y + c.strip;
    const int len = a.rootlen_x > c.rootlen ? a.rootlen_x : c.rootlen;
    for (int j = lane; j < len; j += 64) {
      const size_t k = (size_t)(a.K - 1 - j);
      double zx[3] = {0.0, 0.0, 0.0}, zl[3] = {0.0, 0.0, 0.0};
      if (j < a.rootlen_x) {
        double y[6];
#pragma unroll
        for (int q = 0; q < 6; q++) y[q] = Yx[k * 6 + q];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < 6; q++) t += Jp[i * 6 + q] * y[q];
          zx[i] = t;
        }
      }
      if (j < c.rootlen) {
        double y[3];
#pragma unroll
        for (int q = 0; q < 3; q++) y[q] = Yl[k * 3 + q];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < 3; q++) t += Jl[i * 3 + q] * y[q];
          zl[i] = t;
        }
      }
      // A row of a front both paths pass through (j < common) carries all four products z_x z_x' + z_l z_l' + z_x z_l' + z_l z_x' =
      // (z_x + z_l)(z_x + z_l)': the two are added BEFORE they are multiplied.  A pose and a landmark it sees share most of their
      // uncertainty, z_x is close to -z_l on those rows and S is what is left of the difference: summed first, rounding is relative to
      // |z_x|, multiplied out it would be relative to |z_x|^2 against a result of the size |z_x + z_l|^2.  Rows of fronts the paths do
      // not share keep their two squares apart (no cross term exists there, whatever sits at the same strip index).
      const bool cross = j < c.common;
      const double z[3] = {zx[0] + zl[0], zx[1] + zl[1], zx[2] + zl[2]};
      int e = 0;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int jj = 0; jj <= i; jj++, e++) s[e] += cross ? z[i] * z[jj] : zx[i] * zx[jj] + zl[i] * zl[jj];
    }
  }
#pragma unroll
  for (int e = 0; e < 6; e++) red[(w * 6 + e) * 64 + lane] = s[e];
  __syncthreads();
  // ---- 3. one fixed order of additions per entry, then the 3 x 3 Cholesky solve ----
  if (lane < 6) {
    double t = 0.0;
    for (int k = 0; k < 64; k++) t += red[(w * 6 + lane) * 64 + k];
    gate_lds[kGateLdsS + w * 8 + lane] = t;
  }
  __syncthreads();
  if (lane == 0) {
    double d2 = __builtin_nan("");
    if (valid) {
      const double* __restrict__ t = gate_lds + kGateLdsS + w * 8;
      const double S00 = 1.0 + t[0], S10 = t[1], S11 = 1.0 + t[2], S20 = t[3], S21 = t[4], S22 = 1.0 + t[5];
      const double r0 = J[27], r1 = J[28], r2 = J[29];
      bool pd = false;
      if (gate_pivot_ok(S00)) {
        const double l00 = sqrt(S00), l10 = S10 / l00, l20 = S20 / l00;
        const double p1 = S11 - l10 * l10;
        if (gate_pivot_ok(p1)) {
          const double l11 = sqrt(p1), l21 = (S21 - l20 * l10) / l11;
          const double p2 = S22 - l20 * l20 - l21 * l21;
          if (gate_pivot_ok(p2)) {
            const double l22 = sqrt(p2);
            const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = (r2 - l20 * y0 - l21 * y1) / l22;
            d2 = y0 * y0 + y1 * y1 + y2 * y2;
            pd = true;
          }
        }
      }
      if (!pd) gate_raise(&a.out[0], 1.0);
    }
    gate_lds[kGateLdsD + w] = d2;
  }
  __syncthreads();
  // ---- 4. publish, take a ticket: the workgroup that draws the measurement's last one picks the best candidate ----
  if (tid == 0) {
    for (int ww = 0; ww < kGateWaves; ww++) {
      const int ll = blockIdx.x * kGateWaves + ww;
      if (ll < a.n_planes) d2_out[(size_t)m * a.n_planes + ll] = gate_lds[kGateLdsD + ww];
    }
    __threadfence();
    gate_lds[kGateLdsFlag] = atomicAdd(&a.ticket[m], 1u) == (unsigned int)(gridDim.x - 1) ? 1.0 : 0.0;
  }
  __syncthreads();
  if (gate_lds[kGateLdsFlag] == 0.0) return;
  __threadfence();
  // smallest finite d2, the first candidate on ties (a NaN or an infinity never becomes the best): ascending candidates per thread, strict <
  int bi = -1;
  double bv = 0.0;
  for (int k = tid; k < a.n_planes; k += kGateThreads) {
    const double v = __hip_atomic_load(&d2_out[(size_t)m * a.n_planes + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (fabs(v) <= kGateDblMax && (bi < 0 || v < bv)) { bi = k; bv = v; }
  }
  int* __restrict__ ri = reinterpret_cast<int*>(red + kGateThreads);
  red[tid] = bv; ri[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kGateThreads; k++) {
      const int ki = ri[k];
      const double kv = red[k];
      if (ki >= 0 && (bi < 0 || kv < bv || (kv == bv && ki < bi))) { bi = ki; bv = kv; }
    }
    reinterpret_cast<int*>(d2_out + (size_t)a.n_meas * a.n_planes)[m] = bi;
    a.ticket[m] = 0u;
  }
}

}  // namespace

hipError_t launch_assoc_gate(const DevGraph& d, const GateArgs& a, hipStream_t st) {
  if (a.n_meas <= 0 || a.n_planes <= 0) return hipSuccess;
  if (a.n_meas > 65535) return hipErrorInvalidValue;
  PPS_LAUNCH(k_assoc_gate, dim3((a.n_planes + kGateWaves - 1) / kGateWaves, a.n_meas), dim3(kGateThreads), kGateLdsDoubles * sizeof(double), st, d, a);
  return hipGetLastError();
}

}  // namespace pps
