// pps_gate.hip -- the Mahalanobis gate of plane association (pps_assoc_gate): all n_meas x n_planes squared distances
// d2 = r' (I + Jw Sigma Jw')^-1 r of one pose's measurements against candidate landmarks, and the best candidate per measurement, from the
// strips k_cov_path (pps_cov.hip) has just written for the pose and the candidates.  pps_gate.h has the algebra.
//
// One wave per candidate, kGateWaves candidates of one measurement per workgroup:
// The steps are the shared device functions of pps_gate_dev.h, which state their operation orders:
//   1. r and Jw by the device functions K1 runs for a plane observation -- numeric mode: the 19 evaluations of the lane form, one
//      eval_plane_obs per lane, the column differences through LDS; analytic mode: lin_plane_obs<1> (pps_lin.h) in one lane.  This file is
//      compiled without contraction like pps_k1_lanes.hip, so in numeric mode the bits are those of pps_eval_factor's lane form.
//   2. strip_gram3<6, 3>: lanes over the strip rows, counted from the strips' END, so that a candidate's sums do not depend on which
//      other candidates are in the call.  Each row gives z_x = Jp y_x, z_l = Jl y_l and its contribution to the six distinct entries of S.
//   3. lane_order_sum per entry, then one lane adds the identity and solves: chol_d2<3> with pivot floor 0.
//   4. the workgroup that draws a measurement's last ticket scans the measurement's row of d2: best_scan_thread over the whole
//      workgroup, best_scan_final in thread 0.
// Plain fp64 multiply-add loops: a candidate is 9 + 3 columns against 3 rows of Jw over a few hundred strip rows (DESIGN.md section 5b
// on why such shapes stay off the MFMA unit); the call's time is its two launches and the strips' latency.
#include <hip/hip_runtime.h>

#include "pps_gate.h"
#include "pps_gate_dev.h"

namespace pps {

namespace {

constexpr int kGateThreads = 64 * kGateWaves;
// dynamic LDS, in doubles: Jacobian records | the 19 whitened evaluations per wave | partial sums [wave][entry][lane] | S entries | d2 | flag
constexpr int kGateLdsJ = 0, kGateLdsY = kGateLdsJ + kGateWaves * 30, kGateLdsRed = kGateLdsY + kGateWaves * 3 * kObsLanes,
              kGateLdsS = kGateLdsRed + kGateWaves * 6 * 64, kGateLdsD = kGateLdsS + kGateWaves * 8, kGateLdsFlag = kGateLdsD + kGateWaves,
              kGateLdsDoubles = kGateLdsFlag + 2;
static_assert(kGateWaves * 6 * 64 >= kGateThreads + kGateThreads / 2 + 1, "the best-candidate scan re-uses the partial-sum area");

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
    if (!ok) { if (lane == 0) raise_status(&a.out[0], kStatusInternal); valid = false; }
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
      double y[3];
      eval_plane_obs(pz, pl, ms, sw, lane > 0 ? (lane - 1) >> 1 : 9, (lane & 1) ? 1.0 : -1.0, d.step_ac, y);
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
    strip_gram3<6, 3>(Jp, Jl, a.Y + a.strip_x, a.Y + c.strip, a.rootlen_x, c.rootlen, c.common, a.K, lane, s);
  }
#pragma unroll
  for (int e = 0; e < 6; e++) red[(w * 6 + e) * 64 + lane] = s[e];
  __syncthreads();
  // ---- 3. one fixed order of additions per entry, then the 3 x 3 Cholesky solve ----
  if (lane < 6) gate_lds[kGateLdsS + w * 8 + lane] = lane_order_sum(red + (w * 6 + lane) * 64);
  __syncthreads();
  if (lane == 0) {
    double d2 = __builtin_nan("");
    if (valid) {
      const double* __restrict__ t = gate_lds + kGateLdsS + w * 8;
      const double S[9] = {1.0 + t[0], 0.0, 0.0, t[1], 1.0 + t[2], 0.0, t[3], t[4], 1.0 + t[5]};
      if (!chol_d2<3>(S, J + 27, 0.0, d2)) raise_status(&a.out[0], 1.0);
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
  // the best candidate of the measurement's row of d2: per thread, then the per-thread candidates in thread order
  int bi;
  double bv;
  best_scan_thread(d2_out + (size_t)m * a.n_planes, a.n_planes, -1, tid, kGateThreads, bi, bv);
  int* __restrict__ ri = reinterpret_cast<int*>(red + kGateThreads);
  red[tid] = bv; ri[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    bi = best_scan_final(red, ri, kGateThreads, bi, bv);
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
