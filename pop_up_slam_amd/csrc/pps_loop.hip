// pps_loop.hip -- the Mahalanobis gate for loop-closure pose candidates (pps_loop_gate): d2 = r' (I + Jw Sigma Jw')^-1 r of every listed
// candidate odometry factor between two existing poses, from the strips k_cov_path (pps_cov.hip) has just written for the distinct poses of
// the list.  pps_loop.h has the algebra.
//
// One wave per candidate, kLoopWaves candidates per workgroup, ONE launch; a candidate reads its own record, the two pose states and the two
// strips, and writes its own d2, flag, S and record: no candidate waits for another and nothing is accumulated across candidates, so an
// answer does not depend on what else is in the list.  Steps 1, 2, 3 and 4 are the shared device functions of pps_gate_dev.h, which state
// their operation orders:
//   1. r and Jw at the estimate by the device functions K1 runs for an odometry factor.  Numeric mode: the 25 evaluations of the lane form
//      side by side on lanes 0 .. 24 (eval_odometry: column q at x (+) / (-) eps e_q in lanes 2q / 2q + 1, the nominal residual in lane 24),
//      the column differences through LDS.  Analytic mode: the closed form of pps_lin.h in one lane.  This file is compiled without
//      contraction like pps_gate.hip, pps_merge.hip and pps_fgate.hip: in numeric mode the bits are pps_eval_factor's.  The record is
//      [Jw 6 x 12 row-major | r 6], columns of a then of b: the slot of pps_debug_factor_gate_records for an odometry factor.
//   2. common_root_pivots: the pivots the two root paths have in common, from the parent table and the per-front root lengths.
//   3. strip_gram<6, 6, 6>: lanes over the strip rows, counted from the strips' END; Jw is read from LDS (the same address in every lane),
//      the accumulators are the 21 entries of the lower triangle.
//   4. lane_order_sum per entry (21 lanes, one entry each), then 1 on the diagonal and chol_d2<6> with pivot floor 0 in one lane.  A pivot
//      that is not positive or not finite gives d2 = NaN and flag 2 for that candidate alone: no status is raised.
//   5. d2, the flag byte, S (the lower triangle mirrored by 36 lanes) and the record.  The host reads the accepted list off the flag bytes
//      in order: no atomic orders anything in the output.
// LDS per wave: the record 80 | the partial sums [entry][lane], entries 65 doubles apart (the 21 lanes of step 4 then read 21 banks), 1 365 |
// the entries of S 21 doubles (11 728 bytes); the evaluations of step 1 use the partial sums' area before the sums arrive.
// Plain fp64 multiply-add loops: 6 x 12 against a few hundred strip rows is no MFMA shape.
#include <hip/hip_runtime.h>

#include "pps_loop.h"
#include "pps_gate_dev.h"

namespace pps {

namespace {

constexpr int kLoopThreads = 64 * kLoopWaves;
constexpr int kLoopEntries = 21;                 // the lower triangle of a 6 x 6 matrix, row-major
constexpr int kLoopRedStride = 65;
// dynamic LDS per wave, in doubles
constexpr int kLoopLdsJ = 0, kLoopLdsRed = kLoopLdsJ + 80, kLoopLdsS = kLoopLdsRed + kLoopEntries * kLoopRedStride, kLoopLdsWave = kLoopLdsS + kLoopEntries;
constexpr int kLoopEvalStride = 6;               // doubles per evaluation, 25 evaluations
static_assert(25 * kLoopEvalStride <= kLoopEntries * kLoopRedStride && kLoopRecord <= kLoopEntries * kLoopRedStride, "the evaluations use the partial sums' area");
static_assert((kLoopLdsWave * sizeof(double)) % 16 == 0, "every wave's area starts at a multiple of 16 bytes");

// entry (i, j) of the lower triangle, row-major
__device__ __forceinline__ int loop_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

__global__ __launch_bounds__(kLoopThreads) void k_loop_gate(DevGraph d, LoopArgs a) {
  extern __shared__ __attribute__((aligned(16))) double loop_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long long c = (long long)blockIdx.x * kLoopWaves + w;
  double* J = loop_lds + w * kLoopLdsWave + kLoopLdsJ;                   // (the areas are re-used under other names: no __restrict__)
  double* red = loop_lds + w * kLoopLdsWave + kLoopLdsRed;               // [entry][lane], entries kLoopRedStride apart
  double* Sw = loop_lds + w * kLoopLdsWave + kLoopLdsS;
  double* yb = red;                                                      // step 1 only
  // (every test below is the same in all lanes of a wave; a wave without a candidate still takes part in the barriers)
  bool valid = c < a.n;
  int common = 0, len_a = 0, len_b = 0;
  const LoopCand* cd = a.cands;
  if (valid) {
    cd = a.cands + c;
    const int fa = cd->front_a, fb = cd->front_b;
    bool ok = cd->slot_a >= 0 && cd->slot_a < d.n_pose && cd->slot_b >= 0 && cd->slot_b < d.n_pose && fa >= 0 && fa < a.n_fronts && fb >= 0 &&
              fb < a.n_fronts && a.K >= 1;
    if (ok) {
      len_a = a.rootlen[fa]; len_b = a.rootlen[fb];
      ok = len_a >= 6 && len_a <= a.K && len_b >= 6 && len_b <= a.K && cd->strip_a >= 0 && cd->strip_a + (long long)a.K * 6 <= a.n_strip &&
           cd->strip_b >= 0 && cd->strip_b + (long long)a.K * 6 <= a.n_strip;
    }
    // ---- 2. pivots of the common ancestors ----
    if (ok) ok = common_root_pivots(a.parent, a.rootlen, a.n_fronts, fa, fb, common) && common >= 0 && common <= (len_a < len_b ? len_a : len_b);
    if (!ok) { if (lane == 0) raise_status(a.status, kStatusInternal); valid = false; }
  }
  // ---- 1. whitened residual and Jacobian at the estimate ----
  const bool analytic = a.mode == 1;
  if (valid && (analytic ? lane == 0 : lane < 25)) {
    double p1[7], p2[7], ms[6], sw[21];
    load_pose(d.pose_est, d.pose_ld, cd->slot_a, p1); load_pose(d.pose_est, d.pose_ld, cd->slot_b, p2);
#pragma unroll
    for (int k = 0; k < 6; k++) ms[k] = cd->meas[k];
#pragma unroll
    for (int k = 0; k < 21; k++) sw[k] = cd->sw[k];
    if (analytic) lin_odometry<1>(p1, p2, ms, sw, yb);                   // K1's record [J_a 6 x 6 | J_b 6 x 6 | r]
    else {
      double y[6];
      eval_odometry(p1, p2, ms, sw, lane >> 1, (lane & 1) ? -1.0 : 1.0, d.step_ac, y);      // (lane 24: column 12, the zero step of both poses)
#pragma unroll
      for (int r = 0; r < 6; r++) yb[lane * kLoopEvalStride + r] = y[r];
    }
  }
  __syncthreads();
  if (valid) {
    const double inv2e = 1.0 / (kNumDiffEps + kNumDiffEps);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = lane + 64 * h;
      if (k >= kLoopRecord) continue;
      const bool res = k >= 72;
      const int i = res ? k - 72 : k / 12, j = res ? 0 : k - i * 12;
      double v;
      if (analytic) v = res ? yb[72 + i] : (j < 6 ? yb[i * 6 + j] : yb[36 + i * 6 + (j - 6)]);
      else if (res) v = yb[24 * kLoopEvalStride + i];
      else v = (yb[2 * j * kLoopEvalStride + i] - yb[(2 * j + 1) * kLoopEvalStride + i]) * inv2e;
      J[k] = v;
      if (a.rec) a.rec[(size_t)c * kLoopRecord + k] = v;                 // (what pps_debug_loop_gate_records reads)
    }
  }
  __syncthreads();                                                       // (the evaluations have been read: the partial sums may arrive)
  // ---- 3. the 21 distinct entries of Jw Sigma Jw', lanes over strip rows ----
  double s[kLoopEntries];
#pragma unroll
  for (int e = 0; e < kLoopEntries; e++) s[e] = 0.0;
  if (valid) strip_gram<6, 6, 6>(J, 12, J + 6, 12, a.Y + cd->strip_a, a.Y + cd->strip_b, len_a, len_b, common, a.K, lane, s);
#pragma unroll
  for (int e = 0; e < kLoopEntries; e++) red[e * kLoopRedStride + lane] = s[e];
  __syncthreads();
  // ---- 4. one fixed order of additions per entry, then the 6 x 6 Cholesky solve ----
  if (lane < kLoopEntries) Sw[lane] = lane_order_sum(red + lane * kLoopRedStride);
  __syncthreads();
  // ---- 5. d2, the flag, S ----
  if (valid && lane == 0) {
    double S[36], d2;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) S[i * 6 + j] = j > i ? 0.0 : (i == j ? Sw[loop_tri(i, j)] + 1.0 : Sw[loop_tri(i, j)]);
    const bool pd = chol_d2<6>(S, J + 72, 0.0, d2);
    a.d2[c] = d2;
    a.flag[c] = !pd ? (unsigned char)2 : (is_finite(d2) && d2 < a.threshold) ? (unsigned char)1 : (unsigned char)0;
  }
  if (valid && a.S && lane < 36) {
    const int i = lane / 6, j = lane - i * 6;
    a.S[(size_t)c * 36 + lane] = i == j ? Sw[loop_tri(i, j)] + 1.0 : Sw[loop_tri(i, j)];
  }
}

}  // namespace

hipError_t launch_loop_gate(const DevGraph& d, const LoopArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  PPS_LAUNCH(k_loop_gate, dim3((unsigned int)((a.n + kLoopWaves - 1) / kLoopWaves)), dim3(kLoopThreads), kLoopWaves * kLoopLdsWave * sizeof(double), st, d, a);
  return hipGetLastError();
}

}  // namespace pps
