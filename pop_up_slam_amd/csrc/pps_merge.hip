// pps_merge.hip -- the Mahalanobis merge gate between plane landmarks (pps_merge_gate): d2 = e' S^-1 e of all n (n - 1) / 2 pairs of a list
// of plane nodes, the best partner per plane and the pairs below a threshold, from the strips k_cov_path (pps_cov.hip) has just written
// for the listed planes.  pps_merge.h has the algebra.
//
// One wave per pair, kMergeWaves pairs per workgroup, the grid over the linear pair index ((i, j) ascending, i < j).  Steps 1, 3, 4 and the
// scan of 5 are the shared device functions of pps_gate_dev.h, which state their operation orders:
//   1. lanes 0 .. 12 evaluate the plane-prior residual by the device functions K1 runs for a Plane3d_Factor (eval_plane_prior, whitened
//      with the identity): lane 0 r(a | pi_b) at the estimate, lanes 1 .. 6 the six (+) / (-) steps of a against pi_b, lanes 7 .. 12
//      the six of b against pi_a.  The column differences go through LDS.  The "measurement" of a pair is the other plane's estimate
//      normalised like Plane3d(Vector4d) (normalize4), as pps_add_plane_prior would store it.  This file is compiled without contraction
//      like pps_k1_lanes.hip and pps_gate.hip: the bits are those of pps_eval_factor's lane form.  The Jacobians are central differences
//      whatever the handle's jacobian_mode.
//   2. the pivots the two root paths have in common, from the parent table and the per-front root lengths: the front with the longer
//      path steps to its parent until the two meet (same front; one an ancestor of the other; disjoint subtrees -- or no common root).
//   3. strip_gram3<3, 3>: lanes over the strip rows, counted from the strips' END, so that a pair's sums do not depend on which other
//      planes are in the call.  Rows of common ancestors add (z_a + z_b)(z_a + z_b)', all other rows z_a z_a' + z_b z_b'.
//   4. lane_order_sum per entry, then one lane adds floor_var to the diagonal and solves: chol_d2<3> with pivot floor 0.  A pivot that
//      is not positive or not finite gives d2 = NaN and flag 2 for that pair alone: no status is raised.
//   5. the wave writes d2 twice ((i, j) and (j, i): exactly symmetric), the pair's flag byte, and takes a ticket of row i and of row j;
//      the wave that draws a row's last ticket scans the row's off-diagonal d2 (best_scan_thread over its lanes, best_scan_final in
//      lane 0; the barriers stay workgroup-wide).  The flags are indexed by the linear pair index, which IS the (i, j) order: the host
//      reads the thresholded pairs off them in order -- no atomic orders anything.
// Plain fp64 multiply-add loops: 3 + 3 columns against 3 rows of J over a few hundred strip rows is no MFMA shape.
#include <hip/hip_runtime.h>

#include "pps_merge.h"
#include "pps_gate_dev.h"

namespace pps {

namespace {

constexpr int kMergeThreads = 64 * kMergeWaves;
constexpr int kMergeEvals = 13;                  // the nominal residual + 2 x 3 steps of a + 2 x 3 steps of b
// dynamic LDS, in doubles: the 13 evaluations per wave | the records [J_a 3 x 3 | J_b 3 x 3 | e 3] | partial sums [wave][entry][lane] | S entries |
// the rows a wave has to scan (2 ints per wave)
constexpr int kMergeLdsY = 0, kMergeLdsJ = kMergeLdsY + kMergeWaves * kMergeEvals * 3, kMergeLdsRed = kMergeLdsJ + kMergeWaves * 24,
              kMergeLdsS = kMergeLdsRed + kMergeWaves * 6 * 64, kMergeLdsRow = kMergeLdsS + kMergeWaves * 8, kMergeLdsDoubles = kMergeLdsRow + kMergeWaves;

__device__ __forceinline__ long long merge_row_start(long long i, long long n) { return i * n - i * (i + 1) / 2; }

__global__ __launch_bounds__(kMergeThreads) void k_merge_gate(DevGraph d, MergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double merge_lds[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long long p = (long long)blockIdx.x * kMergeWaves + w;
  double* __restrict__ J = merge_lds + kMergeLdsJ + w * 24;
  double* __restrict__ yb = merge_lds + kMergeLdsY + w * kMergeEvals * 3;
  double* __restrict__ red = merge_lds + kMergeLdsRed + w * 6 * 64;      // [entry][lane]
  double* __restrict__ Sw = merge_lds + kMergeLdsS + w * 8;
  int* __restrict__ rows = reinterpret_cast<int*>(merge_lds + kMergeLdsRow + w);      // the rows whose last ticket this wave drew (-1: none)
  // (every test below is the same in all lanes of a wave; a wave without a pair still takes part in the barriers)
  bool valid = p < a.n_pairs;
  int pi = 0, pj = 1, common = 0, len_a = 0, len_b = 0;
  MergePlane ca = {0, 0, 0}, cb = {0, 0, 0};
  if (valid) {
    // p -> (i, j): the row from the root of i n - i (i + 1) / 2 = p, put right by integer steps
    const double nn = 2.0 * (double)a.n - 1.0;
    long long i = (long long)((nn - sqrt(nn * nn - 8.0 * (double)p)) * 0.5);
    i = i < 0 ? 0 : (i > a.n - 2 ? a.n - 2 : i);
    while (i < a.n - 2 && merge_row_start(i + 1, a.n) <= p) i++;
    while (i > 0 && merge_row_start(i, a.n) > p) i--;
    pi = (int)i; pj = (int)(p - merge_row_start(i, a.n)) + pi + 1;
    bool ok = pj > pi && pj < a.n;
    if (ok) {
      ca = a.planes[pi]; cb = a.planes[pj];
      ok = ca.slot >= 0 && ca.slot < d.n_plane && cb.slot >= 0 && cb.slot < d.n_plane && ca.front >= 0 && ca.front < a.n_fronts && cb.front >= 0 &&
           cb.front < a.n_fronts && a.K >= 1;
    }
    if (ok) {
      len_a = a.rootlen[ca.front]; len_b = a.rootlen[cb.front];
      ok = len_a >= 3 && len_a <= a.K && len_b >= 3 && len_b <= a.K && ca.strip >= 0 && ca.strip + (long long)a.K * 3 <= a.n_strip && cb.strip >= 0 &&
           cb.strip + (long long)a.K * 3 <= a.n_strip;
    }
    if (ok) {
      // ---- 2. pivots of the common ancestors: a front's root length falls strictly on the way up, so the deeper front cannot be the meeting point ----
      ok = common_root_pivots(a.parent, a.rootlen, a.n_fronts, ca.front, cb.front, common) && common >= 0 && common <= (len_a < len_b ? len_a : len_b);
    }
    if (!ok) { if (lane == 0) raise_status(a.status, kStatusInternal); valid = false; }
  }
  // ---- 1. e, J_a, J_b at the estimate ----
  if (valid && lane < kMergeEvals) {
    double pa[4], pb[4], ma[4], mb[4];
    load_plane(d.plane_est, d.plane_ld, ca.slot, pa);
    load_plane(d.plane_est, d.plane_ld, cb.slot, pb);
#pragma unroll
    for (int k = 0; k < 4; k++) { ma[k] = pa[k]; mb[k] = pb[k]; }
    normalize4(ma); normalize4(mb);                         // the measurement as pps_add_plane_prior stores it
    const bool on_a = lane < 7;
    const int t = lane == 0 ? 6 : (lane - 1) % 6;           // lane 0: the nominal residual (no step); 2q: x (+) eps e_q, 2q + 1: x (-) eps e_q
    const int q = t >> 1;
    const double sgn = (t & 1) ? -1.0 : 1.0;
    const double sw[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};    // identity, packed upper triangle
    double base[4], ms[4], y[3];
#pragma unroll
    for (int k = 0; k < 4; k++) { base[k] = on_a ? pa[k] : pb[k]; ms[k] = on_a ? mb[k] : ma[k]; }
    eval_plane_prior(base, ms, sw, q, sgn, d.step_ac, y);
#pragma unroll
    for (int r = 0; r < 3; r++) yb[lane * 3 + r] = y[r];
  }
  __syncthreads();
  if (valid && lane < 7) {
    const double inv2e = 1.0 / (kNumDiffEps + kNumDiffEps);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (lane < 6) {
        const double v = (yb[(2 * lane + 1) * 3 + r] - yb[(2 * lane + 2) * 3 + r]) * inv2e;
        if (lane < 3) J[r * 3 + lane] = v;
        else J[9 + r * 3 + (lane - 3)] = -v;                // J_b = -J(b | pi_a)
      } else J[18 + r] = yb[r];
    }
  }
  __syncthreads();
  if (valid && a.rec && lane < kMergeRecord) a.rec[(size_t)p * kMergeRecord + lane] = J[lane];      // (what pps_debug_merge_gate_records reads)
  // ---- 3. the six distinct entries of S - floor_var I, lanes over strip rows ----
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                        // (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
  if (valid) {
    double Ja[9], Jb[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { Ja[k] = J[k]; Jb[k] = J[9 + k]; }
    strip_gram3<3, 3>(Ja, Jb, a.Y + ca.strip, a.Y + cb.strip, len_a, len_b, common, a.K, lane, s);
  }
#pragma unroll
  for (int e = 0; e < 6; e++) red[e * 64 + lane] = s[e];
  __syncthreads();
  // ---- 4. one fixed order of additions per entry, then the 3 x 3 Cholesky solve ----
  if (lane < 6) Sw[lane] = lane_order_sum(red + lane * 64);
  __syncthreads();
  if (lane == 0) {
    rows[0] = rows[1] = -1;
    if (valid) {
      const double S[9] = {Sw[0] + a.floor_var, 0.0, 0.0, Sw[1], Sw[2] + a.floor_var, 0.0, Sw[3], Sw[4], Sw[5] + a.floor_var};
      double d2;
      const bool pd = chol_d2<3>(S, J + 18, 0.0, d2);
      // ---- 5. publish, take the two tickets: the wave that draws a row's last one picks the row's best partner ----
      __hip_atomic_store(&a.d2[(size_t)pi * a.n + pj], d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&a.d2[(size_t)pj * a.n + pi], d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.flag[p] = !pd ? (unsigned char)2 : (is_finite(d2) && d2 < a.threshold) ? (unsigned char)1 : (unsigned char)0;
      __threadfence();
      if (atomicAdd(&a.ticket[pi], 1u) == (unsigned int)(a.n - 2)) rows[0] = pi;
      if (atomicAdd(&a.ticket[pj], 1u) == (unsigned int)(a.n - 2)) rows[1] = pj;
      if (rows[0] >= 0 || rows[1] >= 0) __threadfence();
    }
  }
  __syncthreads();
  // the best partner of a row: its off-diagonal d2 per lane, the 64 candidates in lane order by one lane.  (every wave passes the
  // barriers; few have a row)
  for (int h = 0; h < 2; h++) {
    const int r = rows[h];
    int bi = -1;
    double bv = 0.0;
    if (r >= 0) best_scan_thread(a.d2 + (size_t)r * a.n, a.n, r, lane, 64, bi, bv);
    int* __restrict__ ri = reinterpret_cast<int*>(red + 64);
    red[lane] = bv; ri[lane] = bi;
    __syncthreads();
    if (r >= 0 && lane == 0) {
      bi = best_scan_final(red, ri, 64, bi, bv);
      a.best[r] = bi;
      a.d2[(size_t)r * a.n + r] = 0.0;
      a.ticket[r] = 0u;
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_merge_gate(const DevGraph& d, const MergeArgs& a, hipStream_t st) {
  if (a.n < 2 || a.n_pairs <= 0) return hipSuccess;
  const long long blocks = (a.n_pairs + kMergeWaves - 1) / kMergeWaves;
  if (blocks > 2147483647LL) return hipErrorInvalidValue;
  PPS_LAUNCH(k_merge_gate, dim3((unsigned int)blocks), dim3(kMergeThreads), kMergeLdsDoubles * sizeof(double), st, d, a);
  return hipGetLastError();
}

}  // namespace pps
