// pps_cov_wide.hip -- what pps_cov_factor adds to pps_cov.hip: the covariance queries on graphs whose fronts fit neither one wave nor LDS
// (the dense-front form of pps_dense.hip: p <= 64 pivots, up to 15 000 rows).
//
//   k_cov_pivots      the not-positive-definite criterion of k_cov_level on its own, for a factorisation that is not followed by the
//                     level pass: one workgroup per front, all fronts in one launch, the diagonal of L_A alone.
//   k_cov_path_wide   k_cov_path (pps_cov.hip) with the right-hand sides in global memory.  One workgroup of 256 threads per walk.  L_A
//                     of the current front (64 x 65 doubles) and y_A (64 x 6) sit in LDS, 36 KB; the two vectors z of (p + b) x dim
//                     doubles -- current front, parent -- ping-pong in a scratch buffer of the handle: at 15 000 rows they are 1.4 MB,
//                     nine times the LDS of a CU, and they are touched once per front (read, updated, scattered through cmap), which
//                     the L2 serves.  The panel rows of L_B are read once each, every thread streaming its own contiguous row.
// Arithmetic: that of cov_walk, operation for operation -- division by the diagonal, the update order of the triangular solve, the
// ascending sum over the pivots from the first non-zero one -- so that on a graph both kernels accept the strips are the same bits.
// Synchronisation: workgroup barriers only (z is written and read by the threads of ONE workgroup, with a barrier in between); walks
// share nothing but the factor they read.  Compiled without contraction, like pps_cov.hip.
#include <hip/hip_runtime.h>

#include "pps_cov.h"
#include "pps_status.h"

namespace pps {

namespace {

constexpr int kWideThreads = 256;
constexpr int kWideMaxP = 64;                    // pivots per front (the tables are checked against it before anything is launched)
constexpr int kWideLdA = kWideMaxP | 1;
constexpr int kPivotThreads = 64;
// (the status word raised to kStatusInternal: an index outside its front -- never with a consistent analysis)

__global__ __launch_bounds__(kPivotThreads) void k_cov_pivots(DevGraph d, int n_fronts) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s >= n_fronts || s >= d.n_fronts) return;
  const int p = d.f_p[s];
  if (p < 1 || p > kPivotThreads) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const double* __restrict__ Lp = d.L + d.f_Loff[s];
  if (tid < p) cov_lds[tid] = Lp[(size_t)tid * p + tid];
  __syncthreads();
  if (tid == 0) {                                // (the loop of k_cov_level, on the same values)
    double mn = cov_lds[0], mx = cov_lds[0];
    bool bad = false;
    for (int k = 0; k < p; k++) {
      const double v = cov_lds[k];
      if (!finite_pos(v)) bad = true;
      mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
    if (bad || !(mn >= kCovPivotRatio * mx)) raise_status(&d.result_dev[2], 1.0);
  }
}

template <int D>
__device__ void cov_walk_wide(const DevGraph& d, const CovWalk w, const CovStep* __restrict__ steps, int K, int max_front, double* __restrict__ Ys,
                              double* zc, double* zn, double* status, double* lds) {
  const int tid = threadIdx.x;
  double* LA = lds;                              // 64 x 65   L_A (lower triangle)
  double* ysh = LA + kWideMaxP * kWideLdA;       // 64 x D    y_A of the current front
  int m0 = w.local;                              // first pivot with a non-zero solution: the node's own in its front, 0 further up
  for (int t = 0; t < w.n_steps; t++) {
    const CovStep st = steps[w.step0 + t];
    const int s = st.front;
    const bool last = t + 1 == w.n_steps;
    const int q = last ? -1 : steps[w.step0 + t + 1].front;
    // (every test below is the same in all threads: the workgroup leaves together, before anything of this front is touched)
    if (s < 0 || s >= d.n_fronts || (!last && (q < 0 || q >= d.n_fronts))) { if (tid == 0) raise_status(status, kStatusInternal); return; }
    const int p = d.f_p[s], b = d.f_b[s];
    const int nq = last ? 0 : d.f_p[q] + d.f_b[q];
    if (p < 1 || p > kWideMaxP || b < 0 || p + b > max_front || nq < 0 || nq > max_front || st.row < 0 || st.row + p > K || (b > 0 && last) || m0 < 0 ||
        (t == 0 && m0 + D > p)) { if (tid == 0) raise_status(status, kStatusInternal); return; }
    const double* __restrict__ Lp = d.L + d.f_Loff[s];
    if (t == 0) {                                // E_node in the local rows of the node's front
      for (int idx = tid; idx < (p + b) * D; idx += kWideThreads) zc[idx] = 0.0;
      __syncthreads();
      if (tid < D) zc[(m0 + tid) * D + tid] = 1.0;
    }
    for (int idx = tid; idx < p * p; idx += kWideThreads) {
      const int i = idx / p, j = idx - i * p;
      if (j <= i) LA[i * kWideLdA + j] = Lp[idx];
    }
    for (int idx = tid; idx < nq * D; idx += kWideThreads) zn[idx] = 0.0;
    __syncthreads();
    double z[D];
    for (int a = 0; a < D; a++) z[a] = tid < p ? zc[tid * D + a] : 0.0;
    // ---- y_A = L_A^-1 z_A: the lanes of wave 0 own the rows, the other waves only keep the barriers ----
    for (int m = m0; m < p; m++) {
      if (tid == m) {
        const double dg = LA[m * kWideLdA + m];
        for (int a = 0; a < D; a++) ysh[m * D + a] = z[a] / dg;
      }
      __syncthreads();
      if (tid > m && tid < p) {
        const double l = LA[tid * kWideLdA + m];
        for (int a = 0; a < D; a++) z[a] -= l * ysh[m * D + a];
      }
    }
    for (int idx = tid; idx < p * D; idx += kWideThreads) Ys[(size_t)st.row * D + idx] = idx < m0 * D ? 0.0 : ysh[idx];
    // ---- z_B -= L_B y_A, into the parent's rows: one row per thread, b rows over 256 threads ----
    if (b > 0) {
      const int* __restrict__ cm = d.cmap + d.f_cmap_off[s];
      for (int r = tid; r < b; r += kWideThreads) {
        const double* __restrict__ lb = Lp + (size_t)(p + r) * p;
        double acc[D];
        for (int a = 0; a < D; a++) acc[a] = 0.0;
        for (int m = m0; m < p; m++) {
          const double l = lb[m];
          for (int a = 0; a < D; a++) acc[a] += l * ysh[m * D + a];
        }
        const int tgt = cm[r];
        if (tgt < 0 || tgt >= nq) { raise_status(status, kStatusInternal); continue; }
        for (int a = 0; a < D; a++) zn[(size_t)tgt * D + a] = zc[(size_t)(p + r) * D + a] - acc[a];
      }
    }
    __syncthreads();
    double* sw = zc; zc = zn; zn = sw;
    m0 = 0;
  }
}

__global__ __launch_bounds__(kWideThreads) void k_cov_path_wide(DevGraph d, const CovWalk* __restrict__ walks, int n_walks, const CovStep* __restrict__ steps,
                                                                int n_steps_total, int K, int max_front, double* Z, long long n_scratch,
                                                                double* __restrict__ Y, long long n_strip, double* out) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];
  if ((int)blockIdx.x >= n_walks) return;
  const CovWalk w = walks[blockIdx.x];
  const long long per_walk = (long long)2 * max_front * 6;
  if ((w.dim != 3 && w.dim != 6) || w.n_steps < 1 || w.step0 < 0 || w.step0 + w.n_steps > n_steps_total || w.strip < 0 ||
      w.strip + (long long)K * w.dim > n_strip || max_front < 1 || ((long long)blockIdx.x + 1) * per_walk > n_scratch) {
    if (threadIdx.x == 0) raise_status(&out[0], kStatusInternal);
    return;
  }
  double* zc = Z + (long long)blockIdx.x * per_walk;
  double* zn = zc + (long long)max_front * 6;
  if (w.dim == 6) cov_walk_wide<6>(d, w, steps, K, max_front, Y + w.strip, zc, zn, &out[0], cov_lds);
  else cov_walk_wide<3>(d, w, steps, K, max_front, Y + w.strip, zc, zn, &out[0], cov_lds);
}

}  // namespace

hipError_t launch_cov_pivots(const DevGraph& d, int n_fronts, hipStream_t st) {
  if (n_fronts <= 0) return hipSuccess;
  PPS_LAUNCH(k_cov_pivots, dim3(n_fronts), dim3(kPivotThreads), kPivotThreads * sizeof(double), st, d, n_fronts);
  return hipGetLastError();
}

hipError_t launch_cov_path_wide(const DevGraph& d, const CovWalk* walks, int n_walks, const CovStep* steps, int n_steps_total, int K, int max_front,
                                double* Z, long long n_scratch, double* Y, long long n_strip, double* out, hipStream_t st) {
  if (n_walks == 0) return hipSuccess;
  if (max_front < 1 || !Z || n_scratch < (long long)n_walks * (long long)cov_wide_scratch(max_front)) return hipErrorInvalidValue;
  const size_t lds = ((size_t)kWideMaxP * kWideLdA + (size_t)kWideMaxP * 6) * sizeof(double);
  PPS_LAUNCH(k_cov_path_wide, dim3(n_walks), dim3(kWideThreads), lds, st, d, walks, n_walks, steps, n_steps_total, K, max_front, Z, n_scratch, Y, n_strip, out);
  return hipGetLastError();
}

}  // namespace pps
