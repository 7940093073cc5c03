// pps_cov.hip -- marginal covariances from the multifrontal factor (isam::Covariances, Thirdparty/isam/isamlib/covariance.cpp): the
// selected inverse of H = L L' on the elimination tree, root -> leaves.  pps_cov.h has the recursion.
//
// Deliberately the plain form -- this pass is a query after a solve, not a link of the LM chain: one launch per tree level (the launch
// boundary is the dependency: no flags, no waiting between workgroups), one workgroup of 256 threads per front, fp64 FMA loops.  The
// products are (b x b)(b x p) and smaller with b <= 126, p <= 64 in shapes that are no multiples of 16; v_mfma_f64_16x16x4_f64 would
// need padded tiles of L_A^-1, G and Sigma_BB in its operand layout for a kernel whose time is set by the level chain, not the flops.
// Compiled without contraction (-ffp-contract=off, like every file outside the solver list of the Makefile).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pps_cov.h"

namespace pps {

namespace {

constexpr int kCovThreads = 256;
constexpr double kCovPivotRatio = 1e-7;          // a pivot of L below this fraction of its front's largest: H is singular to 1e-14 of that diagonal
constexpr double kCovStatusInternal = 64.0;      // = kStatusInternal: an index outside its front (never with a consistent analysis)

__device__ __forceinline__ void cov_raise(double* w, double v) {      // the status word is raised, never overwritten (pps_regtile.h)
  atomicMax(reinterpret_cast<unsigned long long*>(w), (unsigned long long)__double_as_longlong(v));
}

// entry (r, c) of a front's full block [Sigma_AA Sigma_BA'; Sigma_BA Sigma_BB]: panel Sp (ld = p), boundary block Bs (ld = b)
__device__ __forceinline__ double cov_full(const double* __restrict__ Sp, const double* __restrict__ Bs, int p, int b, int r, int c) {
  if (r < c) { const int t = r; r = c; c = t; }
  return c < p ? Sp[(size_t)r * p + c] : Bs[(size_t)(r - p) * b + (c - p)];
}

__global__ __launch_bounds__(kCovThreads) void k_cov_level(DevGraph d, double* __restrict__ S, const int* __restrict__ parent, int level_begin) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];
  const int s = d.level_fronts[level_begin + blockIdx.x];
  const int p = d.f_p[s], b = d.f_b[s];
  const int tid = threadIdx.x;
  const double* __restrict__ Lp = d.L + d.f_Loff[s];
  double* __restrict__ Sp = S + d.f_Loff[s];
  double* __restrict__ Bs = d.U + d.f_Uoff[s];
  double* LA = cov_lds;                         // p x p   L_A (lower triangle)
  double* X = LA + p * p;                       // p x p   L_A^-1 (lower triangle, rest zero)
  double* G = X + p * p;                        // b x p   L_B L_A^-1

  // ---- Sigma_BB from the parent's full block, through cmap (its entry b is the rhs row) ----
  const int q = parent[s];
  if (b > 0) {
    if (q < 0) { if (tid == 0) cov_raise(&d.result_dev[2], kCovStatusInternal); return; }
    const int pq = d.f_p[q], bq = d.f_b[q];
    const double* __restrict__ Sq = S + d.f_Loff[q];
    const double* __restrict__ Bq = d.U + d.f_Uoff[q];
    const int* __restrict__ cm = d.cmap + d.f_cmap_off[s];
    for (int idx = tid; idx < b * b; idx += kCovThreads) {
      const int i = idx / b, j = idx - i * b;
      const int r = cm[i], c = cm[j];
      double v = 0.0;
      if (r >= 0 && c >= 0 && r < pq + bq && c < pq + bq) v = cov_full(Sq, Bq, pq, bq, r, c);
      else cov_raise(&d.result_dev[2], kCovStatusInternal);
      Bs[idx] = v;
    }
  }
  for (int idx = tid; idx < p * p; idx += kCovThreads) {
    const int i = idx / p, j = idx - i * p;
    LA[idx] = j <= i ? Lp[idx] : 0.0;
    X[idx] = 0.0;
  }
  __syncthreads();
  if (tid == 0) {                                // pivots: positive, finite, and not collapsed against the front's largest
    double mn = LA[0], mx = LA[0];
    bool bad = false;
    for (int k = 0; k < p; k++) {
      const double v = LA[k * p + k];
      if (!(v > 0.0) || !(v <= 1.79769313486231570e308)) bad = true;
      mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
    if (bad || !(mn >= kCovPivotRatio * mx)) cov_raise(&d.result_dev[2], 1.0);
  }
  // ---- X = L_A^-1: thread j solves L_A x = e_j (its own column: no hand-over between threads) ----
  if (tid < p) {
    const int j = tid;
    for (int i = j; i < p; i++) {
      double acc = i == j ? 1.0 : 0.0;
      for (int m = j; m < i; m++) acc -= LA[i * p + m] * X[m * p + j];
      X[i * p + j] = acc / LA[i * p + i];
    }
  }
  __syncthreads();
  // ---- G = L_B X (X is lower triangular: the sum starts at m = k) ----
  for (int idx = tid; idx < b * p; idx += kCovThreads) {
    const int i = idx / p, k = idx - i * p;
    const double* __restrict__ lb = Lp + (size_t)(p + i) * p;
    double acc = 0.0;
    for (int m = k; m < p; m++) acc += lb[m] * X[m * p + k];
    G[idx] = acc;
  }
  __syncthreads();                               // (also: Bs, written above by this workgroup, is visible to all of its threads)
  // ---- Sigma_BA = -Sigma_BB G ----
  for (int idx = tid; idx < b * p; idx += kCovThreads) {
    const int i = idx / p, l = idx - i * p;
    const double* __restrict__ row = Bs + (size_t)i * b;
    double acc = 0.0;
    for (int j = 0; j < b; j++) acc += row[j] * G[j * p + l];
    Sp[(size_t)(p + i) * p + l] = -acc;
  }
  __syncthreads();
  // ---- Sigma_AA = X' X - G' Sigma_BA: the lower triangle, mirrored ----
  for (int idx = tid; idx < p * p; idx += kCovThreads) {
    const int k = idx / p, l = idx - k * p;
    if (l > k) continue;
    double acc = 0.0;
    for (int m = k; m < p; m++) acc += X[m * p + k] * X[m * p + l];
    double acc2 = 0.0;
    for (int i = 0; i < b; i++) acc2 += G[i * p + k] * Sp[(size_t)(p + i) * p + l];
    const double v = acc - acc2;
    Sp[(size_t)k * p + l] = v;
    Sp[(size_t)l * p + k] = v;
  }
}

__global__ __launch_bounds__(64) void k_cov_gather(const double* __restrict__ S, const CovReq* __restrict__ req, int n, double* __restrict__ out) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const CovReq r = req[k];
  for (int t = threadIdx.x; t < r.dr * r.dc; t += 64) {
    const int i = t / r.dc, j = t - i * r.dc;
    out[r.dst + t] = r.tr ? S[r.src + (long long)j * r.ld + i] : S[r.src + (long long)i * r.ld + j];
  }
}

}  // namespace

size_t cov_level_lds_bytes(int p, int b) { return ((size_t)2 * p * p + (size_t)b * p + 2) * sizeof(double); }

hipError_t launch_cov_level(const DevGraph& d, double* S, const int* parent, int level_begin, int level_count, size_t lds_bytes, hipStream_t st) {
  if (level_count == 0) return hipSuccess;
  static thread_local int attr_device = -1;      // the LDS ceiling of the kernel is raised once per device and host thread
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (attr_device != dev) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cov_level), hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    if (e != hipSuccess) return e;
    attr_device = dev;
  }
  if (lds_bytes > (size_t)159 * 1024) return hipErrorInvalidValue;
  PPS_LAUNCH(k_cov_level, dim3(level_count), dim3(kCovThreads), lds_bytes, st, d, S, parent, level_begin);
  return hipGetLastError();
}

hipError_t launch_cov_gather(const double* S, const CovReq* req, int n, double* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  PPS_LAUNCH(k_cov_gather, dim3(n), dim3(64), 0, st, S, req, n, out);
  return hipGetLastError();
}

}  // namespace pps
