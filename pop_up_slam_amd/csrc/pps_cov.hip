// pps_cov.hip -- marginal covariances from the multifrontal factor (isam::Covariances, Thirdparty/isam/isamlib/covariance.cpp): the
// selected inverse of H = L L' on the elimination tree, root -> leaves.  pps_cov.h has the recursion.
//
// Deliberately the plain form -- this pass is a query after a solve, not a link of the LM chain: one launch per tree level (the launch
// boundary is the dependency: no flags, no waiting between workgroups), one workgroup of 256 threads per front, fp64 FMA loops.  The
// products are (b x b)(b x p) and smaller with b <= 126, p <= 64 in shapes that are no multiples of 16; v_mfma_f64_16x16x4_f64 would
// need padded tiles of L_A^-1, G and Sigma_BB in its operand layout for a kernel whose time is set by the level chain, not the flops.
// Compiled without contraction (-ffp-contract=off, like every file outside the solver list of the Makefile).
//
// Blocks outside the pattern (pps_cov_block): k_cov_path, one wave per requested node, walks the node's path to the root with a
// forward substitution per front and stores the strip L^-1 E_node; k_cov_gram multiplies two strips over their common suffix.  The
// walks of different nodes share nothing but the factor they read: no flags, no atomics on data, no waiting between workgroups.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pps_cov.h"
#include "pps_status.h"

namespace pps {

namespace {

constexpr int kCovThreads = 256;
// (the status word raised to kStatusInternal: an index outside its front or its strip -- never with a consistent analysis)

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
    if (q < 0) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
    const int pq = d.f_p[q], bq = d.f_b[q];
    const double* __restrict__ Sq = S + d.f_Loff[q];
    const double* __restrict__ Bq = d.U + d.f_Uoff[q];
    const int* __restrict__ cm = d.cmap + d.f_cmap_off[s];
    for (int idx = tid; idx < b * b; idx += kCovThreads) {
      const int i = idx / b, j = idx - i * b;
      const int r = cm[i], c = cm[j];
      double v = 0.0;
      if (r >= 0 && c >= 0 && r < pq + bq && c < pq + bq) v = cov_full(Sq, Bq, pq, bq, r, c);
      else raise_status(&d.result_dev[2], kStatusInternal);
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
      if (!finite_pos(v)) bad = true;
      mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
    if (bad || !(mn >= kCovPivotRatio * mx)) raise_status(&d.result_dev[2], 1.0);
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


// ---- pps_cov_block: the columns of L^-1 that belong to one node, along its path to the root (pps_cov.h has the strip layout) ----
// One wave per node: lane i owns row i of the triangular solve and keeps its D right-hand sides in registers; a pivot's solution
// goes to the other lanes through LDS, one barrier per pivot (p <= 64 per front, L_A staged in LDS with an odd leading dimension).
// The rows below the pivots (z_B -= L_B y_A) are spread over the lanes, each streaming its own row of the panel, and land in the
// parent's rows through cmap; the parent rows that no child row maps to start at zero.
constexpr int kPathThreads = 64;
constexpr int kGramThreads = 256;                // 4 slices of the common suffix x 64 entries of a block (36 used by a pose-pose block)

template <int D>
__device__ void cov_walk(const DevGraph& d, const CovWalk w, const CovStep* __restrict__ steps, int K, int max_p, int max_front,
                         double* __restrict__ Ys, double* status, double* lds) {
  const int tid = threadIdx.x;
  const int ldA = max_p | 1;
  double* LA = lds;                              // max_p x ldA   L_A (lower triangle)
  double* ysh = LA + max_p * ldA;                // max_p x D     y_A of the current front
  double* zc = ysh + max_p * 6;                  // (p + b) x D   right-hand sides of the current front, in its local rows
  double* zn = zc + max_front * 6;               // ... and of its parent
  int m0 = w.local;                              // first pivot with a non-zero solution: the node's own in its front, 0 further up
  for (int t = 0; t < w.n_steps; t++) {
    const CovStep st = steps[w.step0 + t];
    const int s = st.front;
    const bool last = t + 1 == w.n_steps;
    const int q = last ? -1 : steps[w.step0 + t + 1].front;
    // (every test below is the same in all lanes: the wave leaves together)
    if (s < 0 || s >= d.n_fronts || (!last && (q < 0 || q >= d.n_fronts))) { if (tid == 0) raise_status(status, kStatusInternal); return; }
    const int p = d.f_p[s], b = d.f_b[s];
    const int nq = last ? 0 : d.f_p[q] + d.f_b[q];
    if (p < 1 || p > max_p || b < 0 || p + b > max_front || nq > max_front || st.row < 0 || st.row + p > K || (b > 0 && last) || m0 < 0 ||
        (t == 0 && m0 + D > p)) { if (tid == 0) raise_status(status, kStatusInternal); return; }
    const double* __restrict__ Lp = d.L + d.f_Loff[s];
    if (t == 0) {                                // E_node in the local rows of the node's front
      for (int idx = tid; idx < (p + b) * D; idx += kPathThreads) zc[idx] = 0.0;
      __syncthreads();
      if (tid < D) zc[(m0 + tid) * D + tid] = 1.0;
    }
    for (int idx = tid; idx < p * p; idx += kPathThreads) {
      const int i = idx / p, j = idx - i * p;
      if (j <= i) LA[i * ldA + j] = Lp[idx];
    }
    for (int idx = tid; idx < nq * D; idx += kPathThreads) zn[idx] = 0.0;
    __syncthreads();
    double z[D];
    for (int a = 0; a < D; a++) z[a] = tid < p ? zc[tid * D + a] : 0.0;
    // ---- y_A = L_A^-1 z_A ----
    for (int m = m0; m < p; m++) {
      if (tid == m) {
        const double dg = LA[m * ldA + m];
        for (int a = 0; a < D; a++) ysh[m * D + a] = z[a] / dg;
      }
      __syncthreads();
      if (tid > m && tid < p) {
        const double l = LA[tid * ldA + m];
        for (int a = 0; a < D; a++) z[a] -= l * ysh[m * D + a];
      }
    }
    for (int idx = tid; idx < p * D; idx += kPathThreads) Ys[(size_t)st.row * D + idx] = idx < m0 * D ? 0.0 : ysh[idx];
    // ---- z_B -= L_B y_A, into the parent's rows ----
    if (b > 0) {
      const int* __restrict__ cm = d.cmap + d.f_cmap_off[s];
      for (int r = tid; r < b; r += kPathThreads) {
        const double* __restrict__ lb = Lp + (size_t)(p + r) * p;
        double acc[D];
        for (int a = 0; a < D; a++) acc[a] = 0.0;
        for (int m = m0; m < p; m++) {
          const double l = lb[m];
          for (int a = 0; a < D; a++) acc[a] += l * ysh[m * D + a];
        }
        const int tgt = cm[r];
        if (tgt < 0 || tgt >= nq) { raise_status(status, kStatusInternal); continue; }
        for (int a = 0; a < D; a++) zn[tgt * D + a] = zc[(p + r) * D + a] - acc[a];
      }
    }
    __syncthreads();
    double* sw = zc; zc = zn; zn = sw;
    m0 = 0;
  }
}

__global__ __launch_bounds__(kPathThreads) void k_cov_path(DevGraph d, const CovWalk* __restrict__ walks, int n_walks, const CovStep* __restrict__ steps,
                                                           int n_steps_total, int K, int max_p, int max_front, double* __restrict__ Y, long long n_strip,
                                                           double* out) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];
  if ((int)blockIdx.x >= n_walks) return;
  const CovWalk w = walks[blockIdx.x];
  if ((w.dim != 3 && w.dim != 6) || w.n_steps < 1 || w.step0 < 0 || w.step0 + w.n_steps > n_steps_total || w.strip < 0 ||
      w.strip + (long long)K * w.dim > n_strip) { if (threadIdx.x == 0) raise_status(&out[0], kStatusInternal); return; }
  if (w.dim == 6) cov_walk<6>(d, w, steps, K, max_p, max_front, Y + w.strip, &out[0], cov_lds);
  else cov_walk<3>(d, w, steps, K, max_p, max_front, Y + w.strip, &out[0], cov_lds);
}

// One workgroup per block of the result.  Entry (a, c) is summed by four threads, each over every fourth row of the common suffix, and
// their partial sums are added in one fixed order: block (i, j) and block (j, i) add the same products in the same order, so
// Sigma(rows, cols) is the transpose of Sigma(cols, rows) bit for bit, and the diagonal block of a joint marginal is symmetric.
// FMA loops, not v_mfma_f64_16x16x4_f64: the widest query (a pose against every plane of C2) is 201 independent 6 x 3 blocks over
// K <= ~900 rows, 3 MFLOP in all -- the kernel's time is its launch and the strips' latency, and 16-wide tiles would be 3/4 padding.
__global__ __launch_bounds__(kGramThreads) void k_cov_gram(const CovPair* __restrict__ pairs, int n_pairs, const double* __restrict__ Y, long long n_strip,
                                                           double* out, long long n_out) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];
  if ((int)blockIdx.x >= n_pairs) return;
  const CovPair r = pairs[blockIdx.x];
  const int tid = threadIdx.x, e = tid & 63, sl = tid >> 6;
  const bool ok = r.di >= 1 && r.di <= 6 && r.dj >= 1 && r.dj <= 6 && r.len >= 0 && r.ld >= r.dj && r.yi >= 0 && r.yj >= 0 &&
                  r.yi + (long long)r.len * r.di <= n_strip && r.yj + (long long)r.len * r.dj <= n_strip && r.dst >= 0 &&
                  r.dst + (long long)(r.di - 1) * r.ld + r.dj <= n_out &&
                  (r.dst_t < 0 || (r.ld >= r.di && r.dst_t + (long long)(r.dj - 1) * r.ld + r.di <= n_out));
  if (!ok) { if (tid == 0) raise_status(&out[0], kStatusInternal); return; }
  const int a = e / r.dj, c = e - a * r.dj;
  double acc = 0.0;
  if (e < r.di * r.dj) {
    const double* __restrict__ yi = Y + r.yi + a;
    const double* __restrict__ yj = Y + r.yj + c;
    for (int k = sl; k < r.len; k += kGramThreads / 64) acc += yi[(size_t)k * r.di] * yj[(size_t)k * r.dj];
  }
  cov_lds[tid] = acc;
  __syncthreads();
  if (sl == 0 && e < r.di * r.dj) {
    const double v = (cov_lds[e] + cov_lds[64 + e]) + (cov_lds[128 + e] + cov_lds[192 + e]);
    double* __restrict__ blocks = out + 1;       // (out[0] is the status word)
    const bool diag = r.dst_t == r.dst;
    if (!diag || c <= a) {
      blocks[r.dst + (long long)a * r.ld + c] = v;
      if (r.dst_t >= 0 && !(diag && a == c)) blocks[r.dst_t + (long long)c * r.ld + a] = v;
    }
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

size_t cov_path_lds_bytes(int max_p, int max_front) { return ((size_t)max_p * (max_p | 1) + (size_t)max_p * 6 + (size_t)2 * max_front * 6) * sizeof(double); }

hipError_t launch_cov_path(const DevGraph& d, const CovWalk* walks, int n_walks, const CovStep* steps, int n_steps_total, int K, int max_p,
                           int max_front, double* Y, long long n_strip, double* out, hipStream_t st) {
  if (n_walks == 0) return hipSuccess;
  const size_t lds = cov_path_lds_bytes(max_p, max_front);
  if (max_p < 1 || max_p > 64 || max_front < max_p || lds > (size_t)64 * 1024) return hipErrorInvalidValue;
  PPS_LAUNCH(k_cov_path, dim3(n_walks), dim3(kPathThreads), lds, st, d, walks, n_walks, steps, n_steps_total, K, max_p, max_front, Y, n_strip, out);
  return hipGetLastError();
}

hipError_t launch_cov_gram(const CovPair* pairs, int n_pairs, const double* Y, long long n_strip, double* out, long long n_out, hipStream_t st) {
  if (n_pairs == 0) return hipSuccess;
  PPS_LAUNCH(k_cov_gram, dim3(n_pairs), dim3(kGramThreads), kGramThreads * sizeof(double), st, pairs, n_pairs, Y, n_strip, out, n_out);
  return hipGetLastError();
}

}  // namespace pps
