// pps_cov_dense.hip -- the selected inverse (pps_cov.h has the recursion) on trees whose fronts fit neither one wave nor LDS: the dense-front
// form of pps_dense.hip, p <= 64 pivots, boundaries of a thousand rows and more.  What k_cov_level (pps_cov.hip) does per front inside one
// workgroup is spread over many here, and the two products go through v_mfma_f64_16x16x4_f64.
//
//   once per call            k_cov_dense_pre      G = L_B L_A^-1 -> scratch in the panel layout of L, W = L_A^-T L_A^-1 -> the Sigma_AA rows
//                                                 of S.  Both depend on L alone: one launch over all fronts, W or 256 rows of G per workgroup
//                                                 (one thread per row, L_A in LDS with an odd leading dimension, as k_dense_panel solves).
//   per tree level, root     k_cov_dense_gather   Sigma_BB (b x b, both triangles, ld = b) -> the front's update-matrix slot of d.U, from the
//   level first                                   parent's [Sigma_AA Sigma_BA'; Sigma_BA Sigma_BB] through cmap (its last entry: the rhs row)
//                            k_cov_dense_sba      Sigma_BA = -Sigma_BB G: a workgroup owns a 64-row strip and all p columns -- 4 waves x 16
//                                                 rows, up to four 16 x 16 accumulator tiles per wave; k walks b in slabs of 32 staged in LDS
//                            k_cov_dense_saa      Sigma_AA = W - G' Sigma_BA: one workgroup per front, the same tiles reduced over b in one
//                                                 fixed order; the lower triangle is written and mirrored (symmetric bit for bit)
// The launch boundary is the only dependency between the steps and between the levels: no flags, no atomics on data, no waiting between
// workgroups.  MFMA operand layout (k_dense_trailing, tests/cpp/wave_emu.h): lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16];
// register r of the accumulator is row (l / 16) + 4 r, column l % 16.  Rows and k beyond the front are fed zeros by select on clamped
// addresses; every branch around an MFMA is wave-uniform.
// Every kernel checks front, parent, cmap targets and the extents of S, G and U before it writes anything of its front; a bad index
// raises d.result_dev[2] to kStatusInternal (never with a consistent analysis: the host has checked the same tables).
// Compiled without contraction, like pps_cov.hip (the MFMA instruction itself is fused).
#include <hip/hip_runtime.h>

#include "pps_cov.h"
#include "pps_status.h"

namespace pps {

namespace {

#ifndef PPS_COV_DENSE_EMU      // (tests/cpp/cov_dense_emu.cpp compiles this file for the host and brings its own)
typedef double double4_t __attribute__((ext_vector_type(4)));
#endif

constexpr int kDcThreads = 256;
constexpr int kDcMaxP = 64;                      // pivots per front (the tables are checked against it before anything is launched)
constexpr int kDcLdA = kDcMaxP + 1;
constexpr int kDcSlab = 32;                      // k per staged slab
constexpr int kDcLdK = kDcSlab + 1;              // 64 x 32 slab of the left operand
constexpr int kDcLdP = kDcMaxP + 1;              // 32 x 64 slab of the right operand

// workgroup -> (position in the list, work item of that front): the prefix-sum search of pps_dense.hip
__device__ __forceinline__ int dc_locate(const int* __restrict__ off, int count, int wg, int* item) {
  int lo = 0, hi = count;                        // invariant: off[lo] <= wg < off[hi]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= wg) lo = mid; else hi = mid; }
  *item = wg - off[lo];
  return lo;
}

// shape and extents of front s (the same answer in every thread): panel inside S and G, Sigma_BB inside U
__device__ __forceinline__ bool dc_front_ok(const DevGraph& d, int s, CovDenseExtents x) {
  if (s < 0 || s >= d.n_fronts) return false;
  const int p = d.f_p[s], b = d.f_b[s];
  const long long lo = d.f_Loff[s], uo = d.f_Uoff[s];
  return p >= 1 && p <= kDcMaxP && b >= 0 && lo >= 0 && lo + (long long)(p + b) * p <= x.n_panel && uo >= 0 && uo + (long long)b * b <= x.n_U;
}

// x <- x L_A^-1 (a row vector against the lower triangle): x_j = (x_j - sum_{k > j} x_k L_A[k][j]) / L_A[j][j], j descending.  A is
// zero outside the p x p lower triangle and dinv zero from p on, so the entries from p on stay zero without a test in the inner loop.
__device__ __forceinline__ void dc_row_solve(double (&x)[kDcMaxP], const double* A, const double* dinv) {
#pragma unroll
  for (int j = kDcMaxP - 1; j >= 0; j--) {
    double acc = x[j];
#pragma unroll
    for (int k = j + 1; k < kDcMaxP; k++) acc -= x[k] * A[k * kDcLdA + j];
    x[j] = acc * dinv[j];
  }
}

__global__ __launch_bounds__(kDcThreads) void k_cov_dense_pre(DevGraph d, double* __restrict__ S, double* __restrict__ G, CovDenseExtents ext,
                                                               const int* __restrict__ off, int n_fronts) {
  __shared__ double A[kDcMaxP * kDcLdA];
  __shared__ double dinv[kDcMaxP];
  int slab;
  const int s = dc_locate(off, n_fronts, blockIdx.x, &slab);
  const int tid = threadIdx.x;
  if (!dc_front_ok(d, s, ext)) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const int p = d.f_p[s], b = d.f_b[s];
  const double* __restrict__ Lp = d.L + d.f_Loff[s];
  for (int i = tid; i < kDcMaxP * kDcLdA; i += kDcThreads) A[i] = 0.0;
  __syncthreads();
  for (int idx = tid; idx < p * p; idx += kDcThreads) {
    const int i = idx / p, j = idx - i * p;
    if (j <= i) A[i * kDcLdA + j] = Lp[idx];
  }
  __syncthreads();
  if (tid < kDcMaxP) dinv[tid] = tid < p ? 1.0 / A[tid * kDcLdA + tid] : 0.0;
  __syncthreads();
  // ---- one row solve per thread: work item 0 owns X = L_A^-1 (row i = e_i L_A^-1), items 1 .. the rows of G = L_B L_A^-1 ----
  const bool wx = slab == 0;
  const int r = (slab - 1) * kDcThreads + tid;
  const bool mine = wx ? tid < p : r < b;
  double x[kDcMaxP];
  {
    const double* __restrict__ row = Lp + (size_t)(p + (wx || !mine ? 0 : r)) * p;
#pragma unroll
    for (int j = 0; j < kDcMaxP; j++) {
      const double v = mine && !wx && j < p ? row[j] : 0.0;
      x[j] = wx && j == tid ? 1.0 : v;
    }
  }
  if (mine) dc_row_solve(x, A, dinv);
  if (!wx) {
    if (mine) {
      double* __restrict__ g = G + d.f_Loff[s] + (size_t)(p + r) * p;
#pragma unroll
      for (int j = 0; j < kDcMaxP; j++) if (j < p) g[j] = x[j];
    }
    return;
  }
  // ---- W = X' X: X takes the place of L_A in LDS ----
  __syncthreads();                               // (every row solve of this workgroup has read L_A)
  if (mine) {
#pragma unroll
    for (int j = 0; j < kDcMaxP; j++) A[tid * kDcLdA + j] = x[j];
  }
  __syncthreads();
  double* __restrict__ Sp = S + d.f_Loff[s];
  for (int idx = tid; idx < p * p; idx += kDcThreads) {
    const int k = idx / p, l = idx - k * p;
    if (l > k) continue;
    double acc = 0.0;
    for (int m = k; m < p; m++) acc += A[m * kDcLdA + k] * A[m * kDcLdA + l];
    Sp[(size_t)k * p + l] = acc;
    Sp[(size_t)l * p + k] = acc;
  }
}

constexpr int kDcGatherRows = 32;                // rows of Sigma_BB per workgroup of the gather

__global__ __launch_bounds__(kDcThreads) void k_cov_dense_gather(DevGraph d, const double* __restrict__ S, CovDenseExtents ext, const int* __restrict__ parent,
                                                                  int level_begin, const int* __restrict__ off, int count) {
  __shared__ int bad;
  int item;
  const int s = d.level_fronts[level_begin + dc_locate(off, count, blockIdx.x, &item)];
  const int tid = threadIdx.x;
  if (!dc_front_ok(d, s, ext)) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const int b = d.f_b[s];
  if (b == 0) return;
  const int q = parent[s];
  if (!dc_front_ok(d, q, ext) || q == s || d.f_cmap_off[s + 1] - d.f_cmap_off[s] < b) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const int pq = d.f_p[q], bq = d.f_b[q];
  const int* __restrict__ cm = d.cmap + d.f_cmap_off[s];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int i = tid; i < b; i += kDcThreads) if (cm[i] < 0 || cm[i] >= pq + bq) bad = 1;      // every target of the front, before any of its entries is written
  __syncthreads();
  if (bad) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const double* __restrict__ Sq = S + d.f_Loff[q];
  const double* __restrict__ Bq = d.U + d.f_Uoff[q];
  double* __restrict__ Bs = d.U + d.f_Uoff[s];
  const int r0 = item * kDcGatherRows, nr = b - r0 < kDcGatherRows ? b - r0 : kDcGatherRows;
  for (int idx = tid; idx < nr * b; idx += kDcThreads) {
    const int i = r0 + idx / b, j = idx - (idx / b) * b;
    Bs[(size_t)i * b + j] = cov_full(Sq, Bq, pq, bq, cm[i], cm[j]);
  }
}

// acc[t] += Ls (64 x ks, wave w: rows 16 w ..) * Rs (ks x 16 nt) over one staged slab
__device__ __forceinline__ void dc_slab_mfma(const double* Ls, const double* Rs, int nt, double4_t (&acc)[4], int w, int l16, int lq) {
  const double* pa = Ls + (16 * w + l16) * kDcLdK + lq;
  const double* pb = Rs + lq * kDcLdP + l16;
#pragma unroll 2
  for (int kk = 0; kk < kDcSlab; kk += 4) {
    const double a = pa[kk];
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, pb[kk * kDcLdP + 16 * t], acc[t], 0, 0, 0);
  }
}

// rows [k0, k0 + 32) of a b x p matrix (row-major, ld = p) -> Rs; rows from b on are zero (the columns from p on were zeroed once)
__device__ __forceinline__ void dc_stage_rows(const double* __restrict__ M, int b, int p, int k0, double* Rs, int tid) {
  const int last = b * p - 1;
  for (int idx = tid; idx < kDcSlab * p; idx += kDcThreads) {
    const int r = idx / p, c = idx - r * p;
    const int src = k0 * p + idx;
    const double v = M[src < last ? src : last];
    Rs[r * kDcLdP + c] = src <= last ? v : 0.0;
  }
}

__global__ __launch_bounds__(kDcThreads) void k_cov_dense_sba(DevGraph d, double* __restrict__ S, const double* __restrict__ G, CovDenseExtents ext, int level_begin,
                                                               const int* __restrict__ off, int count) {
  __shared__ double Ls[64 * kDcLdK];
  __shared__ double Rs[kDcSlab * kDcLdP];
  int item;
  const int s = d.level_fronts[level_begin + dc_locate(off, count, blockIdx.x, &item)];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  if (!dc_front_ok(d, s, ext)) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const int p = d.f_p[s], b = d.f_b[s];
  if (b == 0) return;
  const int nt = (p + 15) >> 4;
  const int R0 = item * 64;                      // first row of the strip
  const double* __restrict__ Bs = d.U + d.f_Uoff[s];
  const double* __restrict__ Gb = G + d.f_Loff[s] + (size_t)p * p;
  for (int i = tid; i < kDcSlab * kDcLdP; i += kDcThreads) Rs[i] = 0.0;
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < b; k0 += kDcSlab) {
    __syncthreads();
    for (int idx = tid; idx < 64 * kDcSlab; idx += kDcThreads) {      // -Sigma_BB[R0 .. + 64][k0 .. + 32]
      const int r = idx / kDcSlab, c = idx - r * kDcSlab;
      const int row = R0 + r, col = k0 + c;
      const double v = Bs[(size_t)(row < b ? row : b - 1) * b + (col < b ? col : b - 1)];
      Ls[r * kDcLdK + c] = row < b && col < b ? -v : 0.0;
    }
    dc_stage_rows(Gb, b, p, k0, Rs, tid);
    __syncthreads();
    dc_slab_mfma(Ls, Rs, nt, acc, w, l16, lq);
  }
  double* __restrict__ Sp = S + d.f_Loff[s];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int cc = 16 * t + l16;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = R0 + 16 * w + lq + 4 * r;
      if (rr < b && cc < p) Sp[(size_t)(p + rr) * p + cc] = acc[t][r];
    }
  }
}

__global__ __launch_bounds__(kDcThreads) void k_cov_dense_saa(DevGraph d, double* __restrict__ S, const double* __restrict__ G, CovDenseExtents ext, int level_begin,
                                                               int count) {
  __shared__ double Ls[64 * kDcLdK];
  __shared__ double Rs[kDcSlab * kDcLdP];
  if ((int)blockIdx.x >= count) return;
  const int s = d.level_fronts[level_begin + blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  if (!dc_front_ok(d, s, ext)) { if (tid == 0) raise_status(&d.result_dev[2], kStatusInternal); return; }
  const int p = d.f_p[s], b = d.f_b[s];
  if (b == 0) return;                            // (the root: Sigma_AA = W, written by the pre-pass)
  const int nt = (p + 15) >> 4;
  double* __restrict__ Sp = S + d.f_Loff[s];
  const double* __restrict__ Gb = G + d.f_Loff[s] + (size_t)p * p;
  const double* __restrict__ Sba = Sp + (size_t)p * p;
  for (int i = tid; i < kDcSlab * kDcLdP; i += kDcThreads) Rs[i] = 0.0;
  for (int i = tid; i < 64 * kDcLdK; i += kDcThreads) Ls[i] = 0.0;
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int last = b * p - 1;
  for (int k0 = 0; k0 < b; k0 += kDcSlab) {
    __syncthreads();
    for (int idx = tid; idx < kDcSlab * p; idx += kDcThreads) {       // G'[0 .. p)[k0 .. + 32): rows of G read as they lie, written transposed
      const int r = idx / p, c = idx - r * p;
      const int src = k0 * p + idx;
      const double v = Gb[src < last ? src : last];
      Ls[c * kDcLdK + r] = src <= last ? v : 0.0;
    }
    dc_stage_rows(Sba, b, p, k0, Rs, tid);
    __syncthreads();
    if (16 * w < p) dc_slab_mfma(Ls, Rs, nt, acc, w, l16, lq);
  }
  // the lower triangle, mirrored: entry (rr, cc), cc <= rr, is read, written and mirrored by one lane alone
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int cc = 16 * t + l16;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = 16 * w + lq + 4 * r;
      if (rr < p && cc <= rr) {
        const double v = Sp[(size_t)rr * p + cc] - acc[t][r];
        Sp[(size_t)rr * p + cc] = v;
        Sp[(size_t)cc * p + rr] = v;
      }
    }
  }
}

}  // namespace

int cov_dense_pre_items(int b) { return 1 + (b + kDcThreads - 1) / kDcThreads; }
int cov_dense_gather_items(int b) { return (b + kDcGatherRows - 1) / kDcGatherRows; }
int cov_dense_strip_items(int b) { return (b + 63) / 64; }

hipError_t launch_cov_dense_pre(const DevGraph& d, double* S, double* G, CovDenseExtents ext, const int* off, int n_items, int n_fronts, hipStream_t st) {
  if (n_fronts <= 0 || n_items <= 0) return hipSuccess;
  if (!S || !G || !off) return hipErrorInvalidValue;
  PPS_LAUNCH(k_cov_dense_pre, dim3(n_items), dim3(kDcThreads), 0, st, d, S, G, ext, off, n_fronts);
  return hipGetLastError();
}

hipError_t launch_cov_dense_level(const DevGraph& d, double* S, const double* G, CovDenseExtents ext, const int* parent, int level_begin, int level_count,
                                  const int* off_gather, int n_gather, const int* off_strip, int n_strip, hipStream_t st) {
  if (level_count <= 0) return hipSuccess;
  if (!S || !G || !parent) return hipErrorInvalidValue;
  if (n_gather > 0) PPS_LAUNCH(k_cov_dense_gather, dim3(n_gather), dim3(kDcThreads), 0, st, d, S, ext, parent, level_begin, off_gather, level_count);
  if (n_strip > 0) {
    PPS_LAUNCH(k_cov_dense_sba, dim3(n_strip), dim3(kDcThreads), 0, st, d, S, G, ext, level_begin, off_strip, level_count);
    PPS_LAUNCH(k_cov_dense_saa, dim3(level_count), dim3(kDcThreads), 0, st, d, S, G, ext, level_begin, level_count);
  }
  return hipGetLastError();
}

}  // namespace pps
