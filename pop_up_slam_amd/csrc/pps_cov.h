// pps_cov.h -- launchers of the covariance recovery (pps_cov.hip), called from pps_cov.cpp.
//
// The selected inverse of H = L L' over the elimination tree (Takahashi recursion, per front instead of per row): with pivots A,
// boundary B and factor panel [L_A; L_B] of a front,
//   G = L_B L_A^-1,   Sigma_BA = -Sigma_BB G,   Sigma_AA = L_A^-T L_A^-1 - G' Sigma_BA,
// Sigma_BB gathered from the parent's full block through cmap.  Results: S, in the panel layout of L (rows 0 .. p-1 of a front =
// Sigma_AA, full and exactly symmetric; rows p .. p+b-1 = Sigma_BA), and each front's Sigma_BB (b x b, row-major) in its update
// matrix slot of d.U, which nothing reads between a factorisation and the next one.
//
// Blocks OUTSIDE the pattern (pps_cov_block) come from column solves on the same factor: with E_S the unit columns of a node set S,
//   Sigma(R, C) = E_R' H^-1 E_C = (L^-1 E_R)' (L^-1 E_C),
// and the columns of L^-1 E that belong to one node are non-zero only on the pivots of the fronts between the node's front and the
// root.  k_cov_path walks that path once per node (forward substitution per front, the remainder carried up through cmap) and stores
// the node's strip Y = L^-1 E_node; k_cov_gram multiplies two strips over the pivots of their common ancestors.
#pragma once
#include "pps_device.h"

namespace pps {

// one gathered block of a read call: out[dst + i * dc + j] = tr ? S[src + j * ld + i] : S[src + i * ld + j]
struct CovReq { long long src, dst; int ld, dr, dc, tr; };

size_t cov_level_lds_bytes(int p, int b);      // dynamic LDS one front of this shape needs
// one tree level (fronts level_fronts[level_begin .. + level_count)), one workgroup per front; parents must be done.
// lds_bytes: maximum of cov_level_lds_bytes over the level's fronts.  A pivot that is not positive, not finite, or below 1e-7 of the
// largest pivot of its front raises d.result_dev[2] to 1 (not positive definite), like the factorisation.
hipError_t launch_cov_level(const DevGraph& d, double* S, const int* parent, int level_begin, int level_count, size_t lds_bytes, hipStream_t st);
hipError_t launch_cov_gather(const double* S, const CovReq* req, int n, double* out, hipStream_t st);
// entry (r, c) of a front's full block [Sigma_AA Sigma_BA'; Sigma_BA Sigma_BB]: panel Sp (ld = p), boundary block Bs (ld = b)
// (what a child gathers its Sigma_BB from, in k_cov_level and in k_cov_dense_gather)
__device__ __forceinline__ double cov_full(const double* __restrict__ Sp, const double* __restrict__ Bs, int p, int b, int r, int c) {
  if (r < c) { const int t = r; r = c; c = t; }
  return c < p ? Sp[(size_t)r * p + c] : Bs[(size_t)(r - p) * b + (c - p)];
}

// ---- pps_cov_block: root-path solves ----
// A strip holds K rows of dim doubles (row k, column a at strip + k * dim + a), K = the longest requested path in pivots, and is filled
// from its END: the pivots of front s sit at rows K - rootlen(s) .. + p, rootlen(s) = the pivots of s and of all its ancestors.  A front
// that two nodes have in common therefore starts at the same row in both strips, and their common ancestors are a common suffix.
struct CovStep { int front, row; };             // one front of a path and the strip row of its first pivot
// one requested node: its dim unit columns start at pivot `local` of the first front of its path (steps[step0 .. + n_steps), leaf -> root)
struct CovWalk { long long strip; int step0, n_steps, local, dim; };
// one block of the result: out[dst + a * ld + c] = sum over k < len of Yi[k * di + a] * Yj[k * dj + c], Yi / Yj = the two strips from
// the first row of their common suffix.  dst_t >= 0: the transposed block is written as well (at dst_t + c * ld + a); dst_t == dst is
// the diagonal block of a joint marginal, computed on and below its diagonal and mirrored.
struct CovPair { long long yi, yj, dst, dst_t; int di, dj, len, ld; };

size_t cov_path_lds_bytes(int max_p, int max_front);   // dynamic LDS of k_cov_path for fronts of at most max_p pivots and max_front rows
// one workgroup per walk; status (one double, raised to kStatusInternal by an index outside its front or its strip, never overwritten)
// sits in front of the result: out[0], the blocks start at out[1].  n_strip: doubles in the strip buffer Y.
hipError_t launch_cov_path(const DevGraph& d, const CovWalk* walks, int n_walks, const CovStep* steps, int n_steps_total, int K, int max_p,
                           int max_front, double* Y, long long n_strip, double* out, hipStream_t st);
hipError_t launch_cov_gram(const CovPair* pairs, int n_pairs, const double* Y, long long n_strip, double* out, long long n_out, hipStream_t st);

// ---- pps_cov_factor / the path walk for wide fronts (pps_cov_wide.hip) ----
// a pivot of L_A that is not positive, not finite, or below this fraction of the largest pivot of its front: H is singular to 1e-14 of
// that diagonal (the criterion of k_cov_level, and of k_cov_pivots where the level pass does not run)
constexpr double kCovPivotRatio = 1e-7;
// the criterion alone, on the diagonal of every L_A: one workgroup per front, all fronts in one launch; raises d.result_dev[2] to 1
hipError_t launch_cov_pivots(const DevGraph& d, int n_fronts, hipStream_t st);
// k_cov_path for fronts that fit neither one wave nor LDS (p <= 64, any p + b): one workgroup of 256 threads per walk, L_A and y_A in
// LDS, the right-hand sides of the current front and of its parent in Z (global): walk w owns Z[w * cov_wide_scratch(max_front) ...).
// Same walks, steps, strips, status word and arithmetic order as launch_cov_path: the strips are the same bits.
inline size_t cov_wide_scratch(int max_front) { return (size_t)2 * max_front * 6; }      // doubles per walk
hipError_t launch_cov_path_wide(const DevGraph& d, const CovWalk* walks, int n_walks, const CovStep* steps, int n_steps_total, int K, int max_front,
                                double* Z, long long n_scratch, double* Y, long long n_strip, double* out, hipStream_t st);

// ---- pps_cov_select: the selected inverse on dense-front trees (pps_cov_dense.hip) ----
// Same recursion and the same results in the same places as launch_cov_level -- S in the panel layout of L, Sigma_BB (b x b, ld = b) in the
// front's update-matrix slot -- for fronts of p <= 64 pivots and any number of rows.  G = L_B L_A^-1 of every front sits in a scratch
// buffer in the panel layout (rows p .. p + b - 1 of a front's panel; the other rows are not touched).
struct CovDenseExtents { long long n_panel, n_U; };      // doubles in S and in G (both: L_size) | in d.U
// work items per front: W and the 256-row slabs of G, 32-row pieces of Sigma_BB, 64-row strips of Sigma_BA
int cov_dense_pre_items(int b);
int cov_dense_gather_items(int b);
int cov_dense_strip_items(int b);
// G and W = L_A^-T L_A^-1 (into the Sigma_AA rows of S) of all fronts; off: prefix sums of cov_dense_pre_items over the fronts 0 .. n_fronts - 1
// (n_fronts + 1 entries, device), n_items its last entry
hipError_t launch_cov_dense_pre(const DevGraph& d, double* S, double* G, CovDenseExtents ext, const int* off, int n_items, int n_fronts, hipStream_t st);
// one tree level, parents done: gather, Sigma_BA, Sigma_AA (three launches).  off_gather / off_strip: prefix sums of the items of the
// level's fronts in level_fronts order (level_count + 1 entries each, device).  An index outside its front raises d.result_dev[2] to
// kStatusInternal before anything of that front is written.
hipError_t launch_cov_dense_level(const DevGraph& d, double* S, const double* G, CovDenseExtents ext, const int* parent, int level_begin, int level_count,
                                  const int* off_gather, int n_gather, const int* off_strip, int n_strip, hipStream_t st);

}  // namespace pps
