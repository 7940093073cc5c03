// pps_merge.h -- launcher of the Mahalanobis merge gate between plane landmarks (pps_merge.hip), called from pps_merge.cpp (pps_merge_gate).
//
// A pair is two distinct live plane nodes a, b, a the one listed FIRST.  In the tangent coordinates of Plane3d::exmap_3dof:
//   e   = r(a | pi_b)    the residual of a Plane3d_Factor on node a with measurement pi_b and identity sqrt information, at the estimate
//   J_a = its 3 x 3 Jacobian, central differences with K1's eps and the device's step quaternions (pps_eval_factor's bits in JAC_NUMERIC)
//   J_b = -J(b | pi_a)   the NEGATED Jacobian of the mirrored factor: node b, measurement pi_a, the same differences
//   S   = J_a Sigma_aa J_a' + J_b Sigma_bb J_b' + J_a Sigma_ab J_b' + J_b Sigma_ba J_a' + floor_var I,    d2 = e' S^-1 e.
// The Jacobians are central differences WHATEVER the handle's jacobian_mode; Sigma is whatever linearisation the recovery used.
// Sigma is never formed.  With the strips Y_a, Y_b (K x 3 each) of k_cov_path (pps_cov.h: filled from the END), z_a = J_a y_a and
// z_b = J_b y_b per strip row,
//   S = floor_var I + sum over the rows of common ancestors of (z_a + z_b)(z_a + z_b)' + sum over all other rows of z_a z_a' + z_b z_b'.
// The two are added BEFORE they are multiplied: for two estimates of one wall J_b is close to -J_a, the strips nearly agree on the
// common rows and S is what is left of a difference (pps_gate.h has the same argument for a pose and a landmark it sees).
#pragma once
#include "pps_cov.h"

namespace pps {

// one listed plane: its strip (K x 3 doubles at Y + strip; rows K - rootlen .. K - 1 valid), its slot in the plane state, the front that
// holds its pivots
struct MergePlane { long long strip; int slot, front; };

struct MergeArgs {
  const MergePlane* planes; int n;       // the list; pair p (linear, (i, j) ascending, i < j) sits at i * n - i (i + 1) / 2 + (j - i - 1)
  long long n_pairs;
  const int* parent; const int* rootlen; int n_fronts;      // the elimination tree: parent front (-1: a root), pivots of a front and all its ancestors
  int K; const double* Y; long long n_strip;
  double floor_var, threshold;
  unsigned int* ticket;                  // one per listed plane, zero on entry and on exit
  double* status;                        // raised, never overwritten: kStatusInternal = an index outside the tables, the state arrays or the strips
  int* best;                             // n: per row the index of the smallest finite off-diagonal d2 (the first on ties), -1 if none
  unsigned char* flag;                   // n_pairs: 1 = finite d2 below the threshold, 2 = S not positive definite (d2 = NaN), 0 otherwise
  double* d2;                            // n x n, row-major: every pair computed once and written twice; the diagonal is zero
  double* rec = nullptr;                 // optional: [J_a 3 x 3 | J_b 3 x 3 | e 3] of every pair, 21 doubles at p * 21
};

constexpr int kMergeWaves = 4;           // pairs per workgroup, one wave each
constexpr int kMergeRecord = 21;
hipError_t launch_merge_gate(const DevGraph& d, const MergeArgs& a, hipStream_t st);

}  // namespace pps
