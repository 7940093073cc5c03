// pps_loop.h -- launcher of the Mahalanobis gate for loop-closure pose candidates (pps_loop.hip), called from pps_loop.cpp (pps_loop_gate).
//
// A candidate is the factor Pose3d_Pose3d_Factor(a, b, meas, W) that pps_add_odometry would add between two distinct live poses.  With r (6)
// and Jw = [J_a J_b] (6 x 12) its whitened residual and Jacobian at the estimate, in the handle's jacobian_mode and the column order of
// pps_eval_factor, and Sigma (12 x 12) the joint marginal of (a, b) from the current factor,
//   S = I + Jw Sigma Jw',    d2 = r' S^-1 r    (6 x 6 Cholesky solve; chi-square with 6 degrees of freedom for a correct closure).
// Sigma is never formed.  With the strips Y_a, Y_b (K x 6 each) of k_cov_path (pps_cov.h: filled from the END), z_a = J_a y_a and
// z_b = J_b y_b per strip row,
//   S = I + sum over the rows of common ancestors of (z_a + z_b)(z_a + z_b)' + sum over all other rows of z_a z_a' + z_b z_b'.
// The two are added BEFORE they are multiplied: J_b is close to -J_a in its translation rows, neighbouring poses share most of their
// uncertainty, and S is what is left of the difference (pps_gate.h and pps_merge.h have the same argument).
#pragma once
#include "pps_cov.h"

namespace pps {

// one candidate: the strips of its two poses (K x 6 doubles at Y + strip; rows K - rootlen .. K - 1 valid; two candidates that name the
// same pose share its strip), their slots in the pose state, the fronts that hold their pivots, the measurement as pps_add_odometry
// stores it and the packed upper triangle of the sqrt information
struct LoopCand { long long strip_a, strip_b; int slot_a, slot_b, front_a, front_b; double meas[6]; double sw[21]; };

struct LoopArgs {
  const LoopCand* cands; int n;
  const int* parent; const int* rootlen; int n_fronts;      // the elimination tree: parent front (-1: a root), pivots of a front and all its ancestors
  int K; const double* Y; long long n_strip;
  double threshold;
  int mode;                              // the handle's jacobian_mode: 1 = the closed form of pps_lin.h, else central differences in the lane form
  double* status;                        // raised, never overwritten: kStatusInternal = an index outside the tables, the state arrays or the strips
  unsigned char* flag;                   // n: 1 = finite d2 below the threshold, 2 = S not positive definite (d2 = NaN), 0 otherwise
  double* d2;                            // n
  double* S = nullptr;                   // optional: n x 36, row-major, the lower triangle mirrored
  double* rec = nullptr;                 // optional: [Jw 6 x 12 row-major | r 6] of every candidate, 78 doubles at k * 78
};

constexpr int kLoopWaves = 4;            // candidates per workgroup, one wave each
constexpr int kLoopRecord = 78;
hipError_t launch_loop_gate(const DevGraph& d, const LoopArgs& a, hipStream_t st);

}  // namespace pps
