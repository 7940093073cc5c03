// pps_gate.h -- launcher of the Mahalanobis gate (pps_gate.hip), called from pps_gate.cpp (pps_assoc_gate).
//
// A candidate pairs measurement m (a plane in the sensor frame of pose x, sqrt information W) with landmark l.  With r (3) and
// Jw = [Jp 3 x 6 | Jl 3 x 3] the whitened residual and Jacobian of the Pose3d_Plane3d_Factor(x, l, m, W) at the estimate, and Sigma the
// joint marginal of (x, l),
//   S = I + Jw Sigma Jw',   d2 = r' S^-1 r.
// Sigma is never formed.  With the strips Y_x (K x 6), Y_l (K x 3) of k_cov_path (pps_cov.h: Y = L^-1 E_node, filled from the END),
//   Sigma_xx = Y_x' Y_x,  Sigma_ll = Y_l' Y_l,  Sigma_xl = Y_x' Y_l over the rows of the COMMON ancestors only,
// so with Z_x = Y_x Jp', Z_l = Y_l Jl' (K x 3 each)
//   S = I + Z_x' Z_x + Z_l' Z_l + (Z_x' Z_l + Z_l' Z_x over the common suffix).
// strip_gram3 (pps_gate_dev.h) evaluates this per strip row, and says why the sum z_x + z_l comes before the product on the common suffix
// and why the strips are not added row by row.
#pragma once
#include "pps_cov.h"

namespace pps {

// one candidate landmark: its strip (K x 3 doubles at Y + strip), its slot in the plane state, the pivots on its path to the root
// (the strip's rows K - rootlen .. K - 1 are valid, the rows ahead of them unspecified) and the pivots it has in common with the pose's path
struct GatePlane { long long strip; int slot, rootlen, common, pad; };

struct GateArgs {
  const GatePlane* planes; int n_planes;
  const double* meas; int n_meas;        // n_meas x 10: the measurement (4, normalised) | its packed upper-triangular sqrt information (6)
  long long strip_x; int pose_slot, rootlen_x;      // the pose: strip K x 6
  int K; const double* Y; long long n_strip;
  int mode;                              // pps_jacobian_mode
  unsigned int* ticket;                  // one per measurement, zero on entry and on exit
  double* out;                           // [status | d2 n_meas x n_planes | best: n_meas ints]
  double* rec = nullptr;                 // optional: the record [Jp 3 x 6 | Jl 3 x 3 | r 3] of every candidate, 30 doubles at (m * n_planes + l) * 30
};

constexpr int kGateWaves = 4;            // candidates per workgroup, one wave each
// status (out[0], raised, never overwritten): 1 = a pivot of a 3 x 3 S was not positive or not finite, kStatusInternal = an index
// outside the state arrays or the strips.  best[m] = the candidate with the smallest finite d2 (the first one on ties), -1 if none.
hipError_t launch_assoc_gate(const DevGraph& d, const GateArgs& a, hipStream_t st);

}  // namespace pps
