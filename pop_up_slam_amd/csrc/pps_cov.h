// pps_cov.h -- launchers of the covariance recovery (pps_cov.hip), called from pps_cov.cpp.
//
// The selected inverse of H = L L' over the elimination tree (Takahashi recursion, per front instead of per row): with pivots A,
// boundary B and factor panel [L_A; L_B] of a front,
//   G = L_B L_A^-1,   Sigma_BA = -Sigma_BB G,   Sigma_AA = L_A^-T L_A^-1 - G' Sigma_BA,
// Sigma_BB gathered from the parent's full block through cmap.  Results: S, in the panel layout of L (rows 0 .. p-1 of a front =
// Sigma_AA, full and exactly symmetric; rows p .. p+b-1 = Sigma_BA), and each front's Sigma_BB (b x b, row-major) in its update
// matrix slot of d.U, which nothing reads between a factorisation and the next one.
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

}  // namespace pps
