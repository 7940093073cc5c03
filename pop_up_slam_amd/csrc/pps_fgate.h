// pps_fgate.h -- launcher of the leave-one-out chi-square test of the graph's own factors (pps_fgate.hip), called from pps_fgate.cpp
// (pps_factor_gate).
//
// For factor f with whitened residual r (m = 3 or 6) and whitened Jacobian J (m x c, c = 3, 6, 9 or 12 over its one or two nodes, the column
// order of pps_eval_factor) at the estimate, and Sigma_ff (c x c) the joint marginal of its nodes from the selected inverse,
//   P = J Sigma_ff J'    lev = trace(P)    d2 = r' (I - P)^-1 r.
// By Woodbury I + J Sigma_- J' = (I - P)^-1 and r_- = (I - P)^-1 r (Sigma_-, r_-: covariance and residual at the solution of the graph
// WITHOUT f), so d2 is the squared Mahalanobis distance of f's residual against the rest of the graph: chi-square with m degrees of freedom
// for a correct factor.  A factor that alone constrains a direction has a singular I - P: a pivot of its Cholesky factor, taken before the
// square root, that is not finite or <= kFgatePivotMin gives d2 = NaN ("untestable"); lev is still written.
#pragma once
#include "pps_cov.h"

namespace pps {

// one factor of the graph: where the three blocks of Sigma_ff sit in the selected inverse (the panel layout of L; CovReq's source offset,
// leading dimension and transpose flag, pps_cov.h) and which slot of which type's device arrays it is.  Block 0 = Sigma_aa, 1 = Sigma_bb,
// 2 = Sigma_ab (rows a, columns b); a unary factor has block 0 only.  type < 0: no live factor has this id.
struct FgateFactor { long long src[3]; int ld[3]; int tr; int type, slot; };

constexpr int kFgateRecord = 78;            // doubles per record slot: [J m x c row-major, packed | r m], the rest of the slot unspecified
constexpr int kFgateWaves = 4;              // list entries per workgroup, one wave each
constexpr double kFgatePivotMin = 1e-7;     // kCovPivotRatio applied to I - P, whose scale is 1

struct FgateArgs {
  const FgateFactor* factors; int n_factors;   // the table, indexed by factor id
  const int* list; int n;                      // the factor ids asked for
  const double* S; long long n_S;              // the selected inverse and its extent in doubles
  int mode;                                    // pps_jacobian_mode
  double* d2; double* lev;                     // n each
  int* status;                                 // n: 0, or 1 where an index fell outside the table, the state arrays or S (nothing else of that entry is written)
  double* rec = nullptr;                       // optional: the record of every entry, kFgateRecord doubles each
};

// one launch, one wave per list entry; no entry waits for another and nothing is accumulated across entries
hipError_t launch_factor_gate(const DevGraph& d, const FgateArgs& a, hipStream_t st);

}  // namespace pps
