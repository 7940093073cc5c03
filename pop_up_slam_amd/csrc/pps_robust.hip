// pps_robust.hip -- the kernels of a handle with a robust cost function (pps_set_cost_function; pps_cost.h): K1 in its thread-per-factor
// form over all four factor types + the re-popping Factor2 edges, both Jacobian modes, and the two chi2 kernels of the one-step LM loop.
// The bodies are the ones of pps_k1_body.h / pps_lin.h / pps_k4_body.h with their ROBUST flag on; the cost is a kernel argument of its own
// (DevGraph does not grow).  They write what the plain kernels write -- Jacobian records, product records, single-observation H blocks,
// the chi2 result record -- so that K2, K3 and the retraction run unchanged behind them.  Compiled with the contraction setting of
// pps_k1.hip, whose thread form this is.  A handle without a cost function never launches anything in this file.
// A side effect of that setting: k_chi2_trial_robust evaluates at est (+) delta computed on the spot with contraction allowed around the
// exmap (the exmap functions themselves switch it off, pps_geom.h), while k_retract (pps_k4.hip, built without contraction) writes the
// stored state the next K1 reads.  The plain path keeps pps_k4.hip out of the contraction list so that its loop forms agree bit for bit;
// the robust path has ONE loop form, so nothing has to agree with it bit for bit, and a last-bit difference between the trial's chi2 and
// the chi2 of the stored point is far below the 1e-9 its results are held to.
// Every kernel is a template over the KIND of cost and pins cost.kind to it, so that the branches of pps_cost.h fold at compile time: with
// the kind left to run time every robustified evaluation carried all three forms -- the inlined logarithm of the Cauchy cost included --
// and the numeric plane-observation kernel, already register-bound, spilled 60 registers to scratch (tools/kernel_resources.py).
#include <hip/hip_ext.h>

#include "pps_k1_body.h"
#include "pps_k4_body.h"

namespace pps {

template <int KIND, int MODE, int PART>
__global__ __launch_bounds__(kLinBlock) void k_linearize_robust(DevGraph d, CostFn cost, const double* __restrict__ pose,
                                                                 const double* __restrict__ plane, int nb_obs, int nb_odo, int nb_pp) {
  extern __shared__ double lin_lds[];
  cost.kind = KIND;
  body_linearize<MODE, PART, PART == 0, true>(d, pose, plane, nb_obs, nb_odo, nb_pp, blockIdx.x, lin_lds, cost);
}

// the numeric plane observations, held to the two waves per SIMD of k_linearize_obs_numeric (pps_k1.hip) -- see there
template <int KIND>
__global__ __launch_bounds__(kLinBlock) __attribute__((amdgpu_waves_per_eu(kObsNumericWaves, kObsNumericWaves)))
void k_linearize_obs_numeric_robust(DevGraph d, CostFn cost, const double* __restrict__ pose, const double* __restrict__ plane, int nb_obs, int nb_odo, int nb_pp) {
  extern __shared__ double lin_lds[];
  cost.kind = KIND;
  body_linearize<0, 0, true, true>(d, pose, plane, nb_obs, nb_odo, nb_pp, blockIdx.x, lin_lds, cost);
}

template <int KIND>
__global__ __launch_bounds__(64) void k_linearize_repop_robust(DevGraph d, CostFn cost, const double* __restrict__ pose, const double* __restrict__ plane) {
  __shared__ double repop_lds[64 * 31];
  cost.kind = KIND;
  body_linearize_repop<true>(d, pose, plane, blockIdx.x, repop_lds, cost);
}

// launch_linearize (pps_k1.hip) for a handle with a cost function: always the thread form, no guard (the one-step loop does not speculate)
template <int KIND>
static hipError_t launch_linearize_kind(const DevGraph& d, const CostFn& cost, int mode, bool at_estimate, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  const double* pose = at_estimate ? d.pose_est : d.pose_lin;
  const double* plane = at_estimate ? d.plane_est : d.plane_lin;
  if (ev0) { const hipError_t e = hipEventRecord(ev0, st); if (e != hipSuccess) return e; }
  if (d.n_obs > d.n_obs_fixed) PPS_LAUNCH(k_linearize_repop_robust<KIND>, dim3(cdiv(d.n_obs - d.n_obs_fixed, 64)), dim3(64), 0, st, d, cost, pose, plane);
  const int nb_obs = cdiv(d.n_obs_fixed, kLinBlock), nb_odo = cdiv(d.n_odo, kLinBlock), nb_pp = cdiv(d.n_pp, kLinBlock),
            nb_lp = cdiv(d.n_lp, kLinBlock);
  const int nb_rest = nb_odo + nb_pp + nb_lp;
  const size_t lds0 = (size_t)(kLinBlock / 64) * 64 * 31 * sizeof(double), lds1 = (size_t)(kLinBlock / 64) * 64 * 79 * sizeof(double);
  DevGraph dn = d;
  if (!k1_products(d, mode)) dn.P = nullptr;      // (PPS_K1_THREAD_FORM: K2 multiplies the Jacobians itself, as behind the plain thread form)
  if (mode == 1) {
    if (nb_obs) PPS_LAUNCH((k_linearize_robust<KIND, 1, 0>), dim3(nb_obs), dim3(kLinBlock), lds0, st, dn, cost, pose, plane, nb_obs, nb_odo, nb_pp);
    if (nb_rest) PPS_LAUNCH((k_linearize_robust<KIND, 1, 1>), dim3(nb_rest), dim3(kLinBlock), lds1, st, dn, cost, pose, plane, nb_obs, nb_odo, nb_pp);
  } else {
    if (nb_obs) PPS_LAUNCH(k_linearize_obs_numeric_robust<KIND>, dim3(nb_obs), dim3(kLinBlock), lds0, st, dn, cost, pose, plane, nb_obs, nb_odo, nb_pp);
    if (nb_rest) PPS_LAUNCH((k_linearize_robust<KIND, 0, 1>), dim3(nb_rest), dim3(kLinBlock), lds1, st, dn, cost, pose, plane, nb_obs, nb_odo, nb_pp);
  }
  if (ev1) { const hipError_t e = hipEventRecord(ev1, st); if (e != hipSuccess) return e; }
  return hipGetLastError();
}
hipError_t launch_linearize_robust(const DevGraph& d, const CostFn& cost, int mode, bool at_estimate, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  switch (cost.kind) {
    case COST_HUBER: return launch_linearize_kind<COST_HUBER>(d, cost, mode, at_estimate, st, ev0, ev1);
    case COST_PSEUDO_HUBER: return launch_linearize_kind<COST_PSEUDO_HUBER>(d, cost, mode, at_estimate, st, ev0, ev1);
    case COST_CAUCHY: return launch_linearize_kind<COST_CAUCHY>(d, cost, mode, at_estimate, st, ev0, ev1);
    default: return hipErrorInvalidValue;      // (COST_NONE never comes here: pps_graph.h, lin_launch)
  }
}

// chi2 = sum rho(r_i) at the stored state (k_chi2's counterpart) ...
template <int KIND>
__global__ __launch_bounds__(kChiBlock) void k_chi2_robust(DevGraph d, CostFn cost, const double* __restrict__ pose, const double* __restrict__ plane,
                                                           int nb_obs, int nb_odo, int nb_pp, int n_dn, double* __restrict__ out, double seq) {
  cost.kind = KIND;
  body_chi2<true, false, true>(d, pose, plane, nb_obs, nb_odo, nb_pp, n_dn, out, seq, blockIdx.x, gridDim.x, 0, cost);
}
// ... and of the one-step loop's trial, at est (+) delta computed on the spot (k_chi2_trial's)
template <int KIND>
__global__ __launch_bounds__(kChiBlock) void k_chi2_trial_robust(DevGraph d, CostFn cost, int nb_obs, int nb_odo, int nb_pp, int n_dn, double* __restrict__ out, double seq) {
  cost.kind = KIND;
  body_chi2<true, true, true>(d, d.pose_est, d.plane_est, nb_obs, nb_odo, nb_pp, n_dn, out, seq, blockIdx.x, gridDim.x, 0, cost);
}

hipError_t launch_chi2_robust(const DevGraph& d, const CostFn& cost, bool at_estimate, double* host_result, double seq, hipStream_t st) {
  const int nb_obs = cdiv(d.n_obs, kChiBlock), nb_odo = cdiv(d.n_odo, kChiBlock), nb_pp = cdiv(d.n_pp, kChiBlock), nb_lp = cdiv(d.n_lp, kChiBlock);
  const int nb = nb_obs + nb_odo + nb_pp + nb_lp;
  if (nb == 0) return hipErrorInvalidValue;
  const double* pose = at_estimate ? d.pose_est : d.pose_lin;
  const double* plane = at_estimate ? d.plane_est : d.plane_lin;
  const int n_dn = cdiv(d.n_pose + d.n_plane, 256);
  switch (cost.kind) {
    case COST_HUBER: PPS_LAUNCH(k_chi2_robust<COST_HUBER>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, pose, plane, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    case COST_PSEUDO_HUBER: PPS_LAUNCH(k_chi2_robust<COST_PSEUDO_HUBER>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, pose, plane, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    case COST_CAUCHY: PPS_LAUNCH(k_chi2_robust<COST_CAUCHY>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, pose, plane, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_chi2_trial_robust(const DevGraph& d, const CostFn& cost, double* host_result, double seq, hipStream_t st) {
  const int nb_obs = cdiv(d.n_obs, kChiBlock), nb_odo = cdiv(d.n_odo, kChiBlock), nb_pp = cdiv(d.n_pp, kChiBlock), nb_lp = cdiv(d.n_lp, kChiBlock);
  const int nb = nb_obs + nb_odo + nb_pp + nb_lp;
  if (nb == 0) return hipErrorInvalidValue;
  const int n_dn = cdiv(d.n_pose + d.n_plane, 256);
  switch (cost.kind) {
    case COST_HUBER: PPS_LAUNCH(k_chi2_trial_robust<COST_HUBER>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    case COST_PSEUDO_HUBER: PPS_LAUNCH(k_chi2_trial_robust<COST_PSEUDO_HUBER>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    case COST_CAUCHY: PPS_LAUNCH(k_chi2_trial_robust<COST_CAUCHY>, dim3(nb), dim3(kChiBlock), 0, st, d, cost, nb_obs, nb_odo, nb_pp, n_dn, host_result, seq); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pps
