// pps_k4_body.h -- the chi^2 sweep (device bodies): Slam::weighted_errors / chi2 (Slam.cpp:254-268).  Shared by the kernels of pps_k4.hip
// and, with ROBUST, by the chi2 kernels of pps_robust.hip.
#pragma once
#include "pps_cost.h"
#include "pps_geom.h"
#include "pps_kcommon.h"

namespace pps {

constexpr int kChiBlock = 256;

// A block's partial sum for the block that draws the last ticket, WITHOUT a release fence.  On this chip an agent-scope release writes back every
// dirty line of the XCD's L2, whoever wrote it: beside the linearisation sweep of k_trial_lin that is the sweep's output, microseconds per fence.
// The partial leaves as an atomic exchange instead -- performed at the memory side like the ticket's atomicAdd, and returned (the caller's
// s_waitcnt vmcnt(0)) before the ticket is drawn; chi2_finish reads it with an agent-scope atomic load.  Nothing else of the block is published.
__device__ __forceinline__ void publish_partial(double* p, double v) {
  const unsigned long long old = __hip_atomic_exchange(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(old));      // (the returning form: its value is back when vmcnt says so)
}

// sum of the nb block partials and of the n_dn |delta|^2 partials -> the 32-byte result record (one 256-thread block)
// light: no system-scope release in front of the sequence number (see publish_partial: it would wait for the L2 to write back what other
// blocks of the launch have written).  The record is pinned host memory, which the L2 does not hold: its three words go out as system-scope
// stores, and the sequence number follows when they have been acknowledged.  The record then says that the TRIALS are done, nothing more --
// what else the launch writes (k_trial_lin: the sweep's J / P / H) is complete for whoever is queued behind the launch on its stream.
__device__ __forceinline__ void chi2_finish(const DevGraph& d, int nb, int n_dn, double* __restrict__ out, double seq, bool light = false) {
  // (the not-PD flag of the solve before this launch: asked for first, so that its round trip runs beside the partials' instead of behind them)
  const double npd = threadIdx.x == 0 ? __hip_atomic_load(&d.result_dev[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  double cs = 0.0, dn = 0.0;
  for (int i = threadIdx.x; i < nb; i += kChiBlock) cs += __hip_atomic_load(&d.chi2_partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int i = threadIdx.x; i < n_dn; i += kChiBlock) dn += __hip_atomic_load(&d.dn_partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cs += __shfl_down(cs, o, 64); dn += __shfl_down(dn, o, 64); }
  __shared__ double red2[2][kChiBlock / 64];
  if ((threadIdx.x & 63) == 0) { red2[0][threadIdx.x >> 6] = cs; red2[1][threadIdx.x >> 6] = dn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b2 = 0.0;
    for (int k = 0; k < kChiBlock / 64; k++) { a += red2[0][k]; b2 += red2[1][k]; }
    d.result_dev[0] = a; d.result_dev[1] = b2; d.result_dev[2] = 0.0;   // the flag belongs to the solve before this record
    if (light) {
      __hip_atomic_store(&out[0], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&out[1], b2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&out[2], npd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(&out[3], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    out[0] = a; out[1] = b2; out[2] = npd;                 // `out` is pinned host memory: no copy kernel
    // the sequence number goes last, with system-scope release: the host polls it instead of paying a stream sync
    __hip_atomic_store(&out[3], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// bx: block within the graph, nb: blocks of the graph (TICKET: the one that draws the last ticket reduces)
// TOTAL > 0 (fused trial): the ticket counts TOTAL blocks -- the chi2 blocks and the retraction blocks of the same launch
// ROBUST (the chi2 kernels of pps_robust.hip; off everywhere else): r_i <- phi(r_i) behind every whitening (pps_cost.h), chi2 = sum rho(r_i)
// light (k_trial_lin): partial and record leave without release fences (publish_partial, chi2_finish)
template <bool TICKET = true, bool APPLY = false, bool ROBUST = false>
__device__ __forceinline__ void body_chi2(const DevGraph& d, const double* __restrict__ pose,
                                          const double* __restrict__ plane, int nb_obs, int nb_odo, int nb_pp,
                                          int n_dn, double* __restrict__ out, double seq, int bx, int nb, int total_blocks = 0, const CostFn& cost = CostFn{}, bool light = false) {
  __shared__ double red[kChiBlock / 64];
  int b = bx;
  double s = 0.0;
  if (b < nb_obs) {
    const int i = b * kChiBlock + threadIdx.x;
    if (i < d.n_obs) {
      double pz[7], pl[4], ms[4], w[6], e[3], r[3];
      fetch_pose<APPLY>(d, pose, d.obs_pose[i], pz);
      fetch_plane<APPLY>(d, plane, d.obs_plane[i], pl);
      if (i < d.n_obs_fixed) load_soa<4>(d.obs_meas, d.obs_ld, i, ms);
      else {                                  // Pose3d_Plane3d_Factor2: re-pop the measurement at this pose
        double ray[6];
        load_soa<6>(d.obs_ray, d.n_obs - d.n_obs_fixed, i - d.n_obs_fixed, ray);
        repop_wall_plane(pz, ray, ms);
      }
      load_soa<6>(d.obs_w, d.obs_ld, i, w);
      res_plane_obs(pz, pl, ms, e);
      whiten<3>(w, e, r);
      if (ROBUST) robustify<3>(cost, r);
      s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
  } else if ((b -= nb_obs) < nb_odo) {
    const int i = b * kChiBlock + threadIdx.x;
    if (i < d.n_odo) {
      double p1[7], p2[7], ms[6], w[21], e[6], r[6];
      fetch_pose<APPLY>(d, pose, d.odo_a[i], p1);
      fetch_pose<APPLY>(d, pose, d.odo_b[i], p2);
      load_soa<6>(d.odo_meas, d.odo_ld, i, ms);
      load_soa<21>(d.odo_w, d.odo_ld, i, w);
      res_odometry(p1, p2, ms, e);
      whiten<6>(w, e, r);
      if (ROBUST) robustify<6>(cost, r);
#pragma unroll
      for (int k = 0; k < 6; k++) s += r[k] * r[k];
    }
  } else if ((b -= nb_odo) < nb_pp) {
    const int i = b * kChiBlock + threadIdx.x;
    if (i < d.n_pp) {
      double pz[7], ms[6], w[21], e[6], r[6];
      fetch_pose<APPLY>(d, pose, d.pp_pose[i], pz);
      load_soa<6>(d.pp_meas, d.pp_ld, i, ms);
      load_soa<21>(d.pp_w, d.pp_ld, i, w);
      res_pose_prior(pz, ms, e);
      whiten<6>(w, e, r);
      if (ROBUST) robustify<6>(cost, r);
#pragma unroll
      for (int k = 0; k < 6; k++) s += r[k] * r[k];
    }
  } else {
    b -= nb_pp;
    const int i = b * kChiBlock + threadIdx.x;
    if (i < d.n_lp) {
      double pl[4], ms[4], w[6], e[3], r[3];
      fetch_plane<APPLY>(d, plane, d.lp_plane[i], pl);
      load_soa<4>(d.lp_meas, d.lp_ld, i, ms);
      load_soa<6>(d.lp_w, d.lp_ld, i, w);
      res_plane_prior(pl, ms, e);
      whiten<3>(w, e, r);
      if (ROBUST) robustify<3>(cost, r);
      s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
  }
  // wave reduction (64 lanes), then across the 4 waves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (!TICKET) {                                          // a batch: the partials are summed by kb_chi2_finish, a kernel boundary later
    if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < kChiBlock / 64; k++) t += red[k]; d.chi2_partials[bx] = t; }
    return;
  }
  __shared__ bool last;
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < kChiBlock / 64; k++) t += red[k];
    // publish, then take a ticket: the block that draws the last one reduces everything.  (An agent-scope release writes the
    // XCD's L2 back on this chip -- microseconds; fine for the few dozen blocks of one graph, not for the thousands of a batch.)
    if (light) publish_partial(&d.chi2_partials[bx], t);
    else { d.chi2_partials[bx] = t; __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(d.ticket, 1u) == (unsigned int)((total_blocks > 0 ? total_blocks : nb) - 1);
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  chi2_finish(d, nb, n_dn, out, seq, light);
  if (threadIdx.x == 0) *d.ticket = 0u;
}

}  // namespace pps
