// pps_gate.cpp -- pps_assoc_gate: the probabilistic gate of plane association.  For n_meas plane measurements of one pose and n_planes
// candidate landmarks, the squared Mahalanobis distance d2 = r' (I + Jw Sigma Jw')^-1 r of every pairing -- r, Jw the whitened residual
// and Jacobian a Pose3d_Plane3d_Factor(pose, landmark, measurement, noise) would have at the estimate, Sigma the joint marginal of (pose,
// landmark) from the current recovery -- and the best candidate per measurement.  What isam::Covariances is for in a SLAM front end:
// a pairing is accepted when d2 is below a chi-square quantile (3 degrees of freedom: 7.815 at 0.95).
//
// The candidate factors are never added: the call reads the estimate and the lambda = 0 factor pps_cov_recover left in dev.L, and writes
// buffers of its own.  One request upload, the k_cov_path launch of pps_cov_block for the 1 + n_planes distinct nodes, the gate launch
// (pps_gate.hip), one copy back ([status | d2 | best]).  Validity: that of pps_cov_block (cov_factor_current: a factor of pps_cov_recover or of
// pps_cov_factor; the walks take k_cov_path or k_cov_path_wide as pps_cov_block's do).
#include "pps_gate.h"
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void gate_release(pps_graph* g) {
  if (g->gate_out) (void)hipFree(g->gate_out);
  if (g->gate_ticket) (void)hipFree(g->gate_ticket);
  if (g->gate_rec) (void)hipFree(g->gate_rec);
  for (hipEvent_t& e : g->gate_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  g->gate_out = nullptr; g->gate_ticket = nullptr; g->gate_rec = nullptr;
  g->gate_out_cap = g->gate_ticket_cap = g->gate_rec_cap = 0; g->gate_rec_n = 0; g->gate_clean = false;
}

}  // namespace pps_impl

extern "C" {

int pps_assoc_gate_last(const pps_graph* g, double* kernel_sec, int* launches) {
  if (!g) return PPS_EINVAL;
  if (kernel_sec) *kernel_sec = g->gate_sec;
  if (launches) *launches = g->gate_launches;
  return PPS_OK;
}

int pps_debug_assoc_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  if (!g || !needed) return PPS_EINVAL;
  if (g->gate_rec_n == 0 || !g->gate_rec) return fail(g, PPS_ESTATE, "no association gate has been computed on this handle");
  *needed = (int64_t)g->gate_rec_n * 30;
  if (!rec || cap < *needed) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  HIP_TRY(g, hipMemcpyAsync(rec, g->gate_rec, (size_t)*needed * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  return PPS_OK;
}

int pps_assoc_gate(pps_graph* g, int pose_id, int n_meas, const double* meas4, const double* sqrtinf_ut, int n_planes, const int* plane_ids,
                   double* d2, int* best) {
  if (!g || !meas4 || !sqrtinf_ut || !d2 || n_meas < 0 || (plane_ids && n_planes < 0)) return PPS_EINVAL;
  if (!live_node(g, pose_id, NODE_POSE)) return fail(g, PPS_EINVAL, "association gate: node " + std::to_string(pose_id) + " is not a live pose");
  if (n_meas > 65535) return fail(g, PPS_EINVAL, "association gate: more than 65535 measurements in one call");
  // the candidates' r and Jw are the squared-error ones; with a cost function the recovered covariance is that of the robustified system
  if (robust(g)) return fail(g, PPS_ESTATE, "association gate: a robust cost function is set (pps_set_cost_function); the gate has no robustified form -- set PPS_COST_NONE and recover again");
  std::vector<int> all;
  if (!plane_ids) {
    for (size_t i = 0; i < g->nodes.size(); i++) if (!g->nodes[i].deleted && g->nodes[i].type == NODE_PLANE) all.push_back((int)i);
    plane_ids = all.data(); n_planes = (int)all.size();
  }
  { std::vector<char> seen(g->nodes.size(), 0);
    for (int i = 0; i < n_planes; i++) {
      const int id = plane_ids[i];
      if (!live_node(g, id, NODE_PLANE)) return fail(g, PPS_EINVAL, "association gate: node " + std::to_string(id) + " is not a live plane");
      if (seen[id]) return fail(g, PPS_EINVAL, "association gate: plane " + std::to_string(id) + " is listed twice");
      seen[id] = 1;
    } }
  // measurements: normalised like Plane3d(Vector4d), as pps_add_plane_obs stores them
  std::vector<double> meas((size_t)n_meas * 10);
  for (int i = 0; i < n_meas; i++) {
    double* o = meas.data() + (size_t)i * 10;
    for (int k = 0; k < 4; k++) { o[k] = meas4[(size_t)i * 4 + k]; if (!std::isfinite(o[k])) return fail(g, PPS_EINVAL, "association gate: non-finite measurement"); }
    for (int k = 0; k < 6; k++) { o[4 + k] = sqrtinf_ut[(size_t)i * 6 + k]; if (!std::isfinite(o[4 + k])) return fail(g, PPS_EINVAL, "association gate: non-finite sqrtinf"); }
    normalize4(o);
  }
  if (n_meas == 0 || n_planes == 0) return PPS_OK;       // nothing asked for: the outputs stay untouched
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  // walks: the pose first, then the candidates in the order given (the tables of pps_cov_block)
  const int nw = 1 + n_planes;
  std::vector<int> ids((size_t)nw);
  std::vector<CovNode> nd((size_t)nw);
  for (int w = 0; w < nw; w++) {
    ids[w] = w == 0 ? pose_id : plane_ids[w - 1];
    const int rc = cov_node(g, ids[w], &nd[w]); if (rc != PPS_OK) return rc;
  }
  CovWalks cw;
  { const int rc = cov_build_walks(g, ids, nd, &cw); if (rc != PPS_OK) return rc; }
  const int K = cw.K;
  const long long n_strip = cw.n_strip;
  const std::vector<CovWalk>& walks = cw.walks;
  const std::vector<CovStep>& steps = cw.steps;
  std::vector<GatePlane> cand((size_t)n_planes);
  for (int l = 0; l < n_planes; l++)
    cand[l] = GatePlane{walks[1 + l].strip, g->nodes[plane_ids[l]].slot, g->cov_rootlen[nd[1 + l].front], cov_common_pivots(g, cw, 0, 1 + l), 0};
  // one request: [walks | steps | candidates | measurements]
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_steps = walks.size() * sizeof(CovWalk), o_cand = up16(o_steps + steps.size() * sizeof(CovStep)),
               o_meas = up16(o_cand + cand.size() * sizeof(GatePlane));
  std::vector<char> req(o_meas + meas.size() * sizeof(double));
  memcpy(req.data(), walks.data(), walks.size() * sizeof(CovWalk));
  memcpy(req.data() + o_steps, steps.data(), steps.size() * sizeof(CovStep));
  memcpy(req.data() + o_cand, cand.data(), cand.size() * sizeof(GatePlane));
  memcpy(req.data() + o_meas, meas.data(), meas.size() * sizeof(double));
  const size_t n_d2 = (size_t)n_meas * n_planes, n_out = 1 + n_d2 + ((size_t)n_meas + 1) / 2;      // doubles: status | d2 | best (ints)
  HIP_TRY(g, hipSetDevice(g->props.device));
  for (hipEvent_t& e : g->gate_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  // (cov_breq / cov_strip are shared with pps_cov_block: both calls end with a synchronisation, neither is in flight here)
  int rc = cov_reserve(g, &g->cov_breq, &g->cov_breq_cap, req.size()); if (rc != PPS_OK) return rc;
  rc = cov_reserve(g, &g->cov_strip, &g->cov_strip_cap, (size_t)n_strip); if (rc != PPS_OK) return rc;
  rc = cov_walk_scratch(g, cw); if (rc != PPS_OK) return rc;
  const double* out0 = g->gate_out; const unsigned int* ticket0 = g->gate_ticket;
  rc = cov_reserve(g, &g->gate_out, &g->gate_out_cap, n_out); if (rc != PPS_OK) return rc;
  rc = cov_reserve(g, &g->gate_ticket, &g->gate_ticket_cap, (size_t)n_meas); if (rc != PPS_OK) return rc;
  g->gate_rec_n = 0;
  rc = cov_reserve(g, &g->gate_rec, &g->gate_rec_cap, n_d2 * 30); if (rc != PPS_OK) return rc;
  const bool fresh = !g->gate_clean || g->gate_out != out0 || g->gate_ticket != ticket0 || !out0 || !ticket0;
  if (fresh) {                                           // (a new buffer, or a call that failed)
    HIP_TRY(g, hipMemsetAsync(g->gate_out, 0, sizeof(double), g->stream));
    HIP_TRY(g, hipMemsetAsync(g->gate_ticket, 0, g->gate_ticket_cap * sizeof(unsigned int), g->stream));
  }
  g->gate_clean = false;
  GateArgs ga;
  ga.planes = reinterpret_cast<const GatePlane*>(g->cov_breq + o_cand); ga.n_planes = n_planes;
  ga.meas = reinterpret_cast<const double*>(g->cov_breq + o_meas); ga.n_meas = n_meas;
  ga.strip_x = walks[0].strip; ga.pose_slot = g->nodes[pose_id].slot; ga.rootlen_x = g->cov_rootlen[nd[0].front];
  ga.K = K; ga.Y = g->cov_strip; ga.n_strip = n_strip;
  ga.mode = g->props.jacobian_mode;
  ga.ticket = g->gate_ticket; ga.out = g->gate_out; ga.rec = g->gate_rec;
  const unsigned long long launches0 = launch_count();
  HIP_TRY(g, hipMemcpyAsync(g->cov_breq, req.data(), req.size(), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, hipEventRecord(g->gate_ev[0], g->stream));
  HIP_TRY(g, cov_launch_walks(g, cw, reinterpret_cast<const CovWalk*>(g->cov_breq), reinterpret_cast<const CovStep*>(g->cov_breq + o_steps), g->gate_out));
  HIP_TRY(g, launch_assoc_gate(g->dev, ga, g->stream));
  HIP_TRY(g, hipEventRecord(g->gate_ev[1], g->stream));
  std::vector<double> host(n_out);
  HIP_TRY(g, hipMemcpyAsync(host.data(), g->gate_out, n_out * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  g->gate_launches = (int)(launch_count() - launches0);
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->gate_ev[0], g->gate_ev[1]) == hipSuccess) g->gate_sec = 1e-3 * ms;
  if (host[0] >= kStatusInternal) return fail(g, PPS_EHIP, "internal error: the association gate met an index outside its front, its strip or the state arrays");
  if (host[0] != 0.0)
    return fail(g, PPS_ENOTPD, "association gate: the innovation covariance of a candidate is not positive definite (a pivot of the 3 x 3 factor was not positive or not finite)");
  g->gate_clean = true;
  g->gate_rec_n = n_d2;
  memcpy(d2, host.data() + 1, n_d2 * sizeof(double));
  if (best) memcpy(best, host.data() + 1 + n_d2, (size_t)n_meas * sizeof(int));
  return PPS_OK;
}

}  // extern "C"
