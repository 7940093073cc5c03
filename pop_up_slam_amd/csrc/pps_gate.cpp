// pps_gate.cpp -- pps_assoc_gate: the probabilistic gate of plane association.  For n_meas plane measurements of one pose and n_planes
// candidate landmarks, the squared Mahalanobis distance d2 = r' (I + Jw Sigma Jw')^-1 r of every pairing -- r, Jw the whitened residual
// and Jacobian a Pose3d_Plane3d_Factor(pose, landmark, measurement, noise) would have at the estimate, Sigma the joint marginal of (pose,
// landmark) from the current recovery -- and the best candidate per measurement.  What isam::Covariances is for in a SLAM front end:
// a pairing is accepted when d2 is below a chi-square quantile (3 degrees of freedom: 7.815 at 0.95).
//
// The candidate factors are never added: the call reads the estimate and the lambda = 0 factor pps_cov_recover left in dev.L, and writes
// buffers of its own.  A query on the factor by the protocol of pps_query.h, over the 1 + n_planes distinct nodes; what is written here is the call's
// own: the argument checks, the request's candidate and measurement sections, the arguments of the gate launch (pps_gate.hip) and the decoding of
// the result ([status | d2 | best]).  Validity: that of pps_cov_block (cov_factor_current: a factor of any of the three recovery calls).
#include "pps_gate.h"
#include "pps_query.h"

using namespace pps;
using namespace pps_impl;

namespace {

const char* const kName = "association gate";
const char* const kWho = "association gate: ";

}  // namespace

extern "C" {

int pps_assoc_gate_last(const pps_graph* g, double* kernel_sec, int* launches) { return query_last(g, &pps_graph::q_assoc, kernel_sec, launches, nullptr); }

int pps_debug_assoc_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  return query_records(g, &pps_graph::q_assoc, 30, kName, 0, "", cap, rec, needed);
}

int pps_assoc_gate(pps_graph* g, int pose_id, int n_meas, const double* meas4, const double* sqrtinf_ut, int n_planes, const int* plane_ids,
                   double* d2, int* best) try {
  if (!g || !meas4 || !sqrtinf_ut || !d2 || n_meas < 0 || (plane_ids && n_planes < 0)) return PPS_EINVAL;
  if (!live_node(g, pose_id, NODE_POSE)) return fail(g, PPS_EINVAL, "association gate: node " + std::to_string(pose_id) + " is not a live pose");
  if (n_meas > 65535) return fail(g, PPS_EINVAL, "association gate: more than 65535 measurements in one call");
  // the candidates' r and Jw are the squared-error ones; with a cost function the recovered covariance is that of the robustified system
  if (robust(g)) return fail(g, PPS_ESTATE, "association gate: a robust cost function is set (pps_set_cost_function); the gate has no robustified form -- set PPS_COST_NONE and recover again");
  std::vector<int> all;
  { const int rc = plane_list(g, kWho, &plane_ids, &n_planes, &all); if (rc != PPS_OK) return rc; }
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
  // walks: the pose first, then the candidates in the order given
  std::vector<int> ids((size_t)1 + n_planes);
  ids[0] = pose_id;
  std::copy(plane_ids, plane_ids + n_planes, ids.begin() + 1);
  CovQuery q(g);
  int rc = q.build(ids); if (rc != PPS_OK) return rc;
  std::vector<GatePlane> cand((size_t)n_planes);
  for (int l = 0; l < n_planes; l++)
    cand[l] = GatePlane{q.walks[1 + l].strip, g->nodes[plane_ids[l]].slot, g->cov_rootlen[q.nd[1 + l].front], q.common_pivots(0, 1 + l), 0};
  // the request's own sections: [candidates | measurements]
  const size_t o_cand = q.add(cand.data(), cand.size() * sizeof(GatePlane)), o_meas = q.add(meas.data(), meas.size() * sizeof(double));
  const size_t n_d2 = (size_t)n_meas * n_planes, n_out = 1 + n_d2 + ((size_t)n_meas + 1) / 2;      // doubles: status | d2 | best (ints)
  rc = q.reserve(); if (rc != PPS_OK) return rc;
  QueryState& st = g->q_assoc;
  rc = query_begin(g, &st, n_out * sizeof(double), sizeof(double), (size_t)n_meas, n_d2 * 30); if (rc != PPS_OK) return rc;
  double* const out = reinterpret_cast<double*>(st.out.p);
  GateArgs ga;
  ga.planes = q.dev<GatePlane>(o_cand); ga.n_planes = n_planes;
  ga.meas = q.dev<double>(o_meas); ga.n_meas = n_meas;
  ga.strip_x = q.walks[0].strip; ga.pose_slot = g->nodes[pose_id].slot; ga.rootlen_x = g->cov_rootlen[q.nd[0].front];
  ga.K = q.K; ga.Y = g->cov_strip.p; ga.n_strip = q.n_strip;
  ga.mode = g->props.jacobian_mode;
  ga.ticket = st.ticket.p; ga.out = out; ga.rec = st.rec.p;
  rc = q.walk(out); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_assoc_gate(g->dev, ga, g->stream));
  std::vector<double> host(n_out);
  rc = q.finish(host.data(), n_out * sizeof(double), &st); if (rc != PPS_OK) return rc;
  if (host[0] >= kStatusInternal) return fail(g, PPS_EHIP, "internal error: the association gate met an index outside its front, its strip or the state arrays");
  if (host[0] != 0.0)
    return fail(g, PPS_ENOTPD, "association gate: the innovation covariance of a candidate is not positive definite (a pivot of the 3 x 3 factor was not positive or not finite)");
  query_end(&st, n_d2, 0);
  memcpy(d2, host.data() + 1, n_d2 * sizeof(double));
  if (best) memcpy(best, host.data() + 1 + n_d2, (size_t)n_meas * sizeof(int));
  return PPS_OK;
} catch (const std::bad_alloc&) {
  return query_no_memory(g, kWho);
}

}  // extern "C"
