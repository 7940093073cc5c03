// pps_loop.cpp -- pps_loop_gate: the probabilistic test the pose-graph side asks before a loop closure, "is this relative-pose measurement
// between two existing poses consistent with the current estimate?".  For a list of candidates (pose a, pose b, measurement, sqrt
// information), the squared Mahalanobis distance d2 = r' (I + Jw Sigma Jw')^-1 r of every entry -- r, Jw the whitened residual and Jacobian the
// Pose3d_Pose3d_Factor of pps_add_odometry would have at the estimate, Sigma the joint marginal of (a, b) from the current factor (pps_loop.h
// has the algebra) -- and the entries below a threshold (6 degrees of freedom: 12.592 at 0.95).
//
// Nothing is added to the graph: the call reads the estimate and the lambda = 0 factor the recovery left in dev.L, and writes buffers of its
// own.  A query on the factor by the protocol of pps_query.h, over the DISTINCT poses of the list; what is written here is the call's own: the
// argument checks, the request's candidate section (and the tree's), the arguments of the ONE candidate launch (pps_loop.hip) and the decoding of
// the result ([status | flags | d2 | S]; the n x 36 part exists only when the caller asks for S).  Every buffer that cannot be had answers
// PPS_ENOMEM.  Validity: that of pps_cov_block (cov_factor_current).
#include "pps_loop.h"
#include "pps_query.h"

using namespace pps;
using namespace pps_impl;

namespace {

// records are kept for calls of at most this many entries (78 doubles each: 41 MB)
constexpr int kLoopRecMaxEntries = 65536;

const char* const kName = "loop gate";
const char* const kWho = "loop gate: ";
const char* const kAdvice = ": list fewer candidates per call";

}  // namespace

extern "C" {

int pps_loop_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd) {
  return query_last(g, &pps_graph::q_loop, kernel_sec, launches, n_not_pd);
}

int pps_debug_loop_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  return query_records(g, &pps_graph::q_loop, kLoopRecord, kName, kLoopRecMaxEntries, "entries", cap, rec, needed);
}

int pps_loop_gate(pps_graph* g, int n, const int* pose_a, const int* pose_b, const double* meas6, const double* sqrtinf_ut, double threshold, double* d2,
                  double* S, int cap_accepted, int* accepted, int* n_accepted) try {
  if (!g) return PPS_EINVAL;
  if (!pose_a || !pose_b || !meas6 || !sqrtinf_ut) return fail(g, PPS_EINVAL, "loop gate: pose_a, pose_b, meas6 and sqrtinf_ut must be given");
  if (n < 0) return fail(g, PPS_EINVAL, "loop gate: negative candidate count");
  if (cap_accepted < 0) return fail(g, PPS_EINVAL, "loop gate: negative cap_accepted");
  if (!d2 && !S && !accepted && !n_accepted) return fail(g, PPS_EINVAL, "loop gate: no output asked for (d2, S and accepted / n_accepted are all NULL)");
  { const int rc = list_with_count(g, kWho, "accepted", accepted, n_accepted, cap_accepted); if (rc != PPS_OK) return rc; }
  if (n_accepted && !std::isfinite(threshold)) return fail(g, PPS_EINVAL, "loop gate: threshold must be finite");
  for (int k = 0; k < n; k++) {
    for (int i = 0; i < 6; i++) if (!std::isfinite(meas6[(size_t)k * 6 + i])) return fail(g, PPS_EINVAL, "loop gate: non-finite measurement");
    for (int i = 0; i < 21; i++) if (!std::isfinite(sqrtinf_ut[(size_t)k * 21 + i])) return fail(g, PPS_EINVAL, "loop gate: non-finite sqrtinf");
    for (const int id : {pose_a[k], pose_b[k]})
      if (!live_node(g, id, NODE_POSE)) return fail(g, PPS_EINVAL, "loop gate: node " + std::to_string(id) + " is not a live pose");
    if (pose_a[k] == pose_b[k]) return fail(g, PPS_EINVAL, "loop gate: candidate " + std::to_string(k) + " joins pose " + std::to_string(pose_a[k]) + " with itself");
  }
  if (n == 0) return PPS_OK;                               // nothing asked for: the outputs stay untouched, the recovery is not looked at
  // the candidates' r and Jw are the squared-error ones; with a cost function the recovered covariance is that of the robustified system
  if (robust(g)) return fail(g, PPS_ESTATE, "loop gate: a robust cost function is set (pps_set_cost_function); the gate has no robustified form -- set PPS_COST_NONE and recover again");
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  // the distinct poses in the order they first appear, and per candidate its two walk indices
  std::vector<int> ids, wa((size_t)n), wb((size_t)n);
  { std::unordered_map<int, int> walk_of;
    const auto walk_index = [&](int id) {
      const auto it = walk_of.find(id);
      if (it != walk_of.end()) return it->second;
      ids.push_back(id);
      return walk_of[id] = (int)ids.size() - 1;
    };
    for (int k = 0; k < n; k++) { wa[k] = walk_index(pose_a[k]); wb[k] = walk_index(pose_b[k]); } }
  CovQuery q(g);
  int rc = q.build(ids); if (rc != PPS_OK) return rc;
  std::vector<LoopCand> cand((size_t)n);
  for (int k = 0; k < n; k++) {
    LoopCand& c = cand[k];
    c.strip_a = q.walks[wa[k]].strip; c.strip_b = q.walks[wb[k]].strip;
    c.slot_a = g->nodes[pose_a[k]].slot; c.slot_b = g->nodes[pose_b[k]].slot;
    c.front_a = q.nd[wa[k]].front; c.front_b = q.nd[wb[k]].front;
    // the measurement as pps_add_odometry stores it: the six numbers as given (the angles are wrapped where the residual is taken)
    for (int i = 0; i < 6; i++) c.meas[i] = meas6[(size_t)k * 6 + i];
    for (int i = 0; i < 21; i++) c.sw[i] = sqrtinf_ut[(size_t)k * 21 + i];
  }
  // the request's own sections: [candidates | parent | rootlen]
  const size_t o_cand = q.add(cand.data(), cand.size() * sizeof(LoopCand));
  size_t o_par = 0, o_len = 0;
  rc = q.add_tree(kWho, &o_par, &o_len); if (rc != PPS_OK) return rc;
  // the result: [status (16 bytes) | flags: n bytes | d2: n doubles | S: n x 36 doubles]
  const size_t o_flag = 16, o_d2 = up16(o_flag + (size_t)n), o_S = up16(o_d2 + (size_t)n * sizeof(double)), n_bytes = S ? o_S + (size_t)n * 36 * sizeof(double) : o_S;
  rc = q.reserve(kWho, kAdvice); if (rc != PPS_OK) return rc;
  const bool keep_rec = n <= kLoopRecMaxEntries;
  QueryState& st = g->q_loop;
  rc = query_begin(g, &st, n_bytes, 16, 0, keep_rec ? (size_t)n * kLoopRecord : kNoRecords, kWho, kAdvice); if (rc != PPS_OK) return rc;
  LoopArgs la;
  la.cands = q.dev<LoopCand>(o_cand); la.n = n;
  la.parent = q.dev<int>(o_par); la.rootlen = q.dev<int>(o_len); la.n_fronts = g->an.n_fronts;
  la.K = q.K; la.Y = g->cov_strip.p; la.n_strip = q.n_strip;
  la.threshold = threshold; la.mode = g->props.jacobian_mode;
  la.status = reinterpret_cast<double*>(st.out.p);
  la.flag = reinterpret_cast<unsigned char*>(st.out.p + o_flag);
  la.d2 = reinterpret_cast<double*>(st.out.p + o_d2);
  la.S = S ? reinterpret_cast<double*>(st.out.p + o_S) : nullptr;
  la.rec = keep_rec ? st.rec.p : nullptr;
  std::vector<char> host(n_bytes);                       // without S nothing n x 36 comes to the host
  rc = q.walk(la.status); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_loop_gate(g->dev, la, g->stream));
  rc = q.finish(host.data(), n_bytes, &st); if (rc != PPS_OK) return rc;
  double status; memcpy(&status, host.data(), sizeof status);
  if (status != 0.0) return fail(g, PPS_EHIP, "internal error: the loop gate met an index outside its front, its strip, the tree tables or the state arrays");
  int not_pd = 0;
  const long long under = decode_flags(reinterpret_cast<const unsigned char*>(host.data() + o_flag), n, &not_pd, [&](long long k, long long at) {
    if (accepted && at < cap_accepted) accepted[at] = (int)k;
  });
  query_end(&st, keep_rec ? (size_t)n : 0, not_pd);
  if (n_accepted) *n_accepted = (int)under;
  if (d2) memcpy(d2, host.data() + o_d2, (size_t)n * sizeof(double));
  if (S) memcpy(S, host.data() + o_S, (size_t)n * 36 * sizeof(double));
  return PPS_OK;
} catch (const std::bad_alloc&) {
  return query_no_memory(g, kWho);
}

}  // extern "C"
