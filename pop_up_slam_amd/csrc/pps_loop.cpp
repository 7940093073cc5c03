// pps_loop.cpp -- pps_loop_gate: the probabilistic test the pose-graph side asks before a loop closure, "is this relative-pose measurement
// between two existing poses consistent with the current estimate?".  For a list of candidates (pose a, pose b, measurement, sqrt
// information), the squared Mahalanobis distance d2 = r' (I + Jw Sigma Jw')^-1 r of every entry -- r, Jw the whitened residual and Jacobian the
// Pose3d_Pose3d_Factor of pps_add_odometry would have at the estimate, Sigma the joint marginal of (a, b) from the current factor (pps_loop.h
// has the algebra) -- and the entries below a threshold (6 degrees of freedom: 12.592 at 0.95).
//
// Nothing is added to the graph: the call reads the estimate and the lambda = 0 factor the recovery left in dev.L, and writes buffers of its
// own.  A CovQuery (pps_graph.h) over the DISTINCT poses of the list does the protocol -- one request upload, the walk launch of pps_cov_block,
// the copy back ([status | flags | d2 | S]; the n x 36 part only when the caller asks for S) --; what is written here are the argument checks,
// the request's candidate and tree sections, the arguments of the ONE candidate launch (pps_loop.hip) and the decoding of the result.  Every
// buffer that cannot be had answers PPS_ENOMEM.  Validity: that of pps_cov_block (cov_factor_current).
#include "pps_loop.h"
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void loop_release(pps_graph* g) {
  g->loop_out.release(); g->loop_rec.release();
  g->loop_rec_n = 0; g->loop_clean = false;
}

}  // namespace pps_impl

namespace {

// records are kept for calls of at most this many entries (78 doubles each: 41 MB)
constexpr int kLoopRecMaxEntries = 65536;

const char* const kWho = "loop gate: ";
const char* const kAdvice = ": list fewer candidates per call";

int loop_gate(pps_graph* g, int n, const int* pose_a, const int* pose_b, const double* meas6, const double* sqrtinf_ut, double threshold, double* d2,
              double* S, int cap_accepted, int* accepted, int* n_accepted) {
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
  const Analysis& A = g->an;
  CovQuery q(g);
  int rc = q.build(ids); if (rc != PPS_OK) return rc;
  const int n_fronts = A.n_fronts;
  if ((int)A.f_parent.size() < n_fronts || (int)g->cov_rootlen.size() < n_fronts) return fail(g, PPS_ESTATE, "loop gate: inconsistent analysis (front tables)");
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
  const size_t o_cand = q.add(cand.data(), cand.size() * sizeof(LoopCand)), o_par = q.add(A.f_parent.data(), (size_t)n_fronts * sizeof(int)),
               o_len = q.add(g->cov_rootlen.data(), (size_t)n_fronts * sizeof(int));
  // the result: [status (16 bytes) | flags: n bytes | d2: n doubles | S: n x 36 doubles]
  const size_t o_flag = 16, o_d2 = up16(o_flag + (size_t)n), o_S = up16(o_d2 + (size_t)n * sizeof(double)), n_bytes = S ? o_S + (size_t)n * 36 * sizeof(double) : o_S;
  rc = q.reserve(kWho, kAdvice); if (rc != PPS_OK) return rc;
  const size_t out_cap = g->loop_out.cap;
  rc = g->loop_out.reserve(g, n_bytes, kWho, "the result", kAdvice); if (rc != PPS_OK) return rc;
  g->loop_rec_n = 0; g->loop_done = false;
  const bool keep_rec = n <= kLoopRecMaxEntries;
  if (keep_rec) { rc = g->loop_rec.reserve(g, (size_t)n * kLoopRecord, kWho, "the records", kAdvice); if (rc != PPS_OK) return rc; }
  rc = zero_between_calls(g, &g->loop_clean, g->loop_out.p, g->loop_out.cap != out_cap, 16, nullptr, false); if (rc != PPS_OK) return rc;
  LoopArgs la;
  la.cands = q.dev<LoopCand>(o_cand); la.n = n;
  la.parent = q.dev<int>(o_par); la.rootlen = q.dev<int>(o_len); la.n_fronts = n_fronts;
  la.K = q.K; la.Y = g->cov_strip.p; la.n_strip = q.n_strip;
  la.threshold = threshold; la.mode = g->props.jacobian_mode;
  la.status = reinterpret_cast<double*>(g->loop_out.p);
  la.flag = reinterpret_cast<unsigned char*>(g->loop_out.p + o_flag);
  la.d2 = reinterpret_cast<double*>(g->loop_out.p + o_d2);
  la.S = S ? reinterpret_cast<double*>(g->loop_out.p + o_S) : nullptr;
  la.rec = keep_rec ? g->loop_rec.p : nullptr;
  std::vector<char> host(n_bytes);                       // without S nothing n x 36 comes to the host
  rc = q.walk(la.status); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_loop_gate(g->dev, la, g->stream));
  rc = q.finish(host.data(), g->loop_out.p, n_bytes, &g->loop_sec, &g->loop_launches); if (rc != PPS_OK) return rc;
  double status; memcpy(&status, host.data(), sizeof status);
  if (status != 0.0) return fail(g, PPS_EHIP, "internal error: the loop gate met an index outside its front, its strip, the tree tables or the state arrays");
  g->loop_clean = true;
  g->loop_done = true;
  g->loop_rec_n = keep_rec ? (size_t)n : 0;
  const unsigned char* flag = reinterpret_cast<const unsigned char*>(host.data() + o_flag);
  int not_pd = 0, under = 0;
  for (int k = 0; k < n; k++) {
    if (flag[k] == 2) not_pd++;
    else if (flag[k] == 1) {
      if (accepted && under < cap_accepted) accepted[under] = k;
      under++;
    }
  }
  g->loop_not_pd = not_pd;
  if (n_accepted) *n_accepted = under;
  if (d2) memcpy(d2, host.data() + o_d2, (size_t)n * sizeof(double));
  if (S) memcpy(S, host.data() + o_S, (size_t)n * 36 * sizeof(double));
  return PPS_OK;
}

}  // namespace

extern "C" {

int pps_loop_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd) {
  if (!g) return PPS_EINVAL;
  if (kernel_sec) *kernel_sec = g->loop_sec;
  if (launches) *launches = g->loop_launches;
  if (n_not_pd) *n_not_pd = g->loop_not_pd;
  return PPS_OK;
}

int pps_debug_loop_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  if (!g || !needed) return PPS_EINVAL;
  if (!g->loop_done) return fail(g, PPS_ESTATE, "no loop gate has been computed on this handle");
  if (g->loop_rec_n == 0 || !g->loop_rec.p)
    return fail(g, PPS_ESTATE, "loop gate: the records are kept for calls of at most " + std::to_string(kLoopRecMaxEntries) + " entries; the last call had more");
  return copy_records(g, g->loop_rec, g->loop_rec_n * kLoopRecord, cap, rec, needed);
}

int pps_loop_gate(pps_graph* g, int n, const int* pose_a, const int* pose_b, const double* meas6, const double* sqrtinf_ut, double threshold, double* d2,
                  double* S, int cap_accepted, int* accepted, int* n_accepted) {
  if (!g) return PPS_EINVAL;
  if (!pose_a || !pose_b || !meas6 || !sqrtinf_ut) return fail(g, PPS_EINVAL, "loop gate: pose_a, pose_b, meas6 and sqrtinf_ut must be given");
  if (n < 0) return fail(g, PPS_EINVAL, "loop gate: negative candidate count");
  if (cap_accepted < 0) return fail(g, PPS_EINVAL, "loop gate: negative cap_accepted");
  if (!d2 && !S && !accepted && !n_accepted) return fail(g, PPS_EINVAL, "loop gate: no output asked for (d2, S and accepted / n_accepted are all NULL)");
  if ((accepted && !n_accepted) || (!accepted && n_accepted && cap_accepted > 0))
    return fail(g, PPS_EINVAL, "loop gate: accepted and n_accepted go together (accepted may be NULL with cap_accepted 0: the count alone)");
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
  try {
    return loop_gate(g, n, pose_a, pose_b, meas6, sqrtinf_ut, threshold, d2, S, cap_accepted, accepted, n_accepted);
  } catch (const std::bad_alloc&) {
    return fail(g, PPS_ENOMEM, "loop gate: no host memory for the request or the result");
  }
}

}  // extern "C"
