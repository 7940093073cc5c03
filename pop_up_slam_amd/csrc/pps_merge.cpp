// pps_merge.cpp -- pps_merge_gate: the probabilistic test "are these two landmarks the same wall?".  For a list of n plane nodes, the squared
// Mahalanobis distance d2 = e' S^-1 e of every pair -- e the plane-prior residual of the first against the second's estimate, S its
// covariance under the joint marginal of the two from the current recovery (pps_merge.h has the algebra) --, the best partner per plane
// and the pairs below a threshold (3 degrees of freedom: 7.815 at 0.95).  What Mapper_mono::findLoopPlane decides by the image distance of
// end points against frame 0.
//
// Nothing is added to the graph: the call reads the estimate and the lambda = 0 factor the recovery left in dev.L, and writes buffers of its
// own.  One request upload, the walk launch of pps_cov_block for the n planes, ONE pair launch (pps_merge.hip), one copy back
// ([status | best | flags | d2]; the n x n part only when the caller asks for d2).  Validity: that of pps_cov_block (cov_factor_current).
#include "pps_merge.h"
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void merge_release(pps_graph* g) {
  if (g->merge_out) (void)hipFree(g->merge_out);
  if (g->merge_ticket) (void)hipFree(g->merge_ticket);
  if (g->merge_rec) (void)hipFree(g->merge_rec);
  for (hipEvent_t& e : g->merge_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  g->merge_out = nullptr; g->merge_ticket = nullptr; g->merge_rec = nullptr;
  g->merge_out_cap = g->merge_ticket_cap = g->merge_rec_cap = 0; g->merge_rec_n = 0; g->merge_clean = false;
}

}  // namespace pps_impl

namespace {

// records are kept for calls of at most this many pairs (21 doubles each: 44 MB)
constexpr long long kMergeRecMaxPairs = 1 << 18;

// a device buffer of the call: PPS_ENOMEM, never PPS_EHIP, when it cannot be had
template <class T>
int merge_reserve(pps_graph* g, T** buf, size_t* cap, size_t count, const char* what) {
  if (cov_reserve(g, buf, cap, count) == PPS_OK) return PPS_OK;
  (void)hipGetLastError();
  return fail(g, PPS_ENOMEM, std::string("merge gate: no device memory for ") + what + " (" + std::to_string(count * sizeof(T)) + " bytes): list fewer planes per call");
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int pps_merge_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd) {
  if (!g) return PPS_EINVAL;
  if (kernel_sec) *kernel_sec = g->merge_sec;
  if (launches) *launches = g->merge_launches;
  if (n_not_pd) *n_not_pd = g->merge_not_pd;
  return PPS_OK;
}

int pps_debug_merge_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  if (!g || !needed) return PPS_EINVAL;
  if (!g->merge_done) return fail(g, PPS_ESTATE, "no merge gate has been computed on this handle");
  if (g->merge_rec_n == 0 || !g->merge_rec)
    return fail(g, PPS_ESTATE, "merge gate: the records are kept for calls of at most " + std::to_string(kMergeRecMaxPairs) + " pairs; the last call had more");
  *needed = (int64_t)g->merge_rec_n * kMergeRecord;
  if (!rec || cap < *needed) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  HIP_TRY(g, hipMemcpyAsync(rec, g->merge_rec, (size_t)*needed * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  return PPS_OK;
}

int pps_merge_gate(pps_graph* g, int n_planes, const int* plane_ids, double floor_var, double threshold, double* d2, int* best, int cap_pairs,
                   int* pairs, int* n_pairs) {
  if (!g) return PPS_EINVAL;
  if (plane_ids && n_planes < 0) return fail(g, PPS_EINVAL, "merge gate: negative plane count");
  if (cap_pairs < 0) return fail(g, PPS_EINVAL, "merge gate: negative cap_pairs");
  if (!std::isfinite(floor_var) || floor_var < 0.0) return fail(g, PPS_EINVAL, "merge gate: floor_var must be finite and not negative");
  if (!std::isfinite(threshold)) return fail(g, PPS_EINVAL, "merge gate: threshold must be finite");
  if (!d2 && !best && !pairs && !n_pairs) return fail(g, PPS_EINVAL, "merge gate: no output asked for (d2, best and pairs / n_pairs are all NULL)");
  if ((pairs && !n_pairs) || (!pairs && n_pairs && cap_pairs > 0))
    return fail(g, PPS_EINVAL, "merge gate: pairs and n_pairs go together (pairs may be NULL with cap_pairs 0: the count alone)");
  std::vector<int> all;
  if (!plane_ids) {
    for (size_t i = 0; i < g->nodes.size(); i++) if (!g->nodes[i].deleted && g->nodes[i].type == NODE_PLANE) all.push_back((int)i);
    plane_ids = all.data(); n_planes = (int)all.size();
  }
  { std::vector<char> seen(g->nodes.size(), 0);
    for (int i = 0; i < n_planes; i++) {
      const int id = plane_ids[i];
      if (!live_node(g, id, NODE_PLANE)) return fail(g, PPS_EINVAL, "merge gate: node " + std::to_string(id) + " is not a live plane");
      if (seen[id]) return fail(g, PPS_EINVAL, "merge gate: plane " + std::to_string(id) + " is listed twice");
      seen[id] = 1;
    } }
  if (n_planes > 65535) return fail(g, PPS_EINVAL, "merge gate: more than 65535 planes in one call");
  if (n_planes < 2) return PPS_OK;                       // no pair: the outputs stay untouched, the recovery is not looked at
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  const int n = n_planes;
  const long long P = (long long)n * (n - 1) / 2;
  const Analysis& A = g->an;
  std::vector<int> ids(plane_ids, plane_ids + n);
  std::vector<CovNode> nd((size_t)n);
  for (int w = 0; w < n; w++) { const int rc = cov_node(g, ids[w], &nd[w]); if (rc != PPS_OK) return rc; }
  CovWalks cw;
  { const int rc = cov_build_walks(g, ids, nd, &cw); if (rc != PPS_OK) return rc; }
  const int n_fronts = A.n_fronts;
  if ((int)A.f_parent.size() < n_fronts || (int)g->cov_rootlen.size() < n_fronts) return fail(g, PPS_ESTATE, "merge gate: inconsistent analysis (front tables)");
  std::vector<MergePlane> pl((size_t)n);
  for (int l = 0; l < n; l++) pl[l] = MergePlane{cw.walks[l].strip, g->nodes[ids[l]].slot, nd[l].front};
  // one request: [walks | steps | planes | parent | rootlen]
  const size_t o_steps = cw.walks.size() * sizeof(CovWalk), o_pl = up16(o_steps + cw.steps.size() * sizeof(CovStep)),
               o_par = up16(o_pl + pl.size() * sizeof(MergePlane)), o_len = up16(o_par + (size_t)n_fronts * sizeof(int));
  std::vector<char> req(o_len + (size_t)n_fronts * sizeof(int));
  memcpy(req.data(), cw.walks.data(), cw.walks.size() * sizeof(CovWalk));
  memcpy(req.data() + o_steps, cw.steps.data(), cw.steps.size() * sizeof(CovStep));
  memcpy(req.data() + o_pl, pl.data(), pl.size() * sizeof(MergePlane));
  memcpy(req.data() + o_par, A.f_parent.data(), (size_t)n_fronts * sizeof(int));
  memcpy(req.data() + o_len, g->cov_rootlen.data(), (size_t)n_fronts * sizeof(int));
  // the result: [status (16 bytes) | best: n ints | flags: P bytes | d2: n x n doubles]
  const size_t o_best = 16, o_flag = o_best + (size_t)n * sizeof(int), o_d2 = up16(o_flag + (size_t)P), n_bytes = o_d2 + (size_t)n * n * sizeof(double);
  HIP_TRY(g, hipSetDevice(g->props.device));
  for (hipEvent_t& e : g->merge_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  // (cov_breq / cov_strip are shared with pps_cov_block and pps_assoc_gate: every such call ends with a synchronisation, none is in flight here)
  int rc = merge_reserve(g, &g->cov_breq, &g->cov_breq_cap, req.size(), "the request"); if (rc != PPS_OK) return rc;
  rc = merge_reserve(g, &g->cov_strip, &g->cov_strip_cap, (size_t)cw.n_strip, "the strips"); if (rc != PPS_OK) return rc;
  rc = cov_walk_scratch(g, cw); if (rc != PPS_OK) return rc;
  const char* out0 = g->merge_out; const unsigned int* ticket0 = g->merge_ticket;
  rc = merge_reserve(g, &g->merge_out, &g->merge_out_cap, n_bytes, "the n x n result"); if (rc != PPS_OK) return rc;
  rc = merge_reserve(g, &g->merge_ticket, &g->merge_ticket_cap, (size_t)n, "the row tickets"); if (rc != PPS_OK) return rc;
  g->merge_rec_n = 0; g->merge_done = false;
  const bool keep_rec = P <= kMergeRecMaxPairs;
  if (keep_rec) { rc = merge_reserve(g, &g->merge_rec, &g->merge_rec_cap, (size_t)P * kMergeRecord, "the records"); if (rc != PPS_OK) return rc; }
  const bool fresh = !g->merge_clean || g->merge_out != out0 || g->merge_ticket != ticket0 || !out0 || !ticket0;
  if (fresh) {                                           // (a new buffer, or a call that failed)
    HIP_TRY(g, hipMemsetAsync(g->merge_out, 0, 16, g->stream));
    HIP_TRY(g, hipMemsetAsync(g->merge_ticket, 0, g->merge_ticket_cap * sizeof(unsigned int), g->stream));
  }
  g->merge_clean = false;
  MergeArgs ma;
  ma.planes = reinterpret_cast<const MergePlane*>(g->cov_breq + o_pl); ma.n = n; ma.n_pairs = P;
  ma.parent = reinterpret_cast<const int*>(g->cov_breq + o_par); ma.rootlen = reinterpret_cast<const int*>(g->cov_breq + o_len); ma.n_fronts = n_fronts;
  ma.K = cw.K; ma.Y = g->cov_strip; ma.n_strip = cw.n_strip;
  ma.floor_var = floor_var; ma.threshold = threshold;
  ma.ticket = g->merge_ticket; ma.status = reinterpret_cast<double*>(g->merge_out);
  ma.best = reinterpret_cast<int*>(g->merge_out + o_best); ma.flag = reinterpret_cast<unsigned char*>(g->merge_out + o_flag);
  ma.d2 = reinterpret_cast<double*>(g->merge_out + o_d2);
  ma.rec = keep_rec ? g->merge_rec : nullptr;
  const unsigned long long launches0 = launch_count();
  HIP_TRY(g, hipMemcpyAsync(g->cov_breq, req.data(), req.size(), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, hipEventRecord(g->merge_ev[0], g->stream));
  HIP_TRY(g, cov_launch_walks(g, cw, reinterpret_cast<const CovWalk*>(g->cov_breq), reinterpret_cast<const CovStep*>(g->cov_breq + o_steps), ma.status));
  HIP_TRY(g, launch_merge_gate(g->dev, ma, g->stream));
  HIP_TRY(g, hipEventRecord(g->merge_ev[1], g->stream));
  const size_t n_copy = d2 ? n_bytes : o_d2;             // without d2 nothing n x n comes to the host
  std::vector<char> host;
  try { host.resize(n_copy); } catch (const std::bad_alloc&) { return fail(g, PPS_ENOMEM, "merge gate: no host memory for the result"); }
  HIP_TRY(g, hipMemcpyAsync(host.data(), g->merge_out, n_copy, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  g->merge_launches = (int)(launch_count() - launches0);
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->merge_ev[0], g->merge_ev[1]) == hipSuccess) g->merge_sec = 1e-3 * ms;
  double status; memcpy(&status, host.data(), sizeof status);
  if (status != 0.0) return fail(g, PPS_EHIP, "internal error: the merge gate met an index outside its front, its strip, the tree tables or the state arrays");
  g->merge_clean = true;
  g->merge_done = true;
  g->merge_rec_n = keep_rec ? (size_t)P : 0;
  const unsigned char* flag = reinterpret_cast<const unsigned char*>(host.data() + o_flag);
  int not_pd = 0;
  long long under = 0;
  { long long p = 0;                                     // the linear pair index runs in (i, j) order
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++, p++) {
        if (flag[p] == 2) not_pd++;
        else if (flag[p] == 1) {
          if (pairs && under < cap_pairs) { pairs[2 * under] = i; pairs[2 * under + 1] = j; }
          under++;
        }
      } }
  g->merge_not_pd = not_pd;
  if (n_pairs) *n_pairs = (int)std::min<long long>(under, 2147483647LL);
  if (best) memcpy(best, host.data() + o_best, (size_t)n * sizeof(int));
  if (d2) memcpy(d2, host.data() + o_d2, (size_t)n * n * sizeof(double));
  return PPS_OK;
}

}  // extern "C"
