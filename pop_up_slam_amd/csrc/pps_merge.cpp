// pps_merge.cpp -- pps_merge_gate: the probabilistic test "are these two landmarks the same wall?".  For a list of n plane nodes, the squared
// Mahalanobis distance d2 = e' S^-1 e of every pair -- e the plane-prior residual of the first against the second's estimate, S its
// covariance under the joint marginal of the two from the current recovery (pps_merge.h has the algebra) --, the best partner per plane
// and the pairs below a threshold (3 degrees of freedom: 7.815 at 0.95).  What Mapper_mono::findLoopPlane decides by the image distance of
// end points against frame 0.
//
// Nothing is added to the graph: the call reads the estimate and the lambda = 0 factor the recovery left in dev.L, and writes buffers of its
// own.  A CovQuery (pps_graph.h) over the n planes does the protocol -- one request upload, the walk launch of pps_cov_block, the copy back
// ([status | best | flags | d2]; the n x n part only when the caller asks for d2) --; what is written here are the argument checks, the
// request's plane and tree sections, the arguments of the ONE pair launch (pps_merge.hip) and the decoding of the result.  Every buffer that
// cannot be had answers PPS_ENOMEM.  Validity: that of pps_cov_block (cov_factor_current).
#include "pps_merge.h"
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void merge_release(pps_graph* g) {
  g->merge_out.release(); g->merge_ticket.release(); g->merge_rec.release();
  g->merge_rec_n = 0; g->merge_clean = false;
}

}  // namespace pps_impl

namespace {

// records are kept for calls of at most this many pairs (21 doubles each: 44 MB)
constexpr long long kMergeRecMaxPairs = 1 << 18;

// a device buffer of the call: PPS_ENOMEM, never PPS_EHIP, when it cannot be had
const char* const kWho = "merge gate: ";
const char* const kAdvice = ": list fewer planes per call";

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
  if (g->merge_rec_n == 0 || !g->merge_rec.p)
    return fail(g, PPS_ESTATE, "merge gate: the records are kept for calls of at most " + std::to_string(kMergeRecMaxPairs) + " pairs; the last call had more");
  return copy_records(g, g->merge_rec, g->merge_rec_n * kMergeRecord, cap, rec, needed);
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
  { const int rc = plane_list(g, kWho, &plane_ids, &n_planes, &all); if (rc != PPS_OK) return rc; }
  if (n_planes > 65535) return fail(g, PPS_EINVAL, "merge gate: more than 65535 planes in one call");
  if (n_planes < 2) return PPS_OK;                       // no pair: the outputs stay untouched, the recovery is not looked at
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  const int n = n_planes;
  const long long P = (long long)n * (n - 1) / 2;
  const Analysis& A = g->an;
  const std::vector<int> ids(plane_ids, plane_ids + n);
  CovQuery q(g);
  int rc = q.build(ids); if (rc != PPS_OK) return rc;
  const int n_fronts = A.n_fronts;
  if ((int)A.f_parent.size() < n_fronts || (int)g->cov_rootlen.size() < n_fronts) return fail(g, PPS_ESTATE, "merge gate: inconsistent analysis (front tables)");
  std::vector<MergePlane> pl((size_t)n);
  for (int l = 0; l < n; l++) pl[l] = MergePlane{q.walks[l].strip, g->nodes[ids[l]].slot, q.nd[l].front};
  // the request's own sections: [planes | parent | rootlen]
  const size_t o_pl = q.add(pl.data(), pl.size() * sizeof(MergePlane)), o_par = q.add(A.f_parent.data(), (size_t)n_fronts * sizeof(int)),
               o_len = q.add(g->cov_rootlen.data(), (size_t)n_fronts * sizeof(int));
  // the result: [status (16 bytes) | best: n ints | flags: P bytes | d2: n x n doubles]
  const size_t o_best = 16, o_flag = o_best + (size_t)n * sizeof(int), o_d2 = up16(o_flag + (size_t)P), n_bytes = o_d2 + (size_t)n * n * sizeof(double);
  rc = q.reserve(kWho, kAdvice); if (rc != PPS_OK) return rc;
  const size_t out_cap = g->merge_out.cap, ticket_cap = g->merge_ticket.cap;
  rc = g->merge_out.reserve(g, n_bytes, kWho, "the n x n result", kAdvice); if (rc != PPS_OK) return rc;
  rc = g->merge_ticket.reserve(g, (size_t)n, kWho, "the row tickets", kAdvice); if (rc != PPS_OK) return rc;
  g->merge_rec_n = 0; g->merge_done = false;
  const bool keep_rec = P <= kMergeRecMaxPairs;
  if (keep_rec) { rc = g->merge_rec.reserve(g, (size_t)P * kMergeRecord, kWho, "the records", kAdvice); if (rc != PPS_OK) return rc; }
  rc = zero_between_calls(g, &g->merge_clean, g->merge_out.p, g->merge_out.cap != out_cap, 16, &g->merge_ticket, g->merge_ticket.cap != ticket_cap);
  if (rc != PPS_OK) return rc;
  MergeArgs ma;
  ma.planes = q.dev<MergePlane>(o_pl); ma.n = n; ma.n_pairs = P;
  ma.parent = q.dev<int>(o_par); ma.rootlen = q.dev<int>(o_len); ma.n_fronts = n_fronts;
  ma.K = q.K; ma.Y = g->cov_strip.p; ma.n_strip = q.n_strip;
  ma.floor_var = floor_var; ma.threshold = threshold;
  ma.ticket = g->merge_ticket.p; ma.status = reinterpret_cast<double*>(g->merge_out.p);
  ma.best = reinterpret_cast<int*>(g->merge_out.p + o_best); ma.flag = reinterpret_cast<unsigned char*>(g->merge_out.p + o_flag);
  ma.d2 = reinterpret_cast<double*>(g->merge_out.p + o_d2);
  ma.rec = keep_rec ? g->merge_rec.p : nullptr;
  rc = q.walk(ma.status); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_merge_gate(g->dev, ma, g->stream));
  const size_t n_copy = d2 ? n_bytes : o_d2;             // without d2 nothing n x n comes to the host
  std::vector<char> host;
  try { host.resize(n_copy); } catch (const std::bad_alloc&) { return fail(g, PPS_ENOMEM, "merge gate: no host memory for the result"); }
  rc = q.finish(host.data(), g->merge_out.p, n_copy, &g->merge_sec, &g->merge_launches); if (rc != PPS_OK) return rc;
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
