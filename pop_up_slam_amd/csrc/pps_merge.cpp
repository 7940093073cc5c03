// pps_merge.cpp -- pps_merge_gate: the probabilistic test "are these two landmarks the same wall?".  For a list of n plane nodes, the squared
// Mahalanobis distance d2 = e' S^-1 e of every pair -- e the plane-prior residual of the first against the second's estimate, S its
// covariance under the joint marginal of the two from the current recovery (pps_merge.h has the algebra) --, the best partner per plane
// and the pairs below a threshold (3 degrees of freedom: 7.815 at 0.95).  What Mapper_mono::findLoopPlane decides by the image distance of
// end points against frame 0.
//
// Nothing is added to the graph: the call reads the estimate and the lambda = 0 factor the recovery left in dev.L, and writes buffers of its
// own.  A query on the factor by the protocol of pps_query.h, over the n planes; what is written here is the call's own: the argument checks,
// the request's plane section (and the tree's), the arguments of the ONE pair launch (pps_merge.hip) and the decoding of the result ([status |
// best | flags | d2]; the n x n part comes to the host only when the caller asks for d2).  Every buffer that cannot be had answers PPS_ENOMEM.
// Validity: that of pps_cov_block (cov_factor_current).
#include "pps_merge.h"
#include "pps_query.h"

using namespace pps;
using namespace pps_impl;

namespace {

// records are kept for calls of at most this many pairs (21 doubles each: 44 MB)
constexpr long long kMergeRecMaxPairs = 1 << 18;

const char* const kName = "merge gate";
const char* const kWho = "merge gate: ";
const char* const kAdvice = ": list fewer planes per call";

}  // namespace

extern "C" {

int pps_merge_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_not_pd) {
  return query_last(g, &pps_graph::q_merge, kernel_sec, launches, n_not_pd);
}

int pps_debug_merge_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  return query_records(g, &pps_graph::q_merge, kMergeRecord, kName, kMergeRecMaxPairs, "pairs", cap, rec, needed);
}

int pps_merge_gate(pps_graph* g, int n_planes, const int* plane_ids, double floor_var, double threshold, double* d2, int* best, int cap_pairs,
                   int* pairs, int* n_pairs) try {
  if (!g) return PPS_EINVAL;
  if (plane_ids && n_planes < 0) return fail(g, PPS_EINVAL, "merge gate: negative plane count");
  if (cap_pairs < 0) return fail(g, PPS_EINVAL, "merge gate: negative cap_pairs");
  if (!std::isfinite(floor_var) || floor_var < 0.0) return fail(g, PPS_EINVAL, "merge gate: floor_var must be finite and not negative");
  if (!std::isfinite(threshold)) return fail(g, PPS_EINVAL, "merge gate: threshold must be finite");
  if (!d2 && !best && !pairs && !n_pairs) return fail(g, PPS_EINVAL, "merge gate: no output asked for (d2, best and pairs / n_pairs are all NULL)");
  int rc = list_with_count(g, kWho, "pairs", pairs, n_pairs, cap_pairs); if (rc != PPS_OK) return rc;
  std::vector<int> all;
  rc = plane_list(g, kWho, &plane_ids, &n_planes, &all); if (rc != PPS_OK) return rc;
  if (n_planes > 65535) return fail(g, PPS_EINVAL, "merge gate: more than 65535 planes in one call");
  if (n_planes < 2) return PPS_OK;                       // no pair: the outputs stay untouched, the recovery is not looked at
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  const int n = n_planes;
  const long long P = (long long)n * (n - 1) / 2;
  const std::vector<int> ids(plane_ids, plane_ids + n);
  CovQuery q(g);
  rc = q.build(ids); if (rc != PPS_OK) return rc;
  std::vector<MergePlane> pl((size_t)n);
  for (int l = 0; l < n; l++) pl[l] = MergePlane{q.walks[l].strip, g->nodes[ids[l]].slot, q.nd[l].front};
  // the request's own sections: [planes | parent | rootlen]
  const size_t o_pl = q.add(pl.data(), pl.size() * sizeof(MergePlane));
  size_t o_par = 0, o_len = 0;
  rc = q.add_tree(kWho, &o_par, &o_len); if (rc != PPS_OK) return rc;
  // the result: [status (16 bytes) | best: n ints | flags: P bytes | d2: n x n doubles]
  const size_t o_best = 16, o_flag = o_best + (size_t)n * sizeof(int), o_d2 = up16(o_flag + (size_t)P), n_bytes = o_d2 + (size_t)n * n * sizeof(double);
  rc = q.reserve(kWho, kAdvice); if (rc != PPS_OK) return rc;
  const bool keep_rec = P <= kMergeRecMaxPairs;
  QueryState& st = g->q_merge;
  rc = query_begin(g, &st, n_bytes, 16, (size_t)n, keep_rec ? (size_t)P * kMergeRecord : kNoRecords, kWho, kAdvice, "the n x n result", "the row tickets");
  if (rc != PPS_OK) return rc;
  MergeArgs ma;
  ma.planes = q.dev<MergePlane>(o_pl); ma.n = n; ma.n_pairs = P;
  ma.parent = q.dev<int>(o_par); ma.rootlen = q.dev<int>(o_len); ma.n_fronts = g->an.n_fronts;
  ma.K = q.K; ma.Y = g->cov_strip.p; ma.n_strip = q.n_strip;
  ma.floor_var = floor_var; ma.threshold = threshold;
  ma.ticket = st.ticket.p; ma.status = reinterpret_cast<double*>(st.out.p);
  ma.best = reinterpret_cast<int*>(st.out.p + o_best); ma.flag = reinterpret_cast<unsigned char*>(st.out.p + o_flag);
  ma.d2 = reinterpret_cast<double*>(st.out.p + o_d2);
  ma.rec = keep_rec ? st.rec.p : nullptr;
  rc = q.walk(ma.status); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_merge_gate(g->dev, ma, g->stream));
  const size_t n_copy = d2 ? n_bytes : o_d2;             // without d2 nothing n x n comes to the host
  std::vector<char> host(n_copy);
  rc = q.finish(host.data(), n_copy, &st); if (rc != PPS_OK) return rc;
  double status; memcpy(&status, host.data(), sizeof status);
  if (status != 0.0) return fail(g, PPS_EHIP, "internal error: the merge gate met an index outside its front, its strip, the tree tables or the state arrays");
  int not_pd = 0, i = 0;
  long long row0 = 0;                                    // the linear pair index runs in (i, j) order: row i holds the pairs [row0, row0 + n - 1 - i)
  const long long under = decode_flags(reinterpret_cast<const unsigned char*>(host.data() + o_flag), P, &not_pd, [&](long long p, long long k) {
    while (p >= row0 + (n - 1 - i)) { row0 += n - 1 - i; i++; }
    if (pairs && k < cap_pairs) { pairs[2 * k] = i; pairs[2 * k + 1] = i + 1 + (int)(p - row0); }
  });
  query_end(&st, keep_rec ? (size_t)P : 0, not_pd);
  if (n_pairs) *n_pairs = (int)std::min<long long>(under, 2147483647LL);
  if (best) memcpy(best, host.data() + o_best, (size_t)n * sizeof(int));
  if (d2) memcpy(d2, host.data() + o_d2, (size_t)n * n * sizeof(double));
  return PPS_OK;
} catch (const std::bad_alloc&) {
  return query_no_memory(g, kWho);
}

}  // extern "C"
