// pps_query.cpp -- the protocol of the queries on the factor (pps_query.h) and the plainest of them:
//   pps_cov_block      Sigma(rows, cols) for ANY nodes: (L^-1 E_rows)' (L^-1 E_cols) by one walk up the elimination tree per distinct node
//                      and one Gram product over common ancestors (pps_cov.hip) -- one upload, two launches, one copy, whatever the query.
// It reads the lambda = 0 factor the recovery leaves in dev.L (pps_cov.cpp says what keeps that factor and what ends it).
#include "pps_query.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

int query_device(pps_graph* g) {
  HIP_TRY(g, hipSetDevice(g->props.device));
  for (hipEvent_t& e : g->cov_qev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  return PPS_OK;
}

int QueryTimer::start() {
  launches0 = launch_count();
  HIP_TRY(g, hipEventRecord(g->cov_qev[0], g->stream));
  return PPS_OK;
}

int QueryTimer::stop(void* host, size_t bytes, QueryState* st) {
  HIP_TRY(g, hipEventRecord(g->cov_qev[1], g->stream));
  HIP_TRY(g, hipMemcpyAsync(host, st->out.p, bytes, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  st->launches = (int)(launch_count() - launches0);
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->cov_qev[0], g->cov_qev[1]) == hipSuccess) st->sec = 1e-3 * ms;
  return PPS_OK;
}

static bool cov_walk_wide(const pps_graph* g) {
  return g->cov_path_form == 1 || cov_path_lds_bytes(g->cov_max_p, g->cov_max_rows) > (size_t)64 * 1024;
}

int CovQuery::build(const std::vector<int>& ids) {
  const Analysis& A = g->an;
  const int nw = (int)ids.size();
  nd.assign((size_t)nw, CovNode{});
  K = 0;
  for (int w = 0; w < nw; w++) {
    int rc = cov_node(g, ids[w], &nd[w]); if (rc != PPS_OK) return rc;
    rc = cov_locate(g, ids[w], &nd[w]); if (rc != PPS_OK) return rc;
    K = std::max(K, g->cov_rootlen[nd[w].front]);
  }
  walks.assign((size_t)nw, CovWalk{});
  steps.clear();
  step_end.assign((size_t)nw, 0);
  n_strip = 0;
  max_rows = 1;
  for (int w = 0; w < nw; w++) {
    walks[w] = CovWalk{n_strip, (int)steps.size(), 0, nd[w].local, nd[w].dim};
    for (int s = nd[w].front; s >= 0; s = A.f_parent[s]) {
      steps.push_back(CovStep{s, K - g->cov_rootlen[s]});
      max_rows = std::max(max_rows, A.f_p[s] + A.f_b[s]);
    }
    walks[w].n_steps = (int)steps.size() - walks[w].step0;
    step_end[w] = (int)steps.size();
    n_strip += (long long)K * nd[w].dim;
  }
  o_steps = walks.size() * sizeof(CovWalk);
  req.assign(o_steps + steps.size() * sizeof(CovStep), 0);
  if (!walks.empty()) memcpy(req.data(), walks.data(), o_steps);
  if (!steps.empty()) memcpy(req.data() + o_steps, steps.data(), steps.size() * sizeof(CovStep));
  return PPS_OK;
}

// the pivots two paths have in common are a suffix of both
int CovQuery::common_pivots(int a, int b) const {
  int len = 0;
  for (int i = step_end[a] - 1, j = step_end[b] - 1; i >= walks[a].step0 && j >= walks[b].step0 && steps[i].front == steps[j].front; i--, j--)
    len += g->an.f_p[steps[i].front];
  return len;
}

size_t CovQuery::add(const void* data, size_t bytes) {
  const size_t off = up16(req.size());
  req.resize(off + bytes, 0);
  if (bytes) memcpy(req.data() + off, data, bytes);
  return off;
}

int CovQuery::add_tree(const char* who, size_t* o_parent, size_t* o_rootlen) {
  const Analysis& A = g->an;
  const int n_fronts = A.n_fronts;
  if ((int)A.f_parent.size() < n_fronts || (int)g->cov_rootlen.size() < n_fronts) return fail(g, PPS_ESTATE, std::string(who) + "inconsistent analysis (front tables)");
  *o_parent = add(A.f_parent.data(), (size_t)n_fronts * sizeof(int));
  *o_rootlen = add(g->cov_rootlen.data(), (size_t)n_fronts * sizeof(int));
  return PPS_OK;
}

// (cov_breq / cov_strip / cov_qev are shared by all queries: every one ends with a synchronisation, none is in flight here)
int CovQuery::reserve(const char* who, const char* advice) {
  int rc = query_device(g); if (rc != PPS_OK) return rc;
  rc = g->cov_breq.reserve(g, req.size(), who, "the request", advice); if (rc != PPS_OK) return rc;
  rc = g->cov_strip.reserve(g, (size_t)n_strip, who, "the strips", advice); if (rc != PPS_OK) return rc;
  if (!cov_walk_wide(g) || walks.empty()) return PPS_OK;
  // k_cov_path_wide: its right-hand sides, before the query's upload
  const size_t want = walks.size() * cov_wide_scratch(max_rows);
  if (want <= g->cov_zscr.cap && g->cov_zscr.p) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));           // (so that what the reservation can still fail with is the allocation)
  return g->cov_zscr.reserve(g, want, "covariance path solves: ", "the right-hand sides of " + std::to_string(walks.size()) + " walks through fronts of up to " +
                                                                  std::to_string(max_rows) + " rows", ": ask for fewer nodes per call");
}

// k_cov_path where its LDS fits the graph's fronts, k_cov_path_wide otherwise (or when the handle asks for it)
int CovQuery::walk(double* status) {
  HIP_TRY(g, hipMemcpyAsync(g->cov_breq.p, req.data(), req.size(), hipMemcpyHostToDevice, g->stream));
  const int rc = timer.start(); if (rc != PPS_OK) return rc;
  const int nw = (int)walks.size(), ns = (int)steps.size();
  const CovWalk* w = dev<CovWalk>(0);
  const CovStep* s = dev<CovStep>(o_steps);
  if (cov_walk_wide(g))
    HIP_TRY(g, launch_cov_path_wide(g->dev, w, nw, s, ns, K, max_rows, g->cov_zscr.p, (long long)g->cov_zscr.cap, g->cov_strip.p, n_strip, status, g->stream));
  else
    HIP_TRY(g, launch_cov_path(g->dev, w, nw, s, ns, K, g->cov_max_p, g->cov_max_rows, g->cov_strip.p, n_strip, status, g->stream));
  return PPS_OK;
}

int query_begin(pps_graph* g, QueryState* st, size_t out_bytes, size_t status_bytes, size_t tickets, size_t rec_doubles, const char* who, const char* advice,
                const char* out_name, const char* ticket_name) {
  const size_t out_cap = st->out.cap, ticket_cap = st->ticket.cap;      // (a buffer is new when its capacity is not what it was)
  int rc = st->out.reserve(g, out_bytes, who, out_name, advice); if (rc != PPS_OK) return rc;
  if (tickets) { rc = st->ticket.reserve(g, tickets, who, ticket_name, advice); if (rc != PPS_OK) return rc; }
  st->rec_n = 0; st->done = false;
  if (rec_doubles != kNoRecords) { rc = st->rec.reserve(g, rec_doubles, who, "the records", advice); if (rc != PPS_OK) return rc; }
  // zero between calls
  if (status_bytes && (!st->clean || st->out.cap != out_cap || st->ticket.cap != ticket_cap)) {
    HIP_TRY(g, hipMemsetAsync(st->out.p, 0, status_bytes, g->stream));
    if (st->ticket.p) HIP_TRY(g, hipMemsetAsync(st->ticket.p, 0, st->ticket.cap * sizeof(unsigned int), g->stream));
  }
  st->clean = false;
  return PPS_OK;
}

int query_last(const pps_graph* g, QueryState pps_graph::*which, double* kernel_sec, int* launches, int* count) {
  if (!g) return PPS_EINVAL;
  const QueryState& st = g->*which;
  if (kernel_sec) *kernel_sec = st.sec;
  if (launches) *launches = st.launches;
  if (count) *count = st.count;
  return PPS_OK;
}

int query_records(pps_graph* g, QueryState pps_graph::*which, int unit, const char* name, long long max_entries, const char* entries, int64_t cap, double* rec,
                  int64_t* needed) {
  if (!g || !needed) return PPS_EINVAL;
  const QueryState& st = g->*which;
  if (!st.done) return fail(g, PPS_ESTATE, std::string("no ") + name + " has been computed on this handle");
  if (st.rec_n == 0 || !st.rec.p)
    return fail(g, PPS_ESTATE, std::string(name) + ": the records are kept for calls of at most " + std::to_string(max_entries) + " " + entries + "; the last call had more");
  const size_t n = st.rec_n * (size_t)unit;
  *needed = (int64_t)n;
  if (!rec || cap < *needed) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  HIP_TRY(g, hipMemcpyAsync(rec, st.rec.p, n * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  return PPS_OK;
}

int list_with_count(pps_graph* g, const char* who, const char* list_name, const void* list, const void* count, int cap) {
  if ((list && !count) || (!list && count && cap > 0)) {
    const std::string l(list_name);
    return fail(g, PPS_EINVAL, who + l + " and n_" + l + " go together (" + l + " may be NULL with cap_" + l + " 0: the count alone)");
  }
  return PPS_OK;
}

int plane_list(pps_graph* g, const char* prefix, const int** ids, int* n, std::vector<int>* all) {
  if (!*ids) {
    for (size_t i = 0; i < g->nodes.size(); i++) if (!g->nodes[i].deleted && g->nodes[i].type == NODE_PLANE) all->push_back((int)i);
    *ids = all->data(); *n = (int)all->size();
  }
  std::vector<char> seen(g->nodes.size(), 0);
  for (int i = 0; i < *n; i++) {
    const int id = (*ids)[i];
    if (!live_node(g, id, NODE_PLANE)) return fail(g, PPS_EINVAL, prefix + ("node " + std::to_string(id)) + " is not a live plane");
    if (seen[id]) return fail(g, PPS_EINVAL, prefix + ("plane " + std::to_string(id)) + " is listed twice");
    seen[id] = 1;
  }
  return PPS_OK;
}

}  // namespace pps_impl

extern "C" {

int pps_cov_block_last(const pps_graph* g, double* kernel_sec, int* launches) { return query_last(g, &pps_graph::q_block, kernel_sec, launches, nullptr); }

int pps_cov_block(pps_graph* g, int nr, const int* rows, int nc, const int* cols, double* out) try {
  if (!g || !rows || !out || nr < 0 || (cols && nc < 0)) return PPS_EINVAL;
  const bool joint = cols == nullptr;
  if (joint) { cols = rows; nc = nr; }
  // distinct nodes of the query: every one is walked once, however often it is asked for
  std::vector<int> walk_of(g->nodes.size(), -1), ids, ri((size_t)nr), ci((size_t)nc);
  for (int pass = 0; pass < (joint ? 1 : 2); pass++) {
    const int n = pass ? nc : nr;
    const int* list = pass ? cols : rows;
    std::vector<char> seen(g->nodes.size(), 0);
    for (int i = 0; i < n; i++) {
      CovNode c;
      const int rc = cov_node(g, list[i], &c); if (rc != PPS_OK) return rc;
      if (seen[list[i]]) return fail(g, PPS_EINVAL, "covariance block: node " + std::to_string(list[i]) + " is listed twice among the " + (pass ? "columns" : "rows"));
      seen[list[i]] = 1;
      if (walk_of[list[i]] < 0) { walk_of[list[i]] = (int)ids.size(); ids.push_back(list[i]); }
      (pass ? ci : ri)[i] = walk_of[list[i]];
    }
  }
  if (joint) ci = ri;
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  if (nr == 0 || nc == 0) return PPS_OK;
  CovQuery q(g);
  int rc = q.build(ids); if (rc != PPS_OK) return rc;
  const std::vector<CovNode>& nd = q.nd;
  std::vector<int> roff((size_t)nr + 1, 0), coff((size_t)nc + 1, 0);
  for (int i = 0; i < nr; i++) roff[i + 1] = roff[i] + nd[ri[i]].dim;
  for (int j = 0; j < nc; j++) coff[j + 1] = coff[j] + nd[ci[j]].dim;
  const int ld = coff[nc];
  const long long n_out = (long long)roff[nr] * ld;
  std::vector<CovPair> pairs;
  pairs.reserve(joint ? (size_t)nr * (nr + 1) / 2 : (size_t)nr * nc);
  for (int i = 0; i < nr; i++)
    for (int j = 0; j < (joint ? i + 1 : nc); j++) {
      const int a = ri[i], b = ci[j], len = q.common_pivots(a, b);
      CovPair pr;
      pr.yi = q.walks[a].strip + (long long)(q.K - len) * nd[a].dim; pr.yj = q.walks[b].strip + (long long)(q.K - len) * nd[b].dim;
      pr.dst = (long long)roff[i] * ld + coff[j];
      pr.dst_t = joint ? (long long)roff[j] * ld + coff[i] : -1;          // (cols = rows: the lower triangle, mirrored)
      pr.di = nd[a].dim; pr.dj = nd[b].dim; pr.len = len; pr.ld = ld;
      pairs.push_back(pr);
    }
  const size_t o_pairs = q.add(pairs.data(), pairs.size() * sizeof(CovPair));
  rc = q.reserve(); if (rc != PPS_OK) return rc;
  // the result: [status | the block], doubles
  QueryState& st = g->q_block;
  rc = query_begin(g, &st, ((size_t)n_out + 1) * sizeof(double), sizeof(double), 0, kNoRecords); if (rc != PPS_OK) return rc;
  double* const bout = reinterpret_cast<double*>(st.out.p);
  rc = q.walk(bout); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_cov_gram(q.dev<CovPair>(o_pairs), (int)pairs.size(), g->cov_strip.p, q.n_strip, bout, n_out, g->stream));
  std::vector<double> host((size_t)n_out + 1);
  rc = q.finish(host.data(), host.size() * sizeof(double), &st); if (rc != PPS_OK) return rc;
  if (host[0] != 0.0) return fail(g, PPS_EHIP, "internal error: a covariance path solve met an index outside its front or its strip");
  query_end(&st, 0, 0);
  memcpy(out, host.data() + 1, (size_t)n_out * sizeof(double));
  return PPS_OK;
} catch (const std::bad_alloc&) {
  return query_no_memory(g, "covariance block: ");
}

}  // extern "C"
