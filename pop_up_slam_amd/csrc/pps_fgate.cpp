// pps_fgate.cpp -- pps_factor_gate: the question a plane-SLAM front end asks after a solve, "which factor already in the graph is wrong?".
// For a list of factor ids (or all live factors), d2 = r' (I - P)^-1 r and lev = trace(P), P = J Sigma_ff J', of every entry -- r, J the
// whitened residual and Jacobian of the factor at the estimate, Sigma_ff the joint marginal of its nodes (pps_fgate.h has the algebra) -- and
// the entries whose finite d2 exceeds the chi-square threshold of their dimension (7.815 for m = 3, 12.592 for m = 6 at 0.95).
//
// Nothing is added to the graph: the call reads the estimate and the selected inverse a recovery left in cov_S, and writes buffers of its
// own.  Every pair joined by a factor lies in the pattern of L, so the three blocks of Sigma_ff are looked up like pps_cov_access looks its
// blocks up (cov_locate, cov_request) -- once per analysis: the table of all factors stays on the device until the next upload, a second
// call after the same recovery uploads the fid list alone.  ONE launch (pps_fgate.hip), one copy back ([d2 | lev | status]); the flagged
// list and the count of untestable entries are made on the host from it.  The call state, the timed launch and the _last / _records entry points
// are those of the queries on the factor (pps_query.h), without a walk; what is written here is the call's own: the argument checks, the table,
// the kernel's arguments and the decoding of the result.  Validity: that of pps_cov_marginals (cov_current: the selected inverse of
// pps_cov_recover or pps_cov_select).
#include "pps_fgate.h"
#include "pps_query.h"

using namespace pps;
using namespace pps_impl;

namespace {

// records are kept for calls of at most this many entries (78 doubles each: 41 MB)
constexpr int kFgateRecMaxEntries = 65536;

const char* const kName = "factor gate";
const char* const kWho = "factor gate: ";
const char* const kAdvice = ": list fewer factors per call";

bool live_factor(const pps_graph* g, int fid) { return fid >= 0 && fid < (int)g->factors.size() && !g->factors[fid].deleted; }

// does block (dr x dc) of a request stay inside the selected inverse?
bool inside(const CovReq& q, long long n_S) {
  if (q.src < 0 || q.ld < 1) return false;
  const long long last = q.src + (long long)((q.tr ? q.dc : q.dr) - 1) * q.ld + ((q.tr ? q.dr : q.dc) - 1);
  return last < n_S;
}

// the table of all factors for the current analysis, on the device (kept while upload_version stays)
int table_current(pps_graph* g) {
  const int n_tab = (int)g->factors.size();
  if (g->fgate_tab_version == g->upload_version && g->fgate_tab.p && g->fgate_tab_n == n_tab) return PPS_OK;
  const long long n_S = (long long)g->an.L_size;
  std::vector<FgateFactor> tab((size_t)n_tab);
  for (int fid = 0; fid < n_tab; fid++) {
    const HostFactor& f = g->factors[fid];
    FgateFactor& t = tab[fid];
    t = FgateFactor{{0, 0, 0}, {1, 1, 1}, 0, -1, 0};
    if (f.deleted) continue;
    const std::string who = std::string("internal error: ") + kWho + "factor " + std::to_string(fid);
    CovNode na{}, nb{};
    int rc = cov_node(g, f.a, &na); if (rc != PPS_OK) return rc;
    rc = cov_locate(g, f.a, &na); if (rc != PPS_OK) return rc;
    if (f.b >= 0) {
      rc = cov_node(g, f.b, &nb); if (rc != PPS_OK) return rc;
      rc = cov_locate(g, f.b, &nb); if (rc != PPS_OK) return rc;
    }
    CovReq q[3];
    bool found = cov_request(g, na, na, 0, &q[0]);
    if (f.b >= 0) found = found && cov_request(g, nb, nb, 0, &q[1]) && cov_request(g, na, nb, 0, &q[2]);
    if (!found) return fail(g, PPS_ESTATE, who + " joins nodes whose blocks are outside the pattern of the selected inverse");
    for (int k = 0; k < (f.b >= 0 ? 3 : 1); k++) {
      if (!inside(q[k], n_S)) return fail(g, PPS_ESTATE, who + " has a block that ends outside the selected inverse");
      t.src[k] = q[k].src; t.ld[k] = q[k].ld;
    }
    t.tr = f.b >= 0 ? q[2].tr : 0;
    t.type = f.type; t.slot = f.slot;
  }
  g->fgate_tab_version = -1;
  int rc = g->fgate_tab.reserve(g, std::max<size_t>(1, tab.size()) * sizeof(FgateFactor), kWho, "the factor table", ""); if (rc != PPS_OK) return rc;
  if (!tab.empty()) HIP_TRY(g, hipMemcpyAsync(g->fgate_tab.p, tab.data(), tab.size() * sizeof(FgateFactor), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));             // (tab is host memory that does not outlive this function)
  g->fgate_tab_version = g->upload_version; g->fgate_tab_n = n_tab;
  return PPS_OK;
}

}  // namespace

extern "C" {

int pps_factor_gate_last(const pps_graph* g, double* kernel_sec, int* launches, int* n_untestable) {
  return query_last(g, &pps_graph::q_factor, kernel_sec, launches, n_untestable);
}

int pps_debug_factor_gate_records(pps_graph* g, int64_t cap, double* rec, int64_t* needed) {
  return query_records(g, &pps_graph::q_factor, kFgateRecord, kName, kFgateRecMaxEntries, "entries", cap, rec, needed);
}

int pps_factor_gate(pps_graph* g, int n, const int* fids, double thr3, double thr6, double* d2, double* leverage, int cap_flagged, int* flagged,
                    int* n_flagged) try {
  if (!g) return PPS_EINVAL;
  if (fids && n < 0) return fail(g, PPS_EINVAL, "factor gate: negative factor count");
  if (cap_flagged < 0) return fail(g, PPS_EINVAL, "factor gate: negative cap_flagged");
  if (!d2 && !leverage && !flagged && !n_flagged) return fail(g, PPS_EINVAL, "factor gate: no output asked for (d2, leverage and flagged / n_flagged are all NULL)");
  int rc = list_with_count(g, kWho, "flagged", flagged, n_flagged, cap_flagged); if (rc != PPS_OK) return rc;
  if (n_flagged && (!std::isfinite(thr3) || !std::isfinite(thr6))) return fail(g, PPS_EINVAL, "factor gate: the thresholds must be finite");
  std::vector<int> all;
  if (!fids) {
    for (size_t i = 0; i < g->factors.size(); i++) if (!g->factors[i].deleted) all.push_back((int)i);
    fids = all.data(); n = (int)all.size();
  }
  for (int i = 0; i < n; i++)
    if (!live_factor(g, fids[i])) return fail(g, PPS_EINVAL, "factor gate: " + std::to_string(fids[i]) + " is not a live factor");
  // r and J are the squared-error ones; with a cost function the recovered covariance is that of the robustified system
  if (robust(g)) return fail(g, PPS_ESTATE, "factor gate: a robust cost function is set (pps_set_cost_function); the test has no robustified form -- set PPS_COST_NONE and recover again");
  if (n == 0) return PPS_OK;                               // nothing asked for: the outputs stay untouched, the recovery is not looked at
  if (!cov_current(g)) return fail(g, PPS_ESTATE, cov_factor_current(g) ? kFactorOnly : kNoRecovery);
  rc = query_device(g); if (rc != PPS_OK) return rc;
  rc = table_current(g); if (rc != PPS_OK) return rc;
  // the result: [d2 n | lev n | status: n ints], doubles; no status word
  const size_t n_out = 2 * (size_t)n + ((size_t)n + 1) / 2;
  rc = g->fgate_list.reserve(g, (size_t)n, kWho, "the factor list", kAdvice); if (rc != PPS_OK) return rc;
  const bool keep_rec = n <= kFgateRecMaxEntries;
  QueryState& st = g->q_factor;
  rc = query_begin(g, &st, n_out * sizeof(double), 0, 0, keep_rec ? (size_t)n * kFgateRecord : kNoRecords, kWho, kAdvice); if (rc != PPS_OK) return rc;
  double* const out = reinterpret_cast<double*>(st.out.p);
  std::vector<double> host(n_out);
  FgateArgs fa;
  fa.factors = reinterpret_cast<const FgateFactor*>(g->fgate_tab.p); fa.n_factors = g->fgate_tab_n;
  fa.list = g->fgate_list.p; fa.n = n;
  fa.S = g->cov_S.p; fa.n_S = std::min<long long>((long long)g->an.L_size, (long long)g->cov_S.cap);
  fa.mode = g->props.jacobian_mode;
  fa.d2 = out; fa.lev = out + n; fa.status = reinterpret_cast<int*>(out + 2 * (size_t)n);
  fa.rec = keep_rec ? st.rec.p : nullptr;
  QueryTimer timer{g, 0};
  HIP_TRY(g, hipMemcpyAsync(g->fgate_list.p, fids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, g->stream));
  rc = timer.start(); if (rc != PPS_OK) return rc;
  HIP_TRY(g, launch_factor_gate(g->dev, fa, g->stream));
  rc = timer.stop(host.data(), n_out * sizeof(double), &st); if (rc != PPS_OK) return rc;
  const double* h_d2 = host.data();
  const double* h_lev = host.data() + n;
  const int* h_status = reinterpret_cast<const int*>(host.data() + 2 * (size_t)n);
  for (int i = 0; i < n; i++)
    if (h_status[i] != 0) return fail(g, PPS_EHIP, "internal error: the factor gate met an index outside its table, the state arrays or the selected inverse");
  int untestable = 0;
  long long over = 0;
  for (int i = 0; i < n; i++) {
    if (std::isnan(h_d2[i])) { untestable++; continue; }
    if (n_flagged && std::isfinite(h_d2[i]) && h_d2[i] >(kFDim[g->factors[fids[i]].type] == 3 ? thr3 : thr6)) {
      if (flagged && over < cap_flagged) flagged[over] = i;
      over++;
    }
  }
  query_end(&st, keep_rec ? (size_t)n : 0, untestable);
  if (n_flagged) *n_flagged = (int)over;
  if (d2) memcpy(d2, h_d2, (size_t)n * sizeof(double));
  if (leverage) memcpy(leverage, h_lev, (size_t)n * sizeof(double));
  return PPS_OK;
} catch (const std::bad_alloc&) {
  return query_no_memory(g, kWho);
}

}  // extern "C"
