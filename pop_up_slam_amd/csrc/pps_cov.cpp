// pps_cov.cpp -- isam::Covariances on the handle (Thirdparty/isam/include/isam/Covariances.h:42-110, isamlib/covariance.cpp): marginal
// covariances recovered from the multifrontal factor without a dense inverse.
//
// One pipeline, cov_run, is behind the three recovery calls: K1 at the estimate, K2, the lambda = 0 factorisation in the K3 form the graph
// has (enqueue_plain_factor, pps_solve.cpp), and then
//   pps_cov_factor     nothing more than the pivot criterion in one launch (pps_cov_wide.hip).  All pps_cov_block and the gates need
//   pps_cov_recover    the selected inverse root -> leaves by the band level pass (pps_cov.hip), one launch per tree level; band graphs only
//   pps_cov_select     the selected inverse in whatever form the graph has: the band level pass on a band graph (pps_cov_recover, launch for
//                      launch); on a dense-front graph the pivot criterion, then the root -> leaves pass of pps_cov_dense.hip (one launch over
//                      all fronts, three per level)
// What a pass needs of the tree is checked by cov_check_tree before anything is launched; what has been built, checked and uploaded for the
// current analysis is kept in one record (pps_graph::cov_cache).
//   pps_cov_marginals / _access / _joint   look the requested blocks up in the fronts (host tables built at recovery time), collect them with
//                      one gather launch and one copy
// Every entry of Sigma inside the pattern of L is available: the diagonal block of every node and the cross block of every pair of nodes
// that share a front (in particular every pair joined by a factor).  A recovery stays valid until the estimate, the measurements or the
// topology change (cov_invalidate, pps_graph.h); the read calls then answer PPS_ESTATE.
// The five calls that question what a recovery leaves -- pps_cov_block and the gates -- are in pps_query.cpp and the gates' own files (the
// protocol: pps_query.h).  All but pps_factor_gate read the lambda = 0 factor the recovery leaves in dev.L.
// dev.L is written by the factorisations alone (pps_solve.cpp:
// enqueue_factor_solve and do_solve, reached from pps_update, pps_batch_optimize and pps_debug_solve; the pps_multi launches), and each of those callers
// ends the recovery.  What keeps it -- pps_chi2 (K4 reads the states), the getters and pps_save_state (state copies), pps_eval_factor and
// pps_time_linearize (K1: J and the linearisation point), pps_get_stats / pps_get_trace (host fields), pps_analysis_dump, the
// association and reprojection calls -- launches nothing that writes dev.L, so no invalidation had to be added for it.
#include "pps_cov.h"
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void cov_release(pps_graph* g) {
  g->cov_S.release(); g->cov_parent.release(); g->cov_req.release(); g->cov_out.release(); g->cov_breq.release(); g->cov_strip.release();
  g->cov_zscr.release(); g->cov_G.release(); g->cov_dtab.release();
  for (QueryState* st : {&g->q_block, &g->q_assoc, &g->q_merge, &g->q_loop, &g->q_factor}) st->release();
  g->fgate_tab.release(); g->fgate_list.release();
  g->fgate_tab_version = -1; g->fgate_tab_n = 0;
  for (hipEvent_t& e : g->cov_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  for (hipEvent_t& e : g->cov_qev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  g->cov_cache = pps_graph::CovCache{};
  g->cov_valid = g->cov_factor_valid = false;
}

static bool cov_state_current(const pps_graph* g) {
  return g->dev_ready && !g->topo_dirty && !g->analysis_stale && !g->host_values_newer && !g->meas_dirty && g->cov_version == g->upload_version;
}
bool cov_current(const pps_graph* g) { return g->cov_valid && cov_state_current(g); }
bool cov_factor_current(const pps_graph* g) { return g->cov_factor_valid && cov_state_current(g); }

const char* const kNoRecovery = "no valid covariance recovery: call pps_cov_recover (a recovery ends with every change of the estimate, the measurements or the topology)";
const char* const kFactorOnly = "the handle holds the factor of pps_cov_factor, not the selected inverse: this call reads what pps_cov_recover computes (pps_cov_block and pps_assoc_gate read the factor)";
static const char* no_selected_inverse(const pps_graph* g) { return cov_factor_current(g) ? kFactorOnly : kNoRecovery; }

int cov_node(pps_graph* g, int id, CovNode* out) {
  if (id < 0 || id >= (int)g->nodes.size() || g->nodes[id].deleted) return fail(g, PPS_EINVAL, "covariance: unknown node id " + std::to_string(id));
  out->dim = g->nodes[id].type == NODE_POSE ? 6 : 3;
  out->front = -1; out->local = out->epos = out->voff = 0;
  return PPS_OK;
}

// (only with a current recovery: the analysis is the one the tables were built from)
int cov_locate(pps_graph* g, int id, CovNode* n) {
  const Analysis& A = g->an;
  const int c = g->nodes[id].compact;
  if (c < 0 || c >= A.n_nodes) return fail(g, PPS_ESTATE, "covariance: node " + std::to_string(id) + " is not part of the analysed graph");
  n->voff = A.node_voff[c];
  n->epos = g->cov_epos[n->voff];
  n->front = g->cov_front_of[n->epos];
  n->local = n->epos - A.f_poff[n->front];
  return PPS_OK;
}

// the block Sigma(rows, cols) as a gather request; false: the pair is outside the pattern of L
bool cov_request(const pps_graph* g, const CovNode& r, const CovNode& c, long long dst, CovReq* q) {
  const Analysis& A = g->an;
  const bool r_first = r.epos <= c.epos;               // the earlier-eliminated node owns the columns of the panel
  const CovNode& e = r_first ? r : c;
  const CovNode& o = r_first ? c : r;
  const int s = e.front, p = A.f_p[s];
  int lo = -1;
  if (o.front == s) lo = o.local;
  else {
    const int b0 = A.f_bidx_off[s], b1 = A.f_bidx_off[s + 1];
    const int* it = std::find(A.bidx.data() + b0, A.bidx.data() + b1, o.voff);
    if (it != A.bidx.data() + b1 && (it - (A.bidx.data() + b0)) + o.dim <= b1 - b0) lo = p + (int)(it - (A.bidx.data() + b0));
  }
  if (lo < 0) return false;
  q->src = (long long)A.f_Loff[s] + (long long)lo * p + e.local;
  q->dst = dst; q->ld = p;
  q->dr = r.dim; q->dc = c.dim;
  q->tr = r_first ? 1 : 0;                              // rows = the earlier node: the stored block is its transpose
  if (r.epos == c.epos) q->tr = 0;
  return true;
}

// requests -> device, one gather launch, one copy back into `host` (n_out doubles)
static int cov_fetch(pps_graph* g, const std::vector<CovReq>& req, size_t n_out, double* host) {
  if (req.empty() || n_out == 0) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  int rc = g->cov_req.reserve(g, req.size() * sizeof(CovReq)); if (rc != PPS_OK) return rc;
  rc = g->cov_out.reserve(g, n_out); if (rc != PPS_OK) return rc;
  HIP_TRY(g, hipMemcpyAsync(g->cov_req.p, req.data(), req.size() * sizeof(CovReq), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, launch_cov_gather(g->cov_S.p, reinterpret_cast<const CovReq*>(g->cov_req.p), (int)req.size(), g->cov_out.p, g->stream));
  HIP_TRY(g, hipMemcpyAsync(host, g->cov_out.p, n_out * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  return PPS_OK;
}

// node -> front tables of the current analysis; checks what the gather relies on: a node's scalars are consecutive pivots of ONE front
static int cov_build_tables(pps_graph* g) {
  const Analysis& A = g->an;
  g->cov_epos.assign((size_t)std::max(1, A.n_scalars), -1);
  g->cov_front_of.assign((size_t)std::max(1, A.n_scalars), -1);
  for (int s = 0; s < A.n_fronts; s++)
    for (int k = 0; k < A.f_p[s]; k++) {
      const int e = A.f_poff[s] + k;
      if (e < 0 || e >= A.n_scalars || A.pidx[e] < 0 || A.pidx[e] >= A.n_scalars) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (pivot index)");
      g->cov_epos[A.pidx[e]] = e; g->cov_front_of[e] = s;
    }
  for (int c = 0; c < A.n_nodes; c++) {
    const int v = A.node_voff[c], dim = g->sym_nodes[c].dim;
    for (int k = 0; k < dim; k++)
      if (v + k >= A.n_scalars || g->cov_epos[v + k] != g->cov_epos[v] + k || g->cov_front_of[g->cov_epos[v + k]] != g->cov_front_of[g->cov_epos[v]])
        return fail(g, PPS_ESTATE, "covariance: a node's scalars are not consecutive pivots of one front");
  }
  // pps_cov_block: the length of every front's path to the root in pivots (where the front's pivots sit in a strip, counted from its end)
  g->cov_rootlen.assign((size_t)std::max(1, A.n_fronts), 0);
  g->cov_max_p = g->cov_max_rows = 1;
  for (int s = 0; s < A.n_fronts; s++) {
    long long len = 0;
    int hops = 0;
    for (int t = s; t >= 0; t = A.f_parent[t]) {
      if (t >= A.n_fronts || ++hops > A.n_fronts) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (the parents form no tree)");
      len += A.f_p[t];
    }
    if (len > A.n_scalars) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (path longer than the system)");
    g->cov_rootlen[s] = (int)len;
    g->cov_max_p = std::max(g->cov_max_p, A.f_p[s]); g->cov_max_rows = std::max(g->cov_max_rows, A.f_p[s] + A.f_b[s]);
  }
  return PPS_OK;
}

// What the kernels of a pass index with, checked before anything is launched.  Always: the tables, parents, child maps and pivot counts (all
// the path walks rely on).  needs = kCovLevelShapes adds the LDS of k_cov_level, needs = kCovDense the level lists and the L / U extents of
// the dense-front pass (that bit itself is set by cov_run, with the upload of the work lists).
static int cov_check_tree(pps_graph* g, unsigned needs) {
  const Analysis& A = g->an;
  const unsigned want = pps_graph::kCovTables | needs;
  unsigned& have = g->cov_cache.have;
  if ((have & want) == want) return PPS_OK;
  if (!(have & pps_graph::kCovTables)) { const int rc = cov_build_tables(g); if (rc != PPS_OK) return rc; }
  const bool level = (needs & pps_graph::kCovLevelShapes) != 0, dense = (needs & pps_graph::kCovDense) != 0;
  if (dense) {
    if ((int)A.level_off.size() < A.n_levels + 1 || A.level_off[A.n_levels] != A.n_fronts) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (level lists)");
    std::vector<char> listed((size_t)std::max(1, A.n_fronts), 0);
    for (int l = 0; l < A.n_levels; l++)
      for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) {
        const int s = A.level_fronts[k];
        if (s < 0 || s >= A.n_fronts || listed[s] || A.f_level[s] != l) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (level lists)");
        listed[s] = 1;
      }
  }
  for (int s = 0; s < A.n_fronts; s++) {
    const int q = A.f_parent[s], p = A.f_p[s], b = A.f_b[s];
    if (b < 0 || (b > 0 && (q < 0 || q >= A.n_fronts || A.f_level[q] <= A.f_level[s] || A.f_cmap_off[s + 1] - A.f_cmap_off[s] < b)))
      return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (parent / child map)");
    for (int k = 0; k < b; k++) {
      const int r = A.cmap[A.f_cmap_off[s] + k];
      if (r < 0 || r >= A.f_p[q] + A.f_b[q]) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (child map entry)");
    }
    bool ok = p >= 1 && p <= 64;
    if (ok && level) ok = cov_level_lds_bytes(p, b) <= (size_t)159 * 1024;
    if (ok && dense) {
      const int64_t u_end = s + 1 < A.n_fronts ? A.f_Uoff[s + 1] : A.U_size, l_end = s + 1 < A.n_fronts ? A.f_Loff[s + 1] : A.L_size;
      ok = A.f_Uoff[s] >= 0 && u_end - A.f_Uoff[s] >= (int64_t)b * b && A.f_Loff[s] >= 0 && l_end - A.f_Loff[s] >= (int64_t)(p + b) * p;
    }
    if (!ok) return fail(g, PPS_ESTATE, "covariance: front outside the supported shapes");
  }
  have |= want & ~(unsigned)pps_graph::kCovDense;
  return PPS_OK;
}

// the work-item prefix sums of the dense-front pass: [all fronts | per level: gather, strips]
static std::vector<int> cov_dense_work_lists(pps_graph* g) {
  const Analysis& A = g->an;
  std::vector<int> tab;
  tab.push_back(0);
  for (int s = 0; s < A.n_fronts; s++) tab.push_back(tab.back() + cov_dense_pre_items(A.f_b[s]));
  g->cov_dpre_items = tab.back();
  g->cov_dlevel.assign((size_t)4 * std::max(1, A.n_levels), 0);
  for (int l = 0; l < A.n_levels; l++)
    for (int kind = 0; kind < 2; kind++) {
      const size_t at = tab.size();
      int sum = 0;
      tab.push_back(0);
      for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) {
        const int b = A.f_b[A.level_fronts[k]];
        sum += kind == 0 ? cov_dense_gather_items(b) : cov_dense_strip_items(b);
        tab.push_back(sum);
      }
      g->cov_dlevel[4 * l + 2 * kind] = (int)at; g->cov_dlevel[4 * l + 2 * kind + 1] = sum;
    }
  return tab;
}

// which pass follows the factor.  Select: the band level pass on a band graph, the dense-front pass otherwise (or when the handle asks for it)
enum class CovPass { FactorOnly, BandLevels, DenseFronts, Select };

// the end of a recovery: the status record comes home (one synchronisation), the times are read, a raised status is cleared and answered
static int cov_read_status(pps_graph* g, bool pass, const char* who, const char* lost) {
  double status[4] = {0, 0, 0, 0};
  HIP_TRY(g, hipMemcpyAsync(status, g->dev.result_dev, sizeof status, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  float ms = 0;
  if (!pass) g->cov_sec[1] = 0.0;
  if (hipEventElapsedTime(&ms, g->cov_ev[0], g->cov_ev[pass ? 2 : 1]) == hipSuccess) g->cov_sec[0] = 1e-3 * ms;
  if (pass && hipEventElapsedTime(&ms, g->cov_ev[1], g->cov_ev[2]) == hipSuccess) g->cov_sec[1] = 1e-3 * ms;
  if (status[2] != 0.0) {
    HIP_TRY(g, launch_clear_status(g->dev, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->status_clean = true;
  if (status[2] >= kStatusInternal) return fail(g, PPS_EHIP, std::string("internal error: ") + who + " met an index outside its front");
  if (status[2] != 0.0)
    return fail(g, PPS_ENOTPD, std::string("normal equations not positive definite at lambda = 0 (a pivot was not positive, or below 1e-7 of the largest pivot of its front): ") + lost);
  return PPS_OK;
}

// The recovery.  It reads L, f_p, f_b, f_Loff, f_Uoff, cmap, the parents and the level lists; the update matrices in d.U are dead once their
// parents are assembled, which is where the passes put Sigma_BB.
static int cov_run(pps_graph* g, CovPass what) {
  int rc;
  if (!g->analyzed || g->analysis_stale) { rc = pps_analyze(g); if (rc != PPS_OK) return rc; }
  if (what == CovPass::Select) what = g->use_band() && g->cov_select_form == 0 ? CovPass::BandLevels : CovPass::DenseFronts;
  if (what == CovPass::BandLevels && !g->use_band())
    return fail(g, PPS_ESTATE, "covariance recovery is limited to graphs whose fronts all fit the wave-per-front kernels (max front " +
                               std::to_string(g->an.max_front) + " scalars here: loop-closure graphs in the dense-front form are not supported)");
  if (!g->use_band() && !g->use_dense())
    return fail(g, PPS_ESTATE, "pps_cov_factor: the graph is solved by the one-launch-per-level LDS kernels (max front " + std::to_string(g->an.max_front) +
                               " scalars, neither the band nor the dense-front form), whose panels do not pass through the factor array: no factor to keep");
  rc = prepare_solve(g); if (rc != PPS_OK) return rc;
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  const bool levels = what == CovPass::BandLevels, fronts = what == CovPass::DenseFronts, pass = levels || fronts;
  for (hipEvent_t& e : g->cov_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  if (g->cov_cache.version != g->upload_version) g->cov_cache = pps_graph::CovCache{g->upload_version, 0};
  unsigned& have = g->cov_cache.have;
  // the dense-front pass answers PPS_ENOMEM, never an abort, when a buffer cannot be had
  const char* who = fronts ? "pps_cov_select: " : nullptr;
  const size_t n_panel = (size_t)std::max<int64_t>(1, A.L_size);
  if (pass) { rc = g->cov_S.reserve(g, n_panel, who, "the selected inverse"); if (rc != PPS_OK) return rc; }
  if (fronts) { rc = g->cov_G.reserve(g, n_panel, who, "the scratch of L_B L_A^-1"); if (rc != PPS_OK) return rc; }
  rc = cov_check_tree(g, levels ? pps_graph::kCovLevelShapes : fronts && !(have & pps_graph::kCovDense) ? pps_graph::kCovDense : 0u); if (rc != PPS_OK) return rc;
  { const bool up_tab = fronts && !(have & pps_graph::kCovDense), up_parent = pass && !(have & pps_graph::kCovParent);
    std::vector<int> tab;
    if (up_tab) { tab = cov_dense_work_lists(g); rc = g->cov_dtab.reserve(g, tab.size(), who, "the work lists"); if (rc != PPS_OK) return rc; }
    if (up_parent) { rc = g->cov_parent.reserve(g, (size_t)std::max(1, A.n_fronts), who, "the parent list"); if (rc != PPS_OK) return rc; }
    if (up_tab) HIP_TRY(g, hipMemcpyAsync(g->cov_dtab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, g->stream));
    if (up_parent) HIP_TRY(g, hipMemcpyAsync(g->cov_parent.p, A.f_parent.data(), (size_t)A.n_fronts * sizeof(int), hipMemcpyHostToDevice, g->stream));
    if (up_tab || up_parent) HIP_TRY(g, hipStreamSynchronize(g->stream));      // (tab and f_parent are host memory that does not outlive the analysis)
    if (up_tab) have |= pps_graph::kCovDense;
    if (up_parent) have |= pps_graph::kCovParent; }
  rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
  HIP_TRY(g, hipEventRecord(g->cov_ev[0], g->stream));
  // jacobian() at the ESTIMATE (the linearisation point stays what it is; the robustified J with a cost function set), H blocks, factorisation
  // with lambda = 0 in the form whose panels all pass through d.L
  HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, true));
  HIP_TRY(g, launch_hblocks(d, g->stream, nullptr, k1_products(d, g->props.jacobian_mode)));
  rc = enqueue_plain_factor(g, 0.0); if (rc != PPS_OK) return rc;
  if (!levels) HIP_TRY(g, launch_cov_pivots(d, A.n_fronts, g->stream));      // (k_cov_level applies the pivot criterion itself)
  HIP_TRY(g, hipEventRecord(g->cov_ev[1], g->stream));
  if (levels)
    for (int l = A.n_levels - 1; l >= 0; l--) {
      size_t lds = 0;
      for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) lds = std::max(lds, cov_level_lds_bytes(A.f_p[A.level_fronts[k]], A.f_b[A.level_fronts[k]]));
      HIP_TRY(g, launch_cov_level(d, g->cov_S.p, g->cov_parent.p, A.level_off[l], A.level_off[l + 1] - A.level_off[l], lds, g->stream));
    }
  if (fronts) {
    const CovDenseExtents ext{(long long)A.L_size, (long long)A.U_size};
    HIP_TRY(g, launch_cov_dense_pre(d, g->cov_S.p, g->cov_G.p, ext, g->cov_dtab.p, g->cov_dpre_items, A.n_fronts, g->stream));
    for (int l = A.n_levels - 1; l >= 0; l--) {
      const int* lv = g->cov_dlevel.data() + 4 * l;
      HIP_TRY(g, launch_cov_dense_level(d, g->cov_S.p, g->cov_G.p, ext, g->cov_parent.p, A.level_off[l], A.level_off[l + 1] - A.level_off[l], g->cov_dtab.p + lv[0], lv[1],
                                        g->cov_dtab.p + lv[2], lv[3], g->stream));
    }
  }
  if (pass) HIP_TRY(g, hipEventRecord(g->cov_ev[2], g->stream));
  rc = cov_read_status(g, pass, levels ? "the covariance recovery" : fronts ? "pps_cov_select" : "the factorisation of pps_cov_factor", pass ? "no covariance" : "no factor");
  if (rc != PPS_OK) return rc;
  g->cov_version = g->upload_version;
  g->cov_factor_valid = true;
  if (pass) g->cov_valid = true;
  return PPS_OK;
}

// the three recovery calls: no solve, so the figures of the last one stay (NoSolveScope)
static int cov_entry(pps_graph* g, CovPass what) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->n_live_factors == 0) return fail(g, PPS_ENOTPD, "normal equations not positive definite: the graph has no factor");
  int rc;
  { NoSolveScope scope(g); rc = cov_run(g, what); }
  if (rc == PPS_EHIP) abandon_device_copy(g);
  return rc;
}

}  // namespace pps_impl

extern "C" {

int pps_cov_recover(pps_graph* g) { return cov_entry(g, CovPass::BandLevels); }
int pps_cov_factor(pps_graph* g) { return cov_entry(g, CovPass::FactorOnly); }
int pps_cov_select(pps_graph* g) { return cov_entry(g, CovPass::Select); }

int pps_debug_cov_select_form(pps_graph* g, int form) {
  if (!g) return PPS_EINVAL;
  if (form != 0 && form != 1) return fail(g, PPS_EINVAL, "pps_debug_cov_select_form: form is 0 (pps_cov_recover on a band graph) or 1 (always the dense-front pass)");
  g->cov_select_form = form;
  return PPS_OK;
}

int pps_debug_cov_path_form(pps_graph* g, int form) {
  if (!g) return PPS_EINVAL;
  if (form != 0 && form != 1) return fail(g, PPS_EINVAL, "pps_debug_cov_path_form: form is 0 (automatic) or 1 (always the wide kernel)");
  g->cov_path_form = form;
  return PPS_OK;
}

int pps_cov_last_times(const pps_graph* g, double sec[2]) {
  if (!g || !sec) return PPS_EINVAL;
  sec[0] = g->cov_sec[0]; sec[1] = g->cov_sec[1];
  return PPS_OK;
}

int pps_cov_marginals(pps_graph* g, int n, const int* ids, double* out, int64_t* offsets) {
  if (!g || !out || n < 0) return PPS_EINVAL;
  std::vector<int> all;
  if (!ids) {
    for (size_t i = 0; i < g->nodes.size(); i++) if (!g->nodes[i].deleted) all.push_back((int)i);
    if ((int)all.size() != n) return fail(g, PPS_EINVAL, "covariance marginals: count mismatch (ids == NULL asks for all " + std::to_string(all.size()) + " nodes)");
    ids = all.data();
  }
  std::vector<CovNode> nd((size_t)n);
  for (int i = 0; i < n; i++) { const int rc = cov_node(g, ids[i], &nd[i]); if (rc != PPS_OK) return rc; }
  if (!cov_current(g)) return fail(g, PPS_ESTATE, no_selected_inverse(g));
  std::vector<CovReq> req((size_t)n);
  long long o = 0;
  for (int i = 0; i < n; i++) {
    const int rc = cov_locate(g, ids[i], &nd[i]); if (rc != PPS_OK) return rc;
    if (!cov_request(g, nd[i], nd[i], o, &req[i])) return fail(g, PPS_ESTATE, "covariance: diagonal block not found");
    if (offsets) offsets[i] = o;
    o += (long long)nd[i].dim * nd[i].dim;
  }
  if (offsets) offsets[n] = o;
  return cov_fetch(g, req, (size_t)o, out);
}

int pps_cov_access(pps_graph* g, int n, const int* rows, const int* cols, double* out, int64_t* offsets, int* in_pattern) {
  if (!g || !rows || !cols || !out || !in_pattern || n < 0) return PPS_EINVAL;
  std::vector<CovNode> nr((size_t)n), nc((size_t)n);
  for (int i = 0; i < n; i++) {
    int rc = cov_node(g, rows[i], &nr[i]); if (rc != PPS_OK) return rc;
    rc = cov_node(g, cols[i], &nc[i]); if (rc != PPS_OK) return rc;
  }
  if (!cov_current(g)) return fail(g, PPS_ESTATE, no_selected_inverse(g));
  // the blocks are collected densely on the device and copied to their places in `out`, so that a block outside the pattern is left untouched
  std::vector<CovReq> req;
  std::vector<long long> place;
  long long o = 0, packed = 0;
  for (int i = 0; i < n; i++) {
    int rc = cov_locate(g, rows[i], &nr[i]); if (rc != PPS_OK) return rc;
    rc = cov_locate(g, cols[i], &nc[i]); if (rc != PPS_OK) return rc;
    CovReq q;
    in_pattern[i] = cov_request(g, nr[i], nc[i], packed, &q) ? 1 : 0;
    if (in_pattern[i]) { req.push_back(q); place.push_back(o); packed += (long long)q.dr * q.dc; }
    if (offsets) offsets[i] = o;
    o += (long long)nr[i].dim * nc[i].dim;
  }
  if (offsets) offsets[n] = o;
  std::vector<double> tmp((size_t)packed);
  const int rc = cov_fetch(g, req, (size_t)packed, tmp.data());
  if (rc != PPS_OK) return rc;
  for (size_t k = 0; k < req.size(); k++) memcpy(out + place[k], tmp.data() + req[k].dst, sizeof(double) * (size_t)req[k].dr * req[k].dc);
  return PPS_OK;
}

int pps_cov_joint(pps_graph* g, int n, const int* ids, double* out) {
  if (!g || !ids || !out || n < 0) return PPS_EINVAL;
  std::vector<CovNode> nd((size_t)n);
  for (int i = 0; i < n; i++) {
    const int rc = cov_node(g, ids[i], &nd[i]); if (rc != PPS_OK) return rc;
    for (int j = 0; j < i; j++) if (ids[j] == ids[i]) return fail(g, PPS_EINVAL, "covariance joint: node " + std::to_string(ids[i]) + " is listed twice");
  }
  if (!cov_current(g)) return fail(g, PPS_ESTATE, no_selected_inverse(g));
  std::vector<int> off((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) {
    const int rc = cov_locate(g, ids[i], &nd[i]); if (rc != PPS_OK) return rc;
    off[i + 1] = off[i] + nd[i].dim;
  }
  const int N = off[n];
  std::vector<CovReq> req;
  std::vector<std::pair<int, int>> who;
  long long packed = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      CovReq q;
      if (!cov_request(g, nd[i], nd[j], packed, &q))
        return fail(g, PPS_ESTATE, "covariance joint: nodes " + std::to_string(ids[j]) + " and " + std::to_string(ids[i]) +
                                   " share no front (the pair is outside the pattern of the factor: not recoverable without column solves)");
      req.push_back(q); who.emplace_back(i, j); packed += (long long)q.dr * q.dc;
    }
  std::vector<double> tmp((size_t)packed);
  const int rc = cov_fetch(g, req, (size_t)packed, tmp.data());
  if (rc != PPS_OK) return rc;
  for (size_t k = 0; k < req.size(); k++) {
    const int i = who[k].first, j = who[k].second;
    const double* blk = tmp.data() + req[k].dst;
    for (int a = 0; a < nd[i].dim; a++)
      for (int c = 0; c < nd[j].dim; c++) {
        out[(size_t)(off[i] + a) * N + off[j] + c] = blk[a * nd[j].dim + c];
        out[(size_t)(off[j] + c) * N + off[i] + a] = blk[a * nd[j].dim + c];
      }
  }
  return PPS_OK;
}

}  // extern "C"
