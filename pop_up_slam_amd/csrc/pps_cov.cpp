// pps_cov.cpp -- isam::Covariances on the handle (Thirdparty/isam/include/isam/Covariances.h:42-110, isamlib/covariance.cpp): marginal
// covariances recovered from the multifrontal factor without a dense inverse.
//
//   pps_cov_recover    relinearise at the estimate, H = J'J factored with lambda = 0 (the launches of pps_update's factorisation, one per band
//                      stage), then the selected inverse root -> leaves (pps_cov.hip), one launch per tree level
//   pps_cov_factor     the same without the selected inverse: K1 at the estimate, K2, the lambda = 0 factorisation in the K3 form the graph has
//                      (band stages or the dense-front levels), the pivot criterion in one launch (pps_cov_wide.hip).  All pps_cov_block and
//                      pps_assoc_gate need, and the only recovery a dense-front graph has
//   pps_cov_select     the selected inverse in whatever form the graph has: pps_cov_recover on a band graph; on a dense-front graph the factor
//                      stage of pps_cov_factor, then the root -> leaves pass of pps_cov_dense.hip (one launch over all fronts, three per level)
//   pps_cov_marginals / _access / _joint   look the requested blocks up in the fronts (host tables built at recovery time), collect them with
//                      one gather launch and one copy
// Every entry of Sigma inside the pattern of L is available: the diagonal block of every node and the cross block of every pair of nodes
// that share a front (in particular every pair joined by a factor).  A recovery stays valid until the estimate, the measurements or the
// topology change (cov_invalidate, pps_graph.h); the read calls then answer PPS_ESTATE.
//   pps_cov_block      Sigma(rows, cols) for ANY nodes: (L^-1 E_rows)' (L^-1 E_cols) by one walk up the elimination tree per distinct node
//                      and one Gram product over common ancestors (pps_cov.hip) -- one upload, two launches, one copy, whatever the query
// pps_cov_block reads the lambda = 0 factor the recovery leaves in dev.L.  dev.L is written by the factorisations alone (pps_solve.cpp:
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
  if (g->cov_S) (void)hipFree(g->cov_S);
  if (g->cov_parent) (void)hipFree(g->cov_parent);
  if (g->cov_req) (void)hipFree(g->cov_req);
  if (g->cov_out) (void)hipFree(g->cov_out);
  if (g->cov_breq) (void)hipFree(g->cov_breq);
  if (g->cov_strip) (void)hipFree(g->cov_strip);
  if (g->cov_bout) (void)hipFree(g->cov_bout);
  if (g->cov_zscr) (void)hipFree(g->cov_zscr);
  if (g->cov_G) (void)hipFree(g->cov_G);
  if (g->cov_dtab) (void)hipFree(g->cov_dtab);
  g->cov_G = nullptr; g->cov_G_cap = 0; g->cov_dtab = nullptr; g->cov_dtab_cap = 0; g->cov_dtab_version = -1;
  gate_release(g);
  merge_release(g);
  for (hipEvent_t& e : g->cov_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  for (hipEvent_t& e : g->cov_bev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  g->cov_S = nullptr; g->cov_parent = nullptr; g->cov_req = nullptr; g->cov_out = nullptr;
  g->cov_breq = nullptr; g->cov_strip = nullptr; g->cov_bout = nullptr; g->cov_zscr = nullptr; g->cov_zscr_cap = 0;
  g->cov_S_cap = g->cov_parent_cap = g->cov_req_cap = g->cov_out_cap = 0;
  g->cov_breq_cap = g->cov_strip_cap = g->cov_bout_cap = 0; g->cov_bout_clean = false;
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
static bool cov_request(const pps_graph* g, const CovNode& r, const CovNode& c, long long dst, CovReq* q) {
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
  int rc = cov_reserve(g, &g->cov_req, &g->cov_req_cap, req.size() * sizeof(CovReq)); if (rc != PPS_OK) return rc;
  rc = cov_reserve(g, &g->cov_out, &g->cov_out_cap, n_out); if (rc != PPS_OK) return rc;
  HIP_TRY(g, hipMemcpyAsync(g->cov_req, req.data(), req.size() * sizeof(CovReq), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, launch_cov_gather(g->cov_S, reinterpret_cast<const CovReq*>(g->cov_req), (int)req.size(), g->cov_out, g->stream));
  HIP_TRY(g, hipMemcpyAsync(host, g->cov_out, n_out * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  return PPS_OK;
}

// paths (leaf -> root) and strips of a list of distinct, checked nodes; K = the longest path of the query in pivots
int cov_build_walks(pps_graph* g, const std::vector<int>& ids, std::vector<CovNode>& nd, CovWalks* out) {
  const Analysis& A = g->an;
  const int nw = (int)ids.size();
  out->K = 0;
  for (int w = 0; w < nw; w++) {
    const int rc = cov_locate(g, ids[w], &nd[w]); if (rc != PPS_OK) return rc;
    out->K = std::max(out->K, g->cov_rootlen[nd[w].front]);
  }
  out->walks.assign((size_t)nw, CovWalk{});
  out->steps.clear();
  out->step_end.assign((size_t)nw, 0);
  out->n_strip = 0;
  out->max_rows = 1;
  for (int w = 0; w < nw; w++) {
    out->walks[w] = CovWalk{out->n_strip, (int)out->steps.size(), 0, nd[w].local, nd[w].dim};
    for (int s = nd[w].front; s >= 0; s = A.f_parent[s]) {
      out->steps.push_back(CovStep{s, out->K - g->cov_rootlen[s]});
      out->max_rows = std::max(out->max_rows, A.f_p[s] + A.f_b[s]);
    }
    out->walks[w].n_steps = (int)out->steps.size() - out->walks[w].step0;
    out->step_end[w] = (int)out->steps.size();
    out->n_strip += (long long)out->K * nd[w].dim;
  }
  return PPS_OK;
}

// the pivots two paths have in common are a suffix of both
int cov_common_pivots(const pps_graph* g, const CovWalks& cw, int a, int b) {
  int len = 0;
  for (int i = cw.step_end[a] - 1, j = cw.step_end[b] - 1; i >= cw.walks[a].step0 && j >= cw.walks[b].step0 && cw.steps[i].front == cw.steps[j].front; i--, j--)
    len += g->an.f_p[cw.steps[i].front];
  return len;
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

static int cov_recover_impl(pps_graph* g) {
  int rc;
  if (!g->analyzed || g->analysis_stale) { rc = pps_analyze(g); if (rc != PPS_OK) return rc; }
  if (!g->use_band)
    return fail(g, PPS_ESTATE, "covariance recovery is limited to graphs whose fronts all fit the wave-per-front kernels (max front " +
                               std::to_string(g->an.max_front) + " scalars here: loop-closure graphs in the dense-front form are not supported)");
  rc = prepare_solve(g); if (rc != PPS_OK) return rc;
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  for (hipEvent_t& e : g->cov_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  rc = cov_reserve(g, &g->cov_S, &g->cov_S_cap, (size_t)std::max<int64_t>(1, A.L_size)); if (rc != PPS_OK) return rc;
  if (g->cov_parent_version != g->upload_version) {
    rc = cov_build_tables(g); if (rc != PPS_OK) return rc;
    for (int s = 0; s < A.n_fronts; s++) {             // what k_cov_level indexes with: checked here, before anything is launched
      const int q = A.f_parent[s];
      if (A.f_b[s] > 0 && (q < 0 || q >= A.n_fronts || A.f_level[q] <= A.f_level[s] || A.f_cmap_off[s + 1] - A.f_cmap_off[s] < A.f_b[s]))
        return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (parent / child map)");
      for (int k = 0; k < A.f_b[s]; k++) {
        const int r = A.cmap[A.f_cmap_off[s] + k];
        if (r < 0 || r >= A.f_p[q] + A.f_b[q]) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (child map entry)");
      }
      if (A.f_p[s] < 1 || A.f_p[s] > 64 || cov_level_lds_bytes(A.f_p[s], A.f_b[s]) > (size_t)159 * 1024)
        return fail(g, PPS_ESTATE, "covariance: front outside the supported shapes");
    }
    rc = cov_reserve(g, &g->cov_parent, &g->cov_parent_cap, (size_t)std::max(1, A.n_fronts)); if (rc != PPS_OK) return rc;
    HIP_TRY(g, hipMemcpyAsync(g->cov_parent, A.f_parent.data(), (size_t)A.n_fronts * sizeof(int), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));         // (f_parent may be reallocated by the next analysis)
    g->cov_parent_version = g->upload_version;
  }
  if (!g->status_clean) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    if (g->spec_result) HIP_TRY(g, hipMemsetAsync(g->spec_result, 0, 4 * sizeof(double), g->stream));
  }
  g->status_clean = false;
  HIP_TRY(g, hipEventRecord(g->cov_ev[0], g->stream));
  // jacobian() at the ESTIMATE (the linearisation point stays what it is), H blocks, factorisation with lambda = 0: one launch per band
  // stage, the form whose panels all pass through d.L.  The update matrices in d.U are dead once their parents are assembled.
  HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, true));      // (the robustified J with a cost function set)
  HIP_TRY(g, launch_hblocks(d, g->stream, nullptr, k1_products(d, g->props.jacobian_mode)));
  for (int st = 0; st < A.n_stages; st++)
    HIP_TRY(g, launch_band_factor(d, A.stage_grp_off[st], A.stage_grp_off[st + 1] - A.stage_grp_off[st], g->stage_nw_factor[st], A.stage_max_front[st], 0.0, g->stream));
  HIP_TRY(g, hipEventRecord(g->cov_ev[1], g->stream));
  for (int l = A.n_levels - 1; l >= 0; l--) {
    size_t lds = 0;
    for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) lds = std::max(lds, cov_level_lds_bytes(A.f_p[A.level_fronts[k]], A.f_b[A.level_fronts[k]]));
    HIP_TRY(g, launch_cov_level(d, g->cov_S, g->cov_parent, A.level_off[l], A.level_off[l + 1] - A.level_off[l], lds, g->stream));
  }
  HIP_TRY(g, hipEventRecord(g->cov_ev[2], g->stream));
  double status[4] = {0, 0, 0, 0};
  HIP_TRY(g, hipMemcpyAsync(status, d.result_dev, sizeof status, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->cov_ev[0], g->cov_ev[2]) == hipSuccess) g->cov_sec[0] = 1e-3 * ms;
  if (hipEventElapsedTime(&ms, g->cov_ev[1], g->cov_ev[2]) == hipSuccess) g->cov_sec[1] = 1e-3 * ms;
  if (status[2] != 0.0) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->status_clean = true;
  if (status[2] >= kStatusInternal) return fail(g, PPS_EHIP, "internal error: the covariance recovery met an index outside its front");
  if (status[2] != 0.0)
    return fail(g, PPS_ENOTPD, "normal equations not positive definite at lambda = 0 (a pivot was not positive, or below 1e-7 of the largest pivot of its front): no covariance");
  g->cov_version = g->upload_version;
  g->cov_valid = g->cov_factor_valid = true;
  g->cov_tables_version = g->upload_version;             // (built and checked above, with the stricter shape test of the level pass)
  return PPS_OK;
}

static std::string no_factor_array(const pps_graph* g) {
  return "pps_cov_factor: the graph is solved by the one-launch-per-level LDS kernels (max front " + std::to_string(g->an.max_front) +
         " scalars, neither the band nor the dense-front form), whose panels do not pass through the factor array: no factor to keep";
}

// pps_cov_factor: the recovery without the selected inverse, in whatever K3 form the graph has
static int cov_factor_impl(pps_graph* g) {
  int rc;
  if (!g->analyzed || g->analysis_stale) { rc = pps_analyze(g); if (rc != PPS_OK) return rc; }
  if (!g->use_band && !g->use_dense)
    return fail(g, PPS_ESTATE, no_factor_array(g));
  rc = prepare_solve(g); if (rc != PPS_OK) return rc;
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  for (hipEvent_t& e : g->cov_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  if (g->cov_tables_version != g->upload_version && g->cov_parent_version != g->upload_version) {
    rc = cov_build_tables(g); if (rc != PPS_OK) return rc;
    for (int s = 0; s < A.n_fronts; s++) {               // what the path walks index with: checked here, before anything is launched
      const int q = A.f_parent[s];
      if (A.f_b[s] < 0 || (A.f_b[s] > 0 && (q < 0 || q >= A.n_fronts || A.f_level[q] <= A.f_level[s] || A.f_cmap_off[s + 1] - A.f_cmap_off[s] < A.f_b[s])))
        return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (parent / child map)");
      for (int k = 0; k < A.f_b[s]; k++) {
        const int r = A.cmap[A.f_cmap_off[s] + k];
        if (r < 0 || r >= A.f_p[q] + A.f_b[q]) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (child map entry)");
      }
      if (A.f_p[s] < 1 || A.f_p[s] > 64) return fail(g, PPS_ESTATE, "covariance: front outside the supported shapes");
    }
    g->cov_tables_version = g->upload_version;
  }
  if (!g->status_clean) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    if (g->spec_result) HIP_TRY(g, hipMemsetAsync(g->spec_result, 0, 4 * sizeof(double), g->stream));
  }
  g->status_clean = false;
  HIP_TRY(g, hipEventRecord(g->cov_ev[0], g->stream));
  HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, true));      // jacobian() at the ESTIMATE, robustified with a cost function set
  HIP_TRY(g, launch_hblocks(d, g->stream, nullptr, k1_products(d, g->props.jacobian_mode)));
  if (g->use_band) {                                     // one launch per band stage: the form whose panels all pass through d.L
    for (int st = 0; st < A.n_stages; st++)
      HIP_TRY(g, launch_band_factor(d, A.stage_grp_off[st], A.stage_grp_off[st + 1] - A.stage_grp_off[st], g->stage_nw_factor[st], A.stage_max_front[st], 0.0, g->stream));
  } else {                                               // the dense-front levels, as do_solve issues them (pps_solve.cpp)
    HIP_TRY(g, hipMemsetAsync(d.L, 0, (size_t)A.L_size * 8, g->stream));
    HIP_TRY(g, launch_dense_hpush(d, g->max_el_per_front, 0.0, g->stream));
    for (int l = 0; l < A.n_levels; l++) {
      const int base = A.level_off[l] + l, cnt = A.level_off[l + 1] - A.level_off[l];
      HIP_TRY(g, launch_dense_factor_level(d, A.level_off[l], cnt, g->d_dw_asm + base, g->dw_asm[base + cnt], g->d_dw_pan + base, g->dw_pan[base + cnt],
                                           g->d_dw_trl + base, g->dw_trl[base + cnt], g->stream));
    }
  }
  HIP_TRY(g, launch_cov_pivots(d, A.n_fronts, g->stream));
  HIP_TRY(g, hipEventRecord(g->cov_ev[1], g->stream));
  double status[4] = {0, 0, 0, 0};
  HIP_TRY(g, hipMemcpyAsync(status, d.result_dev, sizeof status, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  float ms = 0;
  g->cov_sec[1] = 0.0;
  if (hipEventElapsedTime(&ms, g->cov_ev[0], g->cov_ev[1]) == hipSuccess) g->cov_sec[0] = 1e-3 * ms;
  if (status[2] != 0.0) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->status_clean = true;
  if (status[2] >= kStatusInternal) return fail(g, PPS_EHIP, "internal error: the factorisation of pps_cov_factor met an index outside its front");
  if (status[2] != 0.0)
    return fail(g, PPS_ENOTPD, "normal equations not positive definite at lambda = 0 (a pivot was not positive, or below 1e-7 of the largest pivot of its front): no factor");
  g->cov_version = g->upload_version;
  g->cov_factor_valid = true;
  return PPS_OK;
}

// the device buffers of the dense-front pass: PPS_ENOMEM, never an abort, when one cannot be had
template <class T>
static int cov_select_reserve(pps_graph* g, T** buf, size_t* cap, size_t count, const char* what) {
  if (cov_reserve(g, buf, cap, count) == PPS_OK) return PPS_OK;
  (void)hipGetLastError();
  return fail(g, PPS_ENOMEM, std::string("pps_cov_select: no device memory for ") + what + " (" + std::to_string(count * sizeof(T)) + " bytes)");
}

// pps_cov_select on a dense-front tree (or, with pps_debug_cov_select_form, on a band tree): the lambda = 0 factor in the form the graph is
// solved in, then the root -> leaves pass of pps_cov_dense.hip.  It reads L, f_p, f_b, f_Loff, f_Uoff, cmap, the parents and the level lists.
static int cov_select_dense_impl(pps_graph* g) {
  int rc = prepare_solve(g); if (rc != PPS_OK) return rc;
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  for (hipEvent_t& e : g->cov_ev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  const size_t n_panel = (size_t)std::max<int64_t>(1, A.L_size);
  rc = cov_select_reserve(g, &g->cov_S, &g->cov_S_cap, n_panel, "the selected inverse"); if (rc != PPS_OK) return rc;
  rc = cov_select_reserve(g, &g->cov_G, &g->cov_G_cap, n_panel, "the scratch of L_B L_A^-1"); if (rc != PPS_OK) return rc;
  if (g->cov_dtab_version != g->upload_version) {
    rc = cov_build_tables(g); if (rc != PPS_OK) return rc;
    if ((int)A.level_off.size() < A.n_levels + 1 || A.level_off[A.n_levels] != A.n_fronts) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (level lists)");
    std::vector<char> listed((size_t)std::max(1, A.n_fronts), 0);
    for (int l = 0; l < A.n_levels; l++)
      for (int k = A.level_off[l]; k < A.level_off[l + 1]; k++) {
        const int s = A.level_fronts[k];
        if (s < 0 || s >= A.n_fronts || listed[s] || A.f_level[s] != l) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (level lists)");
        listed[s] = 1;
      }
    for (int s = 0; s < A.n_fronts; s++) {               // what the kernels index with: checked here, before anything is launched
      const int q = A.f_parent[s], p = A.f_p[s], b = A.f_b[s];
      if (b < 0 || (b > 0 && (q < 0 || q >= A.n_fronts || A.f_level[q] <= A.f_level[s] || A.f_cmap_off[s + 1] - A.f_cmap_off[s] < b)))
        return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (parent / child map)");
      for (int k = 0; k < b; k++) {
        const int r = A.cmap[A.f_cmap_off[s] + k];
        if (r < 0 || r >= A.f_p[q] + A.f_b[q]) return fail(g, PPS_ESTATE, "covariance: inconsistent analysis (child map entry)");
      }
      const int64_t u_end = s + 1 < A.n_fronts ? A.f_Uoff[s + 1] : A.U_size, l_end = s + 1 < A.n_fronts ? A.f_Loff[s + 1] : A.L_size;
      if (p < 1 || p > 64 || A.f_Uoff[s] < 0 || u_end - A.f_Uoff[s] < (int64_t)b * b || A.f_Loff[s] < 0 || l_end - A.f_Loff[s] < (int64_t)(p + b) * p)
        return fail(g, PPS_ESTATE, "covariance: front outside the supported shapes");
    }
    // work-item prefix sums: [all fronts | per level: gather, strips]
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
    rc = cov_select_reserve(g, &g->cov_dtab, &g->cov_dtab_cap, tab.size(), "the work lists"); if (rc != PPS_OK) return rc;
    rc = cov_select_reserve(g, &g->cov_parent, &g->cov_parent_cap, (size_t)std::max(1, A.n_fronts), "the parent list"); if (rc != PPS_OK) return rc;
    g->cov_parent_version = -1;                          // (pps_cov_recover has its own, stricter shape test: it checks and uploads again)
    HIP_TRY(g, hipMemcpyAsync(g->cov_dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(g, hipMemcpyAsync(g->cov_parent, A.f_parent.data(), (size_t)A.n_fronts * sizeof(int), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));         // (tab and f_parent are host memory that does not outlive this call)
    g->cov_dtab_version = g->upload_version;
    g->cov_tables_version = g->upload_version;
  }
  if (!g->status_clean) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    if (g->spec_result) HIP_TRY(g, hipMemsetAsync(g->spec_result, 0, 4 * sizeof(double), g->stream));
  }
  g->status_clean = false;
  HIP_TRY(g, hipEventRecord(g->cov_ev[0], g->stream));
  // the factor stage of pps_cov_factor
  HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, true));      // jacobian() at the ESTIMATE, robustified with a cost function set
  HIP_TRY(g, launch_hblocks(d, g->stream, nullptr, k1_products(d, g->props.jacobian_mode)));
  if (g->use_band) {
    for (int st = 0; st < A.n_stages; st++)
      HIP_TRY(g, launch_band_factor(d, A.stage_grp_off[st], A.stage_grp_off[st + 1] - A.stage_grp_off[st], g->stage_nw_factor[st], A.stage_max_front[st], 0.0, g->stream));
  } else {
    HIP_TRY(g, hipMemsetAsync(d.L, 0, (size_t)A.L_size * 8, g->stream));
    HIP_TRY(g, launch_dense_hpush(d, g->max_el_per_front, 0.0, g->stream));
    for (int l = 0; l < A.n_levels; l++) {
      const int base = A.level_off[l] + l, cnt = A.level_off[l + 1] - A.level_off[l];
      HIP_TRY(g, launch_dense_factor_level(d, A.level_off[l], cnt, g->d_dw_asm + base, g->dw_asm[base + cnt], g->d_dw_pan + base, g->dw_pan[base + cnt],
                                           g->d_dw_trl + base, g->dw_trl[base + cnt], g->stream));
    }
  }
  HIP_TRY(g, launch_cov_pivots(d, A.n_fronts, g->stream));
  HIP_TRY(g, hipEventRecord(g->cov_ev[1], g->stream));
  // the root -> leaves pass: the update matrices in d.U are dead once their parents are assembled
  const CovDenseExtents ext{(long long)A.L_size, (long long)A.U_size};
  HIP_TRY(g, launch_cov_dense_pre(d, g->cov_S, g->cov_G, ext, g->cov_dtab, g->cov_dpre_items, A.n_fronts, g->stream));
  for (int l = A.n_levels - 1; l >= 0; l--) {
    const int* lv = g->cov_dlevel.data() + 4 * l;
    HIP_TRY(g, launch_cov_dense_level(d, g->cov_S, g->cov_G, ext, g->cov_parent, A.level_off[l], A.level_off[l + 1] - A.level_off[l], g->cov_dtab + lv[0], lv[1],
                                      g->cov_dtab + lv[2], lv[3], g->stream));
  }
  HIP_TRY(g, hipEventRecord(g->cov_ev[2], g->stream));
  double status[4] = {0, 0, 0, 0};
  HIP_TRY(g, hipMemcpyAsync(status, d.result_dev, sizeof status, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->cov_ev[0], g->cov_ev[2]) == hipSuccess) g->cov_sec[0] = 1e-3 * ms;
  if (hipEventElapsedTime(&ms, g->cov_ev[1], g->cov_ev[2]) == hipSuccess) g->cov_sec[1] = 1e-3 * ms;
  if (status[2] != 0.0) {
    HIP_TRY(g, launch_clear_status(d, g->stream));
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->status_clean = true;
  if (status[2] >= kStatusInternal) return fail(g, PPS_EHIP, "internal error: pps_cov_select met an index outside its front");
  if (status[2] != 0.0)
    return fail(g, PPS_ENOTPD, "normal equations not positive definite at lambda = 0 (a pivot was not positive, or below 1e-7 of the largest pivot of its front): no covariance");
  g->cov_version = g->upload_version;
  g->cov_valid = g->cov_factor_valid = true;
  return PPS_OK;
}

static int cov_select_impl(pps_graph* g) {
  if (!g->analyzed || g->analysis_stale) { const int rc = pps_analyze(g); if (rc != PPS_OK) return rc; }
  if (g->use_band && g->cov_select_form == 0) return cov_recover_impl(g);      // the band form: pps_cov_recover, launch for launch
  if (!g->use_band && !g->use_dense) return fail(g, PPS_ESTATE, no_factor_array(g));
  return cov_select_dense_impl(g);
}

bool cov_walk_wide(const pps_graph* g) {
  return g->cov_path_form == 1 || cov_path_lds_bytes(g->cov_max_p, g->cov_max_rows) > (size_t)64 * 1024;
}

int cov_walk_scratch(pps_graph* g, const CovWalks& cw) {
  if (!cov_walk_wide(g) || cw.walks.empty()) return PPS_OK;
  const size_t want = cw.walks.size() * cov_wide_scratch(cw.max_rows);
  if (want <= g->cov_zscr_cap && g->cov_zscr) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));           // (so that what cov_reserve can still fail with is the allocation)
  if (cov_reserve(g, &g->cov_zscr, &g->cov_zscr_cap, want) != PPS_OK) {
    (void)hipGetLastError();
    return fail(g, PPS_ENOMEM, "covariance path solves: no device memory for the right-hand sides of " + std::to_string(cw.walks.size()) + " walks through fronts of up to " +
                               std::to_string(cw.max_rows) + " rows (" + std::to_string(want * sizeof(double)) + " bytes): ask for fewer nodes per call");
  }
  return PPS_OK;
}

hipError_t cov_launch_walks(pps_graph* g, const CovWalks& cw, const CovWalk* walks, const CovStep* steps, double* out) {
  const int nw = (int)cw.walks.size(), ns = (int)cw.steps.size();
  if (cov_walk_wide(g))
    return launch_cov_path_wide(g->dev, walks, nw, steps, ns, cw.K, cw.max_rows, g->cov_zscr, (long long)g->cov_zscr_cap, g->cov_strip, cw.n_strip, out, g->stream);
  return launch_cov_path(g->dev, walks, nw, steps, ns, cw.K, g->cov_max_p, g->cov_max_rows, g->cov_strip, cw.n_strip, out, g->stream);
}

}  // namespace pps_impl

extern "C" {

int pps_cov_recover(pps_graph* g) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->n_live_factors == 0) return fail(g, PPS_ENOTPD, "normal equations not positive definite: the graph has no factor");
  // the figures of the last solve stay what they were: this call is no solve (the fields that describe the analysis follow the analysis)
  const pps_stats saved = g->stats;
  const int profiling = g->profiling;
  g->profiling = 0;
  const unsigned long long launches0 = g->launches0;
  const int rc = cov_recover_impl(g);
  g->profiling = profiling;
  g->launches0 = launches0;
  { pps_stats s = saved;
    s.n_fronts = g->stats.n_fronts; s.n_levels = g->stats.n_levels; s.max_front = g->stats.max_front; s.nnz_L = g->stats.nnz_L;
    g->stats = s; }
  if (rc == PPS_EHIP) abandon_device_copy(g);
  return rc;
}

int pps_cov_factor(pps_graph* g) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->n_live_factors == 0) return fail(g, PPS_ENOTPD, "normal equations not positive definite: the graph has no factor");
  // like pps_cov_recover: no solve, the figures of the last one stay
  const pps_stats saved = g->stats;
  const int profiling = g->profiling;
  g->profiling = 0;
  const unsigned long long launches0 = g->launches0;
  const int rc = cov_factor_impl(g);
  g->profiling = profiling;
  g->launches0 = launches0;
  { pps_stats s = saved;
    s.n_fronts = g->stats.n_fronts; s.n_levels = g->stats.n_levels; s.max_front = g->stats.max_front; s.nnz_L = g->stats.nnz_L;
    g->stats = s; }
  if (rc == PPS_EHIP) abandon_device_copy(g);
  return rc;
}

int pps_cov_select(pps_graph* g) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->n_live_factors == 0) return fail(g, PPS_ENOTPD, "normal equations not positive definite: the graph has no factor");
  // like pps_cov_recover: no solve, the figures of the last one stay
  const pps_stats saved = g->stats;
  const int profiling = g->profiling;
  g->profiling = 0;
  const unsigned long long launches0 = g->launches0;
  const int rc = cov_select_impl(g);
  g->profiling = profiling;
  g->launches0 = launches0;
  { pps_stats s = saved;
    s.n_fronts = g->stats.n_fronts; s.n_levels = g->stats.n_levels; s.max_front = g->stats.max_front; s.nnz_L = g->stats.nnz_L;
    g->stats = s; }
  if (rc == PPS_EHIP) abandon_device_copy(g);
  return rc;
}

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

int pps_cov_block_last(const pps_graph* g, double* kernel_sec, int* launches) {
  if (!g) return PPS_EINVAL;
  if (kernel_sec) *kernel_sec = g->cov_block_sec;
  if (launches) *launches = g->cov_block_launches;
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

int pps_cov_block(pps_graph* g, int nr, const int* rows, int nc, const int* cols, double* out) {
  if (!g || !rows || !out || nr < 0 || (cols && nc < 0)) return PPS_EINVAL;
  const bool joint = cols == nullptr;
  if (joint) { cols = rows; nc = nr; }
  // distinct nodes of the query: every one is walked once, however often it is asked for
  std::vector<int> walk_of(g->nodes.size(), -1), ids, ri((size_t)nr), ci((size_t)nc);
  std::vector<CovNode> nd;
  for (int pass = 0; pass < (joint ? 1 : 2); pass++) {
    const int n = pass ? nc : nr;
    const int* list = pass ? cols : rows;
    std::vector<char> seen(g->nodes.size(), 0);
    for (int i = 0; i < n; i++) {
      CovNode c;
      const int rc = cov_node(g, list[i], &c); if (rc != PPS_OK) return rc;
      if (seen[list[i]]) return fail(g, PPS_EINVAL, "covariance block: node " + std::to_string(list[i]) + " is listed twice among the " + (pass ? "columns" : "rows"));
      seen[list[i]] = 1;
      if (walk_of[list[i]] < 0) { walk_of[list[i]] = (int)ids.size(); ids.push_back(list[i]); nd.push_back(c); }
      (pass ? ci : ri)[i] = walk_of[list[i]];
    }
  }
  if (joint) ci = ri;
  if (!cov_factor_current(g)) return fail(g, PPS_ESTATE, kNoRecovery);
  if (nr == 0 || nc == 0) return PPS_OK;
  CovWalks cw;
  { const int rc = cov_build_walks(g, ids, nd, &cw); if (rc != PPS_OK) return rc; }
  const int K = cw.K;
  const long long n_strip = cw.n_strip;
  const std::vector<CovWalk>& walks = cw.walks;
  const std::vector<CovStep>& steps = cw.steps;
  auto common = [&](int a, int b) { return cov_common_pivots(g, cw, a, b); };
  std::vector<int> roff((size_t)nr + 1, 0), coff((size_t)nc + 1, 0);
  for (int i = 0; i < nr; i++) roff[i + 1] = roff[i] + nd[ri[i]].dim;
  for (int j = 0; j < nc; j++) coff[j + 1] = coff[j] + nd[ci[j]].dim;
  const int ld = coff[nc];
  const long long n_out = (long long)roff[nr] * ld;
  std::vector<CovPair> pairs;
  pairs.reserve(joint ? (size_t)nr * (nr + 1) / 2 : (size_t)nr * nc);
  for (int i = 0; i < nr; i++)
    for (int j = 0; j < (joint ? i + 1 : nc); j++) {
      const int a = ri[i], b = ci[j], len = common(a, b);
      CovPair q;
      q.yi = walks[a].strip + (long long)(K - len) * nd[a].dim; q.yj = walks[b].strip + (long long)(K - len) * nd[b].dim;
      q.dst = (long long)roff[i] * ld + coff[j];
      q.dst_t = joint ? (long long)roff[j] * ld + coff[i] : -1;          // (cols = rows: the lower triangle, mirrored)
      q.di = nd[a].dim; q.dj = nd[b].dim; q.len = len; q.ld = ld;
      pairs.push_back(q);
    }
  // one request: [walks | steps | pairs]
  const size_t o_steps = walks.size() * sizeof(CovWalk), o_pairs = (o_steps + steps.size() * sizeof(CovStep) + 15) & ~(size_t)15;
  std::vector<char> req(o_pairs + pairs.size() * sizeof(CovPair));
  memcpy(req.data(), walks.data(), walks.size() * sizeof(CovWalk));
  memcpy(req.data() + o_steps, steps.data(), steps.size() * sizeof(CovStep));
  memcpy(req.data() + o_pairs, pairs.data(), pairs.size() * sizeof(CovPair));
  HIP_TRY(g, hipSetDevice(g->props.device));
  for (hipEvent_t& e : g->cov_bev) if (!e) HIP_TRY(g, hipEventCreate(&e));
  int rc = cov_reserve(g, &g->cov_breq, &g->cov_breq_cap, req.size()); if (rc != PPS_OK) return rc;
  rc = cov_reserve(g, &g->cov_strip, &g->cov_strip_cap, (size_t)n_strip); if (rc != PPS_OK) return rc;
  rc = cov_walk_scratch(g, cw); if (rc != PPS_OK) return rc;
  if ((size_t)n_out + 1 > g->cov_bout_cap || !g->cov_bout) g->cov_bout_clean = false;
  rc = cov_reserve(g, &g->cov_bout, &g->cov_bout_cap, (size_t)n_out + 1); if (rc != PPS_OK) return rc;
  if (!g->cov_bout_clean) HIP_TRY(g, hipMemsetAsync(g->cov_bout, 0, sizeof(double), g->stream));      // (a new buffer, or a query that failed)
  g->cov_bout_clean = false;
  const unsigned long long launches0 = launch_count();
  HIP_TRY(g, hipMemcpyAsync(g->cov_breq, req.data(), req.size(), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(g, hipEventRecord(g->cov_bev[0], g->stream));
  HIP_TRY(g, cov_launch_walks(g, cw, reinterpret_cast<const CovWalk*>(g->cov_breq), reinterpret_cast<const CovStep*>(g->cov_breq + o_steps), g->cov_bout));
  HIP_TRY(g, launch_cov_gram(reinterpret_cast<const CovPair*>(g->cov_breq + o_pairs), (int)pairs.size(), g->cov_strip, n_strip, g->cov_bout, n_out, g->stream));
  HIP_TRY(g, hipEventRecord(g->cov_bev[1], g->stream));
  std::vector<double> host((size_t)n_out + 1);
  HIP_TRY(g, hipMemcpyAsync(host.data(), g->cov_bout, host.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  g->cov_block_launches = (int)(launch_count() - launches0);
  float ms = 0;
  if (hipEventElapsedTime(&ms, g->cov_bev[0], g->cov_bev[1]) == hipSuccess) g->cov_block_sec = 1e-3 * ms;
  if (host[0] != 0.0) return fail(g, PPS_EHIP, "internal error: a covariance path solve met an index outside its front or its strip");
  g->cov_bout_clean = true;
  memcpy(out, host.data() + 1, (size_t)n_out * sizeof(double));
  return PPS_OK;
}

}  // extern "C"
