// pps_map_grid.cpp -- host side of the grid map (include/pps.h: pps_map_build_grid and the pps_map_grid_* calls): the plane table of the
// selection (MapSelection, pps_map_host.h), the frames, the layout of the cell arrays between the passes, and the calls that drive the
// kernels of pps_grid.hip.  The record of the last grid (MapGrid) lives in pps_map_grid_host.h: pps_map_render.cpp reads it, and every
// grid call ends the view rendered from the grid before (MapGrid::clear).
//
// One call synchronises the graph's stream three times, each time for a small table the host has to read: after the extent pass (the boxes
// decide the size of the cell arrays and the max_cells refusal), after the count / scan (the emitted cells decide the size of the output),
// and at the end.  The estimate is brought to the device by prepare_solve, like pps_map_build; the frames are computed from the host's
// copy of the same doubles (download_state brings it home when the device holds the newer estimate).
#include "pps_grid.h"
#include "pps_grid_cell.h"
#include "pps_map_grid_host.h"

#include <climits>
#include <cstdlib>

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

void map_grid_release(pps_map* m) {
  MapGrid* gr = m ? m->grid : nullptr;
  if (!gr) return;
  gr->sel.release(); gr->d_planes.release(); gr->small.release(); gr->plane_tab.release(); gr->key.release(); gr->cnt.release();
  gr->tile_count.release(); gr->tile_prefix.release(); gr->out_pts.release(); gr->out_cnt.release(); gr->out_ij.release(); gr->out_src.release();
  for (MapSpan* t : {&gr->t_extent, &gr->t_vote, &gr->t_count, &gr->t_emit, &gr->t_call}) t->release();
  gr->render.release();
  delete gr;
  m->grid = nullptr;
}

}  // namespace pps_impl

namespace {

int64_t sat_add(int64_t a, int64_t b) { return a > INT64_MAX - b ? INT64_MAX : a + b; }

// PPS_GRID_VOTE=direct: every point sends its own atomics (the form tools/map_grid_bench.py measures the in-wave combining against)
bool vote_combines() {
  const char* v = getenv("PPS_GRID_VOTE");
  return !(v && std::string(v) == "direct");
}

int build_grid(pps_map* m, const pps_map_select* sel, const pps_map_grid_params& prm, bool posed, int64_t* n_points, int* n_planes) {
  pps_graph* g = m->g;
  MapGrid& G = *m->grid;
  hipStream_t st = g->stream;
  const double inv_cell = 1.0 / prm.cell;
  // ---- the selection: B's chunks, the plane table
  MapSelection s;
  s.select(m, sel);
  const int n = (int)m->chunks.size();
  std::map<int, int> row_of;                            // live plane node id -> row (ascending ids)
  for (int i = 0; i < n; i++)
    if (s.keep[i] && live_node(g, m->chunks[i].plane_id, NODE_PLANE)) row_of[m->chunks[i].plane_id] = 0;
  std::vector<pps_map_grid_plane> planes(row_of.size());
  {
    int r = 0;
    for (auto& kv : row_of) { kv.second = r; planes[r] = pps_map_grid_plane{}; planes[r].plane_id = kv.first; r++; }
  }
  const int64_t total = s.total;
  int64_t through = 0;
  for (int i = 0; i < n; i++) {
    if (!s.keep[i]) continue;
    const pps_map_chunk& c = m->chunks[i];
    const auto it = live_node(g, c.plane_id, NODE_PLANE) ? row_of.find(c.plane_id) : row_of.end();
    if (it != row_of.end()) planes[it->second].n_chunks++; else through += c.count;
  }
  const int nL = (int)planes.size();
  pps_map_grid_totals tot{};
  tot.n_points = total; tot.n_passed_through = through; tot.n_planes = nL; tot.cell = prm.cell; tot.inv_cell = inv_cell;
  const bool device = total - through > 0;
  std::vector<double> plane_eq;
  int64_t n_box_cells = 0;
  if (device) {
    const int rc = prepare_solve(g);
    if (rc != PPS_OK) return mfail(m, rc, g->err);
  }
  if (nL > 0) {                                         // the frames, from the doubles the device projects with
    const int rc = download_state(g);
    if (rc != PPS_OK) return mfail(m, rc, g->err);
    for (pps_map_grid_plane& p : planes) {
      if (!grid_frame(g->nodes[p.plane_id].v, p.n, p.e1, p.e2))
        return mfail(m, PPS_EINVAL, "build_grid: plane node " + std::to_string(p.plane_id) + " has no normal");
      plane_eq.insert(plane_eq.end(), g->nodes[p.plane_id].v, g->nodes[p.plane_id].v + 4);       // kept with the grid (pps_map_grid_plane_eq)
    }
  }
  if (device) {
    int rc = map_use_device(m);
    if (rc != PPS_OK) return rc;
    std::vector<GridPlaneDev> pd((size_t)nL);
    for (int L = 0; L < nL; L++) {
      pd[L] = GridPlaneDev{};
      for (int k = 0; k < 3; k++) { pd[L].e1[k] = planes[L].e1[k]; pd[L].e2[k] = planes[L].e2[k]; }
    }
    const size_t small_bytes = (size_t)nL * sizeof(GridExtent) + sizeof(unsigned long long);
    std::vector<char> small(small_bytes, 0);
    GridExtent* ext = reinterpret_cast<GridExtent*>(small.data());
    for (int L = 0; L < nL; L++) ext[L] = GridExtent{INT_MAX, INT_MIN, INT_MAX, INT_MIN, 0ull};
    MAP_TRY(m, hipStreamSynchronize(st));
    MAP_TRY(m, G.d_planes.reserve((size_t)nL, st));
    MAP_TRY(m, G.small.reserve(small_bytes, st));
    MAP_TRY(m, G.plane_tab.reserve(2 * ((size_t)nL + 1), st));
    // ---- tables of the selection (posed: the frame rows and records ride in the same upload)
    rc = s.upload(m, posed, &row_of, &G.sel, 1, &G.t_call);
    if (rc != PPS_OK) return rc;
    MAP_TRY(m, hipMemcpyAsync(G.d_planes.p, pd.data(), (size_t)nL * sizeof(GridPlaneDev), hipMemcpyHostToDevice, st));
    MAP_TRY(m, hipMemcpyAsync(G.small.p, small.data(), small_bytes, hipMemcpyHostToDevice, st));
    GridSelArgs a{};
    a.n_out = total; a.n_sel = s.n();
    a.out_off = s.out_off(); a.src_off = s.src_off(); a.slot = s.slot(); a.lm = s.lm();
    a.plane_est = g->dev.plane_est; a.plane_ld = g->dev.plane_ld;
    a.store = m->d_store.p;
    a.planes = G.d_planes.p; a.n_planes = nL;
    a.inv_cell = inv_cell;
    MapMotionTable mt{};                                             // (all null: B is pps_map_build's)
    if (posed) {
      rc = map_motion_launch(m, s, &mt);
      if (rc != PPS_OK) return rc;
    }
    // ---- pass 1: extents
    GridExtent* d_ext = reinterpret_cast<GridExtent*>(G.small.p);
    unsigned long long* d_dropped = reinterpret_cast<unsigned long long*>(G.small.p + (size_t)nL * sizeof(GridExtent));
    MAP_TRY(m, G.t_extent.begin(st));
    MAP_TRY(m, launch_grid_extent(a, d_ext, d_dropped, st, mt));
    MAP_TRY(m, G.t_extent.end(st));
    MAP_TRY(m, hipMemcpyAsync(small.data(), G.small.p, small_bytes, hipMemcpyDeviceToHost, st));
    MAP_TRY(m, hipStreamSynchronize(st));
    tot.launches = 1;
    tot.sec[0] = G.t_extent.seconds();
    if (posed) { m->posed_sec[0] = m->t_motion.seconds(); m->posed_launches = 1; }        // (k_map_motion: counted by pps_map_posed_last)
    tot.n_dropped = (int64_t) * reinterpret_cast<unsigned long long*>(small.data() + (size_t)nL * sizeof(GridExtent));
    // ---- the boxes and the layout of the cell arrays
    int64_t all = 0, largest = -1;
    int largest_row = -1;
    std::vector<long long> ptab(2 * ((size_t)nL + 1), 0);
    for (int L = 0; L < nL; L++) {
      pps_map_grid_plane& p = planes[L];
      p.n_in = (int64_t)ext[L].n_in; tot.n_in += p.n_in;
      if (p.n_in > 0) { p.i0 = ext[L].imin; p.j0 = ext[L].jmin; p.ni = ext[L].imax - ext[L].imin + 1; p.nj = ext[L].jmax - ext[L].jmin + 1; }
      const int64_t box = (int64_t)p.ni * (int64_t)p.nj;
      if (box > largest) { largest = box; largest_row = L; }
      ptab[L] = all;
      pd[L].base = all; pd[L].i0 = p.i0; pd[L].j0 = p.j0; pd[L].ni = p.ni; pd[L].nj = p.nj;
      all = sat_add(all, box);
    }
    ptab[nL] = all;
    if (tot.n_in + tot.n_dropped + tot.n_passed_through != tot.n_points) return mfail(m, PPS_EHIP, "build_grid: the extent pass lost points");
    if (all > prm.max_cells) {
      const pps_map_grid_plane& p = planes[largest_row];
      return mfail(m, PPS_ENOMEM, "build_grid: the boxes of " + std::to_string(nL) + " landmarks hold " + (all == INT64_MAX ? std::string("more than 2^63") : std::to_string(all)) +
                                      " cells, max_cells is " + std::to_string(prm.max_cells) + "; the largest is plane node " + std::to_string(p.plane_id) + ": " +
                                      std::to_string(p.ni) + " x " + std::to_string(p.nj) + " cells of " + std::to_string(prm.cell) + " m from (" + std::to_string(p.i0) + ", " +
                                      std::to_string(p.j0) + ") for " + std::to_string(p.n_in) + " points (a far outlier makes such a box)");
    }
    n_box_cells = all;
    if (all > 0) {
      const GridTiling t = grid_tiling(all);
      MAP_TRY(m, G.key.reserve((size_t)all, st));
      MAP_TRY(m, G.cnt.reserve((size_t)all, st));
      MAP_TRY(m, G.tile_count.reserve((size_t)t.nT, st));
      MAP_TRY(m, G.tile_prefix.reserve((size_t)t.nT + 1, st));
      MAP_TRY(m, hipMemcpyAsync(G.d_planes.p, pd.data(), (size_t)nL * sizeof(GridPlaneDev), hipMemcpyHostToDevice, st));
      MAP_TRY(m, hipMemcpyAsync(G.plane_tab.p, ptab.data(), ((size_t)nL + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
      // ---- pass 2: votes
      MAP_TRY(m, G.t_vote.begin(st));
      MAP_TRY(m, hipMemsetAsync(G.key.p, 0, (size_t)all * sizeof(unsigned long long), st));
      MAP_TRY(m, hipMemsetAsync(G.cnt.p, 0, (size_t)all * sizeof(unsigned int), st));
      MAP_TRY(m, launch_grid_vote(a, prm.rule == PPS_GRID_OLDEST, vote_combines(), G.key.p, G.cnt.p, st, mt));
      MAP_TRY(m, G.t_vote.end(st));
      // ---- pass 3: emission
      GridEmitArgs e{};
      e.n_cells_all = all; e.min_count = (unsigned int)prm.min_count; e.oldest = prm.rule == PPS_GRID_OLDEST;
      e.key = G.key.p; e.cnt = G.cnt.p; e.tile_count = G.tile_count.p; e.tile_prefix = G.tile_prefix.p;
      e.plane_base = G.plane_tab.p; e.plane_off = G.plane_tab.p + (nL + 1);
      MAP_TRY(m, G.t_count.begin(st));
      MAP_TRY(m, launch_grid_count(e, nL, st));
      MAP_TRY(m, G.t_count.end(st));
      MAP_TRY(m, hipMemcpyAsync(ptab.data() + (nL + 1), e.plane_off, ((size_t)nL + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
      MAP_TRY(m, hipStreamSynchronize(st));
      tot.launches += 4;
      const long long* poff = ptab.data() + (nL + 1);
      tot.n_cells = poff[nL];
      for (int L = 0; L < nL; L++) { planes[L].offset = poff[L]; planes[L].count = poff[L + 1] - poff[L]; }
      tot.sec[1] = G.t_vote.seconds(); tot.sec[2] = G.t_count.seconds();
      if (tot.n_cells > 0) {
        const size_t nc = (size_t)tot.n_cells;
        MAP_TRY(m, G.out_pts.reserve(nc, st)); MAP_TRY(m, G.out_cnt.reserve(nc, st)); MAP_TRY(m, G.out_ij.reserve(2 * nc, st)); MAP_TRY(m, G.out_src.reserve(nc, st));
        e.pts = G.out_pts.p; e.counts = G.out_cnt.p; e.ij = G.out_ij.p; e.src = G.out_src.p;
        MAP_TRY(m, G.t_emit.begin(st));
        MAP_TRY(m, launch_grid_emit(a, e, st, mt));
        MAP_TRY(m, G.t_emit.end(st));
        tot.launches += 1;
      }
    }
    MAP_TRY(m, G.t_call.end(st));
    MAP_TRY(m, hipStreamSynchronize(st));
    if (tot.n_cells > 0) tot.sec[2] += G.t_emit.seconds();
    tot.sec[3] = G.t_call.seconds();
  }
  G.planes.swap(planes);
  G.plane_eq.swap(plane_eq);
  G.tot = tot;
  G.n_box_cells = n_box_cells; G.min_count = prm.min_count;
  G.valid = true;
  if (n_points) *n_points = tot.n_cells;
  if (n_planes) *n_planes = nL;
  return PPS_OK;
}

}  // namespace

extern "C" {

void pps_map_grid_default_params(pps_map_grid_params* p) {
  if (!p) return;
  p->cell = 0.02; p->rule = PPS_GRID_NEWEST; p->min_count = 1; p->max_cells = (int64_t)1 << 26;
}

static int build_grid_checked(pps_map* m, const pps_map_select* sel, const pps_map_grid_params* prm, bool posed, int64_t* n_points, int* n_planes) {
  if (!m) return PPS_EINVAL;
  if (posed) map_posed_reset(m);
  if (m->grid) m->grid->clear();
  pps_map_grid_params p;
  pps_map_grid_default_params(&p);
  if (prm) p = *prm;
  if (!(p.cell > 0.0) || !std::isfinite(p.cell) || !std::isfinite(1.0 / p.cell)) return mfail(m, PPS_EINVAL, "build_grid: cell must be finite and positive, and 1 / cell finite");
  if (p.rule != PPS_GRID_NEWEST && p.rule != PPS_GRID_OLDEST) return mfail(m, PPS_EINVAL, "build_grid: rule is PPS_GRID_NEWEST (0) or PPS_GRID_OLDEST (1)");
  if (p.min_count < 1) return mfail(m, PPS_EINVAL, "build_grid: min_count must be at least 1");
  if (p.max_cells < 1) return mfail(m, PPS_EINVAL, "build_grid: max_cells must be at least 1");
  if (!map_select_valid(sel)) return mfail(m, PPS_EINVAL, "build_grid: old_every and new_every must be positive");
  if (!m->grid) {
    m->grid = new (std::nothrow) MapGrid();
    if (!m->grid) return mfail(m, PPS_ENOMEM, "build_grid: out of host memory");
  }
  const int rc = build_grid(m, sel, p, posed, n_points, n_planes);
  if (rc != PPS_OK) m->grid->clear();
  return rc;
}

int pps_map_build_grid(pps_map* m, const pps_map_select* sel, const pps_map_grid_params* prm, int64_t* n_points, int* n_planes) {
  return build_grid_checked(m, sel, prm, false, n_points, n_planes);
}
int pps_map_build_grid_posed(pps_map* m, const pps_map_select* sel, const pps_map_grid_params* prm, int64_t* n_points, int* n_planes) {
  return build_grid_checked(m, sel, prm, true, n_points, n_planes);
}

int pps_map_grid_planes(const pps_map* m, int cap, pps_map_grid_plane* out, int* n) {
  if (!m) return PPS_EINVAL;
  const MapGrid* G = m->grid;
  const bool have = G && G->valid;
  return map_table_copy(have ? G->planes.data() : nullptr, have ? G->planes.size() : 0, cap, out, n);
}

int pps_map_grid_info(const pps_map* m, pps_map_grid_totals* out) {
  if (!m || !out) return PPS_EINVAL;
  *out = m->grid && m->grid->valid ? m->grid->tot : pps_map_grid_totals{};
  return PPS_OK;
}

int pps_map_grid_download(pps_map* m, int64_t first, int64_t n, pps_point* pts, uint32_t* counts, int32_t* ij, int64_t* src) {
  if (!m) return PPS_EINVAL;
  MapGrid* G = m->grid;
  const int64_t have = G && G->valid ? G->tot.n_cells : 0;
  if (first < 0 || n < 0 || first > have || n > have - first) return mfail(m, PPS_EINVAL, "grid_download: range outside the grid");
  if (n == 0 || (!pts && !counts && !ij && !src)) return PPS_OK;
  hipStream_t st = m->g->stream;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  if (pts) MAP_TRY(m, hipMemcpyAsync(pts, G->out_pts.p + first, (size_t)n * sizeof(MapPt), hipMemcpyDeviceToHost, st));
  if (counts) MAP_TRY(m, hipMemcpyAsync(counts, G->out_cnt.p + first, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  if (ij) MAP_TRY(m, hipMemcpyAsync(ij, G->out_ij.p + 2 * first, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (src) MAP_TRY(m, hipMemcpyAsync(src, G->out_src.p + first, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  return PPS_OK;
}

int pps_map_grid_frame_host(const double abcd[4], double n[3], double e1[3], double e2[3]) {
  if (!abcd || !n || !e1 || !e2) return PPS_EINVAL;
  return grid_frame(abcd, n, e1, e2) ? PPS_OK : PPS_EINVAL;
}

int pps_map_grid_cell_host(const double e[3], double inv_cell, const float xyz[3], int64_t* cell, int* dropped) {
  if (!e || !xyz || !cell || !dropped) return PPS_EINVAL;
  long long c = 0;
  *dropped = grid_cell(e, inv_cell, xyz[0], xyz[1], xyz[2], &c) ? 0 : 1;
  *cell = (int64_t)c;
  return PPS_OK;
}

}  // extern "C"
