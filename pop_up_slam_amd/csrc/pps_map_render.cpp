// pps_map_render.cpp -- host side of the rendered view (include/pps.h: pps_map_render and the pps_map_render_* calls): the argument checks,
// the landmark rows of the last grid (pps_map_grid_host.h), the slot table made once per grid, the images, and the calls that drive the
// kernels of pps_render.hip.  A render reads the grid's buffers and writes only its own; it runs on the graph's stream and synchronises
// it once, for the hit count.
#include "pps_map_grid_host.h"
#include "pps_map_move.h"
#include "pps_render.h"
#include "pps_render_ray.h"

#include <climits>

using namespace pps;
using namespace pps_impl;

namespace {

const char* view_refusal(const pps_map_view* v) {
  if (v->width < 1 || v->width > kRenderMaxSide || v->height < 1 || v->height > kRenderMaxSide) return "render: width and height must be 1 .. 4096";
  if (v->reach < 0 || v->reach > kRenderMaxReach) return "render: reach must be 0 .. 4";
  if (v->reserved != 0) return "render: reserved must be 0";
  for (int k = 0; k < 9; k++)
    if (!std::isfinite(v->invK[k])) return "render: invK is not finite";
  if (!map_rigid(v->T_wc)) return "render: T_wc is not a rigid transform (finite, last row 0 0 0 1, R^T R = I to 1e-4)";
  if (!std::isfinite(v->z_near) || v->z_near < 0.0) return "render: z_near must be finite and not negative";
  if (std::isnan(v->z_far) || !(v->z_far > v->z_near)) return "render: z_far must be greater than z_near";
  return nullptr;
}

// room for the slot table of grid G, its landmark rows and their ids on the device (the caller fills the slot table with a launch)
int render_tables(pps_map* m, MapGrid& G, hipStream_t st) {
  MapRender& R = G.render;
  if (G.tot.n_cells > INT_MAX) return mfail(m, PPS_ENOMEM, "render: the slot table holds int indices, the grid has more than 2^31 - 1 cells");
  std::vector<RenderPlane> rows;
  std::vector<int> ids;
  for (size_t L = 0; L < G.planes.size(); L++) {
    const pps_map_grid_plane& p = G.planes[L];
    if ((int64_t)p.ni * (int64_t)p.nj == 0) continue;
    RenderPlane r{};
    if (!render_plane(&G.plane_eq[4 * L], &r)) continue;             // (never: grid_frame accepted these doubles when the grid was built)
    r.base = 0; r.i0 = p.i0; r.j0 = p.j0; r.ni = p.ni; r.nj = p.nj;
    rows.push_back(r); ids.push_back(p.plane_id);
  }
  long long base = 0;                                                // the boxes back to back in row order, empty ones take no room: build_grid's layout
  for (RenderPlane& r : rows) { r.base = base; base += (long long)r.ni * r.nj; }
  if (base != G.n_box_cells) return mfail(m, PPS_EHIP, "render: the boxes of the plane table do not add up to the grid's cell arrays");
  const size_t nr = rows.size();
  MAP_TRY(m, R.slot.reserve((size_t)G.n_box_cells, st));
  MAP_TRY(m, R.rows.reserve(nr, st));
  MAP_TRY(m, R.ids.reserve(nr, st));
  MAP_TRY(m, hipMemcpyAsync(R.rows.p, rows.data(), nr * sizeof(RenderPlane), hipMemcpyHostToDevice, st));
  MAP_TRY(m, hipMemcpyAsync(R.ids.p, ids.data(), nr * sizeof(int), hipMemcpyHostToDevice, st));
  MAP_TRY(m, hipStreamSynchronize(st));                              // (rows and ids go out of scope)
  R.n_rows = (int)nr;
  return PPS_OK;
}

int render(pps_map* m, MapGrid& G, const pps_map_view* v, pps_map_render_totals* tot) {
  MapRender& R = G.render;
  tot->width = v->width; tot->height = v->height;
  if (G.tot.n_cells == 0) { R.on_host = true; return PPS_OK; }       // nothing can answer: every pixel is empty, no device
  R.on_host = false;
  hipStream_t st = m->g->stream;
  int rc = map_use_device(m);
  if (rc != PPS_OK) return rc;
  const size_t npx = (size_t)v->width * (size_t)v->height;
  MAP_TRY(m, R.cloud.reserve(npx, st)); MAP_TRY(m, R.depth.reserve(npx, st)); MAP_TRY(m, R.plane_id.reserve(npx, st)); MAP_TRY(m, R.cell.reserve(npx, st));
  MAP_TRY(m, R.n_hit.reserve(1, st));
  MAP_TRY(m, hipMemsetAsync(R.n_hit.p, 0, sizeof(unsigned long long), st));
  const int slots = R.tables ? 0 : 1;                                // the first render after a grid fills the slot table
  if (slots) {
    rc = render_tables(m, G, st);
    if (rc != PPS_OK) return rc;
  }
  MAP_TRY(m, R.t_kernels.begin(st));
  if (slots) {
    MAP_TRY(m, launch_render_slots(G.n_box_cells, (unsigned int)G.min_count, G.cnt.p, G.tile_prefix.p, R.slot.p, st));
    R.tables = true;
  }
  RenderArgs a{};
  a.width = v->width; a.height = v->height; a.reach = v->reach; a.n_rows = R.n_rows;
  for (int k = 0; k < 9; k++) a.iK[k] = v->invK[k];
  for (int k = 0; k < 16; k++) a.T[k] = v->T_wc[k];
  a.z_near = v->z_near; a.z_far = v->z_far; a.inv_cell = G.tot.inv_cell;
  a.rows = R.rows.p; a.ids = R.ids.p; a.slot = R.slot.p; a.pts = G.out_pts.p;
  a.cloud = R.cloud.p; a.depth = R.depth.p; a.plane_id = R.plane_id.p; a.cell = R.cell.p; a.n_hit = R.n_hit.p;
  MAP_TRY(m, launch_render(a, st));
  MAP_TRY(m, R.t_kernels.end(st));
  unsigned long long n_hit = 0;
  MAP_TRY(m, hipMemcpyAsync(&n_hit, R.n_hit.p, sizeof n_hit, hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  tot->n_planes = R.n_rows; tot->launches = 1 + slots; tot->n_hit = (int64_t)n_hit; tot->sec = R.t_kernels.seconds();
  return PPS_OK;
}

}  // namespace

extern "C" {

void pps_map_default_view(pps_map_view* v, int width, int height, const float invK[9], const float T_wc[16]) {
  if (!v) return;
  *v = pps_map_view{};
  v->width = width; v->height = height; v->reach = 1;
  if (invK) memcpy(v->invK, invK, sizeof v->invK);
  if (T_wc) memcpy(v->T_wc, T_wc, sizeof v->T_wc);
  v->z_near = 0.0; v->z_far = INFINITY;
}

int pps_map_render(pps_map* m, const pps_map_view* v, int64_t* n_hit) {
  if (!m || !v) return PPS_EINVAL;
  if (const char* why = view_refusal(v)) return mfail(m, PPS_EINVAL, why);
  MapGrid* G = m->grid;
  if (!G || !G->valid) return mfail(m, PPS_ESTATE, "render: there is no grid (no pps_map_build_grid call has succeeded, or the last one failed)");
  pps_map_render_totals tot{};
  G->render.compare.valid = false;                                   // a comparison is of the view that goes now
  const int rc = render(m, *G, v, &tot);
  if (rc != PPS_OK) {                                                // the grid stays; the view that was there is gone
    const bool tables = G->render.tables;
    const int n_rows = G->render.n_rows;
    G->render.clear();
    G->render.tables = tables; G->render.n_rows = n_rows;
    return rc;
  }
  G->render.tot = tot;
  G->render.valid = true;
  if (n_hit) *n_hit = tot.n_hit;
  return PPS_OK;
}

int pps_map_render_download(pps_map* m, pps_point* cloud, float* depth, int32_t* plane_id, int64_t* cell) {
  if (!m) return PPS_EINVAL;
  MapGrid* G = m->grid;
  if (!G || !G->valid || !G->render.valid) return mfail(m, PPS_ESTATE, "render_download: no rendered view (pps_map_render first; a grid call ends the view)");
  MapRender& R = G->render;
  const size_t npx = (size_t)R.tot.width * (size_t)R.tot.height;
  if (!cloud && !depth && !plane_id && !cell) return PPS_OK;
  if (R.on_host) {
    if (cloud) memset(cloud, 0, npx * sizeof(pps_point));
    for (size_t i = 0; i < npx; i++) {
      if (depth) depth[i] = 0.f;
      if (plane_id) plane_id[i] = -1;
      if (cell) cell[i] = -1;
    }
    return PPS_OK;
  }
  hipStream_t st = m->g->stream;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  if (cloud) MAP_TRY(m, hipMemcpyAsync(cloud, R.cloud.p, npx * sizeof(MapPt), hipMemcpyDeviceToHost, st));
  if (depth) MAP_TRY(m, hipMemcpyAsync(depth, R.depth.p, npx * sizeof(float), hipMemcpyDeviceToHost, st));
  if (plane_id) MAP_TRY(m, hipMemcpyAsync(plane_id, R.plane_id.p, npx * sizeof(int), hipMemcpyDeviceToHost, st));
  if (cell) MAP_TRY(m, hipMemcpyAsync(cell, R.cell.p, npx * sizeof(long long), hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  return PPS_OK;
}

int pps_map_render_info(const pps_map* m, pps_map_render_totals* out) {
  if (!m || !out) return PPS_EINVAL;
  const MapGrid* G = m->grid;
  if (!G || !G->valid || !G->render.valid) return PPS_ESTATE;
  *out = G->render.tot;
  return PPS_OK;
}

int pps_map_grid_plane_eq(const pps_map* m, int cap, double* abcd, int* n) {
  if (!m || !map_table_args(cap, abcd, n)) return PPS_EINVAL;
  const MapGrid* G = m->grid;
  const size_t have = G && G->valid ? G->planes.size() : 0;
  *n = (int)have;
  const size_t k = std::min<size_t>((size_t)cap, have);
  if (k) memcpy(abcd, G->plane_eq.data(), 4 * k * sizeof(double));
  return PPS_OK;
}

int pps_map_render_ray_host(const pps_map_view* v, int col, int row, double o[3], double ds[3], double dw[3]) {
  if (!v || !o || !ds || !dw) return PPS_EINVAL;
  render_ray(v->invK, v->T_wc, col, row, o, ds, dw);
  return PPS_OK;
}

int pps_map_render_hit_host(const double o[3], const double ds[3], const double dw[3], const double abcd[4], double inv_cell, double z_near,
                            double z_far, double* z, float xyz[3], int64_t ij[2]) {
  if (!o || !ds || !dw || !abcd || !z || !xyz || !ij) return -1;
  RenderPlane r{};
  if (!render_plane(abcd, &r)) return -1;
  double t = 0.0;
  long long ci = 0, cj = 0;
  double zz = 0.0;
  float xf[3] = {0.f, 0.f, 0.f};
  const bool hit = render_depth(o, ds, dw, r, z_near, z_far, &t, &zz) && render_point(o, dw, t, r, inv_cell, xf, &ci, &cj);
  *z = hit ? zz : 0.0;
  for (int k = 0; k < 3; k++) xyz[k] = hit ? xf[k] : 0.f;
  ij[0] = hit ? (int64_t)ci : 0; ij[1] = hit ? (int64_t)cj : 0;
  return hit ? 1 : 0;
}

}  // extern "C"
