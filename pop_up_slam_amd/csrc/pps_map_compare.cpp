// pps_map_compare.cpp -- host side of the compared views (include/pps.h: pps_map_compare and the pps_map_compare_* calls): the argument
// checks, the plane rows of the last grid as the kernel wants them, the table and the result buffers, and the one function that drives the
// kernels of pps_compare.hip for both entry points.  A comparison reads the render's plane ids and the frame's pixels and writes only its
// own buffers; it runs on the graph's stream and synchronises it once, for the totals and the plane records.
#include "pps_compare.h"
#include "pps_compare_px.h"
#include "pps_map_grid_host.h"
#include "pps_popup_host.h"

#include <climits>

using namespace pps;
using namespace pps_impl;

namespace {

// what both entry points ask before they look at the frame: *G the grid whose view is compared
int compare_checked(pps_map* m, const char* who, int nplanes, double tol, MapGrid** G) {
  if (nplanes < 1 || nplanes > kComparePlanes) return mfail(m, PPS_EINVAL, std::string(who) + ": nplanes must be 1 .. 65");
  if (!std::isfinite(tol) || tol < 0.0) return mfail(m, PPS_EINVAL, std::string(who) + ": tol must be finite and not negative");
  *G = m->grid;
  if (!*G || !(*G)->valid || !(*G)->render.valid)
    return mfail(m, PPS_ESTATE, std::string(who) + ": no rendered view (pps_map_render first; a grid call ends the view)");
  return PPS_OK;
}

// the plane rows and their node ids on the device, once per grid
int compare_tables(pps_map* m, MapGrid& G, hipStream_t st) {
  MapCompare& C = G.render.compare;
  const size_t nr = G.planes.size();
  std::vector<ComparePlane> rows(nr);
  std::vector<int> ids(nr);
  for (size_t L = 0; L < nr; L++) {
    ids[L] = G.planes[L].plane_id;
    if (!compare_plane(&G.plane_eq[4 * L], &rows[L])) rows[L] = ComparePlane{};    // (never: grid_frame accepted these doubles when the grid was built)
  }
  MAP_TRY(m, C.planes.reserve(nr, st));
  MAP_TRY(m, C.ids.reserve(nr, st));
  if (nr) {
    MAP_TRY(m, hipMemcpyAsync(C.planes.p, rows.data(), nr * sizeof(ComparePlane), hipMemcpyHostToDevice, st));
    MAP_TRY(m, hipMemcpyAsync(C.ids.p, ids.data(), nr * sizeof(int), hipMemcpyHostToDevice, st));
    MAP_TRY(m, hipStreamSynchronize(st));                            // (rows and ids go out of scope)
  }
  C.tables = true;
  return PPS_OK;
}

// A comparison from the point where the frame's pixels are on the device (cloud, frame_id: width * height records each, complete for the
// graph's stream) and every argument has been checked.
int compare(pps_map* m, MapGrid& G, const MapPt* cloud, const int* frame_id, int nplanes, double tol, pps_map_compare_plane* planes) {
  MapRender& R = G.render;
  MapCompare& C = R.compare;
  C.valid = false;                                                   // the comparison before ends here
  hipStream_t st = m->g->stream;
  const int n_rows = (int)G.planes.size();
  const size_t npx = (size_t)R.tot.width * (size_t)R.tot.height;
  const size_t entries = compare_entries(nplanes, n_rows);
  if (entries > (size_t)INT_MAX) return mfail(m, PPS_ENOMEM, "compare: the table has more than 2^31 - 1 entries");
  if (!C.tables) {
    const int rc = compare_tables(m, G, st);
    if (rc != PPS_OK) return rc;
  }
  const size_t words = compare_table_words(nplanes, n_rows);
  MAP_TRY(m, C.table.reserve(words, st));
  MAP_TRY(m, C.block.reserve(1, st));
  MAP_TRY(m, C.rows.reserve((size_t)n_rows, st));
  MAP_TRY(m, C.pairs.reserve(std::min((size_t)nplanes * (size_t)n_rows, npx), st));
  MAP_TRY(m, hipMemsetAsync(C.table.p, 0, words * sizeof(unsigned long long), st));
  CompareArgs a{};
  a.npx = (int)npx; a.nplanes = nplanes; a.n_rows = n_rows; a.tol = tol;
  a.cloud = cloud; a.frame_id = frame_id; a.view_id = R.on_host ? nullptr : R.plane_id.p;
  a.ids = C.ids.p; a.planes = C.planes.p; a.table = C.table.p;
  CompareFinishArgs f{};
  f.nplanes = nplanes; f.n_rows = n_rows; f.ids = C.ids.p; f.table = C.table.p; f.block = C.block.p; f.rows = C.rows.p; f.pairs = C.pairs.p;
  MAP_TRY(m, C.t_kernels.begin(st));
  MAP_TRY(m, launch_compare(a, st));
  MAP_TRY(m, launch_compare_finish(f, st));
  MAP_TRY(m, C.t_kernels.end(st));
  struct { CompareHead head; pps_map_compare_plane planes[kComparePlanes]; } h;
  static_assert(offsetof(CompareBlock, planes) == sizeof(CompareHead), "the head and the plane records are one block");
  MAP_TRY(m, hipMemcpyAsync(&h, C.block.p, sizeof(CompareHead) + (size_t)nplanes * sizeof(pps_map_compare_plane), hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  pps_map_compare_totals t{};
  t.width = R.tot.width; t.height = R.tot.height; t.nplanes = nplanes; t.n_rows = n_rows;
  t.n_both = h.head.n_both; t.n_frame_only = h.head.n_frame_only; t.n_view_only = h.head.n_view_only; t.n_neither = h.head.n_neither;
  t.n_bad_id = h.head.n_bad_id; t.n_pairs = h.head.n_pairs;
  t.launches = 3; t.tol = tol; t.sec = C.t_kernels.seconds();
  C.tot = t;
  C.valid = true;
  if (planes) memcpy(planes, h.planes, (size_t)nplanes * sizeof(pps_map_compare_plane));
  return PPS_OK;
}

int compare_device(pps_map* m) {
  const int rc = ensure_device(m->g);
  if (rc != PPS_OK) return mfail(m, rc, m->g->err);
  return map_use_device(m);
}

MapCompare* compare_present(const pps_map* m) {
  MapGrid* G = m->grid;
  return (G && G->valid && G->render.valid && G->render.compare.valid) ? &G->render.compare : nullptr;
}

}  // namespace

extern "C" {

int pps_map_compare(pps_map* m, pps_popup* p, int nplanes, double tol, pps_map_compare_plane* planes) {
  if (!m || !p) return mfail(m, PPS_EINVAL, "compare: null handle");
  MapGrid* G = nullptr;
  int rc = compare_checked(m, "compare", nplanes, tol, &G);
  if (rc != PPS_OK) return rc;
  PopupRunView v{};
  rc = popup_last_run(p, &v);
  if (rc != PPS_OK) return mfail(m, rc, std::string("compare: ") + pps_popup_last_error(p));
  if (v.device != m->g->props.device) return mfail(m, PPS_EINVAL, "compare: the pop-up context lives on another device than the graph");
  if ((int64_t)v.width * v.height != (int64_t)G->render.tot.width * G->render.tot.height)
    return mfail(m, PPS_EINVAL, "compare: the run has " + std::to_string((int64_t)v.width * v.height) + " pixels, the rendered view " +
                                    std::to_string((int64_t)G->render.tot.width * G->render.tot.height));
  rc = compare_device(m);
  if (rc != PPS_OK) return rc;
  return compare(m, *G, reinterpret_cast<const MapPt*>(v.cloud), v.plane_id, nplanes, tol, planes);
}

int pps_debug_map_compare_points(pps_map* m, const pps_point* cloud, const int* plane_id, int64_t npx, int nplanes, double tol,
                                 pps_map_compare_plane* planes) {
  if (!m || !cloud || !plane_id) return mfail(m, PPS_EINVAL, "debug_compare_points: null pointer");
  MapGrid* G = nullptr;
  int rc = compare_checked(m, "debug_compare_points", nplanes, tol, &G);
  if (rc != PPS_OK) return rc;
  if (npx != (int64_t)G->render.tot.width * G->render.tot.height)
    return mfail(m, PPS_EINVAL, "debug_compare_points: npx is not width * height of the rendered view");
  rc = compare_device(m);
  if (rc != PPS_OK) return rc;
  hipStream_t st = m->g->stream;
  MAP_TRY(m, m->d_dbg_cloud.reserve((size_t)npx, st));
  MAP_TRY(m, m->d_dbg_pid.reserve((size_t)npx, st));
  MAP_TRY(m, hipMemcpyAsync(m->d_dbg_cloud.p, cloud, (size_t)npx * sizeof(MapPt), hipMemcpyHostToDevice, st));
  MAP_TRY(m, hipMemcpyAsync(m->d_dbg_pid.p, plane_id, (size_t)npx * sizeof(int), hipMemcpyHostToDevice, st));
  return compare(m, *G, m->d_dbg_cloud.p, m->d_dbg_pid.p, nplanes, tol, planes);
}

int pps_map_compare_info(const pps_map* m, pps_map_compare_totals* out) {
  if (!m || !out) return PPS_EINVAL;
  const MapCompare* C = compare_present(m);
  if (!C) return PPS_ESTATE;
  *out = C->tot;
  return PPS_OK;
}

int pps_map_compare_rows(pps_map* m, int cap, pps_map_compare_row* out, int* n) {
  if (!m || !map_table_args(cap, out, n)) return PPS_EINVAL;
  MapCompare* C = compare_present(m);
  if (!C) return mfail(m, PPS_ESTATE, "compare_rows: no comparison (pps_map_compare first; a render or a grid call ends it)");
  *n = C->tot.n_rows;
  const size_t k = std::min<size_t>((size_t)cap, (size_t)C->tot.n_rows);
  if (!k) return PPS_OK;
  hipStream_t st = m->g->stream;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  MAP_TRY(m, hipMemcpyAsync(out, C->rows.p, k * sizeof(pps_map_compare_row), hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  return PPS_OK;
}

int pps_map_compare_pairs(pps_map* m, int64_t first, int64_t count, pps_map_compare_pair* out) {
  if (!m) return PPS_EINVAL;
  MapCompare* C = compare_present(m);
  if (!C) return mfail(m, PPS_ESTATE, "compare_pairs: no comparison (pps_map_compare first; a render or a grid call ends it)");
  if (first < 0 || count < 0 || first > C->tot.n_pairs || count > C->tot.n_pairs - first)
    return mfail(m, PPS_EINVAL, "compare_pairs: the range is outside [0, n_pairs]");
  if (count == 0) return PPS_OK;
  if (!out) return mfail(m, PPS_EINVAL, "compare_pairs: null pointer");
  hipStream_t st = m->g->stream;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  MAP_TRY(m, hipMemcpyAsync(out, C->pairs.p + first, (size_t)count * sizeof(pps_map_compare_pair), hipMemcpyDeviceToHost, st));
  MAP_TRY(m, hipStreamSynchronize(st));
  return PPS_OK;
}

int pps_map_compare_point_host(const double abcd[4], const float xyz[3], double tol, double* e, int64_t* q) {
  if (!abcd || !xyz || !e || !q) return -1;
  ComparePlane c{};
  if (!compare_plane(abcd, &c)) return -1;
  long long qq = 0;
  const bool agree = compare_point(c, xyz[0], xyz[1], xyz[2], tol, e, &qq);
  *q = (int64_t)qq;
  return agree ? 1 : 0;
}

}  // extern "C"
