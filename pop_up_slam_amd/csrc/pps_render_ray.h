// pps_render_ray.h -- the ray of a pixel and its hit on one landmark plane, as include/pps.h (pps_map_render) states them.
// One text for the kernel of pps_render.hip and for the host entry points pps_map_render_ray_host / pps_map_render_hit_host; every file
// that includes it is compiled without contraction (Makefile), like every file that includes pps_grid_cell.h: a product and the sum it
// goes into are rounded separately on both sides.
#pragma once
#include <cmath>

#include "pps_grid_cell.h"

namespace pps {

// a landmark of the grid as the render kernel sees it: the plane (n . x + dn = 0), the axes of its lattice and where its cells lie
struct RenderPlane {
  double n[3], dn, e1[3], e2[3];
  long long base;            // first cell of its box in the cell arrays
  int i0, j0, ni, nj;
};

// n, dn, e1, e2 from the plane's four doubles: grid_frame's frame and dn = p[3] / l with grid_frame's l; false if grid_frame refuses
PPS_GRID_HD bool render_plane(const double p[4], RenderPlane* r) {
  if (!grid_frame(p, r->n, r->e1, r->e2)) return false;
  const double l = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  r->dn = p[3] / l;
  return true;
}

// the ray of pixel (col, row): o its origin and dw its direction in the world, ds the direction in the sensor frame (ds[2] scales t to depth)
PPS_GRID_HD void render_ray(const float iK[9], const float T[16], int col, int row, double o[3], double ds[3], double dw[3]) {
  const double x = (double)col, y = (double)row;
  for (int k = 0; k < 3; k++) ds[k] = ((double)iK[3 * k] * x + (double)iK[3 * k + 1] * y) + (double)iK[3 * k + 2];
  for (int k = 0; k < 3; k++) {
    dw[k] = ((double)T[4 * k] * ds[0] + (double)T[4 * k + 1] * ds[1]) + (double)T[4 * k + 2] * ds[2];
    o[k] = (double)T[4 * k + 3];
  }
}

// the depth of the ray on the plane: false if the ray is parallel to it, the plane lies behind the origin or z is outside [z_near, z_far]
PPS_GRID_HD bool render_depth(const double o[3], const double ds[3], const double dw[3], const RenderPlane& r, double z_near, double z_far,
                              double* t, double* z) {
  const double den = (r.n[0] * dw[0] + r.n[1] * dw[1]) + r.n[2] * dw[2];
  const double h = ((r.n[0] * o[0] + r.n[1] * o[1]) + r.n[2] * o[2]) + r.dn;
  if (den == 0.0 || !(fabs(den) < INFINITY)) return false;
  *t = (-h) / den;
  if (!(*t > 0.0)) return false;
  *z = *t * ds[2];
  return *z >= z_near && *z <= z_far;                      // (a NaN fails both)
}

// the point of the hit, cast to fp32, and its lattice cell; false if a coordinate is not finite or an axis drops the point
PPS_GRID_HD bool render_point(const double o[3], const double dw[3], double t, const RenderPlane& r, double inv_cell, float xf[3], long long* ci,
                              long long* cj) {
  for (int k = 0; k < 3; k++) {
    const double X = o[k] + t * dw[k];
    xf[k] = (float)X;
    if (!(fabsf(xf[k]) < INFINITY)) return false;
  }
  const bool oi = grid_cell(r.e1, inv_cell, xf[0], xf[1], xf[2], ci);
  const bool oj = grid_cell(r.e2, inv_cell, xf[0], xf[1], xf[2], cj);
  return oi && oj;
}

// The rings around cell (i, j): ring k = 0 .. reach, dj = -k .. k ascending, di = -k .. k ascending, pairs with max(|di|, |dj|) = k only.
// occupied(c): the answer of cell c of the cell arrays (>= 0: it answers), asked only for cells inside the row's box.  Returns the first
// answer, -1 if there is none.
template <class F>
PPS_GRID_HD long long render_lookup(const RenderPlane& r, long long i, long long j, int reach, F occupied) {
  const long long ri = i - r.i0, rj = j - r.j0;
  for (int k = 0; k <= reach; k++)
    for (int dj = -k; dj <= k; dj++) {
      const long long cj = rj + dj;
      if (cj < 0 || cj >= r.nj) continue;
      const int step = (dj == -k || dj == k) ? 1 : 2 * k;  // inner rows of the ring: its two ends only
      for (int di = -k; di <= k; di += step) {
        const long long ci = ri + di;
        if (ci < 0 || ci >= r.ni) continue;
        const long long s = occupied(r.base + cj * r.ni + ci);
        if (s >= 0) return s;
      }
    }
  return -1;
}

}  // namespace pps
