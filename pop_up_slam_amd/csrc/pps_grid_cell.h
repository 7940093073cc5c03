// pps_grid_cell.h -- the frame of a landmark plane and the lattice cell of a point, as include/pps.h (pps_map_build_grid) states them.
// One text for the kernels of pps_grid.hip and for the host entry points pps_map_grid_frame_host / pps_map_grid_cell_host; every file
// that includes it is compiled without contraction (Makefile), so a product and the sum it goes into are rounded separately on both sides.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PPS_GRID_HD __host__ __device__ inline
#else
#define PPS_GRID_HD inline
#endif

namespace pps {

constexpr double kGridCellLimit = 1073741824.0;          // 2^30: a cell index at or beyond it drops the point

// n, e1, e2 from the plane's four doubles; false if (p0, p1, p2) has no finite positive length
PPS_GRID_HD bool grid_frame(const double p[4], double n[3], double e1[3], double e2[3]) {
  const double l = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  if (!(l > 0.0) || !(l < INFINITY)) return false;
  n[0] = p[0] / l; n[1] = p[1] / l; n[2] = p[2] / l;
  double c[3];                                           // a x n, written out: the component along a is an exact zero
  if (fabs(n[2]) <= 0.7) { c[0] = -n[1]; c[1] = n[0]; c[2] = 0.0; }      // a = (0, 0, 1)
  else { c[0] = 0.0; c[1] = -n[2]; c[2] = n[1]; }                        // a = (1, 0, 0)
  const double lc = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  e1[0] = c[0] / lc; e1[1] = c[1] / lc; e1[2] = c[2] / lc;
  e2[0] = n[1] * e1[2] - n[2] * e1[1];
  e2[1] = n[2] * e1[0] - n[0] * e1[2];
  e2[2] = n[0] * e1[1] - n[1] * e1[0];
  return true;
}

// floor((x*e[0] + y*e[1]) + z*e[2]) * inv_cell) of an fp32 point along the axis e; false if the point is dropped on this axis
PPS_GRID_HD bool grid_cell(const double e[3], double inv_cell, float xf, float yf, float zf, long long* cell) {
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  const double u = (x * e[0] + y * e[1]) + z * e[2];
  const double t = floor(u * inv_cell);
  if (!(fabs(u) < INFINITY) || !(fabs(t) < kGridCellLimit)) { *cell = 0; return false; }
  *cell = (long long)t;
  return true;
}

}  // namespace pps
