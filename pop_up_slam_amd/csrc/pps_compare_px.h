// pps_compare_px.h -- one pop-up point against one landmark plane of the map, as include/pps.h (pps_map_compare) states it: the signed
// distance e, its quantised form q and the agree bit.  One text for the kernel of pps_compare.hip and for pps_map_compare_point_host; every
// file that includes it is compiled without contraction (Makefile), like every file that includes pps_grid_cell.h.
#pragma once
#include <cmath>

#include "pps_grid_cell.h"

namespace pps {

constexpr double kCompareScale = 4096.0;                 // q counts 1 / 4096 m
constexpr long long kCompareQMax = 524288;               // |q| saturates at 128 m; NaN goes to +kCompareQMax

// a row of the plane table as the compare kernel sees it: n . x + dn = 0
struct ComparePlane { double n[3], dn; };

// n and dn from the plane's four doubles: grid_frame's n and dn = p[3] / l with grid_frame's l, as render_plane has them; false if grid_frame refuses
PPS_GRID_HD bool compare_plane(const double p[4], ComparePlane* c) {
  double e1[3], e2[3];
  if (!grid_frame(p, c->n, e1, e2)) return false;
  const double l = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  c->dn = p[3] / l;
  return true;
}

// the fp32 point against the plane: *e the signed distance, *q its quantised form; returns agree
PPS_GRID_HD bool compare_point(const ComparePlane& c, float xf, float yf, float zf, double tol, double* e, long long* q) {
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  const double d = ((c.n[0] * x + c.n[1] * y) + c.n[2] * z) + c.dn;
  const double s = d * kCompareScale;
  if (s != s || s >= (double)kCompareQMax) *q = kCompareQMax;
  else if (s <= -(double)kCompareQMax) *q = -kCompareQMax;
  else *q = (long long)rint(s);
  *e = d;
  return fabs(d) <= tol;                                 // (a NaN fails)
}

}  // namespace pps
