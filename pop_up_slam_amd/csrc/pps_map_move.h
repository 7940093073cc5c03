// pps_map_move.h -- the rigid motion of a stored frame and the moved point of the posed map, as include/pps.h (pps_map_build_posed) states
// them.  One text for k_map_motion / k_map_build_posed (pps_map.hip), the grid kernels (pps_grid.hip) and the host entry points
// pps_map_motion_host / pps_map_move_point_host; every file that includes it is compiled without contraction (Makefile), so a product and
// the sum it goes into are rounded separately on both sides.
#pragma once
#include <cmath>

#include "pps_geom.h"

namespace pps {

constexpr double kMapRigidTol = 1e-4;        // max |R0^T R0 - I| of a T_wc that pps_map_set_frame_pose accepts

// T (row-major 4x4 fp32) is a rigid transform to fp32: finite, last row (0, 0, 0, 1), R^T R within kMapRigidTol of I
inline bool map_rigid(const float T[16]) {
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(T[k])) return false;
  if (T[12] != 0.f || T[13] != 0.f || T[14] != 0.f || T[15] != 1.f) return false;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double v = ((double)T[i] * (double)T[j] + (double)T[4 + i] * (double)T[4 + j]) + (double)T[8 + i] * (double)T[8 + j];
      if (!(fabs(v - (i == j ? 1.0 : 0.0)) <= kMapRigidTol)) return false;
    }
  return true;
}

// D = (R_D row-major | t_D): R_D = R(q) R0^T, t_D = t - R_D t0, with (R0, t0) of the capture pose T0 and (t, q) the pose node's estimate
PPS_HD void map_motion(const float T0[16], const double tq[7], double D[12]) {
  double R[9];
  quat_to_R(tq + 3, R);
  const double t0[3] = {(double)T0[3], (double)T0[7], (double)T0[11]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++)
      D[3 * i + j] = (R[3 * i] * (double)T0[4 * j] + R[3 * i + 1] * (double)T0[4 * j + 1]) + R[3 * i + 2] * (double)T0[4 * j + 2];
    D[9 + i] = tq[i] - ((D[3 * i] * t0[0] + D[3 * i + 1] * t0[1]) + D[3 * i + 2] * t0[2]);
  }
}

// Plane3d::project_to_plane with the arithmetic of project_to_plane_f32 (pps_project.h) on a point that is already in fp64
PPS_HD void project_to_plane_f64(const double p[4], double x, double y, double z, float* ox, float* oy, float* oz) {
  const double l = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const double nx = p[0] / l, ny = p[1] / l, nz = p[2] / l, dd = -p[3] / l;
  const double s = (nx * x + ny * y + nz * z) - dd;
  *ox = (float)(x - nx * s); *oy = (float)(y - ny * s); *oz = (float)(z - nz * s);
}

// (x, y, z) <- R_D (x, y, z) + t_D
PPS_HD void map_move_xyz(const double D[12], double* x, double* y, double* z) {
  const double mx = ((D[0] * *x + D[1] * *y) + D[2] * *z) + D[9];
  const double my = ((D[3] * *x + D[4] * *y) + D[5] * *z) + D[10];
  const double mz = ((D[6] * *x + D[7] * *y) + D[8] * *z) + D[11];
  *x = mx; *y = my; *z = mz;
}

// a point of a frame that has a motion, in place: moved by D, then projected onto p, or only moved when the landmark is gone (`project`
// false: p is not read); cast once.  What the kernels call for such a point (k_map_build_posed, grid_b_point).
PPS_HD void map_moved_point(const double D[12], const double* p, bool project, float* px, float* py, float* pz) {
  double x = (double)*px, y = (double)*py, z = (double)*pz;
  map_move_xyz(D, &x, &y, &z);
  if (project) project_to_plane_f64(p, x, y, z, px, py, pz);
  else { *px = (float)x; *py = (float)y; *pz = (float)z; }
}

// the point of the posed map: moved by D (NULL: the frame has no motion), then projected onto p (NULL: the landmark is gone), cast once.
// With D == NULL this is project_to_plane_f32 (p given) or the stored point itself.
PPS_HD void map_move_point(const double* D, const double* p, float xf, float yf, float zf, float* ox, float* oy, float* oz) {
  *ox = xf; *oy = yf; *oz = zf;
  if (D) map_moved_point(D, p, p != nullptr, ox, oy, oz);
  else if (p) project_to_plane_f64(p, (double)xf, (double)yf, (double)zf, ox, oy, oz);
}

}  // namespace pps
