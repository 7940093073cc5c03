// pps_project.h -- Plane3d::project_to_plane (src/isam_plane3d.h:173-178) as the device code of this library evaluates it: the plane's four
// doubles as the solver state holds them, the point in fp32, the arithmetic in fp64, the result cast to fp32.  One function for
// k_reproject (pps_assoc.hip: Mapper_mono::reproj_to_newplane) and k_map_build (pps_map.hip: the dense map of main_3d.cpp:563-577); both
// files are compiled without contraction, so a point gives the same bits through either kernel.
#pragma once
#include <cmath>

namespace pps {

__device__ __forceinline__ void project_to_plane_f32(const double p[4], float xf, float yf, float zf, float* ox, float* oy, float* oz) {
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  const double l = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const double nx = p[0] / l, ny = p[1] / l, nz = p[2] / l, dd = -p[3] / l;
  const double s = (nx * x + ny * y + nz * z) - dd;
  *ox = (float)(x - nx * s); *oy = (float)(y - ny * s); *oz = (float)(z - nz * s);
}

}  // namespace pps
