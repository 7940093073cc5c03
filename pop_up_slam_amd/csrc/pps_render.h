// pps_render.h -- argument blocks and launch functions of the render kernels (pps_render.hip), shared with the host side (pps_map_render.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pps_grid.h"
#include "pps_render_ray.h"

namespace pps {

constexpr int kRenderTile = 16;                  // a workgroup owns a tile of 16 x 16 pixels
constexpr int kRenderSlice = 256;                // landmark rows staged in LDS at a time
constexpr int kRenderMaxSide = 4096, kRenderMaxReach = 4;

// The slot table: slot[c] = the index of box cell c in the grid map, -1 if the cell was not emitted.  k_grid_emit's compaction again, from
// the cnt[] and tile_prefix[] the grid passes left (cpw and the tile count: grid_tiling(n_cells_all), as launch_grid_emit takes them).
hipError_t launch_render_slots(long long n_cells_all, unsigned int min_count, const unsigned int* cnt, const long long* tile_prefix, int* slot,
                               hipStream_t st);

struct RenderArgs {
  int width, height, reach, n_rows;
  float iK[9], T[16];
  double z_near, z_far, inv_cell;
  const RenderPlane* rows;             // [n_rows] the landmarks with a box, ascending plane node id
  const int* ids;                      // [n_rows] their node ids
  const int* slot;                     // the slot table
  const MapPt* pts;                    // the grid map (its rgba)
  MapPt* cloud; float* depth; int* plane_id; long long* cell;      // [width * height] each
  unsigned long long* n_hit;           // += the pixels with a hit
};
hipError_t launch_render(const RenderArgs& a, hipStream_t st);

}  // namespace pps
