// pps_grid.h -- argument blocks and launch functions of the grid-map kernels (pps_grid.hip), shared with the host side (pps_map_grid.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pps_map.h"

namespace pps {

// a landmark of the grid as the kernels see it: its axes, and (from the vote pass on) where its cells lie
struct GridPlaneDev {
  double e1[3], e2[3];
  long long base;            // first cell of its box in the cell arrays
  int i0, j0, ni, nj;
};

// per landmark, written by the extent pass with integer atomics only (the result does not depend on the order they arrive in)
struct GridExtent {
  int imin, imax, jmin, jmax;          // start: INT_MAX, INT_MIN, INT_MAX, INT_MIN
  unsigned long long n_in;             // points that voted
};

constexpr unsigned long long kGridOldestBias = 0x7fffffffffffffffULL;     // key of the OLDEST rule: bias - index in B (the vote is a max)

// the selection the way k_map_build reads it (MapBuildArgs), plus the landmark of every chunk
struct GridSelArgs {
  long long n_out;
  int n_sel;
  const long long* out_off;            // [n_sel + 1]
  const long long* src_off;            // [n_sel]
  const int* slot;                     // [n_sel] slot in plane_est, -1: the points pass through
  const int* lm;                       // [n_sel] row of the plane table, -1 with slot
  const double* plane_est; int plane_ld;
  const MapPt* store;
  const GridPlaneDev* planes; int n_planes;
  double inv_cell;
};

// The kernels that form a point of B take a motion table beside the selection: mt.motion == nullptr (the default), B is pps_map_build's;
// otherwise B is the posed map (pps_map_build_grid_posed) and mt.fidx has n_sel rows.
// pass 1: per landmark the extent of (i, j) and the points that voted; *n_dropped += the dropped ones
hipError_t launch_grid_extent(const GridSelArgs& a, GridExtent* ext, unsigned long long* n_dropped, hipStream_t st, const MapMotionTable& mt = MapMotionTable{});
// pass 2: key[c] = max over the cell's points of the rule's key, cnt[c] += 1.  combine: one atomic pair per distinct cell and wave
hipError_t launch_grid_vote(const GridSelArgs& a, int oldest, bool combine, unsigned long long* key, unsigned int* cnt, hipStream_t st,
                            const MapMotionTable& mt = MapMotionTable{});

// pass 3.  A workgroup owns `cpw` consecutive cells (a multiple of 256); nT such tiles cover the n cells.
struct GridTiling { long long cpw; int nT; };
inline GridTiling grid_tiling(long long n) {
  GridTiling t;
  t.cpw = 2048;
  if ((n + t.cpw - 1) / t.cpw > (1 << 20)) t.cpw = (((n + (1 << 20) - 1) >> 20) + 255) / 256 * 256;
  t.nT = (int)((n + t.cpw - 1) / t.cpw);
  return t;
}
struct GridEmitArgs {
  long long n_cells_all;               // cells of all boxes
  unsigned int min_count;
  int oldest;
  const unsigned long long* key;
  const unsigned int* cnt;
  int* tile_count;                     // [nT]
  long long* tile_prefix;              // [nT + 1]: emitted cells before tile T; [nT] = all of them
  const long long* plane_base;         // [n_planes + 1]: GridPlaneDev::base, then n_cells_all
  long long* plane_off;                // [n_planes + 1]: emitted cells before landmark L; [n_planes] = all of them
  MapPt* pts; unsigned int* counts; int* ij; long long* src;
};
// count per tile, scan over the tiles, emitted cells before every landmark (three launches)
hipError_t launch_grid_count(const GridEmitArgs& e, int n_planes, hipStream_t st);
// the stable compaction: cell c with cnt[c] >= min_count goes to tile_prefix[T] + its rank inside the tile
hipError_t launch_grid_emit(const GridSelArgs& a, const GridEmitArgs& e, hipStream_t st, const MapMotionTable& mt = MapMotionTable{});

}  // namespace pps
