// pps_map.h -- argument blocks and launch functions of the dense-map kernels (pps_map.hip), shared with the host side (pps_map.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace pps {

constexpr int kMapPlanes = 65;       // planes of one frame: kMaxPlanes + 1 of pps_popup.hip (what a plane-id pixel can hold)
constexpr int kMapThreads = 256;     // four waves per workgroup
constexpr int kMapWaves = kMapThreads / 64;

struct alignas(16) MapPt { float x, y, z; unsigned int rgba; };      // pps_point, moved as one 16-byte load / store

// How a frame of npx pixels is cut: a wave owns `wt` consecutive pixels in raster order (a multiple of 64), nT such wave tiles cover the
// frame.  256 pixels per wave until the count table (planes x nT) would pass 8192 columns, larger tiles beyond.
constexpr int kMapMaxPixels = 1 << 30;   // what pps_debug_map_add_points accepts: the tiling and the kernels index pixels with int, tile ends included
struct MapTiling { int wt, nT; };
inline MapTiling map_tiling(int npx) {
  MapTiling t;
  t.wt = 256;
  if ((npx + t.wt - 1) / t.wt > 8192) t.wt = (((npx + 8191) / 8192) + 63) / 64 * 64;
  t.nT = (npx + t.wt - 1) / t.wt;
  return t;
}

// store position of the first point of frame plane k (-1: the plane is skipped, its points are dropped)
struct MapScatterBase { long long base[kMapPlanes]; };

// pass 1 + 2: table[k * nT + T] = kept points of plane k in the wave tiles before T (exclusive scan in raster order), totals[k] = all of them
hipError_t launch_map_count(const MapPt* cloud, const int* plane_id, int npx, int nplanes, int* table, int* totals, hipStream_t st);
// pass 3: every kept point to base[k] + table[k][T] + its rank inside the tile
hipError_t launch_map_scatter(const MapPt* cloud, const int* plane_id, int npx, int nplanes, const int* table, const MapScatterBase& base,
                              MapPt* store, hipStream_t st);

// The build: n_sel non-empty chunks, written back to back.  out_off[n_sel + 1] ascending output offsets (out_off[n_sel] = n_out),
// src_off[c] the chunk's first point in the store, slot[c] the landmark's slot in plane_est (-1: the points pass through).
struct MapBuildArgs {
  long long n_out;
  int n_sel;
  const long long* out_off;
  const long long* src_off;
  const int* slot;
  const double* plane_est; int plane_ld;
  const MapPt* store;
  MapPt* built;
};
hipError_t launch_map_build(const MapBuildArgs& a, hipStream_t st);

// The posed build (include/pps.h: pps_map_build_posed).  One record per frame of the selection: the capture pose and the slot of the
// frame's pose node in pose_est (-1: the frame has no motion).  k_map_motion writes the motion table from them -- motion[12 * f ..] =
// (R_D | t_D), moved[f] = 1, or the identity and 0 --, the build reads it through fidx[c], the row of chunk c's frame.
struct MapFrameDev { float T[16]; int pose_slot; int pad; };
struct MapMotionArgs {
  int n_frames;
  const MapFrameDev* recs;
  const double* pose_est; int pose_ld;
  double* motion;                      // [12 * n_frames]
  int* moved;                          // [n_frames]
};
hipError_t launch_map_motion(const MapMotionArgs& a, hipStream_t st);
struct MapMotionTable {                // what a kernel reads of the table; motion == nullptr: no point is moved
  const int* fidx;                     // [n_sel]
  const double* motion;
  const int* moved;
};
hipError_t launch_map_build_posed(const MapBuildArgs& a, const MapMotionTable& t, hipStream_t st);

}  // namespace pps
