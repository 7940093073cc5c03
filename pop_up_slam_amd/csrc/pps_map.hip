// pps_map.hip -- the dense map on the device: the per-plane clouds of every frame kept in one store, and the final map built from them.
//
// The reference keeps, per frame, one pcl cloud per good plane (partplane_clouds_open_all, popup_plane.cpp:925-985 -> main_3d.cpp:475,493)
// and, at the end, projects every kept point onto the optimised plane of its landmark (main_3d.cpp:563-577).  Here the pop-up kernel has
// written one point per pixel (cloud) and the plane index of every pixel (plane_id); k_map_count / k_map_scan / k_map_scatter split that
// frame into one chunk per plane -- a stable partition: the points of a chunk keep the raster order of their pixels --, k_map_build
// projects the selected chunks.
//
// The partition uses no atomic cursor (the order of the points would then depend on the order the waves arrive in).  A wave owns `wt`
// consecutive pixels (MapTiling); the lanes of a wave that hold the same plane find each other with 64-bit ballots, a lane's rank among
// them is the population count of the ballot below its lane (mbcnt).  Pass 1 counts per wave tile and plane, pass 2 scans those counts
// over the tiles (one workgroup per plane), pass 3 repeats the ballots and writes: chunk base + tile prefix + running count of the tile +
// rank.  The waves of a workgroup do not talk to each other: every wave has its own row of counters in LDS, read and written by that wave
// alone (LDS operations of one wave execute in order), so there is no workgroup barrier in pass 1 and 3.
//
// Compiled without contraction (Makefile): k_map_build gives the bits of k_reproject (pps_project.h).
//
// The posed build (pps_map_build_posed) moves every point rigidly with the correction of its frame's pose before it is projected:
// k_map_motion computes one motion per frame of the selection from pose_est in place (pps_map_move.h: the text the host entry points are
// compiled from), k_map_build_posed is k_map_build with the motion of the point's frame applied.  Both find a point's chunk in the
// workgroup's chunk window (pps_map_window.h), which the grid kernels (pps_grid.hip) share with them.
#include <hip/hip_runtime.h>

#include "pps_map.h"
#include "pps_map_move.h"
#include "pps_map_window.h"
#include "pps_project.h"

namespace pps {
namespace {

// plane of pixel i if its point is kept: valid bit set and a plane index of this frame
__device__ __forceinline__ int map_key(unsigned int rgba, int p, int nplanes) { return (((rgba >> 24) & 1u) && p >= 0 && p < nplanes) ? p : -1; }

__global__ __launch_bounds__(kMapThreads) void k_map_count(const MapPt* __restrict__ cloud, const int* __restrict__ plane_id, int npx, int nplanes,
                                                           int wt, int nT, int* __restrict__ table) {
  __shared__ int s_cnt[kMapWaves][kMapPlanes];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = blockIdx.x * kMapWaves + w;
  volatile int* cnt = s_cnt[w];
  if (T >= nT) return;                                           // (whole waves; nothing below synchronises across waves)
  for (int k = lane; k < nplanes; k += 64) cnt[k] = 0;
  __builtin_amdgcn_wave_barrier();
  const int i0 = T * wt, i1 = min(npx, i0 + wt);
  for (int b = i0; b < i1; b += 64) {
    const int i = b + lane;
    int key = -1;
    if (i < i1) key = map_key(cloud[i].rgba, plane_id[i], nplanes);
    unsigned long long rem = __ballot(key >= 0);
    while (rem) {                                                // one turn per distinct plane among the 64 pixels (wave-uniform)
      const int leader = __ffsll((long long)rem) - 1;
      const int kk = __builtin_amdgcn_readlane(key, leader);
      const unsigned long long m = __ballot(key == kk);
      if (lane == leader) cnt[kk] = cnt[kk] + __popcll(m);
      rem &= ~m;
    }
  }
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < nplanes; k += 64) table[(size_t)k * nT + T] = cnt[k];
}

// exclusive scan of one plane's row of tile counts, in place; one workgroup per plane
__global__ __launch_bounds__(kMapThreads) void k_map_scan(int* __restrict__ table, int nT, int* __restrict__ totals) {
  __shared__ int s_sum[kMapThreads];
  const int tid = threadIdx.x;
  int* row = table + (size_t)blockIdx.x * nT;
  const int seg = (nT + kMapThreads - 1) / kMapThreads;
  const int a = min(nT, tid * seg), b = min(nT, a + seg);
  int sum = 0;
  for (int i = a; i < b; i++) sum += row[i];
  const int upto = map_block_scan(s_sum, sum);
  int run = upto - sum;
  for (int i = a; i < b; i++) { const int c = row[i]; row[i] = run; run += c; }
  if (tid == kMapThreads - 1) totals[blockIdx.x] = upto;
}

__global__ __launch_bounds__(kMapThreads) void k_map_scatter(const MapPt* __restrict__ cloud, const int* __restrict__ plane_id, int npx, int nplanes,
                                                             int wt, int nT, const int* __restrict__ table, MapScatterBase base,
                                                             MapPt* __restrict__ store) {
  __shared__ int s_cur[kMapWaves][kMapPlanes];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = blockIdx.x * kMapWaves + w;
  volatile int* cur = s_cur[w];
  if (T >= nT) return;
  for (int k = lane; k < nplanes; k += 64) cur[k] = table[(size_t)k * nT + T];
  __builtin_amdgcn_wave_barrier();
  const int i0 = T * wt, i1 = min(npx, i0 + wt);
  for (int b = i0; b < i1; b += 64) {
    const int i = b + lane;
    int key = -1;
    MapPt pt = {0.f, 0.f, 0.f, 0u};
    if (i < i1) { pt = cloud[i]; key = map_key(pt.rgba, plane_id[i], nplanes); }
    unsigned long long rem = __ballot(key >= 0);
    while (rem) {
      const int leader = __ffsll((long long)rem) - 1;
      const int kk = __builtin_amdgcn_readlane(key, leader);
      const unsigned long long m = __ballot(key == kk);
      const int c = cur[kk];                                     // (every lane reads before the leader moves the cursor)
      const long long cb = base.base[kk];
      if (key == kk && cb >= 0) store[cb + c + map_lanes_below(m)] = pt;
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) cur[kk] = c + __popcll(m);
      rem &= ~m;
    }
  }
}

// One thread per point of the built map; the workgroup's chunk window (pps_map_window.h) tells a point its chunk.  16 B in, 16 B out.
__global__ __launch_bounds__(kMapThreads) void k_map_build(MapBuildArgs a) {
  __shared__ MapWindow<false> w;
  const long long first = (long long)blockIdx.x * kMapThreads;
  map_stage_window(w, a.out_off, a.src_off, a.slot, nullptr, a.n_sel, first);
  const long long i = first + threadIdx.x;
  if (i >= a.n_out) return;
  const int lo = map_window_find(w, i);
  MapPt pt = a.store[w.src[lo] + (i - w.off[lo])];
  const int sl = w.slot[lo];
  if (sl >= 0) {                                                 // (a landmark that is gone and was not redirected: untouched, like k_reproject)
    double p[4];
    for (int k = 0; k < 4; k++) p[k] = a.plane_est[(size_t)k * a.plane_ld + sl];
    project_to_plane_f32(p, pt.x, pt.y, pt.z, &pt.x, &pt.y, &pt.z);
  }
  a.built[i] = pt;
}

// One thread per frame of the selection: D = (R R0^T | t - R_D t0) from the frame's capture pose and the estimate of its pose node.
__global__ __launch_bounds__(kMapThreads) void k_map_motion(MapMotionArgs a) {
  const int f = blockIdx.x * kMapThreads + threadIdx.x;
  if (f >= a.n_frames) return;
  const MapFrameDev r = a.recs[f];
  double D[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  int mv = 0;
  if (r.pose_slot >= 0) {
    double tq[7];
    for (int k = 0; k < 7; k++) tq[k] = a.pose_est[(size_t)k * a.pose_ld + r.pose_slot];
    map_motion(r.T, tq, D);
    mv = 1;
  }
  for (int k = 0; k < 12; k++) a.motion[12 * (size_t)f + k] = D[k];
  a.moved[f] = mv;
}

// k_map_build with the motion of the point's frame: the window's fourth row is the row of every chunk's frame in the motion table.
// The 256 points of a workgroup belong to few frames (a chunk is one plane of one frame), so a motion is not loaded per point: the lanes
// of a wave that share a frame find each other with a ballot, the 96 bytes of that frame's motion are read at a wave-uniform address
// (scalar loads, one turn per distinct frame of the wave), and the lanes of that frame move their point.  16 B in, 16 B out.
__global__ __launch_bounds__(kMapThreads) void k_map_build_posed(MapBuildArgs a, const int* __restrict__ fidx, const double* __restrict__ motion,
                                                                 const int* __restrict__ moved) {
  __shared__ MapWindow<true> w;
  const long long first = (long long)blockIdx.x * kMapThreads;
  map_stage_window(w, a.out_off, a.src_off, a.slot, fidx, a.n_sel, first);
  const long long i = first + threadIdx.x;
  const bool in = i < a.n_out;                                   // (no early return: the ballots below are the whole wave's)
  MapPt pt = {0.f, 0.f, 0.f, 0u};
  int sl = -1, f = -1;
  if (in) {
    const int lo = map_window_find(w, i);
    pt = a.store[w.src[lo] + (i - w.off[lo])];
    sl = w.slot[lo]; f = w.aux[lo];
  }
  double p[4] = {0.0, 0.0, 1.0, 0.0};
  if (sl >= 0)
    for (int k = 0; k < 4; k++) p[k] = a.plane_est[(size_t)k * a.plane_ld + sl];
  unsigned long long rem = __ballot(f >= 0);
  while (rem) {                                                  // one turn per distinct frame among the 64 points (wave-uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const int F = __builtin_amdgcn_readlane(f, leader);
    const unsigned long long mk = __ballot(f == F);
    if (moved[F]) {
      double D[12];
      for (int k = 0; k < 12; k++) D[k] = motion[12 * (size_t)F + k];
      if (f == F) map_moved_point(D, p, sl >= 0, &pt.x, &pt.y, &pt.z);       // (gone landmark: moved, not projected)
    } else if (f == F && sl >= 0) {                              // a frame without motion: k_map_build's point
      project_to_plane_f32(p, pt.x, pt.y, pt.z, &pt.x, &pt.y, &pt.z);
    }
    rem &= ~mk;
  }
  if (in) a.built[i] = pt;
}

}  // namespace

hipError_t launch_map_count(const MapPt* cloud, const int* plane_id, int npx, int nplanes, int* table, int* totals, hipStream_t st) {
  if (npx <= 0 || nplanes <= 0) return hipSuccess;
  const MapTiling t = map_tiling(npx);
  hipLaunchKernelGGL(k_map_count, dim3((t.nT + kMapWaves - 1) / kMapWaves), dim3(kMapThreads), 0, st, cloud, plane_id, npx, nplanes, t.wt, t.nT, table);
  hipLaunchKernelGGL(k_map_scan, dim3(nplanes), dim3(kMapThreads), 0, st, table, t.nT, totals);
  return hipGetLastError();
}

hipError_t launch_map_scatter(const MapPt* cloud, const int* plane_id, int npx, int nplanes, const int* table, const MapScatterBase& base,
                              MapPt* store, hipStream_t st) {
  if (npx <= 0 || nplanes <= 0) return hipSuccess;
  const MapTiling t = map_tiling(npx);
  hipLaunchKernelGGL(k_map_scatter, dim3((t.nT + kMapWaves - 1) / kMapWaves), dim3(kMapThreads), 0, st, cloud, plane_id, npx, nplanes, t.wt, t.nT, table,
                     base, store);
  return hipGetLastError();
}

hipError_t launch_map_build(const MapBuildArgs& a, hipStream_t st) {
  if (a.n_out <= 0 || a.n_sel <= 0) return hipSuccess;
  const long long nwg = (a.n_out + kMapThreads - 1) / kMapThreads;
  if (nwg > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_map_build, dim3((unsigned int)nwg), dim3(kMapThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_motion(const MapMotionArgs& a, hipStream_t st) {
  if (a.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_map_motion, dim3((a.n_frames + kMapThreads - 1) / kMapThreads), dim3(kMapThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_map_build_posed(const MapBuildArgs& a, const MapMotionTable& t, hipStream_t st) {
  if (a.n_out <= 0 || a.n_sel <= 0) return hipSuccess;
  const long long nwg = (a.n_out + kMapThreads - 1) / kMapThreads;
  if (nwg > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_map_build_posed, dim3((unsigned int)nwg), dim3(kMapThreads), 0, st, a, t.fidx, t.motion, t.moved);
  return hipGetLastError();
}

}  // namespace pps
