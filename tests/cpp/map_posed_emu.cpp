// map_posed_emu.cpp -- k_map_motion and k_map_build_posed of csrc/pps_map.hip compiled for the host (map_emu/hip/hip_runtime.h: one
// std::thread per thread of a workgroup, barriers at the wave operations).  tests/test_host_map_posed.py compares what they write with
// the host entry points pps_map_motion_host / pps_map_move_point_host, and the posed build without motions with k_map_build.
#include <memory>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
EmuGroup g_emu;
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
  const unsigned nw = block.x / 64;
  for (unsigned b = 0; b < grid.x; b++) {
    std::barrier<> wg(block.x);
    std::vector<std::unique_ptr<std::barrier<>>> wave;
    for (unsigned w = 0; w < nw; w++) { wave.emplace_back(new std::barrier<>(64)); g_emu.wave[w] = wave.back().get(); }
    g_emu.wg = &wg;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++)
      th.emplace_back([&, t]() { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); g_emu.wave[t >> 6]->arrive_and_drop(); g_emu.wg->arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
#include "pps_map.hip"
using namespace pps;
extern "C" {
int emu_frame_rec_size() { return (int)sizeof(MapFrameDev); }
int emu_map_motion(int n_frames, const void* recs, const double* pose_est, int pose_ld, double* motion, int* moved) {
  MapMotionArgs a{n_frames, (const MapFrameDev*)recs, pose_est, pose_ld, motion, moved};
  return launch_map_motion(a, nullptr);
}
int emu_map_build(long long n_out, int n_sel, const long long* out_off, const long long* src_off, const int* slot, const double* plane_est,
                  int plane_ld, const void* store, void* built) {
  MapBuildArgs a{n_out, n_sel, out_off, src_off, slot, plane_est, plane_ld, (const MapPt*)store, (MapPt*)built};
  return launch_map_build(a, nullptr);
}
int emu_map_build_posed(long long n_out, int n_sel, const long long* out_off, const long long* src_off, const int* slot, const double* plane_est,
                        int plane_ld, const void* store, void* built, const int* fidx, const double* motion, const int* moved) {
  MapBuildArgs a{n_out, n_sel, out_off, src_off, slot, plane_est, plane_ld, (const MapPt*)store, (MapPt*)built};
  return launch_map_build_posed(a, MapMotionTable{fidx, motion, moved}, nullptr);
}
}
