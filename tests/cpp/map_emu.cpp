// map_emu.cpp -- the kernels of csrc/pps_map.hip compiled for the host (map_emu/hip/hip_runtime.h: one std::thread per thread of a
// workgroup, barriers at the wave operations).  tests/test_host_map.py feeds them random valid / plane-id grids and compares the
// stable partition they write with numpy, and the build with a numpy fp64 projection.
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
int emu_map_tiles(int npx) { return map_tiling(npx).nT; }
int emu_map_wt(int npx) { return map_tiling(npx).wt; }
// table: kMapPlanes * nT ints, totals: kMapPlanes
int emu_map_count(const void* cloud, const int* pid, int npx, int nplanes, int* table, int* totals) {
  return launch_map_count((const MapPt*)cloud, pid, npx, nplanes, table, totals, nullptr);
}
int emu_map_scatter(const void* cloud, const int* pid, int npx, int nplanes, const int* table, const long long* base, void* store) {
  MapScatterBase b;
  for (int k = 0; k < kMapPlanes; k++) b.base[k] = base[k];
  return launch_map_scatter((const MapPt*)cloud, pid, npx, nplanes, table, b, (MapPt*)store, nullptr);
}
int emu_map_build(long long n_out, int n_sel, const long long* out_off, const long long* src_off, const int* slot, const double* plane_est,
                  int plane_ld, const void* store, void* built) {
  MapBuildArgs a{n_out, n_sel, out_off, src_off, slot, plane_est, plane_ld, (const MapPt*)store, (MapPt*)built};
  return launch_map_build(a, nullptr);
}
}
