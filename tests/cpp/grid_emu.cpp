// grid_emu.cpp -- the kernels of csrc/pps_grid.hip compiled for the host (grid_emu/hip/hip_runtime.h: one std::thread per thread of a
// workgroup, barriers at the wave operations, real atomics).  tests/test_host_map_grid.py drives the passes the way pps_map_grid.cpp does
// and compares the grid they write with the numpy statement.  The argument blocks are passed as they are: the test mirrors GridSelArgs,
// GridEmitArgs, GridPlaneDev and GridExtent (csrc/pps_grid.h) with ctypes, and emu_grid_sizes tells it whether the mirrors fit.
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
#include "pps_grid.hip"
using namespace pps;
extern "C" {
void emu_grid_sizes(int out[4]) { out[0] = sizeof(GridSelArgs); out[1] = sizeof(GridEmitArgs); out[2] = sizeof(GridPlaneDev); out[3] = sizeof(GridExtent); }
int emu_grid_tiles(long long n) { return grid_tiling(n).nT; }
long long emu_grid_cpw(long long n) { return grid_tiling(n).cpw; }
int emu_grid_extent(const GridSelArgs* a, GridExtent* ext, unsigned long long* n_dropped) { return launch_grid_extent(*a, ext, n_dropped, nullptr); }
int emu_grid_vote(const GridSelArgs* a, int oldest, int combine, unsigned long long* key, unsigned int* cnt) {
  return launch_grid_vote(*a, oldest, combine != 0, key, cnt, nullptr);
}
int emu_grid_count(const GridEmitArgs* e, int n_planes) { return launch_grid_count(*e, n_planes, nullptr); }
int emu_grid_emit(const GridSelArgs* a, const GridEmitArgs* e) { return launch_grid_emit(*a, *e, nullptr); }
}
