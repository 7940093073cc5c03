// render_emu.cpp -- the kernels of csrc/pps_render.hip compiled for the host under the emulation of grid_emu/ (one std::thread per thread
// of a workgroup, barriers at the wave operations, real atomics).  tests/test_host_map_render.py hands them the cell arrays of a grid it
// made up and compares the view with the numpy statement.  RenderArgs and RenderPlane (csrc/pps_render.h, pps_render_ray.h) are mirrored
// with ctypes; emu_render_sizes tells the test whether the mirrors fit.
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
#include "pps_render.hip"
using namespace pps;
extern "C" {
void emu_render_sizes(int out[2]) { out[0] = sizeof(RenderArgs); out[1] = sizeof(RenderPlane); }
int emu_render_slots(long long n_cells_all, unsigned int min_count, const unsigned int* cnt, const long long* tile_prefix, int* slot) {
  return launch_render_slots(n_cells_all, min_count, cnt, tile_prefix, slot, nullptr);
}
int emu_render(const RenderArgs* a) { return launch_render(*a, nullptr); }
}
