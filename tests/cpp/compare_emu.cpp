// compare_emu.cpp -- the kernels of csrc/pps_compare.hip compiled for the host under the emulation of grid_emu/ (one std::thread per thread
// of a workgroup, barriers at the wave operations, real atomics), as render_emu.cpp does for the render.  tests/test_host_map_compare.py
// hands them images and a plane table it made up and compares every output with the numpy statement.  emu_compare drives the three
// kernels the way pps_map_compare.cpp does: the plane rows from the four doubles, the zeroed table, k_compare, the two finish kernels.
#include <cstddef>
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
// what pps_compare.hip uses beyond pps_grid.hip: the compare-and-swap that claims a slot of the workgroup's table
inline int atomicCAS(int* p, int expected, int desired) {
  std::atomic_ref<int>(*p).compare_exchange_strong(expected, desired);
  return expected;
}
#include "pps_compare.hip"
using namespace pps;
extern "C" {
void emu_compare_sizes(int out[4]) {
  out[0] = sizeof(CompareBlock); out[1] = offsetof(CompareBlock, planes); out[2] = kCompareSlots; out[3] = kComparePasses * kMapThreads;
}
// table: compare_table_words(nplanes, n_rows) words; block: sizeof(CompareBlock) bytes; rows: n_rows records; pairs: nplanes * n_rows records
int emu_compare(int npx, int nplanes, int n_rows, double tol, const MapPt* cloud, const int* frame_id, const int* view_id, const int* ids,
                const double* abcd, unsigned long long* table, CompareBlock* block, pps_map_compare_row* rows, pps_map_compare_pair* pairs) {
  std::vector<ComparePlane> planes((size_t)n_rows);
  for (int r = 0; r < n_rows; r++)
    if (!compare_plane(abcd + 4 * r, &planes[r])) return -1;
  memset(table, 0, compare_table_words(nplanes, n_rows) * sizeof(unsigned long long));
  CompareArgs a{};
  a.npx = npx; a.nplanes = nplanes; a.n_rows = n_rows; a.tol = tol;
  a.cloud = cloud; a.frame_id = frame_id; a.view_id = view_id; a.ids = ids; a.planes = planes.data(); a.table = table;
  if (launch_compare(a, nullptr) != hipSuccess) return -2;
  CompareFinishArgs f{};
  f.nplanes = nplanes; f.n_rows = n_rows; f.ids = ids; f.table = table; f.block = block; f.rows = rows; f.pairs = pairs;
  return launch_compare_finish(f, nullptr) == hipSuccess ? 0 : -3;
}
}
