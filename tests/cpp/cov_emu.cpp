// cov_emu.cpp -- csrc/pps_cov.hip itself, compiled for the host (block_emu/hip/hip_runtime.h): the kernels of the covariance recovery run as
// 256 std::threads per workgroup with std::barrier as __syncthreads.  tests/test_host_cov.py feeds them the factor panels of a dense Cholesky
// factor in the device layout (what is unspecified on the device is NaN here) and compares every entry they write with np.linalg.inv.
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
namespace pps { namespace { alignas(16) double cov_lds[32768]; } }
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
  for (unsigned b = 0; b < grid.x; b++) {
    std::barrier<> bar(block.x); g_barrier = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([&, t]() { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); g_barrier->arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
#include "pps_cov.hip"
namespace pps { unsigned long long launch_count() { return 0; } void count_launch() {} }
using namespace pps;
extern "C" int emu_cov(int n_fronts, int n_levels, const int* level_off, int* level_fronts, int* f_p, int* f_b, int64_t* f_Loff, int64_t* f_Uoff,
                       int* f_cmap_off, int* cmap, const int* parent, double* L, double* U, double* S, double* status) {
  DevGraph d; d.level_fronts = level_fronts; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_Uoff = f_Uoff; d.f_cmap_off = f_cmap_off; d.cmap = cmap;
  d.L = L; d.U = U; d.result_dev = status;
  for (int l = n_levels - 1; l >= 0; l--) launch_cov_level(d, S, parent, level_off[l], level_off[l + 1] - level_off[l], 1000, nullptr);
  return 0;
}
extern "C" int emu_gather(const double* S, const void* req, int n, double* out) { return launch_cov_gather(S, (const CovReq*)req, n, out, nullptr); }
