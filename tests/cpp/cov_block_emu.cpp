// cov_block_emu.cpp -- k_cov_path and k_cov_gram of csrc/pps_cov.hip, compiled for the host like tests/cpp/cov_emu.cpp compiles the recovery
// (block_emu/hip/hip_runtime.h: one std::thread per thread of a workgroup, std::barrier as __syncthreads).  tests/test_host_cov_block.py
// feeds them the factor panels of a dense Cholesky factor in the device layout (what is unspecified on the device is NaN here) and the
// request tables of a query, and compares the blocks they write with np.linalg.inv.
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
// out: [status | blocks]; Y: the strip buffer (n_strip doubles)
extern "C" int emu_cov_block(int n_fronts, int* f_p, int* f_b, int64_t* f_Loff, int* f_cmap_off, int* cmap, double* L, const void* walks, int n_walks,
                             const void* steps, int n_steps, int K, int max_p, int max_front, double* Y, long long n_strip, const void* pairs,
                             int n_pairs, double* out, long long n_out) {
  DevGraph d; d.n_fronts = n_fronts; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_cmap_off = f_cmap_off; d.cmap = cmap; d.L = L;
  if (cov_path_lds_bytes(max_p, max_front) > sizeof(cov_lds)) return -1;
  int rc = launch_cov_path(d, (const CovWalk*)walks, n_walks, (const CovStep*)steps, n_steps, K, max_p, max_front, Y, n_strip, out, nullptr);
  if (rc != 0) return rc;
  return launch_cov_gram((const CovPair*)pairs, n_pairs, Y, n_strip, out, n_out, nullptr);
}
