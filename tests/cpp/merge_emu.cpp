// merge_emu.cpp -- k_cov_path (csrc/pps_cov.hip) and k_merge_gate (csrc/pps_merge.hip) compiled for the host, in the manner of
// tests/cpp/gate_emu.cpp: one std::thread per thread of a workgroup, std::barrier as __syncthreads, the workgroups one after the other (the
// last ticket of a row is therefore drawn by the workgroup of the row's last pair, as on the device by whichever finishes last).
// tests/test_host_merge_gate.py feeds them the panels of a dense Cholesky factor in the device layout, plane states and the tree tables, and
// compares d2 / best / the flags with the dense formula; emu_lin_plane_prior gives it J and r of a plane prior by csrc/pps_lin.h on the host.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
// what pps_merge.hip and the K1 headers use beyond block_emu/hip/hip_runtime.h
using std::min;
struct double2 { double x, y; };
inline unsigned int atomicAdd(unsigned int* p, unsigned int v) { std::lock_guard<std::mutex> l(g_mu); const unsigned int o = *p; *p += v; return o; }
inline void __threadfence() { std::atomic_thread_fence(std::memory_order_seq_cst); }
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __hip_atomic_store(p, v, order, scope) (*(p) = (v))
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_amdgcn_wave_barrier() ((void)0)
inline double __shfl_down(double v, int, int) { return v; }      // (the lane form of K1 itself is not run here: the merge gate goes through LDS)
inline double __shfl(double v, int, int) { return v; }
inline double __shfl_xor(double v, int, int) { return v; }
namespace pps { namespace { alignas(16) double cov_lds[32768]; alignas(16) double merge_lds[4096]; } }
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
  gridDim = grid;
  for (unsigned b = 0; b < grid.x; b++) {
    std::barrier<> bar(block.x); g_barrier = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([&, t]() { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); g_barrier->arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
#include "pps_cov.hip"
#include "pps_merge.hip"
namespace pps { unsigned long long launch_count() { return 0; } void count_launch() {} }
using namespace pps;

// record = [J 3 x 3 | r 3] of a plane prior, central differences, by the thread form of K1 on the host
extern "C" void emu_lin_plane_prior(const double* plane4, const double* ms4, const double* w6, double* out12) { lin_plane_prior<0>(plane4, ms4, w6, out12); }

// status: one double (zero on entry); Y: the strip buffer (n_strip doubles); ticket: n zeros; planes: n records {strip, slot, front}
extern "C" int emu_merge(int n_fronts, int* f_p, int* f_b, int64_t* f_Loff, int* f_cmap_off, int* cmap, double* L, const void* walks, int n_walks,
                         const void* steps, int n_steps, int K, int max_p, int max_front, double* Y, long long n_strip, int n_plane, int plane_ld,
                         double* plane_est, const void* planes, int n, const int* parent, const int* rootlen, double floor_var, double threshold,
                         unsigned int* ticket, double* status, int* best, unsigned char* flag, double* d2, double* rec) {
  DevGraph d; d.n_fronts = n_fronts; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_cmap_off = f_cmap_off; d.cmap = cmap; d.L = L;
  d.n_plane = n_plane; d.plane_ld = plane_ld; d.plane_est = plane_est;
  rot_step_quat(d.step_ac); plane_step_quat(d.step_ac + 2);
  if (cov_path_lds_bytes(max_p, max_front) > sizeof(cov_lds)) return -1;
  int rc = launch_cov_path(d, (const CovWalk*)walks, n_walks, (const CovStep*)steps, n_steps, K, max_p, max_front, Y, n_strip, status, nullptr);
  if (rc != 0) return rc;
  MergeArgs a;
  a.planes = (const MergePlane*)planes; a.n = n; a.n_pairs = (long long)n * (n - 1) / 2; a.parent = parent; a.rootlen = rootlen; a.n_fronts = n_fronts;
  a.K = K; a.Y = Y; a.n_strip = n_strip; a.floor_var = floor_var; a.threshold = threshold; a.ticket = ticket; a.status = status; a.best = best;
  a.flag = flag; a.d2 = d2; a.rec = rec;
  return launch_merge_gate(d, a, nullptr);
}
