// loop_emu.cpp -- k_cov_path (csrc/pps_cov.hip) and k_loop_gate (csrc/pps_loop.hip) compiled for the host, in the manner of
// tests/cpp/merge_emu.cpp: one std::thread per thread of a workgroup, std::barrier as __syncthreads, the workgroups one after the other.
// tests/test_host_loop_gate.py feeds them the panels of a dense Cholesky factor in the device layout, pose states, the candidates and the tree
// tables, and compares d2 / S / the flags with the dense formula; emu_lin_odometry gives it Jw and r of an odometry factor by csrc/pps_lin.h
// on the host.
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
// what pps_loop.hip and the K1 headers use beyond block_emu/hip/hip_runtime.h
using std::min;
struct double2 { double x, y; };
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_amdgcn_wave_barrier() ((void)0)
inline double __shfl_down(double v, int, int) { return v; }      // (the lane form of K1 itself is not run here: the loop gate goes through LDS)
inline double __shfl(double v, int, int) { return v; }
inline double __shfl_xor(double v, int, int) { return v; }
namespace pps { namespace { alignas(16) double cov_lds[32768]; alignas(16) double loop_lds[8192]; } }
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
#include "pps_loop.hip"
namespace pps { unsigned long long launch_count() { return 0; } void count_launch() {} }
using namespace pps;
static_assert(sizeof(LoopCand) == 248, "tests/loop_gate_helpers.py: CAND");

// record = [J_a 6 x 6 | J_b 6 x 6 | r 6] of an odometry factor by the thread form of K1 on the host; mode 1: the closed form
extern "C" void emu_lin_odometry(int mode, const double* p1, const double* p2, const double* ms6, const double* w21, double* out78) {
  if (mode == 1) lin_odometry<1>(p1, p2, ms6, w21, out78); else lin_odometry<0>(p1, p2, ms6, w21, out78);
}

// status: one double (zero on entry); Y: the strip buffer (n_strip doubles); cands: n records LoopCand; S and rec may be null
extern "C" int emu_loop(int n_fronts, int* f_p, int* f_b, int64_t* f_Loff, int* f_cmap_off, int* cmap, double* L, const void* walks, int n_walks,
                        const void* steps, int n_steps, int K, int max_p, int max_front, double* Y, long long n_strip, int n_pose, int pose_ld,
                        double* pose_est, const void* cands, int n, const int* parent, const int* rootlen, double threshold, int mode, double* status,
                        unsigned char* flag, double* d2, double* S, double* rec) {
  DevGraph d; d.n_fronts = n_fronts; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_cmap_off = f_cmap_off; d.cmap = cmap; d.L = L;
  d.n_pose = n_pose; d.pose_ld = pose_ld; d.pose_est = pose_est;
  rot_step_quat(d.step_ac); plane_step_quat(d.step_ac + 2);
  if (cov_path_lds_bytes(max_p, max_front) > sizeof(cov_lds)) return -1;
  int rc = launch_cov_path(d, (const CovWalk*)walks, n_walks, (const CovStep*)steps, n_steps, K, max_p, max_front, Y, n_strip, status, nullptr);
  if (rc != 0) return rc;
  LoopArgs a;
  a.cands = (const LoopCand*)cands; a.n = n; a.parent = parent; a.rootlen = rootlen; a.n_fronts = n_fronts;
  a.K = K; a.Y = Y; a.n_strip = n_strip; a.threshold = threshold; a.mode = mode; a.status = status; a.flag = flag; a.d2 = d2; a.S = S; a.rec = rec;
  return launch_loop_gate(d, a, nullptr);
}
