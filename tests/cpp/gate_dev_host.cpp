// gate_dev_host.cpp -- csrc/pps_gate_dev.h on the host (test infrastructure, tests/test_host_gate_dev.py): the Cholesky solve behind d2
// and the strip products of the Mahalanobis gate kernels, called as the kernels call them.  Built with g++ and -ffp-contract=off
// through tests/cpp/block_emu/hip/hip_runtime.h, so that every operation is the IEEE double operation the header's comments name.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
// what the K1 headers use beyond block_emu/hip/hip_runtime.h (as in gate_emu.cpp; none of it is run here)
using std::min;
struct double2 { double x, y; };
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_amdgcn_wave_barrier() ((void)0)
inline double __shfl_down(double v, int, int) { return v; }
inline double __shfl(double v, int, int) { return v; }
inline double __shfl_xor(double v, int, int) { return v; }
#include "pps_gate_dev.h"
using namespace pps;

// A: M x M row-major (read on and below the diagonal), r: M.  Returns 1 if every pivot passed; *d2 as chol_d2 leaves it.
extern "C" int gate_dev_chol_d2(int M, const double* A, const double* r, double pivot_min, double* d2) {
  if (M == 3) return chol_d2<3>(A, r, pivot_min, *d2) ? 1 : 0;
  if (M == 6) return chol_d2<6>(A, r, pivot_min, *d2) ? 1 : 0;
  return -1;
}

// the 64 lanes of a wave one after the other over strip_gram3<DA, 3>, their partial sums [entry][lane], then lane_order_sum per entry
template <int DA>
static void gram(const double* Ja, const double* Jb, const double* Ya, const double* Yb, int len_a, int len_b, int common, int K, double* s6) {
  double part[6 * 64];
  for (int lane = 0; lane < 64; lane++) {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    strip_gram3<DA, 3>(Ja, Jb, Ya, Yb, len_a, len_b, common, K, lane, s);
    for (int e = 0; e < 6; e++) part[e * 64 + lane] = s[e];
  }
  for (int e = 0; e < 6; e++) s6[e] = lane_order_sum(part + e * 64);
}
extern "C" int gate_dev_strip_gram3(int DA, const double* Ja, const double* Jb, const double* Ya, const double* Yb, int len_a, int len_b, int common,
                                    int K, double* s6) {
  if (DA == 6) gram<6>(Ja, Jb, Ya, Yb, len_a, len_b, common, K, s6);
  else if (DA == 3) gram<3>(Ja, Jb, Ya, Yb, len_a, len_b, common, K, s6);
  else return -1;
  return 0;
}
