// gate_dev_m6_host.cpp -- csrc/pps_gate_dev.h on the host (test infrastructure, tests/test_host_gate_dev_m6.py): strip_gram<M, DA, DB> as the
// loop gate calls it (M = 6, a 6 x 12 Jacobian whose halves are 12 doubles apart), its M = 3 case next to strip_gram3, and the
// common-ancestor walk the merge gate and the loop gate share.  Built like tests/cpp/gate_dev_host.cpp: g++ and -ffp-contract=off through
// tests/cpp/block_emu/hip/hip_runtime.h, so that every operation is the IEEE double operation the header's comments name.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
// what the K1 headers use beyond block_emu/hip/hip_runtime.h (as in gate_dev_host.cpp; none of it is run here)
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

// the 64 lanes of a wave one after the other, their partial sums [entry][lane], then lane_order_sum per entry
template <int M, class F>
static void lanes(F gram_of_lane, double* out) {
  constexpr int E = M * (M + 1) / 2;
  double part[E * 64];
  for (int lane = 0; lane < 64; lane++) {
    double s[E];
    for (int e = 0; e < E; e++) s[e] = 0.0;
    gram_of_lane(lane, s);
    for (int e = 0; e < E; e++) part[e * 64 + lane] = s[e];
  }
  for (int e = 0; e < E; e++) out[e] = lane_order_sum(part + e * 64);
}

// J: 6 x 12 row-major, columns of a then of b (read as the kernel reads it: two halves, 12 doubles between rows); s21: the lower triangle
extern "C" void gate_dev_strip_gram6(const double* J, const double* Ya, const double* Yb, int len_a, int len_b, int common, int K, double* s21) {
  lanes<6>([&](int lane, double* s) { strip_gram<6, 6, 6>(J, 12, J + 6, 12, Ya, Yb, len_a, len_b, common, K, lane, s); }, s21);
}
// Ja, Jb: 3 x 3 packed.  generic != 0: strip_gram<3, 3, 3>; else strip_gram3<3, 3>
extern "C" void gate_dev_strip_gram33(int generic, const double* Ja, const double* Jb, const double* Ya, const double* Yb, int len_a, int len_b, int common,
                                      int K, double* s6) {
  if (generic) lanes<3>([&](int lane, double* s) { strip_gram<3, 3, 3>(Ja, 3, Jb, 3, Ya, Yb, len_a, len_b, common, K, lane, s); }, s6);
  else lanes<3>([&](int lane, double* s) { strip_gram3<3, 3>(Ja, Jb, Ya, Yb, len_a, len_b, common, K, lane, s); }, s6);
}
// returns 1 with *common set, 0 when the walk met an index outside the tables
extern "C" int gate_dev_common_root_pivots(const int* parent, const int* rootlen, int n_fronts, int fa, int fb, int* common) {
  return common_root_pivots(parent, rootlen, n_fronts, fa, fb, *common) ? 1 : 0;
}
