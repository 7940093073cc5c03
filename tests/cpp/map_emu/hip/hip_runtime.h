// A stand-in for <hip/hip_runtime.h> that lets tests/cpp/map_emu.cpp compile csrc/pps_map.hip for the HOST (beside block_emu/, which has no
// wave primitives): one std::thread per thread of a workgroup, the workgroups one after the other.  __syncthreads is a barrier over the
// workgroup; the wave operations pps_map.hip uses -- __ballot, readlane, mbcnt, the wave barrier -- meet at a barrier over the 64 threads
// of a wave, so a lane that read LDS another lane wrote WITHOUT such a meeting point in between would be a data race here.
// __shared__ variables become function-local statics (workgroups do not overlap).  Only what pps_map.hip uses.
#pragma once
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstring>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
extern thread_local dim3 threadIdx, blockIdx;
constexpr int kEmuMaxWaves = 16;
struct EmuGroup {
  std::barrier<>* wg;
  std::barrier<>* wave[kEmuMaxWaves];
  unsigned char pred[kEmuMaxWaves][64];
  int xi[kEmuMaxWaves][64];
};
extern EmuGroup g_emu;
using std::min;
inline void __syncthreads() { g_emu.wg->arrive_and_wait(); }
inline void __builtin_amdgcn_wave_barrier() { g_emu.wave[threadIdx.x >> 6]->arrive_and_wait(); }
inline unsigned long long __ballot(int p) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_emu.pred[w][l] = p != 0;
  g_emu.wave[w]->arrive_and_wait();
  unsigned long long m = 0;
  for (int i = 0; i < 64; i++) m |= (unsigned long long)g_emu.pred[w][i] << i;
  g_emu.wave[w]->arrive_and_wait();
  return m;
}
inline int __builtin_amdgcn_readlane(int v, int lane) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_emu.xi[w][l] = v;
  g_emu.wave[w]->arrive_and_wait();
  const int r = g_emu.xi[w][lane & 63];
  g_emu.wave[w]->arrive_and_wait();
  return r;
}
// v_mbcnt_lo / _hi: bits of the mask below the calling lane, added to the accumulator
inline unsigned int __builtin_amdgcn_mbcnt_lo(unsigned int m, unsigned int acc) {
  const int l = threadIdx.x & 63;
  return acc + (unsigned int)__builtin_popcount(l >= 32 ? m : (m & ((1u << l) - 1u)));
}
inline unsigned int __builtin_amdgcn_mbcnt_hi(unsigned int m, unsigned int acc) {
  const int l = threadIdx.x & 63;
  return acc + (unsigned int)__builtin_popcount(l <= 32 ? 0u : (m & ((1u << (l - 32)) - 1u)));
}
inline int __popcll(unsigned long long m) { return __builtin_popcountll(m); }
inline int __ffsll(long long m) { return __builtin_ffsll(m); }
typedef int hipError_t; typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1 };
inline hipError_t hipGetLastError() { return 0; }
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a);
#define hipLaunchKernelGGL(k, grid, block, lds, st, ...) emu_launch(k, grid, block, __VA_ARGS__)
