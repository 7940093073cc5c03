// A stand-in for <hip/hip_runtime.h> that lets tests/cpp/grid_emu.cpp compile csrc/pps_grid.hip for the HOST: the stand-in of map_emu/
// (one std::thread per thread of a workgroup, barriers at the wave operations) plus what pps_grid.hip uses beyond pps_map.hip -- the
// wave shuffles and integer atomics on global memory.  The workgroups run one after the other, the threads of one at the same time:
// the atomics are real ones (std::atomic_ref), so the votes of a workgroup do race the way they do on the device.
#pragma once
#include "../../map_emu/hip/hip_runtime.h"

#include <atomic>
using std::max;

inline int emu_shuffle(int v, int from) {                          // lane `from` of the caller's wave, the caller's own value if it is outside
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  g_emu.xi[w][l] = v;
  g_emu.wave[w]->arrive_and_wait();
  const int r = from >= 0 && from < 64 ? g_emu.xi[w][from] : v;
  g_emu.wave[w]->arrive_and_wait();
  return r;
}
inline int __shfl_xor(int v, int mask) { return emu_shuffle(v, (int)(threadIdx.x & 63) ^ mask); }
inline unsigned int __shfl_up(unsigned int v, unsigned int d) { return (unsigned int)emu_shuffle((int)v, (int)(threadIdx.x & 63) - (int)d); }

template <class T> inline T emu_fetch_max(T* p, T v) {
  std::atomic_ref<T> a(*p);
  T old = a.load();
  while (old < v && !a.compare_exchange_weak(old, v)) {}
  return old;
}
template <class T> inline T emu_fetch_min(T* p, T v) {
  std::atomic_ref<T> a(*p);
  T old = a.load();
  while (old > v && !a.compare_exchange_weak(old, v)) {}
  return old;
}
inline int atomicMin(int* p, int v) { return emu_fetch_min(p, v); }
inline int atomicMax(int* p, int v) { return emu_fetch_max(p, v); }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { return emu_fetch_max(p, v); }
inline unsigned int atomicAdd(unsigned int* p, unsigned int v) { return std::atomic_ref<unsigned int>(*p).fetch_add(v); }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return std::atomic_ref<unsigned long long>(*p).fetch_add(v); }
