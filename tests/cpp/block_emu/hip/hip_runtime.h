// A stand-in for <hip/hip_runtime.h> that lets tests/cpp/cov_emu.cpp compile csrc/pps_cov.hip for the HOST: one std::thread per thread of a
// workgroup, std::barrier as __syncthreads, the launch macros run the workgroups one after the other.  Only what pps_cov.hip uses.
#pragma once
#include <barrier>
#include <cstdint>
#include <cstring>
#include <mutex>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
extern thread_local dim3 threadIdx, blockIdx;
extern std::barrier<>* g_barrier;
inline void __syncthreads() { g_barrier->arrive_and_wait(); }
typedef int hipError_t; typedef void* hipStream_t; typedef void* hipEvent_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipGetDevice(int* d) { *d = 0; return 0; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline long long __double_as_longlong(double v) { long long r; memcpy(&r, &v, 8); return r; }
extern std::mutex g_mu;
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { std::lock_guard<std::mutex> l(g_mu); unsigned long long o = *p; if (v > o) *p = v; return o; }
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a);
#define hipLaunchKernelGGL(k, grid, block, lds, st, ...) emu_launch(k, grid, block, __VA_ARGS__)
#define hipExtLaunchKernelGGL(k, grid, block, lds, st, e0, e1, f, ...) emu_launch(k, grid, block, __VA_ARGS__)
