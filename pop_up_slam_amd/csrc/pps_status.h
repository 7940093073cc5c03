// pps_status.h -- the status word of a device call and the finiteness tests that decide what is raised into it.  A light header: it needs
// <hip/hip_runtime.h> alone, so the kernels, the register-tile header and the host emulations under tests/cpp/ all share this one copy.
#pragma once
#ifndef PPS_WAVE_EMU        // (tests/cpp/wave_emu.h compiles this header for the host, one coroutine per lane)
#include <hip/hip_runtime.h>
#endif
#include <math.h>

namespace pps {

// The status word of a solve or a query (result_dev[2], out[0], MergeArgs::status: 0 ok | 1 not positive definite | >= kStatusInternal an
// internal error) is RAISED, never overwritten: a not-PD front that reports after a hand-over time-out must not turn the internal error
// into an ordinary rejected step.  Non-negative doubles order like their bit patterns, so the maximum is one integer atomic without a
// return value.
#ifndef PPS_WAVE_EMU
__device__ __forceinline__ void raise_status(double* w, double v) {
  atomicMax(reinterpret_cast<unsigned long long*>(w), (unsigned long long)__double_as_longlong(v));
}
#else
inline void raise_status(double* w, double v) { if (v > *w) *w = v; }
#endif

constexpr double kDblMax = 1.79769313486231570e308;
__device__ __forceinline__ bool finite_pos(double p) { return p > 0.0 && p <= kDblMax; }      // positive and finite (false for NaN)
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= kDblMax; }            // (false for NaN)

}  // namespace pps
