// The arithmetic of the polyphase resampler, stated once for k_resample (qasr_resample.hip) and the streaming kernels
// (qasr_stream_rs.hip): the launch parameters, the channel sum of a frame, one tap, the final rounding and the header check.
// The host statement is qasr/resample.py (RULES).
#pragma once
#include "qasr_internal.h"

namespace qasr {

#define RS_MAGIC 0x31535251

struct ResampleP {
  const int32_t* blob;          // header (32 words) + table [2 W][L]
  const void* in;               // int16 or float32 [B][in_pitch][ch]
  const int32_t* in_lens;       // [B] frames
  float* out;                   // [B][out_pitch]
  int32_t* out_lens;            // [B]
  long long in_pitch, out_pitch;
  int L, M, W, ch;
};

template <typename T>
struct RsAcc;
template <>
struct RsAcc<int16_t> {
  typedef long long acc_t;
  typedef int32_t stage_t;
};
template <>
struct RsAcc<float> {
  typedef double acc_t;
  typedef double stage_t;
};

// frame k of a row as the sum of its channels (k inside [0, n) is the caller's business)
__device__ __forceinline__ int32_t rs_frame(const int16_t* row, long long k, int ch) {
  const int16_t* f = row + k * ch;
  int32_t v = f[0];
  for (int c = 1; c < ch; ++c) v += f[c];
  return v;
}
__device__ __forceinline__ double rs_frame(const float* row, long long k, int ch) {
  const float* f = row + k * ch;
  double v = (double)f[0];
  for (int c = 1; c < ch; ++c) v = v + (double)f[c];
  return v;
}

__device__ __forceinline__ long long rs_tap(long long acc, int32_t c, int32_t x) { return acc + (long long)c * (long long)x; }
__device__ __forceinline__ double rs_tap(double acc, int32_t c, double x) {
#pragma clang fp contract(off)
  const double hq = (double)c * 9.313225746154785e-10;      // 2^-30: exact
  const double pr = hq * x;
  return acc + pr;
}

__device__ __forceinline__ float rs_finish(long long acc, int ch) {
  return (float)((double)acc / ((double)ch * 35184372088832.0));       // ch * 2^45
}
__device__ __forceinline__ float rs_finish(double acc, int ch) { return (float)(acc / (double)ch); }

// the header lies in device memory; the launch repeats L, M, W: a disagreement ends the row empty
__device__ __forceinline__ bool rs_header_ok(const ResampleP& p) {
  const int32_t* h = p.blob;
  return h[0] == RS_MAGIC && h[3] == p.L && h[4] == p.M && h[5] == p.W;
}

}  // namespace qasr
