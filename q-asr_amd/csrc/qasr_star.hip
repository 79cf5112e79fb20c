// The wildcard's emission plane (k_star); the host statement is STAR_RULES and star_host of qasr/align.py, and this file follows
// it bit for bit: star[u][t] = (the float32 maximum of logp[u][t][0 .. C) in align_key's order) - penalty for t < lim, 0 behind.
//
// k_star: one wave per frame, four frames to a work-group of 256 threads.  The lanes stride the frame's C classes with 16-byte
// loads where the row's address allows: a scalar head up to the first 16-byte boundary (at most 3 floats), float4s, a scalar
// tail (at most 3).  Each lane keeps the largest key it saw, six __shfl_xor steps spread the wave's maximum, lane 0 subtracts
// the penalty with one __fsub_rn and stores one float.  Every byte of logp is read once, so the kernel is memory-bound:
// 4 B T C bytes in, 4 B T out.  LDS: none.  Global memory sees plain vector stores.  Nothing is allocated and no length is read
// on the host.  The key (align_key of the host statement) is qasr_fixed_dev.h's fx_key.
#include <climits>

#include "qasr_fixed_dev.h"

namespace qasr {

#define STAR_NT 256
#define STAR_WAVE 64
#define STAR_FRAMES (STAR_NT / STAR_WAVE)

struct StarP {
  const float* logp;
  const int32_t* lens;          // optional [B]
  float* star;                  // [B][star_pitch]
  long long pitch_b, pitch_t, star_pitch, frames;                   // frames = B * T
  int T, C;
  float penalty;
};

__global__ void __launch_bounds__(STAR_NT) k_star(StarP p) {
  const int lane = threadIdx.x & (STAR_WAVE - 1);
  const long long f = (long long)blockIdx.x * STAR_FRAMES + (threadIdx.x / STAR_WAVE);
  if (f >= p.frames) return;                                        // wave-uniform; no barrier follows
  const int u = (int)(f / p.T), t = (int)(f - (long long)u * p.T);
  const int lim = p.lens ? min(max(p.lens[u], 0), p.T) : p.T;
  float* const out = p.star + (long long)u * p.star_pitch + t;      // t < T <= star_pitch
  if (t >= lim) {
    if (lane == 0) *out = 0.f;
    return;
  }
  const int C = p.C;
  const float* const row = p.logp + (long long)u * p.pitch_b + (long long)t * p.pitch_t;   // [0, C) inside the row: C <= pitch_t
  const int head = min((int)((4 - (((uintptr_t)row >> 2) & 3)) & 3), C);       // floats before the first 16-byte boundary
  const int nvec = (C - head) >> 2, tail0 = head + 4 * nvec;        // float4s; the first float behind them
  int best = INT_MIN;
  if (lane < head) best = fx_key(__float_as_int(row[lane]));        // head <= 3
  const float4* const v = reinterpret_cast<const float4*>(row + head);
  for (int i = lane; i < nvec; i += STAR_WAVE) {                    // head + 4 i + 3 < head + 4 nvec <= C
    const float4 x = v[i];
    const int k0 = fx_key(__float_as_int(x.x)), k1 = fx_key(__float_as_int(x.y));
    const int k2 = fx_key(__float_as_int(x.z)), k3 = fx_key(__float_as_int(x.w));
    best = max(best, max(max(k0, k1), max(k2, k3)));
  }
  if (tail0 + lane < C) best = max(best, fx_key(__float_as_int(row[tail0 + lane])));       // C - tail0 <= 3
#pragma unroll
  for (int o = STAR_WAVE / 2; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
  if (lane == 0) *out = __fsub_rn(__int_as_float(fx_key(best)), p.penalty);
}

int launch_star(hipStream_t s, const qasr_ctc_star_args& a) {
  StarP p{};
  p.logp = a.log_probs, p.lens = a.lens, p.star = a.star;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame, p.star_pitch = a.star_pitch;
  p.frames = (long long)a.B * a.T;
  p.T = a.T, p.C = a.C, p.penalty = a.penalty;
  const long long groups = (p.frames + STAR_FRAMES - 1) / STAR_FRAMES;
  if (groups > INT_MAX) return QASR_ERR_ARG;
  hipLaunchKernelGGL(k_star, dim3((unsigned)groups), dim3(STAR_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
