// Rational polyphase resampling of PCM audio to the model's rate (k_resample); the host statement is qasr/resample.py (RULES),
// and this file follows it byte for byte.
//
// k_resample<T, STAGED>: one work-group of 256 threads per (utterance, tile of RS_TILE = 256 outputs); thread tid owns output
// i = 256 tile + tid.  Output i sits at p = i M (int64), q = p / L, slot r = i mod L; its 2 W taps j read frame k = q + W - j.
// STAGED: the frames the tile needs, k_lo = q(first) - W + 1 .. q(last) + W, are read ONCE from global memory (coalesced, the
// channels summed: int32 for int16 input, float64 in ascending channel order for float32 input, zero outside [0, n)) into LDS;
// the tap loop then reads LDS and the table.  The table is [j][r]: the 64 lanes of a wave read 64 consecutive words per tap
// (wrapping at L), and for L <= 4 one to four words that every lane shares; it is read-only and stays in L2 / the vector cache.
// The host picks STAGED when the stretch, at most ceil(255 M / L) + 1 + 2 W frames, fits RS_STAGE; a steeper ratio (above
// about 10 : 1 with 'best', 14 : 1 with 'fast') takes the direct instantiation, which reads the frames from global memory per tap.
// int16: acc is the exact int64 sum of c * xs (one 32 x 32 + 64 multiply-add per tap), out = float32(double(acc) / (ch 2^45)).
// float32: acc = acc + hq * xs in float64 with contraction off (a rounded product, then a rounded sum), out = float32(acc / ch).
// A frame at or behind in_lens[b] is never read.  Every output row is written to its pitch (zeros behind out_len); work-group
// 0 of a row writes out_lens[b].  Global memory sees plain vector stores; no atomics; nothing is read back on the host.
#include "qasr_internal.h"
#include "qasr_resample_dev.h"

namespace qasr {

#define RS_NT 256
#define RS_TILE 256
#define RS_STAGE 4096

template <typename T, bool STAGED>
__global__ void __launch_bounds__(RS_NT) k_resample(ResampleP p) {
  typedef typename RsAcc<T>::acc_t acc_t;
  typedef typename RsAcc<T>::stage_t stage_t;
  __shared__ stage_t xs[STAGED ? RS_STAGE : 1];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long L = p.L, M = p.M;
  const int W = p.W, ch = p.ch;
  const long long n = rs_header_ok(p) ? min(max((long long)p.in_lens[b], 0ll), p.in_pitch) : 0;
  const long long out_len = min((n * L + M - 1) / M, p.out_pitch);
  const long long i0 = (long long)blockIdx.x * RS_TILE, i = i0 + tid;
  float* const orow = p.out + (long long)b * p.out_pitch;
  if (blockIdx.x == 0 && tid == 0) p.out_lens[b] = (int32_t)out_len;
  if (i0 >= out_len) {                                                // uniform: a tile behind the utterance
    if (i < p.out_pitch) orow[i] = 0.f;
    return;
  }
  const T* const row = (const T*)p.in + (long long)b * p.in_pitch * ch;
  const long long i1 = min(i0 + RS_TILE - 1, out_len - 1);
  const long long k_lo = (i0 * M) / L - W + 1;
  if (STAGED) {
    const int count = (int)((i1 * M) / L + W - k_lo + 1);             // <= RS_STAGE: the host chose this instantiation by it
    for (int s = tid; s < count && s < RS_STAGE; s += RS_NT) {
      const long long k = k_lo + s;
      xs[s] = (k >= 0 && k < n) ? rs_frame(row, k, ch) : (stage_t)0;
    }
    __syncthreads();
  }
  float y = 0.f;
  if (i < out_len) {
    const long long pp = i * M, q = pp / L;
    const int r = (int)(i % L);
    const int32_t* tab = p.blob + 32 + r;
    acc_t acc = 0;
    if (STAGED) {
      const stage_t* x = xs + (int)(q + W - k_lo);                    // tap j reads x[-j]: inside [0, count)
#pragma unroll 4
      for (int j = 0; j < 2 * W; ++j) acc = rs_tap(acc, tab[(size_t)j * (size_t)L], x[-j]);
    } else {
      for (int j = 0; j < 2 * W; ++j) {
        const long long k = q + W - j;
        const stage_t x = (k >= 0 && k < n) ? rs_frame(row, k, ch) : (stage_t)0;
        acc = rs_tap(acc, tab[(size_t)j * (size_t)L], x);
      }
    }
    y = rs_finish(acc, ch);
  }
  if (i < p.out_pitch) orow[i] = y;
}

// equal rates: no filter.  int16: the float32 channel mean of sample / 32768 (the sum of <= 8 such values is exact in float32);
// float32: a copy, or float32(float64 channel sum / ch)
template <typename T>
__global__ void __launch_bounds__(RS_NT) k_resample_copy(ResampleP p) {
  const int b = blockIdx.y, ch = p.ch;
  const long long n = rs_header_ok(p) ? min(max((long long)p.in_lens[b], 0ll), p.in_pitch) : 0;
  const long long out_len = min(n, p.out_pitch);
  const long long i = (long long)blockIdx.x * RS_TILE + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) p.out_lens[b] = (int32_t)out_len;
  if (i >= p.out_pitch) return;
  const T* const row = (const T*)p.in + (long long)b * p.in_pitch * ch;
  float y = 0.f;
  if (i < out_len) {
    if constexpr (sizeof(T) == 2) {
      const float sum = (float)rs_frame(row, i, ch) * 3.0517578125e-05f;      // 2^-15: exact
      y = ch > 1 ? sum / (float)ch : sum;
    } else {
      y = ch > 1 ? (float)(rs_frame(row, i, ch) / (double)ch) : row[i];
    }
  }
  p.out[(long long)b * p.out_pitch + i] = y;
}

static bool resample_staged(int L, int M, int W) {
  return ((long long)(RS_TILE - 1) * M + L - 1) / L + 1 + 2ll * W <= RS_STAGE;
}

int launch_resample(hipStream_t s, const qasr_resample_args& a) {
  ResampleP p{};
  p.blob = (const int32_t*)a.blob, p.in = a.in, p.in_lens = a.in_lens, p.out = a.out, p.out_lens = a.out_lens;
  p.in_pitch = a.in_pitch, p.out_pitch = a.out_pitch;
  p.L = a.L, p.M = a.M, p.W = a.W, p.ch = a.channels;
  const long long tiles = a.out_pitch > 0 ? (a.out_pitch + RS_TILE - 1) / RS_TILE : 1;       // one work-group writes out_lens even for an empty row
  const dim3 grid((unsigned)tiles, (unsigned)a.B), block(RS_NT);
  const bool f32 = a.dtype == QASR_PCM_F32;
  if (a.L == 1 && a.M == 1) {
    if (f32) hipLaunchKernelGGL(k_resample_copy<float>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_resample_copy<int16_t>, grid, block, 0, s, p);
  } else if (resample_staged(a.L, a.M, a.W)) {
    if (f32) hipLaunchKernelGGL((k_resample<float, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_resample<int16_t, true>), grid, block, 0, s, p);
  } else {
    if (f32) hipLaunchKernelGGL((k_resample<float, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_resample<int16_t, false>), grid, block, 0, s, p);
  }
  return QASR_OK;
}

}  // namespace qasr
