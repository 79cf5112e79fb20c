// The fixed-point arithmetic of every CTC kernel, stated once: the beam kernels (qasr_beam_dev.h, qasr_beam.hip) and the lattice
// kernels (qasr_lattice_dev.h).  The host statement is qasr/beam.py (NEG, quantize, lae, _order_key).  Scores are int64 sums of
// q = rint(logp * 2^16); NEG is "no path" and is never added to.  k_stream_beam_ep keeps its own text.
// Bounds.  fx_lae reads tab[d >> 6] only for 0 <= d < FX_DMAX = 2^20, so the index is below FX_TAB = 2^14: the caller passes a
// table of FX_TAB entries (the entry points check the count).  fx_quantize and fx_key touch no memory.
#pragma once
#include "qasr_internal.h"

namespace qasr {

#define FX_NEG (-(1ll << 62))
#define FX_QFLOOR (-1073741824.f)
#define FX_QCEIL (1073741824.f)
#define FX_DMAX (16ll << 16)
#define FX_TAB QASR_BEAM_TABLE_ENTRIES

// the order-preserving integer image of a float's bits (its own inverse)
__device__ __forceinline__ int fx_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

__device__ __forceinline__ int fx_quantize(float x) {
  float y = x * 65536.f;
  if (!(y >= FX_QFLOOR)) y = FX_QFLOOR;            // NaN and -inf take the floor
  if (y > FX_QCEIL) y = FX_QCEIL;
  return (int)rintf(y);
}

__device__ __forceinline__ long long fx_lae(long long a, long long b, const uint16_t* tab) {
  const long long m = a > b ? a : b, n = a > b ? b : a;
  if (n == FX_NEG) return m;
  const long long d = m - n;
  if (d >= FX_DMAX) return m;
  return m + (long long)tab[d >> 6];
}

}  // namespace qasr
