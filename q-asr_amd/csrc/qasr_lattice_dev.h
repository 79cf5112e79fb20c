// What the CTC lattice kernels share beyond the arithmetic of qasr_fixed_dev.h, stated once for k_align (qasr_align.hip),
// k_align_band (qasr_align_band.hip), k_post (qasr_post.hip), k_post_band (qasr_post_band.hip) and k_spot (qasr_spot.hip): the
// checks of device data, a state's label and skip rule, the wildcard-aware emission read, the back-walk's window constants, the
// posterior's clamp and the launch ladders.  The host statements are qasr/align.py (RULES, STAR_RULES, BAND_RULES, POST_RULES) and qasr/spot.py.
// The lattice of a target y[0 .. L) has the states s = 0 .. 2L: even states are blanks, the odd state s carries y[s >> 1].
// Bounds each helper relies on.
//   lattice_check_target / lattice_check_runs read y, start, nframes at i (and i - 1 where i >= 1) for first <= i < L only: the
//     caller has checked 0 <= L <= ML, the row pitch.  They read nothing through a label or a run; runs are summed in 64 bits.
//   lattice_slot(y, s, S) is called for an odd s < S = 2L + 1 only (spot: s < 2L): it reads y[i - 1], y[i], y[i + 1] at
//     i = s >> 1 < L, the first only where s >= 3 (i >= 1), the last only where s + 2 < S (i + 1 < L).  Only the posterior
//     kernels use skip_bwd; in the three others the read of y[i + 1] is dead after inlining and is not issued.
//   LatticeEmit reads logp[u][t][c] for a checked label or the blank, c < C <= pitch_frame, and a frame t < lim <= T, inside the
//     utterance's pitch_utt >= T * pitch_frame; with STAR the wildcard c == C reads star[u][t], t < T <= star_pitch, and nothing
//     at [.. + C].  The entry points (qasr_engine.hip) check the pitches.
#pragma once
#include <type_traits>

#include "qasr_fixed_dev.h"

namespace qasr {

#define LATTICE_NT 256                          /* threads of a work-group of the four work-group kernels */
#define LATTICE_BLOCK 32                        /* frames between two moves of the band's base = frames per entry of band_base */
#define LATTICE_G 16                            /* byte rows (4 frames each) per back-walk window */
#define LATTICE_WINW (8 * LATTICE_G + 4)        /* states per window row: the path descends <= 2 * 4 * G inside one window */
#define LATTICE_GFLOOR (-(1ll << 30))

// a label outside [0, C) (STAR: [0, C]) or equal to blank, among the labels first, first + stride, ... < L
template <bool STAR>
__device__ __forceinline__ bool lattice_check_target(const int32_t* y, int L, int C, int blank, int first, int stride) {
  bool bad = false;
  for (int i = first; i < L; i += stride) {
    const int c = y[i];
    if (c < 0 || c >= C + (STAR ? 1 : 0) || c == blank) bad = true;
  }
  return bad;
}

// start / nframes do not describe a CTC alignment of y over lim frames: every run has a frame, runs do not overlap, equal
// neighbours leave a frame for the blank between them, the last run ends inside lim
__device__ __forceinline__ bool lattice_check_runs(const int32_t* y, const int32_t* start, const int32_t* nframes, int L, int lim,
                                                   int first, int stride) {
  bool bad = false;
  for (int i = first; i < L; i += stride) {
    const long long st = start[i], n = nframes[i];
    const long long end_before = i ? (long long)start[i - 1] + (long long)nframes[i - 1] : 0;         // one past run i - 1
    bad |= n < 1 || st < end_before || (i && y[i] == y[i - 1] && st < end_before + 1);
    bad |= i == L - 1 && st + n > (long long)lim;
  }
  return bad;
}

// the odd state s < S: its label, and whether it may skip the blank below it (forward) / above it (backward)
struct LatticeSlot {
  int label;
  bool skip_fwd, skip_bwd;
};
__device__ __forceinline__ LatticeSlot lattice_slot(const int32_t* y, int s, int S) {
  const int i = s >> 1;
  return {y[i], s >= 3 && y[i] != y[i - 1], s + 2 < S && y[i + 1] != y[i]};
}

template <bool STAR>
struct LatticeEmit {
  const float* base;                            // logp[u]
  const float* star;                            // star[u] (STAR only)
  long long pitch_t;
  int C;
  struct Column {
    const float* ptr;
    long long step;
  };
  __device__ __forceinline__ float operator()(long long t, int c) const {
    if constexpr (STAR)
      if (c == C) return star[t];
    return base[t * pitch_t + c];
  }
  __device__ __forceinline__ Column column(int c) const {           // frame t of class c is ptr[t * step]
    if constexpr (STAR)
      if (c == C) return {star, 1};
    return {base + c, pitch_t};
  }
};
template <bool STAR, class P>
__device__ __forceinline__ LatticeEmit<STAR> lattice_emit(const P& p, int u) {
  LatticeEmit<STAR> e{p.logp + (long long)u * p.pitch_b, nullptr, p.pitch_t, p.C};
  if constexpr (STAR) e.star = p.star + (long long)u * p.star_pitch;
  return e;
}

// g = A + B - q - total of the posterior kernels, clamped to [-2^30, 0]
__device__ __forceinline__ int lattice_post_clamp(long long a, long long b, long long q, long long tot) {
  const long long g = a + b - q - tot;
  return (int)(g < LATTICE_GFLOOR ? LATTICE_GFLOOR : (g > 0 ? 0 : g));
}

// the launch ladders: f(std::integral_constant<int, NS>) for the smallest NS of 1 / 2 / 4 / 8 / 17 whose NS * 256 holds `states`
// (17 holds the longest target: the caller asserts it), and for the NS of 1 / 4 / 17 with NS * 256 == band_states
template <class F>
static inline void lattice_dispatch_ns(int states, F f) {
  if (states <= 1 * LATTICE_NT) f(std::integral_constant<int, 1>{});
  else if (states <= 2 * LATTICE_NT) f(std::integral_constant<int, 2>{});
  else if (states <= 4 * LATTICE_NT) f(std::integral_constant<int, 4>{});
  else if (states <= 8 * LATTICE_NT) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 17>{});
}
template <class F>
static inline int lattice_dispatch_band_ns(int band_states, F f) {
  if (band_states == 1 * LATTICE_NT) f(std::integral_constant<int, 1>{});
  else if (band_states == 4 * LATTICE_NT) f(std::integral_constant<int, 4>{});
  else if (band_states == 17 * LATTICE_NT) f(std::integral_constant<int, 17>{});
  else return QASR_ERR_ARG;
  return QASR_OK;
}

}  // namespace qasr
