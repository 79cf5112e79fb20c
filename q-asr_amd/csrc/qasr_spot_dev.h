// k_spot's frame step (qasr_spot.hip) as functions, for k_stream_spot (qasr_stream_spot.hip): a lane's labels and skip bits, the
// frame step of SPOT_RULES (qasr/spot.py) on a row that lives in registers, and the candidate / overlap rule on one open hit.
// k_spot itself keeps its own loop: built from these functions its NS = 1 instantiation measured 4.7 % slower.
// A change to the rule goes into both files; the twins pin each kernel on every byte.
// One WAVE per problem; lane l owns the NS contiguous states l * NS .. l * NS + NS - 1 (NS = 1, 2, 4: 2 ML + 1 <= 64 / 128 / 256).
// Per frame a lane needs two pairs from below itself: states l * NS - 1 and l * NS - 2, that is the top two states of lane l - 1
// (NS >= 2) or the states of lanes l - 1 and l - 2 (NS = 1); they cross lanes with __shfl_up, everything else is in the lane's
// own registers.  No LDS, no barrier, no memory access in here but spot_slots' reads of a checked target.
#pragma once

#include "qasr_lattice_dev.h"

namespace qasr {

#define SPOT_NT 256
#define SPOT_WAVE 64
#define SPOT_WAVES (SPOT_NT / SPOT_WAVE)

// the labels and "may skip the blank" bits of a lane's states; y is checked, S = 2L: states s >= S and even states carry the blank
template <int NS>
__device__ __forceinline__ void spot_slots(const int32_t* y, int S, int blank, int lane, int (&lab)[NS], bool (&skp)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k;
    lab[k] = blank, skp[k] = false;
    if (s < S && (s & 1)) {                                         // s >> 1 < L
      const LatticeSlot sl = lattice_slot(y, s, S);
      lab[k] = sl.label, skp[k] = sl.skip_fwd;
    }
  }
}

// frame t: the row (D, st) of the lane's states is replaced by the next one; pf: the frame's log-probabilities of the lane's
// labels, ps: the plane's value; t is the start that the fresh start hands to state 1.  (fd, fs) is the pair of the state at
// index f_k of this lane, meaningful in the lane that owns F.
template <int NS>
__device__ __forceinline__ void spot_frame(long long (&D)[NS], int (&st)[NS], const bool (&skp)[NS], const float (&pf)[NS], float ps,
                                           int lane, int t, int f_k, long long& fd, int& fs) {
  // the two pairs below this lane's states: b1 = state lane * NS - 1, b2 = state lane * NS - 2 (NEG below state 0)
  long long b1d = __shfl_up(D[NS - 1], 1), b2d = NS >= 2 ? __shfl_up(D[NS >= 2 ? NS - 2 : 0], 1) : __shfl_up(D[0], 2);
  int b1s = __shfl_up(st[NS - 1], 1), b2s = NS >= 2 ? __shfl_up(st[NS >= 2 ? NS - 2 : 0], 1) : __shfl_up(st[0], 2);
  if (lane < 1) b1d = FX_NEG, b1s = -1;
  if (lane < (NS >= 2 ? 1 : 2)) b2d = FX_NEG, b2s = -1;
  const long long qs = fx_quantize(ps);
  long long nd[NS];
  int nst[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k;
    long long e = fx_quantize(pf[k]) - qs;
    e = e < 0 ? e : 0;
    long long a1 = k >= 1 ? D[k >= 1 ? k - 1 : 0] : b1d;
    int s1 = k >= 1 ? st[k >= 1 ? k - 1 : 0] : b1s;
    if (s == 1) a1 = 0, s1 = t;                                     // the fresh start
    long long a2 = k >= 2 ? D[k >= 2 ? k - 2 : 0] : (k == 1 ? b1d : b2d);
    int s2 = k >= 2 ? st[k >= 2 ? k - 2 : 0] : (k == 1 ? b1s : b2s);
    if (!skp[k]) a2 = FX_NEG;
    long long best = D[k];
    int bs = st[k];
    if (a1 > best) best = a1, bs = s1;
    if (a2 > best) best = a2, bs = s2;
    const bool live = best != FX_NEG && s >= 1;                     // (state 0 is not computed: it stays dead)
    nd[k] = live ? best + e : FX_NEG;
    nst[k] = live ? bs : -1;
  }
  fd = FX_NEG, fs = -1;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    D[k] = nd[k], st[k] = nst[k];
    if (k == f_k) fd = nd[k], fs = nst[k];
  }
}

// the one open hit of a problem, kept by the lane that owns F
struct SpotHit {
  bool open;
  int start, end;
  long long d;
};

// the candidate and overlap rule at frame t for F's pair (fd, fs), 0 <= fs <= t where F is live.  True when a candidate that does
// not overlap closed the open hit: `closed` is then that hit, to be emitted, and `h` the new one.
__device__ __forceinline__ bool spot_candidate(SpotHit& h, long long fd, int fs, int t, long long thr, int max_span, SpotHit& closed) {
  if (fd == FX_NEG) return false;
  const long long n = (long long)t - fs + 1;
  if (n > max_span || fd < thr * n) return false;                   // not a candidate
  if (h.open && fs <= h.end) {                                      // overlaps the open hit: the higher mean stays
    const long long n_open = (long long)h.end - h.start + 1;
    if (fd * n_open > h.d * n) h.start = fs, h.end = t, h.d = fd;
    return false;
  }
  const bool was = h.open;
  closed = h;
  h.open = true, h.start = fs, h.end = t, h.d = fd;
  return was;
}

}  // namespace qasr
