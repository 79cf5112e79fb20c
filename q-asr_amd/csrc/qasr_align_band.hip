// Banded CTC alignment of one long recording against its whole transcript (k_align_band); the host statement is BAND_RULES and
// align_band_host of qasr/align.py, and this file follows it bit for bit.  The per-frame step is k_align's (qasr_align.hip):
// int64 sums of q = rint(logp * 2^16), Viterbi only.
//
// k_align_band<NS>: one work-group of 256 threads per recording, sequential over frames.  The band holds BW = 256 * NS states
// [base, base + BW); V is two int64 rows of BW entries in LDS (double-buffered: one barrier per frame).  Ownership is circular:
// state s lives in thread s % 256, slot (s >> 8) % NS, LDS index s % BW - so a slot's LDS index never changes, and when the base
// moves, state s + BW takes the place of the dropped state s: nothing rotates, the owning thread reloads that slot's label and
// skip bit and writes NEG.  The slot loops are unrolled and predicated, so the per-slot arrays stay in registers.
// s - 1 and s - 2 wrap in the circular row: "a predecessor below base is NEG" is tested on the state number, not on the index.
// Every 32 frames the band is re-centred on the lowest state that holds the row's maximum: a wave reduction, four partial
// results through LDS, two barriers.  The gathers logp[t + 1][lab(s)] are in flight across frame t as in k_align; a slot that
// was replaced by a move gathers its frame again with the new label.
// Backpointers: 2 bits at (t, s % BW), four frames to a byte; 32 is a multiple of 4, so the four frames of a byte share a base.
// Back-walk: k_align's 64-frame LDS window with wrapped indices; thread 0 walks it and the state of every frame goes to the
// workspace.  Then one thread per frame: frame_logp, and at the first frame of a label's run its start, count and best score.
// Workspace per problem: ceil(T / 4) * BW bytes of backpointers, then T int32 states.
// k_align_band<NS, STAR>: with STAR the label id C is the wildcard of STAR_RULES (qasr/align.py): wherever a state's or a label's
// log-probability is gathered, c == C reads star[p][t] in place of logp[p][t][c], and the target check accepts c == C.  The
// STAR = false instantiations take the kernel argument they always took (BandP) and are the code they were.
// LDS atomics: none.  Global memory sees plain vector stores.  Every loop is bounded by T, L, the row pitch or a constant; nothing
// is allocated and no length is read on the host.
// The arithmetic (FX_NEG, fx_quantize, fx_key) is qasr_fixed_dev.h's; LATTICE_BLOCK (the 32 frames between two moves, shared with
// k_post_band), the target check, a state's label and skip rule, the emission read, the back-walk's window constants and the
// launch ladder are qasr_lattice_dev.h's.
#include <climits>

#include "qasr_lattice_dev.h"

namespace qasr {

#define BAND_SKIP ((int)0x80000000)             /* bit 31 of a slot's label word: the state may skip the blank below it */

struct BandP {
  const float* logp;
  const int32_t* lens;          // optional [P]
  const int32_t* targets;       // [P][ML]
  const int32_t* target_lens;   // [P]
  unsigned char* ws;            // [P][G4 * BW + 4 T]
  int32_t* start;               // [P][ML] optional
  int32_t* nframes;             // [P][ML] optional
  float* score;                 // [P][ML] optional
  long long* path_score;        // [P] optional
  float* frame_logp;            // [P][T] optional
  int32_t* band_base;           // [P][NB] optional
  int32_t* ok;                  // [P]
  long long pitch_b, pitch_t;
  int T, C, blank, ML, G4, NB;
};

struct BandPS : BandP {         // k_align_band<NS, true>'s argument
  const float* star;            // [P][star_pitch]
  long long star_pitch;
};

static size_t band_problem_bytes(int T, int band_states) {
  return (size_t)((T + 3) / 4) * (size_t)band_states + 4 * (size_t)T;
}

size_t align_band_workspace_bytes(int P, int T, int band_states) { return (size_t)P * band_problem_bytes(T, band_states); }

template <int NS, bool STAR>
__global__ void __launch_bounds__(LATTICE_NT) k_align_band(std::conditional_t<STAR, BandPS, BandP> p) {
  constexpr int BW = NS * LATTICE_NT;
  __shared__ long long rows[2][BW];
  __shared__ unsigned char win[LATTICE_G * LATTICE_WINW];
  __shared__ int wstate[4 * LATTICE_G];
  __shared__ long long red_v[LATTICE_NT / 64];
  __shared__ int red_s[LATTICE_NT / 64];
  __shared__ int sh_bad, sh_s, sh_t;
  const int tid = threadIdx.x, pr = blockIdx.x;
  const int T = p.T, C = p.C, blank = p.blank, ML = p.ML;
  const int lim = p.lens ? min(max(p.lens[pr], 0), T) : T;
  const int L = p.target_lens[pr];
  const int32_t* const y = p.targets + (size_t)pr * ML;
  int32_t* const o_start = p.start ? p.start + (size_t)pr * ML : nullptr;
  int32_t* const o_nframes = p.nframes ? p.nframes + (size_t)pr * ML : nullptr;
  float* const o_score = p.score ? p.score + (size_t)pr * ML : nullptr;
  float* const o_flp = p.frame_logp ? p.frame_logp + (size_t)pr * T : nullptr;
  int32_t* const o_base = p.band_base ? p.band_base + (size_t)pr * p.NB : nullptr;

  if (tid == 0) sh_bad = 0;
  __syncthreads();
  // the target is device data: its length and every label are checked here, before anything is read through them
  const bool len_ok = L >= 0 && L <= ML && L <= QASR_BAND_MAX_LABELS;
  if (len_ok && lattice_check_target<STAR>(y, L, C, blank, tid, LATTICE_NT)) sh_bad = 1;
  __syncthreads();
  bool alignable = len_ok && !sh_bad && !(lim == 0 && L > 0);
  const int S = alignable ? 2 * L + 1 : 0;
  const int top = max(0, S - BW);
  const int nblk = alignable ? (lim + LATTICE_BLOCK - 1) / LATTICE_BLOCK : 0;  // blocks that have a frame < lim

  unsigned char* const wsp = p.ws + (size_t)pr * ((size_t)p.G4 * BW + 4 * (size_t)T);
  int* const wst = reinterpret_cast<int*>(wsp + (size_t)p.G4 * BW);       // the path's state per frame (G4 * BW is a multiple of 4)
  const LatticeEmit<STAR> emit = lattice_emit<STAR>(p, pr);         // logp[pr][t][c], the wildcard's plane where c == C

  // ---- Viterbi inside the band
  // a slot's label word: the odd state s < S carries y[s >> 1], bit 31 says that it may skip the blank below it
  auto label_word = [&](int s) -> int {
    const LatticeSlot sl = lattice_slot(y, s, S);
    return sl.skip_fwd ? sl.label | BAND_SKIP : sl.label;
  };
  long long vf = FX_NEG;
  int fin = 0;
  if (alignable && lim == 0) vf = 0;                                // L == 0: the empty path
  if (alignable && lim > 0) {
    int st[NS], lab[NS];                                            // the slot's state; its label, "may skip the blank" in bit 31
    float pf[NS];
    unsigned acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * LATTICE_NT;                           // base 0
      st[k] = s, lab[k] = (s < S && (s & 1)) ? label_word(s) : blank, acc[k] = 0;
      pf[k] = s < S ? emit(0, lab[k] & ~BAND_SKIP) : 0.f;           // frame 0
      rows[0][s] = (s < S && s < 2) ? fx_quantize(pf[k]) : FX_NEG;
      pf[k] = (s < S && lim > 1) ? emit(1, lab[k] & ~BAND_SKIP) : 0.f;
    }
    if (tid == 0 && o_base) o_base[0] = 0;
    int cur = 0, base = 0;
    __syncthreads();
    for (int t = 1; t < lim; ++t) {
      if ((t & (LATTICE_BLOCK - 1)) == 0) {                         // uniform: where should the band be?
        if (top > 0) {                                              // (S <= BW: the base never moves)
          const long long* const R = rows[cur];
          long long bv = FX_NEG;
          int bs = INT_MAX;
#pragma unroll
          for (int k = 0; k < NS; ++k) {                            // (top > 0: every slot holds a state < S)
            const long long v = R[tid + k * LATTICE_NT];
            if (v > bv || (v == bv && st[k] < bs)) bv = v, bs = st[k];
          }
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
            const long long ov = __shfl_xor(bv, o);
            const int os = __shfl_xor(bs, o);
            if (ov > bv || (ov == bv && os < bs)) bv = ov, bs = os;
          }
          if ((tid & 63) == 0) red_v[tid >> 6] = bv, red_s[tid >> 6] = bs;
          __syncthreads();
          bv = red_v[0], bs = red_s[0];
#pragma unroll
          for (int w = 1; w < LATTICE_NT / 64; ++w)
            if (red_v[w] > bv || (red_v[w] == bv && red_s[w] < bs)) bv = red_v[w], bs = red_s[w];
          if (bv != FX_NEG) {
            const int nb = max(base, min(bs - BW / 2, top));        // nb - base < BW / 2: a slot is replaced at most once
            if (nb > base) {
              long long* const Rw = rows[cur];
#pragma unroll
              for (int k = 0; k < NS; ++k)
                if (st[k] < nb) {                                   // dropped: state st + BW enters (nb + BW <= S)
                  const int s = st[k] + BW;
                  st[k] = s, lab[k] = (s & 1) ? label_word(s) : blank;
                  Rw[tid + k * LATTICE_NT] = FX_NEG;
                  pf[k] = emit(t, lab[k] & ~BAND_SKIP);             // this frame again, with the new label
                }
              base = nb;
            }
          }
          __syncthreads();                                          // the NEGs are in place; red_* may be rewritten
        }
        if (tid == 0 && o_base) o_base[t >> 5] = base;
      }
      float nx[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k)                                  // frame t + 1's gathers, in flight across this frame
        nx[k] = (st[k] < S && t + 1 < lim) ? emit(t + 1, lab[k] & ~BAND_SKIP) : 0.f;
      const long long* const R = rows[cur];
      long long* const W = rows[cur ^ 1];
      const bool flush = (t & 3) == 3 || t == lim - 1;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int i0 = tid + k * LATTICE_NT;                        // s % BW
        const int s = st[k];
        if (s < S) {
          const int i1 = i0 >= 1 ? i0 - 1 : i0 - 1 + BW, i2 = i0 >= 2 ? i0 - 2 : i0 - 2 + BW;
          const long long q = fx_quantize(pf[k]);
          const long long a0 = R[i0], a1 = s - 1 >= base ? R[i1] : FX_NEG, a2 = (lab[k] < 0 && s - 2 >= base) ? R[i2] : FX_NEG;
          long long best = a0;
          unsigned step = 0;
          if (a1 > best) best = a1, step = 1;
          if (a2 > best) best = a2, step = 2;
          W[i0] = best == FX_NEG ? FX_NEG : best + q;
          acc[k] |= step << (2 * (t & 3));
          if (flush) {
            wsp[(size_t)(t >> 2) * BW + i0] = (unsigned char)acc[k];      // t >> 2 < G4, i0 < BW
            acc[k] = 0;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) pf[k] = nx[k];
      cur ^= 1;
      __syncthreads();
    }
    const long long* const R = rows[cur];
    if (L == 0) {
      vf = R[0];
    } else {                                                        // an end state outside the last band is NEG
      const int s2 = 2 * L, s1 = 2 * L - 1;
      const long long a = (s2 >= base && s2 < base + BW) ? R[s2 % BW] : FX_NEG;
      const long long b = (s1 >= base && s1 < base + BW) ? R[s1 % BW] : FX_NEG;
      fin = a > b ? s2 : s1;
      vf = a > b ? a : b;
    }
  }
  for (int i = nblk + tid; i < p.NB; i += LATTICE_NT)
    if (o_base) o_base[i] = 0;
  alignable = alignable && vf != FX_NEG;
  __syncthreads();
  if (!alignable) {                                                 // uniform
    for (int i = tid; i < ML; i += LATTICE_NT) {
      if (o_start) o_start[i] = 0;
      if (o_nframes) o_nframes[i] = 0;
      if (o_score) o_score[i] = 0.f;
    }
    if (o_flp)
      for (int t = tid; t < T; t += LATTICE_NT) o_flp[t] = 0.f;
    if (tid == 0) {
      if (p.path_score) p.path_score[pr] = FX_NEG;
      p.ok[pr] = 0;
    }
    return;
  }
  // ---- back-walk: the state of every frame < lim goes to wst
  if (lim > 0) {
    if (tid == 0) sh_s = fin, sh_t = lim - 1;
    __syncthreads();
    for (int guard = 0; guard <= p.G4; ++guard) {                   // bounded: every window consumes at least one byte row
      const int s_hi = sh_s, t_hi = sh_t;
      if (t_hi < 0) break;                                          // uniform
      const int g_top = t_hi >> 2, g_lo = max(g_top - LATTICE_G + 1, 0), ng = g_top - g_lo + 1;
      const int lo = max(s_hi - 8 * LATTICE_G, 0), width = s_hi - lo + 1;        // <= 8 G + 1 states
      for (int i = tid; i < ng * LATTICE_WINW; i += LATTICE_NT) {
        const int gi = i / LATTICE_WINW, si = i - gi * LATTICE_WINW;
        if (si < width) win[i] = wsp[(size_t)(g_lo + gi) * BW + (lo + si) % BW];
      }
      __syncthreads();
      if (tid == 0) {
        int s = s_hi;
        for (int t = t_hi; t >= 4 * g_lo; --t) {
          wstate[t - 4 * g_lo] = s;                                 // t - 4 g_lo < 4 G
          if (t > 0) {
            const int at = min(max(s - lo, 0), LATTICE_WINW - 1);
            const int step = (win[((t >> 2) - g_lo) * LATTICE_WINW + at] >> (2 * (t & 3))) & 3;
            s = max(s - step, 0);
          }
        }
        sh_s = s, sh_t = 4 * g_lo - 1;
      }
      __syncthreads();
      if (tid <= t_hi - 4 * g_lo) wst[4 * g_lo + tid] = wstate[tid];           // 4 g_lo + tid <= t_hi < lim <= T
      __syncthreads();                                              // wstate, win, sh_s and sh_t have been read
    }
  }
  // ---- outputs: one thread per frame; the first frame of a label's run writes the label's row entries
  for (int i = L + tid; i < ML; i += LATTICE_NT) {                  // the tails (every label < L has exactly one run)
    if (o_start) o_start[i] = 0;
    if (o_nframes) o_nframes[i] = 0;
    if (o_score) o_score[i] = 0.f;
  }
  for (int t = tid; t < T; t += LATTICE_NT) {
    if (t >= lim) {
      if (o_flp) o_flp[t] = 0.f;
      continue;
    }
    const int s = min(max(wst[t], 0), S - 1);
    const int i = s >> 1;                                           // (odd s: i < L)
    const int c = (s & 1) ? y[i] : blank;
    const auto col = emit.column(c);
    if (o_flp) o_flp[t] = col.ptr[(long long)t * col.step];
    if ((s & 1) && (t == 0 || wst[t - 1] != s)) {
      int n = 0, best = INT_MIN;
      for (int f = t; f < lim && wst[f] == s; ++f) {
        ++n;
        if (o_score) {
          const int key = fx_key(__float_as_int(col.ptr[(long long)f * col.step]));
          best = key > best ? key : best;
        }
      }
      if (o_start) o_start[i] = t;
      if (o_nframes) o_nframes[i] = n;
      if (o_score) o_score[i] = __int_as_float(fx_key(best));
    }
  }
  if (tid == 0) {
    if (p.path_score) p.path_score[pr] = vf;
    p.ok[pr] = 1;
  }
}

template <bool STAR>
static int launch_align_band_ns(hipStream_t s, const std::conditional_t<STAR, BandPS, BandP>& p, int B, int band_states) {
  return lattice_dispatch_band_ns(band_states, [&](auto ns) {
    hipLaunchKernelGGL((k_align_band<decltype(ns)::value, STAR>), dim3((unsigned)B), dim3(LATTICE_NT), 0, s, p);
  });
}

int launch_align_band(hipStream_t s, const qasr_ctc_align_band_args& a) {
  BandPS p{};
  p.logp = a.log_probs, p.lens = a.lens, p.targets = a.targets, p.target_lens = a.target_lens;
  p.ws = (unsigned char*)a.workspace;
  p.start = a.start, p.nframes = a.nframes, p.score = a.score;
  p.path_score = (long long*)a.path_score, p.frame_logp = a.frame_logp, p.band_base = a.band_base, p.ok = a.ok;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame;
  p.T = a.T, p.C = a.C, p.blank = a.blank, p.ML = a.max_labels;
  p.G4 = (a.T + 3) / 4, p.NB = (a.T + LATTICE_BLOCK - 1) / LATTICE_BLOCK;
  p.star = a.star_logp, p.star_pitch = a.star_pitch;
  if (a.star_logp) return launch_align_band_ns<true>(s, p, a.B, a.band_states);
  return launch_align_band_ns<false>(s, static_cast<const BandP&>(p), a.B, a.band_states);
}

}  // namespace qasr
