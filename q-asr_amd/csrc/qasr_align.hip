// CTC forced alignment and transcript scoring in fixed point (k_align); the host statement is qasr/align.py (RULES), and this
// file follows it bit for bit.  Scores are int64 sums of q = rint(logp * 2^16) as in qasr_beam.hip; the forward pass adds with
// the caller's log-add-exp table (LDS resident), so the kernel calls neither exp nor log.
//
// k_align<NS>: one work-group of 256 threads per problem (utterance p / K, target row p), sequential over frames.  Thread tid
// owns the states tid, tid + 256, ... (NS of them at most; NS is chosen from the row pitch of the targets, so a short-pitch
// call pays neither the registers nor the LDS of the 4097-state case).  A state's label and its "may skip the blank" bit
// stay in registers; the only global reads of a frame are the gathers logp[u][t][lab(s)], and frame t + 1's are issued
// before frame t's arithmetic, so the serial chain per frame is: 3 LDS reads, compare / add, 1 LDS write, 1 barrier (the
// row is double-buffered).
// Two passes over the same two int64 rows, one after the other in ONE launch: Viterbi first, then - only when `total` is
// requested - forward.  Both at once would need four rows: 4 x 4352 x 8 B = 136 KB plus the 32 KB table is past a work-
// group's 160 KB; one pair is 68 KB + 32 KB + 2 KB at NS = 17 and 4 KB + 32 KB + 2 KB at NS = 1.
// Backpointers: 2 bits per (frame, state), four frames of one state to a byte (a thread collects its states' steps in
// registers and stores one byte per state every fourth frame; consecutive threads store consecutive bytes) in the
// caller's workspace: P x ceil(T / 4) x pitch bytes, pitch = 2 * max_labels + 1 rounded up to 4.
// Back-walk: the path moves by at most 2 states per frame, so 64 frames (16 byte rows) need a window of 129 states.  All
// threads copy that window into LDS (one global round trip per 64 frames), thread 0 walks it there and leaves, per label,
// its first frame and frame count in LDS; then one thread per label takes the maximum of its frames' log-probabilities.
// k_align<NS, STAR>: with STAR the label id C is the wildcard of STAR_RULES (qasr/align.py): wherever a state's or a label's
// log-probability is gathered, c == C reads star[u][t] in place of logp[u][t][c], and the target check accepts c == C.  The
// STAR = false instantiations take the kernel argument they always took (AlignP) and are the code they were.
// LDS atomics: none.  Global memory sees plain vector stores.  Every loop is bounded by T, the number of states, the row
// pitch or a constant; nothing is allocated and no length is read on the host.
// The arithmetic (FX_NEG, fx_quantize, fx_lae, fx_key) is qasr_fixed_dev.h's; the target check, a state's label and skip rule,
// the emission read, the back-walk's window constants and the launch ladder are qasr_lattice_dev.h's.  The back-walk itself is
// this file's text and k_align_band's: one function for both measured 2 to 3 % slower here at 250 frames.
#include <climits>

#include "qasr_lattice_dev.h"

namespace qasr {

struct AlignP {
  const float* logp;
  const int32_t* lens;          // optional [B]
  const int32_t* targets;       // [P][ML]
  const int32_t* target_lens;   // [P]
  const uint16_t* tab;          // [FX_TAB], with total
  unsigned char* ws;            // [P][G4][pitch_s]
  int32_t* start;               // [P][ML] optional
  int32_t* nframes;             // [P][ML] optional
  float* score;                 // [P][ML] optional
  long long* path_score;        // [P] optional
  long long* total;             // [P] optional
  int32_t* ok;                  // [P]
  long long pitch_b, pitch_t;
  int T, C, K, blank, ML, pitch_s, G4;
};

struct AlignPS : AlignP {       // k_align<NS, true>'s argument
  const float* star;            // [B][star_pitch]
  long long star_pitch;
};

static int align_pitch(int max_labels) { return (2 * max_labels + 1 + 3) & ~3; }

size_t align_workspace_bytes(int P, int T, int max_labels) {
  return (size_t)P * (size_t)((T + 3) / 4) * (size_t)align_pitch(max_labels);
}

template <int NS, bool STAR>
__global__ void __launch_bounds__(LATTICE_NT) k_align(std::conditional_t<STAR, AlignPS, AlignP> p) {
  __shared__ long long rows[2][NS * LATTICE_NT];
  __shared__ uint16_t tab[FX_TAB];
  __shared__ unsigned char win[LATTICE_G * LATTICE_WINW];
  __shared__ int sh_bad, sh_s, sh_t;
  const int tid = threadIdx.x, pr = blockIdx.x, u = pr / p.K;
  const int T = p.T, C = p.C, blank = p.blank, ML = p.ML;
  const int lim = p.lens ? min(max(p.lens[u], 0), T) : T;
  const int L = p.target_lens[pr];
  const int32_t* const y = p.targets + (size_t)pr * ML;
  const bool want_total = p.total != nullptr;
  int32_t* const o_start = p.start ? p.start + (size_t)pr * ML : nullptr;
  int32_t* const o_nframes = p.nframes ? p.nframes + (size_t)pr * ML : nullptr;
  float* const o_score = p.score ? p.score + (size_t)pr * ML : nullptr;

  if (tid == 0) sh_bad = 0;
  if (want_total)
    for (int i = tid; i < FX_TAB; i += LATTICE_NT) tab[i] = p.tab[i];
  __syncthreads();
  // the target is device data: its length and every label are checked here, before anything is read through them
  const bool len_ok = L >= 0 && L <= ML && L <= QASR_ALIGN_MAX_LABELS && 2 * L + 1 <= NS * LATTICE_NT;
  if (len_ok && lattice_check_target<STAR>(y, L, C, blank, tid, LATTICE_NT)) sh_bad = 1;
  __syncthreads();
  bool alignable = len_ok && !sh_bad && !(lim == 0 && L > 0);
  const int S = alignable ? 2 * L + 1 : 0;

  int lab[NS];
  bool skp[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT;
    lab[k] = blank, skp[k] = false;
    if (s < S && (s & 1)) {
      const LatticeSlot sl = lattice_slot(y, s, S);
      lab[k] = sl.label, skp[k] = sl.skip_fwd;
    }
  }
  unsigned char* const wsp = p.ws + (size_t)pr * (size_t)p.G4 * (size_t)p.pitch_s;
  const size_t pitch_s = (size_t)p.pitch_s;
  const LatticeEmit<STAR> emit = lattice_emit<STAR>(p, u);          // logp[u][t][c], the wildcard's plane where c == C

  // one pass over the frames (vit: Viterbi with backpointers, else forward); returns the row that holds frame lim - 1
  auto run = [&](auto vit_tag) -> int {
    constexpr bool VIT = decltype(vit_tag)::value;
    float pf[NS];
    unsigned acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * LATTICE_NT;
      acc[k] = 0;
      pf[k] = s < S ? emit(0, lab[k]) : 0.f;                        // frame 0 (lim >= 1 here)
      if (s < S) rows[0][s] = s < 2 ? fx_quantize(pf[k]) : FX_NEG;
      pf[k] = (s < S && lim > 1) ? emit(1, lab[k]) : 0.f;
    }
    int cur = 0;
    __syncthreads();
    for (int t = 1; t < lim; ++t) {
      float nx[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) {                                // frame t + 1's gathers, in flight across this frame
        const int s = tid + k * LATTICE_NT;
        nx[k] = (s < S && t + 1 < lim) ? emit(t + 1, lab[k]) : 0.f;
      }
      const long long* const R = rows[cur];
      long long* const W = rows[cur ^ 1];
      const bool flush = (t & 3) == 3 || t == lim - 1;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int s = tid + k * LATTICE_NT;
        if (s < S) {
          const long long q = fx_quantize(pf[k]);
          const long long a0 = R[s], a1 = s >= 1 ? R[s - 1] : FX_NEG, a2 = skp[k] ? R[s - 2] : FX_NEG;
          if constexpr (VIT) {
            long long best = a0;
            unsigned step = 0;
            if (a1 > best) best = a1, step = 1;
            if (a2 > best) best = a2, step = 2;
            W[s] = best == FX_NEG ? FX_NEG : best + q;
            acc[k] |= step << (2 * (t & 3));
            if (flush) {
              wsp[(size_t)(t >> 2) * pitch_s + s] = (unsigned char)acc[k];      // t >> 2 < G4, s < S <= pitch_s
              acc[k] = 0;
            }
          } else {
            const long long x = fx_lae(fx_lae(a0, a1, tab), a2, tab);
            W[s] = x == FX_NEG ? FX_NEG : x + q;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < NS; ++k) pf[k] = nx[k];
      cur ^= 1;
      __syncthreads();
    }
    return cur;
  };

  // ---- Viterbi
  long long vf = FX_NEG;
  int fin = 0;
  if (alignable) {
    if (lim == 0) {
      vf = 0;                                                       // L == 0: the empty path
    } else {
      const int cur = run(std::true_type{});
      const long long* const R = rows[cur];
      if (L == 0) {
        vf = R[0];
      } else {
        const long long a = R[2 * L], b = R[2 * L - 1];
        fin = a > b ? 2 * L : 2 * L - 1;
        vf = a > b ? a : b;
      }
    }
    alignable = vf != FX_NEG;
  }
  __syncthreads();                                                  // the rows have been read: their LDS is reused below
  if (!alignable) {                                                 // uniform
    for (int i = tid; i < ML; i += LATTICE_NT) {
      if (o_start) o_start[i] = 0;
      if (o_nframes) o_nframes[i] = 0;
      if (o_score) o_score[i] = 0.f;
    }
    if (tid == 0) {
      if (p.path_score) p.path_score[pr] = FX_NEG;
      if (p.total) p.total[pr] = FX_NEG;
      p.ok[pr] = 0;
    }
    return;
  }
  // ---- back-walk: per label its first frame and frame count (L <= NS * 128 - 1: both arrays fit rows[0])
  int* const lstart = reinterpret_cast<int*>(&rows[0][0]);
  int* const lcnt = lstart + NS * (LATTICE_NT / 2);
  if (L > 0) {                                                      // (then lim > 0)
    for (int i = tid; i < L; i += LATTICE_NT) lstart[i] = 0, lcnt[i] = 0;
    if (tid == 0) sh_s = fin, sh_t = lim - 1;
    __syncthreads();
    int cur_i = -1, cnt = 0, first = 0;                             // thread 0: the label run being walked
    for (int guard = 0; guard <= p.G4; ++guard) {                   // bounded: every window consumes at least one byte row
      const int s_hi = sh_s, t_hi = sh_t;
      if (t_hi < 0) break;                                          // uniform
      const int g_top = t_hi >> 2, g_lo = max(g_top - LATTICE_G + 1, 0), ng = g_top - g_lo + 1;
      const int lo = max(s_hi - 8 * LATTICE_G, 0), width = s_hi - lo + 1;        // <= 8 G + 1 states, all < S
      for (int i = tid; i < ng * LATTICE_WINW; i += LATTICE_NT) {
        const int gi = i / LATTICE_WINW, si = i - gi * LATTICE_WINW;
        if (si < width) win[i] = wsp[(size_t)(g_lo + gi) * pitch_s + lo + si];
      }
      __syncthreads();
      if (tid == 0) {
        int s = s_hi;
        for (int t = t_hi; t >= 4 * g_lo; --t) {
          if (s & 1) {
            const int i = s >> 1;
            if (i != cur_i) {
              if (cur_i >= 0) lstart[cur_i] = first, lcnt[cur_i] = cnt;
              cur_i = i, cnt = 0;
            }
            ++cnt, first = t;
          }
          if (t > 0) {
            const int at = min(max(s - lo, 0), LATTICE_WINW - 1);
            const int step = (win[((t >> 2) - g_lo) * LATTICE_WINW + at] >> (2 * (t & 3))) & 3;
            s = max(s - step, 0);
          }
        }
        sh_s = s, sh_t = 4 * g_lo - 1;
      }
      __syncthreads();
    }
    if (tid == 0 && cur_i >= 0) lstart[cur_i] = first, lcnt[cur_i] = cnt;
    __syncthreads();
  }
  // ---- outputs: one thread per label; the score is the largest log-probability of the label inside its run
  for (int i = tid; i < ML; i += LATTICE_NT) {
    int st = 0, n = 0;
    float sc = 0.f;
    if (i < L) {
      st = min(max(lstart[i], 0), lim - 1), n = min(max(lcnt[i], 0), lim - st);
      if (o_score && n > 0) {
        const auto col = emit.column(y[i]);
        int best = INT_MIN;
        for (int f = 0; f < n; ++f) {
          const int key = fx_key(__float_as_int(col.ptr[(long long)(st + f) * col.step]));
          best = key > best ? key : best;
        }
        sc = __int_as_float(fx_key(best));
      }
    }
    if (o_start) o_start[i] = st;
    if (o_nframes) o_nframes[i] = n;
    if (o_score) o_score[i] = sc;
  }
  if (tid == 0) {
    if (p.path_score) p.path_score[pr] = vf;
    p.ok[pr] = 1;
  }
  // ---- forward
  if (want_total) {
    long long tot = 0;                                              // lim == 0 (and L == 0)
    if (lim > 0) {
      __syncthreads();                                              // lstart / lcnt have been read
      const int cur = run(std::false_type{});
      const long long* const R = rows[cur];
      tot = L == 0 ? R[0] : fx_lae(R[2 * L], R[2 * L - 1], tab);
    }
    if (tid == 0) p.total[pr] = tot;
  }
}

template <bool STAR>
static void launch_align_ns(hipStream_t s, const std::conditional_t<STAR, AlignPS, AlignP>& p, int P, int states) {
  static_assert(2 * QASR_ALIGN_MAX_LABELS + 1 <= 17 * LATTICE_NT, "k_align<17> holds the longest target");
  lattice_dispatch_ns(states, [&](auto ns) {
    hipLaunchKernelGGL((k_align<decltype(ns)::value, STAR>), dim3((unsigned)P), dim3(LATTICE_NT), 0, s, p);
  });
}

int launch_align(hipStream_t s, const qasr_ctc_align_args& a) {
  AlignPS p{};
  p.logp = a.log_probs, p.lens = a.lens, p.targets = a.targets, p.target_lens = a.target_lens, p.tab = a.lae_table;
  p.ws = (unsigned char*)a.workspace;
  p.start = a.start, p.nframes = a.nframes, p.score = a.score;
  p.path_score = (long long*)a.path_score, p.total = (long long*)a.total, p.ok = a.ok;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame;
  p.T = a.T, p.C = a.C, p.K = a.K, p.blank = a.blank, p.ML = a.max_labels;
  p.pitch_s = align_pitch(a.max_labels), p.G4 = (a.T + 3) / 4;
  p.star = a.star_logp, p.star_pitch = a.star_pitch;
  const int states = 2 * a.max_labels + 1;                          // <= 4097
  if (a.star_logp) launch_align_ns<true>(s, p, a.P, states);
  else launch_align_ns<false>(s, static_cast<const AlignP&>(p), a.P, states);
  return QASR_OK;
}

}  // namespace qasr
