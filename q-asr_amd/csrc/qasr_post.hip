// CTC posteriors along a given alignment in fixed point (k_post): forward-backward over the lattice of k_align.  The host
// statement is qasr/align.py (POST_RULES, post_host), and this file follows it bit for bit.  Scores are int64 sums of
// q = rint(logp * 2^16); both passes add with the caller's log-add-exp table (LDS resident), so the kernel calls neither exp
// nor log.
//
// k_post<NS, STAR>: one work-group of 256 threads per problem (utterance p / K, target row p), sequential over frames.  The
// ownership is k_align's: thread tid owns the states tid, tid + 256, ... (NS of them at most, NS chosen from the row pitch of
// the targets).  Per state in registers: its label, the forward and the backward "may skip the blank" bits - kept as the LDS
// index of the third term, s - 2 / s + 2 or a slot that always holds NEG, so the frame step carries no lane mask per state
// (as bools they cost 562 spilled SGPRs at NS = 17, as indices 142) - and the interval
// [lo, hi) of frames in which the alignment (start / nframes) sits in that state - the intervals of a valid alignment tile
// [0, lim), so at every frame exactly one thread is "on the path".  Frame t +- 1's gathers are issued before frame t's
// arithmetic; the serial chain per frame is 3 LDS reads, two table look-ups, 1 LDS write, 1 barrier (the row is double-buffered).
// Two passes over the same two int64 rows in ONE launch:
//   forward,  t = 0 .. lim - 1: k_align's forward step; the on-path thread stores A(t, s_t) to the workspace fa[p][t] (one plain
//     8-byte store per frame); at the end total = lae(A[2L], A[2L - 1]).
//   backward, t = lim - 1 .. 0: the mirrored step over the successors s, s + 1, s + 2; the on-path thread loads fa[p][t] (issued
//     a frame ahead), forms g = A + Bk - q - total, clamps it to [-2^30, 0], stores frame_post[p][t] and keeps the minimum of
//     its run in a register: the owner of state 2i + 1 sees every frame of label i, so label_post needs no further pass.
// start / nframes / ok_in are device data.  Before anything else the work-group checks, one thread per label, that they describe
// a CTC alignment of the target over lim frames (in 64-bit sums: garbage cannot wrap); a bad row stores zeros and the whole
// group leaves together.  start / nframes are only ever compared with frame numbers, never used as an index.
// LDS: 2 x NS x 256 x 8 B of rows + 32 KB of table + a few words: 100 KB at NS = 17, 36 KB at NS = 1.  LDS atomics: none.
// Global memory sees plain vector stores.  Every loop is bounded by T, the number of states, the row pitch or a constant;
// nothing is allocated and no length is read on the host.
// The arithmetic (FX_NEG, fx_quantize, fx_lae) is qasr_fixed_dev.h's; the checks of the target and of start / nframes, a state's
// label and skip rules, the emission read, the clamp of g and the launch ladder are qasr_lattice_dev.h's, with their bounds.
#include "qasr_lattice_dev.h"

namespace qasr {

struct PostP {
  const float* logp;
  const int32_t* lens;          // optional [B]
  const int32_t* targets;       // [P][ML]
  const int32_t* target_lens;   // [P]
  const uint16_t* tab;          // [FX_TAB]
  const int32_t* start;         // [P][ML]
  const int32_t* nframes;       // [P][ML]
  const int32_t* ok_in;         // [P] optional
  long long* fa;                // [P][T]: the forward score along the path
  int32_t* frame_post;          // [P][post_pitch]
  int32_t* label_post;          // [P][ML]
  long long* total;             // [P] optional
  int32_t* ok;                  // [P]
  const float* star;            // [B][star_pitch], k_post<NS, true> only
  long long pitch_b, pitch_t, post_pitch, star_pitch;
  int T, C, K, blank, ML;
};

size_t post_workspace_bytes(int P, int T) { return (size_t)P * (size_t)T * sizeof(long long); }

template <int NS, bool STAR>
__global__ void __launch_bounds__(LATTICE_NT) k_post(PostP p) {
  __shared__ long long rows[2][NS * LATTICE_NT];
  __shared__ uint16_t tab[FX_TAB];
  __shared__ int sh_bad;
  const int tid = threadIdx.x, pr = blockIdx.x, u = pr / p.K;
  const int T = p.T, C = p.C, blank = p.blank, ML = p.ML;
  const int lim = p.lens ? min(max(p.lens[u], 0), T) : T;
  const int L = p.target_lens[pr];
  const int32_t* const y = p.targets + (size_t)pr * ML;
  const int32_t* const a_start = p.start + (size_t)pr * ML;
  const int32_t* const a_nframes = p.nframes + (size_t)pr * ML;
  int32_t* const o_frame = p.frame_post + (long long)pr * p.post_pitch;
  int32_t* const o_label = p.label_post + (size_t)pr * ML;
  long long* const fa = p.fa + (size_t)pr * (size_t)T;

  // a state that may not skip the blank reads this slot instead: 2L + 1 is odd and <= NS * 256, so no state lives here, nothing
  // but the next line writes it, and the frame step needs no mask per state for the third term
  constexpr int SENT = NS * LATTICE_NT - 1;
  if (tid == 0) sh_bad = 0, rows[0][SENT] = rows[1][SENT] = FX_NEG;
  for (int i = tid; i < FX_TAB; i += LATTICE_NT) tab[i] = p.tab[i];
  __syncthreads();
  // the target and the alignment are device data: lengths, labels and runs are checked here, before anything is read through them
  const bool len_ok = L >= 0 && L <= ML && L <= QASR_ALIGN_MAX_LABELS && 2 * L + 1 <= NS * LATTICE_NT;
  if (len_ok && (lattice_check_target<STAR>(y, L, C, blank, tid, LATTICE_NT) |
                 lattice_check_runs(y, a_start, a_nframes, L, lim, tid, LATTICE_NT)))
    sh_bad = 1;
  __syncthreads();
  const bool valid = len_ok && !sh_bad && !(p.ok_in && p.ok_in[pr] == 0) && !(lim == 0 && L > 0);
  if (!valid) {                                                     // uniform: sh_bad was read behind the barrier
    for (int i = tid; i < T; i += LATTICE_NT) o_frame[i] = 0;
    for (int i = tid; i < ML; i += LATTICE_NT) o_label[i] = 0;
    if (tid == 0) {
      if (p.total) p.total[pr] = FX_NEG;
      p.ok[pr] = 0;
    }
    return;
  }
  for (int i = lim + tid; i < T; i += LATTICE_NT) o_frame[i] = 0;   // behind lim
  for (int i = L + tid; i < ML; i += LATTICE_NT) o_label[i] = 0;    // the tails
  if (lim == 0) {                                                   // L == 0: the empty path
    if (tid == 0) {
      if (p.total) p.total[pr] = 0;
      p.ok[pr] = 1;
    }
    return;
  }
  const int S = 2 * L + 1;

  // a valid alignment: 0 <= start, start + nframes <= lim, so lo and hi below are frame numbers in 0 .. lim
  int lab[NS], lo[NS], hi[NS], lmin[NS];
  int i2f[NS], i2b[NS];                                             // where the third term lives: s - 2 / s + 2, or SENT
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT, i = s >> 1;
    lab[k] = blank, i2f[k] = i2b[k] = SENT, lo[k] = hi[k] = 0, lmin[k] = 0;
    if (s < S) {
      if (s & 1) {
        const LatticeSlot sl = lattice_slot(y, s, S);
        lab[k] = sl.label;
        if (sl.skip_fwd) i2f[k] = s - 2;
        if (sl.skip_bwd) i2b[k] = s + 2;
        lo[k] = a_start[i], hi[k] = a_start[i] + a_nframes[i];
      } else {
        lo[k] = i ? a_start[i - 1] + a_nframes[i - 1] : 0;
        hi[k] = i < L ? a_start[i] : lim;
      }
    }
  }
  const LatticeEmit<STAR> emit = lattice_emit<STAR>(p, u);          // logp[u][t][c], the wildcard's plane where c == C

  float pf[NS];
  // ---- forward: k_align's step; the on-path thread leaves A(t, s_t) in fa[t]
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT;
    pf[k] = s < S ? emit(0, lab[k]) : 0.f;
    if (s < S) {
      const long long a = s < 2 ? fx_quantize(pf[k]) : FX_NEG;
      rows[0][s] = a;
      if (0 >= lo[k] && 0 < hi[k]) fa[0] = a;
    }
    pf[k] = (s < S && lim > 1) ? emit(1, lab[k]) : 0.f;
  }
  int cur = 0;
  __syncthreads();
  for (int t = 1; t < lim; ++t) {
    float nx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {                                  // frame t + 1's gathers, in flight across this frame
      const int s = tid + k * LATTICE_NT;
      nx[k] = (s < S && t + 1 < lim) ? emit(t + 1, lab[k]) : 0.f;
    }
    const long long* const R = rows[cur];
    long long* const W = rows[cur ^ 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * LATTICE_NT;
      if (s < S) {
        const long long q = fx_quantize(pf[k]);
        const long long a0 = R[s], a1 = s >= 1 ? R[s - 1] : FX_NEG, a2 = R[i2f[k]];
        const long long x = fx_lae(fx_lae(a0, a1, tab), a2, tab);
        const long long a = x == FX_NEG ? FX_NEG : x + q;
        W[s] = a;
        if (t >= lo[k] && t < hi[k]) fa[t] = a;                     // t < lim <= T
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) pf[k] = nx[k];
    cur ^= 1;
    __syncthreads();
  }
  const long long tot = L == 0 ? rows[cur][0] : fx_lae(rows[cur][2 * L], rows[cur][2 * L - 1], tab);
  __syncthreads();                                                  // the rows have been read: the backward pass starts over in them

  // ---- backward: frame lim - 1 first, then the mirrored step; fa[t] was stored by this work-group in front of a barrier
  auto post = [&](int t, int k, long long a, long long b, long long q) {
    const int g = lattice_post_clamp(a, b, q, tot);
    o_frame[t] = g;                                                 // t < lim <= T <= post_pitch
    lmin[k] = min(lmin[k], g);
  };
  long long fa_cur = 0, fa_nx = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT;
    pf[k] = s < S ? emit(lim - 1, lab[k]) : 0.f;
    if (s < S) {
      const long long q = fx_quantize(pf[k]);
      const long long b = (s == S - 1 || s == S - 2) ? q : FX_NEG;
      rows[0][s] = b;
      if (lim - 1 >= lo[k] && lim - 1 < hi[k]) post(lim - 1, k, fa[lim - 1], b, q);
      if (lim - 2 >= lo[k] && lim - 2 < hi[k]) fa_cur = fa[lim - 2];    // (lo >= 0: never with lim == 1)
    }
    pf[k] = (s < S && lim > 1) ? emit(lim - 2, lab[k]) : 0.f;
  }
  cur = 0;
  __syncthreads();
  for (int t = lim - 2; t >= 0; --t) {
    float nx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {                                  // frame t - 1's gathers, in flight across this frame
      const int s = tid + k * LATTICE_NT;
      nx[k] = (s < S && t >= 1) ? emit(t - 1, lab[k]) : 0.f;
      if (s < S && t - 1 >= lo[k] && t - 1 < hi[k]) fa_nx = fa[t - 1];
    }
    const long long* const R = rows[cur];
    long long* const W = rows[cur ^ 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int s = tid + k * LATTICE_NT;
      if (s < S) {
        const long long q = fx_quantize(pf[k]);
        const long long b0 = R[s], b1 = s + 1 < S ? R[s + 1] : FX_NEG, b2 = R[i2b[k]];
        const long long x = fx_lae(fx_lae(b0, b1, tab), b2, tab);
        const long long b = x == FX_NEG ? FX_NEG : x + q;
        W[s] = b;
        if (t >= lo[k] && t < hi[k]) post(t, k, fa_cur, b, q);
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) pf[k] = nx[k];
    fa_cur = fa_nx;
    cur ^= 1;
    __syncthreads();
  }
  // ---- per label the least certain frame of its run: the owner of state 2i + 1 has seen them all
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT;
    if (s < S && (s & 1)) o_label[s >> 1] = lmin[k];                // s >> 1 < L <= ML
  }
  if (tid == 0) {
    if (p.total) p.total[pr] = tot;
    p.ok[pr] = 1;
  }
}

template <bool STAR>
static void launch_post_ns(hipStream_t s, const PostP& p, int P, int states) {
  static_assert(2 * QASR_ALIGN_MAX_LABELS + 1 <= 17 * LATTICE_NT, "k_post<17> holds the longest target");
  lattice_dispatch_ns(states, [&](auto ns) {
    hipLaunchKernelGGL((k_post<decltype(ns)::value, STAR>), dim3((unsigned)P), dim3(LATTICE_NT), 0, s, p);
  });
}

int launch_post(hipStream_t s, const qasr_ctc_post_args& a) {
  PostP p{};
  p.logp = a.log_probs, p.lens = a.lens, p.targets = a.targets, p.target_lens = a.target_lens, p.tab = a.lae_table;
  p.start = a.start, p.nframes = a.nframes, p.ok_in = a.ok_in;
  p.fa = (long long*)a.workspace;
  p.frame_post = a.frame_post, p.label_post = a.label_post, p.total = (long long*)a.total, p.ok = a.ok;
  p.star = a.star_logp, p.star_pitch = a.star_pitch;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame, p.post_pitch = a.post_pitch;
  p.T = a.T, p.C = a.C, p.K = a.K, p.blank = a.blank, p.ML = a.max_labels;
  const int states = 2 * a.max_labels + 1;                          // <= 4097
  if (a.star_logp) launch_post_ns<true>(s, p, a.P, states);
  else launch_post_ns<false>(s, p, a.P, states);
  return QASR_OK;
}

}  // namespace qasr
