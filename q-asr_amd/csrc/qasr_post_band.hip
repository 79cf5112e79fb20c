// CTC posteriors along a banded alignment in fixed point (k_post_band): k_post's forward and backward passes (qasr_post.hip)
// inside the band k_align_band chose (qasr_align_band.hip), with that kernel's circular ownership.  The host statement is
// qasr/align.py (POST_BAND_RULES, post_band_host), and this file follows it bit for bit.  Scores are int64 sums of
// q = rint(logp * 2^16); both passes add with the caller's log-add-exp table (LDS resident): no exp, no log.
//
// k_post_band<NS, STAR>: one work-group of 256 threads per recording, sequential over frames.  The band holds BW = 256 * NS
// states [base, base + BW), base = band_base[p][t / 32] - read, not searched for.  State s lives in thread s % 256, slot
// (s >> 8) % NS, LDS index s % BW, so a slot's LDS index never changes and nothing rotates when the base moves.  Per slot in
// registers: its state, its label, the LDS index of the third term of either direction (s - 2 / s + 2, or a slot past the row
// that always holds NEG: no lane mask per state, see qasr_post.hip) and the interval [lo, hi) of frames in which the alignment
// (start / nframes) sits in that state.  s +- 1 and s +- 2 wrap in the circular row: whether a neighbour is a cell of the band
// is tested on the state number, not on the index.
//   forward, t = 0 .. lim - 1.  Where a block begins with a higher base, state s + BW takes the slot of every dropped state
//     s < base: the owner reloads label, indices and interval, writes NEG and gathers the frame again with the new label (one
//     more barrier, at most once in 32 frames).  Then k_post's step with "a predecessor below base is NEG"; the on-path thread
//     stores A(t, s_t) to the workspace fa[p][t].  total = lae(A[2L], A[2L - 1]), an end state outside the last band is NEG.
//   backward, t = lim - 1 .. 0.  Where frame t + 1 began a block with a higher base, the slot of every state s >= base(t) + BW
//     goes back to s - BW: the owner first stores the running minimum of the label it gives up (a label's run lies wholly inside
//     the frames in which its state is in the band, so that minimum is final), then reloads.  A state below base(t + 1) has no
//     edge out: it is NEG at frame t - that covers every cell that has just entered.  A successor at or above
//     min(base(t + 1) + BW, S) is NEG.  The on-path thread forms g = A + Bk - q - total from fa[p][t] (loaded a frame ahead: the
//     path's state at t is already resident at t + 1, because s_t >= base(t + 1) is checked), clamps, stores frame_post.
//     What is still resident at the end is stored then: every label exactly once, no third pass.
// Gathers run one frame ahead; one barrier per frame; the rows are double-buffered.
// start / nframes / ok_in / band_base are device data.  Before anything else: one thread per label checks the alignment as
// k_post does, one thread per block checks the trajectory (starts at 0, never decreases, a step < BW / 2, inside [0, top]),
// all in 64-bit; behind a barrier - runs are now frame intervals inside [0, lim] and may select a block - one thread per label
// checks that its run and the blank run before it lie inside the band and on its edges: s >= base(min(hi, lim - 1)) and
// s < base(lo) + BW (the base never decreases, so the two ends decide).  A bad row stores zeros; the group leaves together.
// LDS: 2 x (BW + 1) x 8 B of rows + 32 KB of table + two words: 102 424 B at NS = 17, 36 888 B at NS = 1.  LDS atomics: none.
// Global memory sees plain vector stores.  Every loop is bounded by T, L, the row pitch or a constant; nothing is allocated and
// no length is read on the host.  The STAR = false instantiations take no plane argument.
// The arithmetic (FX_NEG, fx_quantize, fx_lae) is qasr_fixed_dev.h's; LATTICE_BLOCK (the frames per entry of band_base, the one
// k_align_band moves by), the checks of the target and of start / nframes, a state's label and skip rules, the emission read,
// the clamp of g and the launch ladder are qasr_lattice_dev.h's, with their bounds.
#include "qasr_lattice_dev.h"

namespace qasr {

struct PostBandP {
  const float* logp;
  const int32_t* lens;          // optional [P]
  const int32_t* targets;       // [P][ML]
  const int32_t* target_lens;   // [P]
  const uint16_t* tab;          // [FX_TAB]
  const int32_t* start;         // [P][ML]
  const int32_t* nframes;       // [P][ML]
  const int32_t* ok_in;         // [P] optional
  const int32_t* band_base;     // [P][NB]
  long long* fa;                // [P][T]: the forward score along the path
  int32_t* frame_post;          // [P][post_pitch]
  int32_t* label_post;          // [P][ML]
  long long* total;             // [P] optional
  int32_t* ok;                  // [P]
  long long pitch_b, pitch_t, post_pitch;
  int T, C, blank, ML, NB;
};

struct PostBandPS : PostBandP {  // k_post_band<NS, true>'s argument
  const float* star;            // [P][star_pitch]
  long long star_pitch;
};

size_t post_band_workspace_bytes(int P, int T) { return (size_t)P * (size_t)T * sizeof(long long); }

template <int NS, bool STAR>
__global__ void __launch_bounds__(LATTICE_NT) k_post_band(std::conditional_t<STAR, PostBandPS, PostBandP> p) {
  constexpr int BW = NS * LATTICE_NT;
  constexpr int SENT = BW;                                          // one entry past the circular row: always NEG
  __shared__ long long rows[2][BW + 1];
  __shared__ uint16_t tab[FX_TAB];
  __shared__ int sh_bad, sh_out;
  const int tid = threadIdx.x, pr = blockIdx.x;
  const int T = p.T, C = p.C, blank = p.blank, ML = p.ML;
  const int lim = p.lens ? min(max(p.lens[pr], 0), T) : T;
  const int L = p.target_lens[pr];
  const int32_t* const y = p.targets + (size_t)pr * ML;
  const int32_t* const a_start = p.start + (size_t)pr * ML;
  const int32_t* const a_nframes = p.nframes + (size_t)pr * ML;
  const int32_t* const bb = p.band_base + (size_t)pr * p.NB;
  int32_t* const o_frame = p.frame_post + (long long)pr * p.post_pitch;
  int32_t* const o_label = p.label_post + (size_t)pr * ML;
  long long* const fa = p.fa + (size_t)pr * (size_t)T;

  if (tid == 0) sh_bad = 0, sh_out = 0, rows[0][SENT] = rows[1][SENT] = FX_NEG;
  for (int i = tid; i < FX_TAB; i += LATTICE_NT) tab[i] = p.tab[i];
  __syncthreads();
  // the target, the alignment and the trajectory are device data: checked here, before anything is read through them
  const bool len_ok = L >= 0 && L <= ML && L <= QASR_BAND_MAX_LABELS;
  const int S = len_ok ? 2 * L + 1 : 1;
  const int top = max(0, S - BW);
  const int nblk = (lim + LATTICE_BLOCK - 1) / LATTICE_BLOCK;       // blocks that have a frame < lim (<= NB: lim <= T)
  if (len_ok) {
    if (lattice_check_target<STAR>(y, L, C, blank, tid, LATTICE_NT) | lattice_check_runs(y, a_start, a_nframes, L, lim, tid, LATTICE_NT))
      sh_bad = 1;
    for (int j = tid; j < nblk; j += LATTICE_NT) {
      const long long b = bb[j], before = j ? (long long)bb[j - 1] : 0;
      if (b < 0 || b > top || (j ? (b < before || b - before >= BW / 2) : b != 0)) sh_bad = 1;
    }
  }
  __syncthreads();
  bool valid = len_ok && !sh_bad && !(p.ok_in && p.ok_in[pr] == 0) && !(lim == 0 && L > 0);
  if (valid && lim > 0) {
    // every run is a frame interval inside [0, lim] now and every base of a block < nblk lies in [0, top]: a frame may select
    // a block.  The state s of the frames [lo, hi), lo < hi, needs a cell at each and an edge out of each but the last of all
    auto outside = [&](int s, int lo, int hi) -> bool { return s < bb[min(hi, lim - 1) >> 5] || s >= bb[lo >> 5] + BW; };
    for (int i = tid; i < L; i += LATTICE_NT) {
      const int st = a_start[i], en = st + a_nframes[i];
      const int end_before = i ? a_start[i - 1] + a_nframes[i - 1] : 0;
      bool bad = outside(2 * i + 1, st, en);
      if (end_before < st) bad |= outside(2 * i, end_before, st);
      if (bad) sh_out = 1;
    }
    if (tid == 0) {                                                 // the blank behind the last label
      const int end_before = L ? a_start[L - 1] + a_nframes[L - 1] : 0;
      if (end_before < lim && outside(2 * L, end_before, lim)) sh_out = 1;
    }
  }
  __syncthreads();
  valid = valid && !sh_out;
  auto refuse = [&]() {
    for (int i = tid; i < T; i += LATTICE_NT) o_frame[i] = 0;
    for (int i = tid; i < ML; i += LATTICE_NT) o_label[i] = 0;
    if (tid == 0) {
      if (p.total) p.total[pr] = FX_NEG;
      p.ok[pr] = 0;
    }
  };
  if (!valid) {                                                     // uniform: both flags were read behind a barrier
    refuse();
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

  const LatticeEmit<STAR> emit = lattice_emit<STAR>(p, pr);         // logp[pr][t][c], the wildcard's plane where c == C

  int st[NS], lab[NS], lo[NS], hi[NS], lmin[NS];
  int i2f[NS], i2b[NS];                                             // where the third term lives: (s - 2) % BW / (s + 2) % BW, or SENT
  float pf[NS];
  // slot k takes the state s < S, s % BW == tid + k * 256 (a valid alignment: lo and hi are frame numbers in 0 .. lim)
  auto load_slot = [&](int k, int s) {
    const int i = s >> 1, i0 = tid + k * LATTICE_NT;
    st[k] = s, lab[k] = blank, i2f[k] = i2b[k] = SENT, lmin[k] = 0;
    if (s & 1) {
      const LatticeSlot sl = lattice_slot(y, s, S);
      lab[k] = sl.label;
      if (sl.skip_fwd) i2f[k] = i0 >= 2 ? i0 - 2 : i0 - 2 + BW;
      if (sl.skip_bwd) i2b[k] = i0 + 2 < BW ? i0 + 2 : i0 + 2 - BW;
      lo[k] = a_start[i], hi[k] = a_start[i] + a_nframes[i];
    } else {
      lo[k] = i ? a_start[i - 1] + a_nframes[i - 1] : 0;
      hi[k] = i < L ? a_start[i] : lim;
    }
  };

  // ---- forward: k_align_band's step with lae for max; the on-path thread leaves A(t, s_t) in fa[t]
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * LATTICE_NT;                             // base 0
    st[k] = s, lab[k] = blank, i2f[k] = i2b[k] = SENT, lo[k] = hi[k] = 0, lmin[k] = 0;
    if (s < S) load_slot(k, s);
    pf[k] = s < S ? emit(0, lab[k]) : 0.f;
    if (s < S) {
      const long long a = s < 2 ? fx_quantize(pf[k]) : FX_NEG;
      rows[0][s] = a;
      if (0 >= lo[k] && 0 < hi[k]) fa[0] = a;
    }
    pf[k] = (s < S && lim > 1) ? emit(1, lab[k]) : 0.f;
  }
  int cur = 0, base = 0;
  __syncthreads();
  for (int t = 1; t < lim; ++t) {
    if ((t & (LATTICE_BLOCK - 1)) == 0) {                           // uniform: a block begins
      const int nb = bb[t >> 5];                                    // t < lim: a checked entry, base <= nb < base + BW / 2
      if (nb > base) {                                              // (then top > 0: every slot holds a state < S)
        long long* const Rw = rows[cur];
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (st[k] < nb) {                                         // dropped: state st + BW enters (nb + BW <= S)
            load_slot(k, st[k] + BW);
            Rw[tid + k * LATTICE_NT] = FX_NEG;
            pf[k] = emit(t, lab[k]);                                // this frame again, with the new label
          }
        base = nb;
        __syncthreads();                                            // the NEGs are in place
      }
    }
    float nx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k)                                    // frame t + 1's gathers, in flight across this frame
      nx[k] = (st[k] < S && t + 1 < lim) ? emit(t + 1, lab[k]) : 0.f;
    const long long* const R = rows[cur];
    long long* const W = rows[cur ^ 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i0 = tid + k * LATTICE_NT;                          // s % BW
      const int s = st[k];
      if (s < S) {
        const int i1 = i0 >= 1 ? i0 - 1 : i0 - 1 + BW;
        const long long q = fx_quantize(pf[k]);
        const long long a0 = R[i0], a1 = s - 1 >= base ? R[i1] : FX_NEG, a2 = R[s - 2 >= base ? i2f[k] : SENT];
        const long long x = fx_lae(fx_lae(a0, a1, tab), a2, tab);
        const long long a = x == FX_NEG ? FX_NEG : x + q;
        W[i0] = a;
        if (t >= lo[k] && t < hi[k]) fa[t] = a;                     // t < lim <= T
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) pf[k] = nx[k];
    cur ^= 1;
    __syncthreads();
  }
  long long tot;
  {
    const long long* const R = rows[cur];
    if (L == 0) {
      tot = R[0];
    } else {                                                        // an end state outside the last band is NEG
      const int s2 = 2 * L, s1 = 2 * L - 1;
      const long long a = (s2 >= base && s2 < base + BW) ? R[s2 % BW] : FX_NEG;
      const long long b = (s1 >= base && s1 < base + BW) ? R[s1 % BW] : FX_NEG;
      tot = fx_lae(a, b, tab);
    }
  }
  __syncthreads();                                                  // the rows have been read: the backward pass starts over in them
  if (tot == FX_NEG) {                                              // uniform (a checked path has a finite score: not expected)
    refuse();
    return;
  }

  // ---- backward: frame lim - 1 first (the slots are the last band's), then the mirrored step
  auto post = [&](int t, int k, long long a, long long b, long long q) {
    const int g = lattice_post_clamp(a, b, q, tot);
    o_frame[t] = g;                                                 // t < lim <= T <= post_pitch
    lmin[k] = min(lmin[k], g);
  };
  long long fa_cur = 0, fa_nx = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int i0 = tid + k * LATTICE_NT;
    const int s = st[k];
    pf[k] = s < S ? emit(lim - 1, lab[k]) : 0.f;
    if (s < S) {
      const long long q = fx_quantize(pf[k]);
      const long long b = (s == S - 1 || s == S - 2) ? q : FX_NEG;
      rows[0][i0] = b;
      if (lim - 1 >= lo[k] && lim - 1 < hi[k]) post(lim - 1, k, fa[lim - 1], b, q);
      if (lim - 2 >= lo[k] && lim - 2 < hi[k]) fa_cur = fa[lim - 2];    // (lo >= 0: never with lim == 1)
    }
    pf[k] = (s < S && lim > 1) ? emit(lim - 2, lab[k]) : 0.f;
  }
  cur = 0;
  __syncthreads();
  for (int t = lim - 2; t >= 0; --t) {
    const int bnext = base;                                         // base(t + 1)
    if (((t + 1) & (LATTICE_BLOCK - 1)) == 0) {                     // uniform: frame t + 1 began a block
      const int nb = bb[t >> 5];
      if (nb < base) {
#pragma unroll
        for (int k = 0; k < NS; ++k)
          if (st[k] >= nb + BW) {                                   // above the band of t: state st - BW comes back (>= nb)
            if (st[k] & 1) o_label[st[k] >> 1] = lmin[k];           // its run is over: st >> 1 < L <= ML
            load_slot(k, st[k] - BW);
          }
        base = nb;
      }
    }
    const int hi_b = min(bnext + BW, S);                            // successors at or above this have no cell at t + 1
    float nx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {                                  // frame t - 1's gathers, in flight across this frame
      nx[k] = (st[k] < S && t >= 1) ? emit(t - 1, lab[k]) : 0.f;
      if (st[k] < S && t - 1 >= lo[k] && t - 1 < hi[k]) fa_nx = fa[t - 1];
    }
    const long long* const R = rows[cur];
    long long* const W = rows[cur ^ 1];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i0 = tid + k * LATTICE_NT;
      const int s = st[k];
      if (s < S) {
        const int i1 = i0 + 1 < BW ? i0 + 1 : i0 + 1 - BW;
        const long long q = fx_quantize(pf[k]);
        const long long b0 = R[i0], b1 = s + 1 < hi_b ? R[i1] : FX_NEG, b2 = R[s + 2 < hi_b ? i2b[k] : SENT];
        const long long x = fx_lae(fx_lae(b0, b1, tab), b2, tab);
        const long long b = (s < bnext || x == FX_NEG) ? FX_NEG : x + q;      // below base(t + 1): no edge out
        W[i0] = b;
        if (t >= lo[k] && t < hi[k]) post(t, k, fa_cur, b, q);
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) pf[k] = nx[k];
    fa_cur = fa_nx;
    cur ^= 1;
    __syncthreads();
  }
  // ---- the labels still resident: the owner of state 2i + 1 has seen every frame of label i's run
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = st[k];
    if (s < S && (s & 1)) o_label[s >> 1] = lmin[k];                // s >> 1 < L <= ML
  }
  if (tid == 0) {
    if (p.total) p.total[pr] = tot;
    p.ok[pr] = 1;
  }
}

template <bool STAR>
static int launch_post_band_ns(hipStream_t s, const std::conditional_t<STAR, PostBandPS, PostBandP>& p, int B, int band_states) {
  return lattice_dispatch_band_ns(band_states, [&](auto ns) {
    hipLaunchKernelGGL((k_post_band<decltype(ns)::value, STAR>), dim3((unsigned)B), dim3(LATTICE_NT), 0, s, p);
  });
}

int launch_post_band(hipStream_t s, const qasr_ctc_post_band_args& a) {
  PostBandPS p{};
  p.logp = a.log_probs, p.lens = a.lens, p.targets = a.targets, p.target_lens = a.target_lens, p.tab = a.lae_table;
  p.start = a.start, p.nframes = a.nframes, p.ok_in = a.ok_in, p.band_base = a.band_base;
  p.fa = (long long*)a.workspace;
  p.frame_post = a.frame_post, p.label_post = a.label_post, p.total = (long long*)a.total, p.ok = a.ok;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame, p.post_pitch = a.post_pitch;
  p.T = a.T, p.C = a.C, p.blank = a.blank, p.ML = a.max_labels, p.NB = (a.T + LATTICE_BLOCK - 1) / LATTICE_BLOCK;
  p.star = a.star_logp, p.star_pitch = a.star_pitch;
  if (a.star_logp) return launch_post_band_ns<true>(s, p, a.B, a.band_states);
  return launch_post_band_ns<false>(s, static_cast<const PostBandP&>(p), a.B, a.band_states);
}

}  // namespace qasr
