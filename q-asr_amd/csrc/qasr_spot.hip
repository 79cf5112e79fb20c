// Keyword spotting over CTC log-probabilities (k_spot); the host statement is SPOT_RULES and spot_host of qasr/spot.py, and this
// file follows it bit for bit.  Every keyword's lattice (k_align's states s = 1 .. 2L - 1) runs over the frames with a free start
// - state 0 is the constant fresh start (0, t) - and a free end at F = 2L - 1; a state carries the pair (D int64, start int32);
// the emission is e(t, s) = min(q(logp[u][t][lab(s)]) - q(star[u][t]), 0), q = rint(x * 2^16) clamped (fx_quantize).
//
// k_spot<NS>: one WAVE per problem p = u * K + k, four problems to a work-group of 256 threads.  Lane l owns the NS contiguous
// states l * NS .. l * NS + NS - 1 (NS = 1, 2, 4 from the row pitch of the targets: 2 ML + 1 <= 64 / 128 / 256).  A state's
// label, its "may skip the blank" bit and its pair stay in registers; there is no LDS row and no barrier anywhere, so the four
// waves of a work-group run to their own lim.  Per frame a lane needs two pairs from below itself: states l * NS - 1 and
// l * NS - 2, that is the top two states of lane l - 1 (NS >= 2) or the states of lanes l - 1 and l - 2 (NS = 1); they cross
// lanes with __shfl_up, everything else is in the lane's own registers.  The only global reads of a frame are the NS gathers
// logp[u][t][lab(s)] and star[u][t]; frame t + 1's are issued before frame t's arithmetic.
// The lane that owns F applies the candidate and hit rules in its own registers (one open hit) and stores closed hits, and the
// optional trace, with plain vector stores.  The tails (hit rows behind the stored hits, trace frames behind lim) are zeroed by
// all lanes.  LDS: none.  Atomics: none.  Nothing is read back.  Every loop is bounded by T, ML, max_hits or a constant; nothing
// is allocated and no length is read on the host.
// FX_NEG and fx_quantize are qasr_fixed_dev.h's; the target check and a state's label and skip rule are qasr_lattice_dev.h's.
#include <climits>

#include "qasr_lattice_dev.h"

namespace qasr {

#define SPOT_NT 256
#define SPOT_WAVE 64
#define SPOT_WAVES (SPOT_NT / SPOT_WAVE)

struct SpotP {
  const float* logp;
  const int32_t* lens;          // optional [B]
  const float* star;            // [B][star_pitch]
  const int32_t* targets;       // [K][ML]
  const int32_t* target_lens;   // [K]
  int32_t* hit_start;           // [P][max_hits]
  int32_t* hit_end;             // [P][max_hits]
  long long* hit_score;         // [P][max_hits]
  int32_t* n_hits;              // [P]
  int32_t* ok;                  // [P]
  long long* trace_score;       // [P][trace_pitch] optional
  int32_t* trace_start;         // [P][trace_pitch] optional
  long long pitch_b, pitch_t, star_pitch, trace_pitch;
  int P, T, C, K, ML, blank, threshold_q, max_span, max_hits;
};

template <int NS>
__global__ void __launch_bounds__(SPOT_NT) k_spot(SpotP p) {
  const int lane = threadIdx.x & (SPOT_WAVE - 1);
  const long long pl = (long long)blockIdx.x * SPOT_WAVES + (threadIdx.x / SPOT_WAVE);
  if (pl >= p.P) return;                                            // wave-uniform; no barrier follows
  const int pr = (int)pl, u = pr / p.K, kw = pr - u * p.K;
  const int T = p.T, C = p.C, blank = p.blank, ML = p.ML, MH = p.max_hits;
  const int lim = p.lens ? min(max(p.lens[u], 0), T) : T;
  const int L = p.target_lens[kw];
  const int32_t* const y = p.targets + (size_t)kw * ML;
  int32_t* const o_start = p.hit_start + (size_t)pr * MH;
  int32_t* const o_end = p.hit_end + (size_t)pr * MH;
  long long* const o_score = p.hit_score + (size_t)pr * MH;
  long long* const tr_d = p.trace_score ? p.trace_score + (long long)pr * p.trace_pitch : nullptr;
  int32_t* const tr_s = p.trace_score ? p.trace_start + (long long)pr * p.trace_pitch : nullptr;

  // the target is device data: its length and every label are checked here, before anything is read through them
  const bool len_ok = L >= 1 && L <= ML && L <= QASR_SPOT_MAX_LABELS && 2 * L <= NS * SPOT_WAVE;
  const bool bad = len_ok && lattice_check_target<false>(y, L, C, blank, lane, SPOT_WAVE);
  const bool valid = len_ok && __ballot(bad) == 0;                  // wave-uniform
  if (!valid) {
    for (int i = lane; i < MH; i += SPOT_WAVE) o_start[i] = 0, o_end[i] = 0, o_score[i] = 0;
    if (tr_d)
      for (int t = lane; t < T; t += SPOT_WAVE) tr_d[t] = 0, tr_s[t] = 0;      // t < T <= trace_pitch
    if (lane == 0) p.n_hits[pr] = 0, p.ok[pr] = 0;
    return;
  }
  const int S = 2 * L, F = S - 1;                                   // states 0 .. F; F <= NS * 64 - 1
  const int f_lane = F / NS, f_k = F - f_lane * NS;

  int lab[NS];
  bool skp[NS];
  long long D[NS];
  int st[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = lane * NS + k;
    lab[k] = blank, skp[k] = false;
    if (s < S && (s & 1)) {                                         // s >> 1 < L
      const LatticeSlot sl = lattice_slot(y, s, S);
      lab[k] = sl.label, skp[k] = sl.skip_fwd;
    }
    D[k] = FX_NEG, st[k] = -1;                                      // the row before frame 0: every state dead
  }
  const float* const base = p.logp + (long long)u * p.pitch_b;      // [t * pitch_t + c], c < C <= pitch_t
  const float* const srow = p.star + (long long)u * p.star_pitch;   // [t], t < T <= star_pitch
  float pf[NS], ps = 0.f;
#pragma unroll
  for (int k = 0; k < NS; ++k) pf[k] = lim > 0 ? base[lab[k]] : 0.f;
  if (lim > 0) ps = srow[0];

  const long long thr = p.threshold_q;
  const int max_span = p.max_span;
  bool open = false;                                                // the open hit: meaningful in lane f_lane only
  int h_start = 0, h_end = 0, count = 0;
  long long h_d = 0;

  for (int t = 0; t < lim; ++t) {
    float nx[NS], ns = 0.f;
    const bool more = t + 1 < lim;
#pragma unroll
    for (int k = 0; k < NS; ++k)                                    // frame t + 1's gathers, in flight across this frame
      nx[k] = more ? base[(long long)(t + 1) * p.pitch_t + lab[k]] : 0.f;
    if (more) ns = srow[t + 1];
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
      if (s == 1) a1 = 0, s1 = t;                                   // the fresh start
      long long a2 = k >= 2 ? D[k >= 2 ? k - 2 : 0] : (k == 1 ? b1d : b2d);
      int s2 = k >= 2 ? st[k >= 2 ? k - 2 : 0] : (k == 1 ? b1s : b2s);
      if (!skp[k]) a2 = FX_NEG;
      long long best = D[k];
      int bs = st[k];
      if (a1 > best) best = a1, bs = s1;
      if (a2 > best) best = a2, bs = s2;
      const bool live = best != FX_NEG && s >= 1;                   // (state 0 is not computed: it stays dead)
      nd[k] = live ? best + e : FX_NEG;
      nst[k] = live ? bs : -1;
    }
    long long fd = FX_NEG;
    int fs = -1;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      D[k] = nd[k], st[k] = nst[k], pf[k] = nx[k];
      if (k == f_k) fd = nd[k], fs = nst[k];
    }
    ps = ns;
    if (lane == f_lane) {
      if (tr_d) tr_d[t] = fd, tr_s[t] = fs;                         // t < lim <= T <= trace_pitch
      if (fd != FX_NEG) {
        const long long n = (long long)t - fs + 1;                  // 0 <= fs <= t
        if (n <= max_span && fd >= thr * n) {                       // a candidate
          if (open && fs <= h_end) {                                // overlaps the open hit: the higher mean stays
            const long long n_open = (long long)h_end - h_start + 1;
            if (fd * n_open > h_d * n) h_start = fs, h_end = t, h_d = fd;
          } else {
            if (open) {
              if (count < MH) o_start[count] = h_start, o_end[count] = h_end, o_score[count] = h_d;
              ++count;
            }
            open = true, h_start = fs, h_end = t, h_d = fd;
          }
        }
      }
    }
  }
  if (lane == f_lane) {
    if (open) {
      if (count < MH) o_start[count] = h_start, o_end[count] = h_end, o_score[count] = h_d;
      ++count;
    }
    p.n_hits[pr] = count, p.ok[pr] = 1;
  }
  const int stored = min(__shfl(count, f_lane), MH);
  for (int i = stored + lane; i < MH; i += SPOT_WAVE) o_start[i] = 0, o_end[i] = 0, o_score[i] = 0;
  if (tr_d)
    for (int t = lim + lane; t < T; t += SPOT_WAVE) tr_d[t] = 0, tr_s[t] = 0;
}

int launch_spot(hipStream_t s, const qasr_ctc_spot_args& a) {
  SpotP p{};
  p.logp = a.log_probs, p.lens = a.lens, p.star = a.star_logp, p.targets = a.targets, p.target_lens = a.target_lens;
  p.hit_start = a.hit_start, p.hit_end = a.hit_end, p.hit_score = (long long*)a.hit_score, p.n_hits = a.n_hits, p.ok = a.ok;
  p.trace_score = (long long*)a.trace_score, p.trace_start = a.trace_start;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame, p.star_pitch = a.star_pitch, p.trace_pitch = a.trace_pitch;
  const long long P = (long long)a.B * a.K;
  if (P > INT_MAX) return QASR_ERR_ARG;
  p.P = (int)P, p.T = a.T, p.C = a.C, p.K = a.K, p.ML = a.max_labels, p.blank = a.blank;
  p.threshold_q = a.threshold_q, p.max_span = a.max_span, p.max_hits = a.max_hits;
  const dim3 grid((unsigned)((P + SPOT_WAVES - 1) / SPOT_WAVES)), block(SPOT_NT);
  const int states = 2 * a.max_labels + 1;                          // <= 255
  static_assert(2 * QASR_SPOT_MAX_LABELS + 1 <= 4 * SPOT_WAVE, "k_spot<4> holds the longest keyword");
  if (states <= 1 * SPOT_WAVE) hipLaunchKernelGGL(k_spot<1>, grid, block, 0, s, p);
  else if (states <= 2 * SPOT_WAVE) hipLaunchKernelGGL(k_spot<2>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_spot<4>, grid, block, 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
