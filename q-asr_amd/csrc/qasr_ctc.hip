// Greedy CTC collapse on the device: the loop of WER.ctc_decoder_predictions_tensor
// (nemo/collections/asr/metrics/wer.py: keep p when (p != previous or previous == blank) and p != blank) over a token
// matrix [B][T], with what the host loop throws away: the first frame and the length of every emitted run, the best
// per-frame score inside the run, and the log-probability of the whole greedy path.
//
// One work-group per utterance.  Each wave takes 64-frame chunks (chunk = round * waves + wave).  Inside a chunk the
// "a non-blank run starts here" mask comes from __ballot (64 bits), a lane's label index is the number of starts before
// it (__popcll of the lower bits) plus the starts of all earlier chunks, and the lane that ends a run finds the run's
// first frame as the highest start bit at or below itself.  The run maximum is a segmented Hillis-Steele scan inside
// the chunk.  What crosses a chunk boundary - starts so far, first frame and running maximum of the run that is open at
// the boundary - is a three-word summary per chunk in LDS which every thread folds in chunk order, so the result does not
// depend on how many waves the work-group has.  Scores are compared as order-preserving integers (a total order on
// float32 bit patterns: exact, and -0 < +0 on every path).
//
// utt_score is summed by wave 0 alone in the order the header fixes: lane l adds the frames t = l, l + 64, ... in
// increasing t, then one lane adds the 64 partial sums in lane order.  Plain float32 adds, no atomics.
#include <climits>

#include "qasr_internal.h"

namespace qasr {

#define CTC_NT 256
#define CTC_MAX_WAVES 16

struct CtcP {
  const int32_t* tokens;    // [B][T]
  const float* fs;          // optional [B][T]
  const int32_t* lens;      // optional [B]
  int32_t* labels;          // [B][T]
  int32_t* n_labels;        // [B]
  int32_t* start;           // optional [B][T]
  int32_t* nframes;         // optional [B][T]
  float* score;             // optional [B][T] (needs fs)
  float* utt_score;         // optional [B] (needs fs)
  int B, T, blank;
  const int32_t* t_act;     // optional (device): frames of the batch inside rows of pitch T (reserved engines)
};

// float32 bits <-> an int that orders like the float (its own inverse)
__device__ __forceinline__ int ctc_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

__global__ void __launch_bounds__(CTC_NT) k_ctc(CtcP p) {
  __shared__ int sm_cnt[2][CTC_MAX_WAVES], sm_last[2][CTC_MAX_WAVES], sm_max[2][CTC_MAX_WAVES];
  __shared__ float sm_part[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int b = blockIdx.x, T = p.T;
  const int Ta = p.t_act ? min(*p.t_act, T) : T;
  const int lim = p.lens ? min(max(p.lens[b], 0), Ta) : Ta;
  const int32_t* const tok = p.tokens + (size_t)b * T;
  const float* const fs = p.fs ? p.fs + (size_t)b * T : nullptr;
  const size_t row = (size_t)b * T;
  const bool want_max = fs && p.score;
  const int nchunks = (lim + 63) >> 6, rounds = (nchunks + nw - 1) / nw;
  int base = 0, cs = 0, cm = INT_MIN;          // carried over chunks: starts so far, the open run's first frame and maximum
  for (int r = 0; r < rounds; ++r) {
    const int t0 = (r * nw + wave) << 6, t = t0 + lane;
    const bool valid = t < lim;
    int me = p.blank, v = INT_MIN;
    bool is_start = false, is_end = false;
    if (valid) {
      me = tok[t];
      if (me != p.blank) {
        is_start = t == 0 || tok[t - 1] != me;
        is_end = t + 1 == lim || tok[t + 1] != me;
      }
      if (want_max) v = ctc_key(__float_as_int(fs[t]));
    }
    const unsigned long long smask = __ballot(is_start);
    const unsigned long long le = smask & ((2ull << lane) - 1ull);       // starts at or below this lane
    const int h = le ? 63 - __clzll((long long)le) : -1;                  // lane of this frame's run start (-1: an earlier chunk)
    if (want_max) {
      const int hs = max(h, 0);
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane - d >= hs) v = max(v, o);
      }
    }
    // the chunk's summary is what lane 63 sees: its scan covers the last start (or the whole chunk) to the chunk's end
    const int buf = r & 1;
    if (lane == 63) {
      sm_cnt[buf][wave] = __popcll(smask);
      sm_last[buf][wave] = h >= 0 ? t0 + h : -1;
      sm_max[buf][wave] = v;
    }
    __syncthreads();
    int mybase = 0, mycs = 0, mycm = INT_MIN;
    for (int w = 0; w < nw; ++w) {
      if (w == wave) { mybase = base; mycs = cs; mycm = cm; }
      base += sm_cnt[buf][w];
      const int last = sm_last[buf][w], mx = sm_max[buf][w];
      if (last >= 0) { cs = last; cm = mx; } else { cm = max(cm, mx); }
    }
    const int nle = __popcll(le);
    if (is_start) {
      const int idx = mybase + nle - 1;
      if (idx >= 0 && idx < T) {
        p.labels[row + idx] = me;
        if (p.start) p.start[row + idx] = t;
      }
    }
    if (is_end) {
      const int idx = mybase + nle - 1;
      if (idx >= 0 && idx < T) {
        const int rs = h >= 0 ? t0 + h : mycs;
        if (p.nframes) p.nframes[row + idx] = t - rs + 1;
        if (want_max) p.score[row + idx] = __int_as_float(ctc_key(h >= 0 ? v : max(v, mycm)));
      }
    }
  }
  // every thread holds the same total now; tails: blank / 0
  const int n = min(base, T);
  for (int i = n + tid; i < T; i += blockDim.x) {
    p.labels[row + i] = p.blank;
    if (p.start) p.start[row + i] = 0;
    if (p.nframes) p.nframes[row + i] = 0;
    if (p.score) p.score[row + i] = 0.f;
  }
  if (tid == 0) p.n_labels[b] = n;
  if (p.utt_score) {
    if (wave == 0) {
      float part = 0.f;
      for (int t = lane; t < lim; t += 64) part += fs[t];
      sm_part[lane] = part;
    }
    __syncthreads();
    if (tid == 0) {
      float acc = 0.f;
      for (int l = 0; l < 64; ++l) acc += sm_part[l];
      p.utt_score[b] = acc;
    }
  }
}

int launch_ctc(hipStream_t s, const int32_t* tokens, const float* frame_score, const int32_t* lens, int B, int T, int blank,
               const qasr_ctc_out& out, const int32_t* t_act) {
  if (!tokens || !out.labels || !out.n_labels || B < 1 || T < 1) return QASR_ERR_ARG;
  if ((out.score || out.utt_score) && !frame_score) return QASR_ERR_ARG;
  CtcP p{};
  p.tokens = tokens, p.fs = frame_score, p.lens = lens;
  p.labels = out.labels, p.n_labels = out.n_labels, p.start = out.start, p.nframes = out.nframes;
  p.score = out.score, p.utt_score = out.utt_score;
  p.B = B, p.T = T, p.blank = blank, p.t_act = t_act;
  hipLaunchKernelGGL(k_ctc, dim3(B), dim3(CTC_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
