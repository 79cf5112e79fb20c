// Streaming keyword spotting (k_stream_spot); the host statement is qasr/stream_spot.py (STREAM_SPOT_RULES), and this file
// follows it byte for byte, the state block included.
//
// State: S * K blocks of 8 + 3 SP 32-bit words (SP = 64 NS), a buffer of its own next to the stream state: a header (frames_done
// of this block, stepped, the open hit, count) and the keyword's Viterbi row D int64 [SP], start int32 [SP].  A block is read and
// written by the ONE wave that owns (slot, keyword) in that launch (the rows' slots are distinct), with plain vector stores; no
// word is written by one wave and read by another; no atomics; nothing is read back.  The stream block (frames_done) is read,
// never written: the launch goes behind k_stream_emit on the same queue and can be captured with it.
//
// k_stream_spot<NS>: one WAVE per problem p = row * K + k, four problems to a work-group of 256 threads, lane l owning the states
// l * NS .. l * NS + NS - 1 as in k_spot, so a lane loads and stores NS contiguous pairs of the block.  The frame loop is
// k_spot's, taken as functions (qasr_spot_dev.h: spot_frame, spot_candidate), frame t + 1's gathers in flight across frame t, over the frames
// lo .. hi - 1 that became final, at window index t - first_frame.  Behind the candidate rule the early close: the lane that owns
// F hands out the open hit's end (-1: none) with one __shfl; while a hit is open every lane evaluates one predicate over its NS
// states and one __ballot tells whether any state could still grow into an overlapping candidate.  The lane that owns F keeps the
// open hit in registers and stores closed hits; every output tail is written.  LDS: none.  Barriers: none.  Every loop is bounded
// by max_final_frames, ML, PH or a constant: a step that would walk more than max_final_frames frames is refused (status 3).
#include <climits>

#include "qasr_spot_dev.h"

namespace qasr {

#define SSPOT_HEADER 8
#define SSPOT_DONE 0
#define SSPOT_STEPPED 1
#define SSPOT_OPEN 2
#define SSPOT_HSTART 3
#define SSPOT_HEND 4
#define SSPOT_COUNT 5
#define SSPOT_HD 6
// the stream block of qasr_stream.hip, read-only here
#define SSPOT_ST_WORDS 80
#define SSPOT_ST_DONE 2

struct StreamSpotP {
  const int32_t* state;         // the stream state
  int32_t* sp;                  // [S][K][8 + 3 SP]
  const int32_t* slots;         // [B]
  const int32_t* flags;         // [B]
  const float* logp;            // [B][Tw][C] with pitches
  const float* star;            // [B][star_pitch]
  const int32_t* enc_lens;      // [B]
  const int32_t* first_frame;   // [B]
  const int32_t* em_status;     // [B]
  const int32_t* targets;       // [K][ML]
  const int32_t* target_lens;   // [K]
  int32_t* hit_start;           // [P][PH]
  int32_t* hit_end;             // [P][PH]
  int32_t* hit_detect;          // [P][PH]
  long long* hit_score;         // [P][PH]
  int32_t* n_new;               // [P]
  int32_t* n_total;             // [P]
  int32_t* open_start;          // [P]
  int32_t* open_end;            // [P]
  long long* open_score;        // [P]
  int32_t* ok;                  // [P]
  int32_t* status;              // [P]
  long long pitch_b, pitch_t, star_pitch;
  int P, S, Tw, C, K, ML, blank, threshold_q, max_span, PH, max_final;
};

template <int NS>
__global__ void __launch_bounds__(SPOT_NT) k_stream_spot(StreamSpotP p) {
  constexpr int SP = NS * SPOT_WAVE, WORDS = SSPOT_HEADER + 3 * SP;
  const int lane = threadIdx.x & (SPOT_WAVE - 1);
  const long long pl = (long long)blockIdx.x * SPOT_WAVES + (threadIdx.x / SPOT_WAVE);
  if (pl >= p.P) return;                                            // wave-uniform; no barrier follows
  const int pr = (int)pl, row = pr / p.K, kw = pr - row * p.K;
  const int C = p.C, blank = p.blank, ML = p.ML, PH = p.PH;
  int32_t* const o_start = p.hit_start + (size_t)pr * PH;
  int32_t* const o_end = p.hit_end + (size_t)pr * PH;
  int32_t* const o_detect = p.hit_detect + (size_t)pr * PH;
  long long* const o_score = p.hit_score + (size_t)pr * PH;
  const int slot = p.slots[row];
  const bool slot_ok = slot >= 0 && slot < p.S;
  int status = !slot_ok ? 2 : (p.em_status[row] != 0 ? 1 : 0);

  // the target is device data: its length and every label are checked here, before anything is read through them
  const int L = p.target_lens[kw];
  const int32_t* const y = p.targets + (size_t)kw * ML;
  const bool len_ok = L >= 1 && L <= ML && L <= QASR_SPOT_MAX_LABELS && 2 * L <= NS * SPOT_WAVE;
  const bool bad = len_ok && lattice_check_target<false>(y, L, C, blank, lane, SPOT_WAVE);
  const bool valid = len_ok && __ballot(bad) == 0;                  // wave-uniform

  int32_t* const blk = p.sp + ((long long)(slot_ok ? slot : 0) * p.K + kw) * WORDS;
  const int fl = p.flags[row];
  const bool end = (fl & QASR_STREAM_END) != 0;
  int lo = 0, hi = 0, first = 0;
  bool fresh = true;
  if (valid && !status) {
    fresh = (fl & QASR_STREAM_BEGIN) != 0 || blk[SSPOT_STEPPED] == 0;
    lo = fresh ? 0 : blk[SSPOT_DONE];
    hi = p.state[(long long)slot * SSPOT_ST_WORDS + SSPOT_ST_DONE];
    first = p.first_frame[row];
    const int e = min(max(p.enc_lens[row], 0), p.Tw);
    if (lo > hi || lo < first || (lo < hi && (long long)hi > (long long)first + e) || (long long)hi - lo > p.max_final) status = 3;
  }
  if (!valid || status) {                                           // an empty step, the block untouched
    for (int i = lane; i < PH; i += SPOT_WAVE) o_start[i] = 0, o_end[i] = 0, o_detect[i] = 0, o_score[i] = 0;
    if (lane == 0) {
      p.n_new[pr] = 0, p.n_total[pr] = 0, p.open_start[pr] = -1, p.open_end[pr] = -1, p.open_score[pr] = 0;
      p.ok[pr] = valid ? 1 : 0, p.status[pr] = status;
    }
    return;
  }
  const int S = 2 * L, F = S - 1;                                   // states 0 .. F; F <= NS * 64 - 1
  const int f_lane = F / NS, f_k = F - f_lane * NS;

  int lab[NS];
  bool skp[NS];
  long long D[NS];
  int st[NS];
  spot_slots<NS>(y, S, blank, lane, lab, skp);
  long long* const blk_d = (long long*)(blk + SSPOT_HEADER);        // [SP]; the block is 8-byte aligned: WORDS is even
  int32_t* const blk_s = blk + SSPOT_HEADER + 2 * SP;               // [SP]
  SpotHit h{false, 0, 0, 0}, closed{};                              // the open hit: meaningful in lane f_lane only
  int count = 0;
#pragma unroll
  for (int k = 0; k < NS; ++k) D[k] = FX_NEG, st[k] = -1;          // a fresh stream: every state dead
  if (!fresh) {
#pragma unroll
    for (int k = 0; k < NS; ++k) D[k] = blk_d[lane * NS + k], st[k] = blk_s[lane * NS + k];
    h.open = blk[SSPOT_OPEN] != 0, h.start = blk[SSPOT_HSTART], h.end = blk[SSPOT_HEND];
    h.d = *(const long long*)(blk + SSPOT_HD);
    count = blk[SSPOT_COUNT];
  }
  // first <= lo and hi <= first + e <= first + Tw wherever a frame is read: window indices t - first lie in 0 .. Tw - 1
  const float* const base = p.logp + (long long)row * p.pitch_b - (long long)first * p.pitch_t;   // indexed by the global frame
  const float* const srow = p.star + (long long)row * p.star_pitch - first;
  float pf[NS], ps = 0.f;
#pragma unroll
  for (int k = 0; k < NS; ++k) pf[k] = lo < hi ? base[(long long)lo * p.pitch_t + lab[k]] : 0.f;
  if (lo < hi) ps = srow[lo];

  const long long thr = p.threshold_q;
  const int max_span = p.max_span;
  int nnew = 0;

  for (int t = lo; t < hi; ++t) {                                   // at most max_final frames
    float nx[NS], ns = 0.f;
    const bool more = t + 1 < hi;
#pragma unroll
    for (int k = 0; k < NS; ++k)                                    // frame t + 1's gathers, in flight across this frame
      nx[k] = more ? base[(long long)(t + 1) * p.pitch_t + lab[k]] : 0.f;
    if (more) ns = srow[t + 1];
    long long fd;
    int fs;
    spot_frame<NS>(D, st, skp, pf, ps, lane, t, f_k, fd, fs);
#pragma unroll
    for (int k = 0; k < NS; ++k) pf[k] = nx[k];
    ps = ns;
    if (lane == f_lane && spot_candidate(h, fd, fs, t, thr, max_span, closed)) {
      if (nnew < PH) o_start[nnew] = closed.start, o_end[nnew] = closed.end, o_detect[nnew] = t, o_score[nnew] = closed.d;
      ++nnew, ++count;
    }
    // the early close: no live state 1 .. F whose start overlaps the open hit can still end inside max_span
    const int he = __shfl(h.open ? h.end : -1, f_lane);             // wave-uniform
    if (he >= 0) {
      bool keep = false;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int s = lane * NS + k;
        keep |= s >= 1 && s <= F && D[k] != FX_NEG && st[k] <= he && (long long)t + 2 - st[k] <= max_span;
      }
      if (__ballot(keep) == 0 && lane == f_lane) {
        if (nnew < PH) o_start[nnew] = h.start, o_end[nnew] = h.end, o_detect[nnew] = t, o_score[nnew] = h.d;
        ++nnew, ++count;
        h.open = false;
      }
    }
  }
  if (lane == f_lane) {
    if (end && h.open) {                                            // END closes the open hit behind the last frame
      if (nnew < PH) o_start[nnew] = h.start, o_end[nnew] = h.end, o_detect[nnew] = hi - 1, o_score[nnew] = h.d;
      ++nnew, ++count;
      h.open = false;
    }
    p.n_new[pr] = nnew, p.n_total[pr] = count;
    p.open_start[pr] = h.open ? h.start : -1, p.open_end[pr] = h.open ? h.end : -1, p.open_score[pr] = h.open ? h.d : 0;
    p.ok[pr] = 1, p.status[pr] = 0;
    blk[SSPOT_DONE] = hi, blk[SSPOT_STEPPED] = 1, blk[SSPOT_OPEN] = h.open ? 1 : 0;
    blk[SSPOT_HSTART] = h.open ? h.start : 0, blk[SSPOT_HEND] = h.open ? h.end : 0, blk[SSPOT_COUNT] = count;
    *(long long*)(blk + SSPOT_HD) = h.open ? h.d : 0;
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {                                    // state 0 and the states above F are stored dead
    const int s = lane * NS + k;
    const bool own = s >= 1 && s <= F;
    blk_d[s] = own ? D[k] : FX_NEG, blk_s[s] = own ? st[k] : -1;
  }
  const int stored = min(__shfl(nnew, f_lane), PH);
  for (int i = stored + lane; i < PH; i += SPOT_WAVE) o_start[i] = 0, o_end[i] = 0, o_detect[i] = 0, o_score[i] = 0;
}

size_t stream_spot_state_bytes(int S, int K, int max_labels) {
  if (S < 1 || K < 1 || max_labels < 1 || max_labels > QASR_SPOT_MAX_LABELS) return 0;
  const int states = 2 * max_labels + 1;
  const size_t ns = states <= 1 * SPOT_WAVE ? 1 : (states <= 2 * SPOT_WAVE ? 2 : 4);
  return (size_t)S * (size_t)K * 4 * (SSPOT_HEADER + 3 * ns * SPOT_WAVE);
}

int launch_stream_spot(hipStream_t s, const qasr_stream_spot_args& a) {
  StreamSpotP p{};
  p.state = (const int32_t*)a.state, p.sp = (int32_t*)a.spot_state, p.slots = a.slots, p.flags = a.flags;
  p.logp = a.log_probs, p.star = a.star_logp, p.enc_lens = a.enc_lens, p.first_frame = a.first_frame, p.em_status = a.emit_status;
  p.targets = a.targets, p.target_lens = a.target_lens;
  p.hit_start = a.hit_start, p.hit_end = a.hit_end, p.hit_detect = a.hit_detect, p.hit_score = (long long*)a.hit_score;
  p.n_new = a.n_new_hits, p.n_total = a.n_hits_total, p.open_start = a.open_start, p.open_end = a.open_end;
  p.open_score = (long long*)a.open_score, p.ok = a.ok, p.status = a.status;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame, p.star_pitch = a.star_pitch;
  const long long P = (long long)a.B * a.K;
  if (P > INT_MAX) return QASR_ERR_ARG;
  p.P = (int)P, p.S = a.S, p.Tw = a.Tw, p.C = a.n_classes, p.K = a.K, p.ML = a.max_labels, p.blank = a.blank;
  p.threshold_q = a.threshold_q, p.max_span = a.max_span, p.PH = a.PH, p.max_final = a.max_final_frames;
  const dim3 grid((unsigned)((P + SPOT_WAVES - 1) / SPOT_WAVES)), block(SPOT_NT);
  const int states = 2 * a.max_labels + 1;                          // <= 255
  static_assert(2 * QASR_SPOT_MAX_LABELS + 1 <= 4 * SPOT_WAVE, "k_stream_spot<4> holds the longest keyword");
  if (states <= 1 * SPOT_WAVE) hipLaunchKernelGGL(k_stream_spot<1>, grid, block, 0, s, p);
  else if (states <= 2 * SPOT_WAVE) hipLaunchKernelGGL(k_stream_spot<2>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_stream_spot<4>, grid, block, 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
