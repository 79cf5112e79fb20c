// Streaming CTC prefix beam search with phrase boosting (k_stream_beam_boost<LM>): k_stream_beam (qasr_stream_beam.hip) with
// k_beam_boost's look-up (qasr_beam_boost.hip) in the candidate evaluation, the automaton state `bst` and the running bonus
// `boost_tot` of every entry kept in the slot's block between steps.  The host statement is qasr/stream_beam.py
// (STREAM_BOOST_RULES, with BOOST_RULES of qasr/boost.py for the automaton).  The kernel is the <LM, true> use of the shared
// body (stream_beam_body in qasr_stream_beam_dev.h, which also holds the layout of a slot's block and the bounds).  What this
// file adds over it:
//   * the phrase sets as kernel arguments (up to 8 (pointer, bytes, whole_words) triples that the host call validated); the
//     packed set stays in global memory and is read with plain vector loads.  Header word 4 of a slot's block holds the slot's
//     set + 1: a BEGIN row stores boost_set[row] + 1 (outside -1 .. n_sets - 1: status 5), later rows read it.  A row whose
//     set is 0 makes no look-up at all;
//   * a slot's block of 16 + 24 W words ahead of the ring, and END rows that also write end_boost_score.
#include "qasr_stream_beam_dev.h"

namespace qasr {

struct StreamBeamBoostP {
  StreamBeamP e;
  StreamBeamSets g;
};

template <bool LM>
__global__ void __launch_bounds__(BEAM_NT) k_stream_beam_boost(StreamBeamBoostP p) {
  __shared__ StreamBeamLds<LM, true> L;
  stream_beam_body<LM, true>(p.e, &p.g, L);
}

size_t stream_beam_boost_state_bytes(int S, int W, int F) { return stream_beam_block_bytes(S, W, F, true); }

int launch_stream_beam_boost(hipStream_t s, const qasr_stream_beam_boost_args& q) {
  const qasr_stream_beam_args& a = q.beam;
  StreamBeamBoostP p{};
  stream_beam_fill(p.e, a, true);
  p.e.end_boost_score = (long long*)q.end_boost_score;
  stream_beam_fill_sets(p.g, q);
  if (a.lm) hipLaunchKernelGGL(k_stream_beam_boost<true>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, p);
  else hipLaunchKernelGGL(k_stream_beam_boost<false>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
