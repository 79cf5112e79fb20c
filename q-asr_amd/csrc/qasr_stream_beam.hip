// Streaming CTC prefix beam search (k_stream_beam<LM>): the search of k_beam / k_beam_lm (qasr_beam.hip) over the frames that
// one streaming step makes final, with the beam kept per slot on the device between steps and a fixed-lag commit that prunes.
// The host statement is qasr/stream_beam.py (STREAM_BEAM_RULES).  The kernel is the <LM, false> use of the shared body
// (stream_beam_body in qasr_stream_beam_dev.h, which also holds the layout of a slot's block and the bounds); this file adds
// the kernel's name, its launch and the size of the state.  It reads the stream block of qasr_stream.hip read-only
// (frames_done, received) and is launched BEFORE k_stream_emit, which advances frames_done.  The outputs of a step: the delta
// with creation frames, the best entry's uncommitted tail, and on END the n-best suffixes behind commit_len.
#include "qasr_stream_beam_dev.h"

namespace qasr {

template <bool LM>
__global__ void __launch_bounds__(BEAM_NT) k_stream_beam(StreamBeamP p) {
  __shared__ StreamBeamLds<LM, false> L;
  stream_beam_body<LM, false>(p, nullptr, L);
}

size_t stream_beam_state_bytes(int S, int W, int F) { return stream_beam_block_bytes(S, W, F, false); }

int launch_stream_beam(hipStream_t s, const qasr_stream_beam_args& a) {
  StreamBeamP p{};
  stream_beam_fill(p, a, false);
  if (a.lm) hipLaunchKernelGGL(k_stream_beam<true>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, p);
  else hipLaunchKernelGGL(k_stream_beam<false>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
