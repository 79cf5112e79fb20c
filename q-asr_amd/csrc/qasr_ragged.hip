// Reserved engines (qasr_engine_reserve): the bucket policy and the one kernel a ragged forward launches eagerly.
//
// A reserved engine owns every buffer of its forward, sized once for an envelope (max_batch x max_frames).  A call
// with any shape inside the envelope is rounded up to a bucket - all max_batch rows, frames up to a bucket edge - and
// each bucket owns one captured hipGraph over the engine's buffers.  What changes from call to call is the caller's
// input pointer, so the copy into the engine's staging buffers cannot be part of a graph: k_ragged_stage is launched
// directly in front of the graph.  In one pass it
//   - copies the caller's [B][S] audio (or [B][n_mels][T] features) into staging rows of the bucket's pitch,
//     16 bytes per lane where both sides allow it,
//   - copies the lengths and writes length 0 for the rows B .. max_batch - 1 (every kernel masks them out),
//   - writes the shape block: the batch's own B, S, STFT frame count and frame count per time domain, which the
//     captured kernels read with a plain load (k_mel's reflect padding must fold at the batch's S, k_ctc walks the
//     batch's own T').
#include <algorithm>

#include "qasr_internal.h"

namespace qasr {

// Bucket edge for a batch of T frames: the envelope's max_frames (a multiple of QASR_RAGGED_TILE) is cut into at most
// max_graphs equal steps of whole tiles; the last edge is max_frames itself.  -1: outside the envelope / bad argument.
// qasr/ragged.py restates this; tests/test_ragged_cpu.py holds the two together.
int ragged_bucket(int max_frames, int max_graphs, int T) {
  if (max_frames < 1 || max_graphs < 1 || T < 1 || max_frames % QASR_RAGGED_TILE || T > max_frames) return -1;
  const int units = max_frames / QASR_RAGGED_TILE;
  const int step = (units + max_graphs - 1) / max_graphs * QASR_RAGGED_TILE;
  const int edge = (T + step - 1) / step * step;
  return edge < max_frames ? edge : max_frames;
}

#define STAGE_NT 256
// grid (chunks of a row, rows of the batch); work-group (0, 0) also writes the lengths and the shape block
template <bool VEC>
__global__ void __launch_bounds__(STAGE_NT) k_ragged_stage(RaggedStageP p) {
  const int r = blockIdx.y;                                  // row: utterance r / n_rows, feature row r % n_rows
  const float* src = p.src + (size_t)r * p.src_pitch;
  float* dst = p.dst + (size_t)r * p.dst_pitch;
  if (VEC) {
    const int n4 = p.row >> 2;
    for (int i = blockIdx.x * STAGE_NT + threadIdx.x; i < n4; i += gridDim.x * STAGE_NT)
      reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
  } else {
    for (int i = blockIdx.x * STAGE_NT + threadIdx.x; i < p.row; i += gridDim.x * STAGE_NT) dst[i] = src[i];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int b = threadIdx.x; b < p.max_batch; b += STAGE_NT) p.lens_out[b] = b < p.B ? p.lens_in[b] : 0;
    if (threadIdx.x < QASR_SHAPE_WORDS) p.shp[threadIdx.x] = p.shape[threadIdx.x];
  }
}

int launch_ragged_stage(hipStream_t s, const RaggedStageP& p) {
  if (!p.src || !p.dst || !p.lens_in || !p.lens_out || !p.shp || p.B < 1 || p.B > p.max_batch || p.row < 1 || p.n_rows < 1 ||
      p.row > p.dst_pitch || p.row > p.src_pitch ||
      (long long)p.B * p.n_rows > 65535)
    return QASR_ERR_ARG;
  // 16-byte path: both bases and both pitches on 16-byte boundaries, rows a whole number of float4
  const bool vec = !((uintptr_t)p.src & 15) && !((uintptr_t)p.dst & 15) && !(p.src_pitch & 3) && !(p.dst_pitch & 3) && !(p.row & 3);
  const int per = vec ? 4 * STAGE_NT : STAGE_NT;
  const dim3 grid((unsigned)std::min((p.row + per - 1) / per, 64), (unsigned)(p.B * p.n_rows));
  if (vec) hipLaunchKernelGGL(k_ragged_stage<true>, grid, dim3(STAGE_NT), 0, s, p);
  else hipLaunchKernelGGL(k_ragged_stage<false>, grid, dim3(STAGE_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
