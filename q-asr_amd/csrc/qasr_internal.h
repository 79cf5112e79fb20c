// Internal parameter blocks shared by the engine (qasr_engine.hip) and the kernels (qasr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qasr.h"

namespace qasr {

// One consumer of an op's integer result (device view of qasr_out).
struct OutP {
  void* ptr;            // i8 [B][C][Tp]  (mode 3: i32 [B][C][Tp])
  const double* mtab;   // mode 1: per-channel multipliers
  double m;             // mode 0: scalar multiplier
  int lo, hi, mode;
  int pad_;
};

struct PaneP {          // one residual 1x1 conv of a RESADD op
  const int8_t* x;      // [B][cin][Tp]
  const int8_t* w;      // [cout_pad][cin_pad]
  const int32_t* bias;  // [cout_pad]
  const double* m;      // [cout_pad]
  const float* sb;      // [cout_pad]
  int32_t* acc_dbg;     // optional [B][cout][Tp]
  int cin, cin_pad, x_unsigned, pad_;
};

struct EpiP {
  OutP outs[QASR_MAX_OUTS];
  int n_outs;
  unsigned flags;
  const float* sb;        // conv output scale (EXACT_Z, LOGITS)
  const double* m_main;   // RESADD
  const int32_t* lens;    // [B] valid frames in the OUTPUT domain
  int32_t* acc_dbg;       // optional i32 [B][cout][Tp]
  float* logits;          // LOGITS: f32 [B][T][cout]
  int qlo, qhi;
  int T, Tp;              // output frames / row pitch
  int cout, B;
};

struct DwP {              // depthwise conv
  const int8_t* x;        // [B][C][Tp_in]
  const int8_t* w;        // [C][kpad]
  const int32_t* bias;    // [C_pad] (128*sum(w) for u8 inputs, else 0)
  int C, K, kpad, stride, dilation, padding;
  int T_in, Tp_in, x_unsigned, pad_;
  EpiP e;
};

struct DenseP {           // dense k>1 conv as implicit GEMM (+ residual panes)
  const int8_t* x;        // [B][cin][Tp_in]
  const int8_t* w;        // [cout_pad][K][cin_pad]
  const int32_t* bias;
  int cin, cin_pad, K, stride, dilation, padding;
  int T_in, Tp_in, x_unsigned, n_panes;
  PaneP panes[QASR_MAX_PANES];
  EpiP e;
};

struct SepP {             // fused separable layer: depthwise stencil -> QuantAct -> 1x1 GEMM (+ panes) -> epilogue
  // depthwise stage (absent when K == 0: the 1x1 conv reads `x` directly)
  const int8_t* x;        // [B][cin][Tp]   input of the depthwise conv (or of the 1x1 conv when K == 0)
  const int8_t* wdw;      // [cin][kpad4]
  const int8_t* wdw2;     // [cin][kpad4 + 32]: the same taps behind 8 zero bytes and followed by zeros (MFMA depthwise)
  const int32_t* bias_dw; // [cin_pad]  128*sum(w) for u8 inputs
  const double* m_dw;     // [cin_pad]  requant of the dw accumulator towards the 1x1 conv's QuantAct
  int32_t* dw_acc_dbg;    // optional i32 [B][cin][Tp]
  int dw_lo, dw_hi;       // clamp of that QuantAct
  int K, x_unsigned;      // taps (stride 1, 'same' padding)
  int dilation, tile;     // dilation 1, or 2 (window staged de-interleaved by parity); tile: frames per work-group, 32 or 64
  // pointwise stage
  const int8_t* w;        // [cout_pad][cin_pad]
  const int32_t* bias;    // [cout_pad]
  int cin, cin_pad, pw_unsigned, n_panes;
  int dense_k, gen;       // dense_k > 1: dense conv with that many taps (K == 0 kernels; `w` tap-major, `dilation` = tap spacing);
                          // gen: 2 = route to k_sep2 where it has the shape (engine default), else k_sep
  long long* prof;        // diagnostics: s_memtime stamps of work-group (0,0,0), wave 0 (qasr_debug_prof)
  int prof_mode;          // 1 (qasr_debug_timeline): every work-group writes {start, end (s_memrealtime, 100 MHz), HW_ID | XCC_ID << 32, shader cycles}
  int prof_cap;           // ... for work-groups below this count (the caller's buffer)
  int etile;              // the engine's tile_frames option (32: built for one step in flight; 64 / 128: several), before per-op adjustments
  int mask_skip;          // k_sep2: route to the k_sep2s instantiations (mask-skip rule; reserved engines, qasr_engine_opts.mask_skip)
  int pair;               // k_sep2: the paired form k_sep2p (two work-groups per tile, 64 frames each; plain 512 -> 512 layers at 128 frames)
  int half;               // k_sep2: a 128-frame op launched as its 64-frame instantiation on grid (B, Tp / 64) (sep_half_ok; never with pair)
  unsigned* pair_flags;   // ... its completion words, 2 per (utterance, tile), zero before the launch: each member adds 1 at its end
  PaneP panes[QASR_MAX_PANES];
  EpiP e;
};

// qasr_dense2.hip: Jasper's plain dense convs (no residual panes) on 128-channel x 256-frame work-groups
bool dense2_takes(const SepP& p);
int launch_dense2(hipStream_t s, const SepP& p);
void dense2_label(const SepP& p, char* buf, size_t cap);

extern long long* g_prof;
extern int g_prof_mode;
extern int g_prof_cap;      // timeline mode: work-groups the buffer holds (4 int64 each)

struct QuantInP {
  const float* x;         // [B][C][T]
  int8_t* out;            // [B][C][Tp]
  const int32_t* lens;
  float inv_scale;
  int lo, hi, C, T, Tp, B;
};

#define QASR_RQ_MAX 8      /* consumers one k_requant launch serves (Jasper's dense residual: up to 11 per stored value) */
struct RequantP {         // stand-alone requant of a stored value towards n_outs consumers (read once)
  const void* in;         // i32 or s8 [B][C][Tp]
  int in_is_i32, n_outs;
  OutP outs[QASR_RQ_MAX];
  const float* sb;
  const int32_t* lens;
  unsigned flags;
  int C, T, Tp, B;
};

void launch_quant_in(hipStream_t s, const QuantInP& p);
void launch_dw(hipStream_t s, const DwP& p);
void launch_dense(hipStream_t s, const DenseP& p);
bool sep_supported(int K, int dilation);
int launch_sep(hipStream_t s, const SepP& p);      // QASR_OK, or QASR_ERR_UNSUPPORTED / QASR_ERR_ARG without launching
void sep_kernel_label(const SepP& p, char* buf, size_t cap);
int sep_tile_for(const SepP& p);
bool sep_pair_ok(const SepP& p);                   // does launch_sep have the paired form (p.pair) for this op?
bool sep_half_ok(const SepP& p);                   // does launch_sep have the halved form (p.half) for this op?
size_t sep_pair_flag_bytes(int B, int Tp);         // completion words of one paired launch
size_t sep_pair_x_bytes(int B, int Tp);            // the former exchange buffer's bytes (qasr_sep_pair_workspace_bytes keeps its values)
int launch_pair_zero(hipStream_t s, unsigned* flags, size_t bytes);   // k_pair_zero: flag words (16-byte granules) back to zero
void launch_requant(hipStream_t s, const RequantP& p);
// frame_score (optional, [rows]): the log-probability of each row's argmax class, bit-identical to logp[row][tokens[row]]
void launch_logsoftmax(hipStream_t s, const float* logits, float* logp, int32_t* tokens, float* frame_score, int rows, int ncls);
// qasr_stem.hip: lengths + first-layer QuantAct + strided depthwise conv + 1x1 conv of block 0 as one launch
bool stem_supported(const QuantInP& qi, const DwP& dw, const SepP& pw);
// stats != nullptr: x holds un-normalised log-mel and normalize_batch runs inside (per-tile sums from frontend_mel_stats)
// pair_flags != nullptr: the launch also zeroes these flag words of the forward's paired ops (16-byte granules), in place of a
// k_pair_zero node
int launch_stem(hipStream_t s, const QuantInP& qi, const DwP& dw, const SepP& pw, const qasr_domain_desc* doms, int n_domains,
                const int32_t* lens_in, int32_t* lens_all, const double* stats = nullptr, int n_stat_tiles = 0, int n_frames = 0,
                unsigned* pair_flags = nullptr, size_t pair_flag_bytes = 0);
// qasr_frontend.hip: k_mel alone (un-normalised log-mel, feat_lens, per-tile statistics [B][tiles][n_mels][2] f64)
#define QASR_MEL_TILE 16
size_t frontend_stats_bytes(int B, int S, int n_mels);
// front-end of a reserved engine's bucket (qasr_ragged.hip): engine-owned staging rows `pitch` samples apart, feature rows
// of T_pad frames (the bucket edge), and the batch's own S / frame count in the device-resident shape block
struct RaggedFront {
  int pitch, T_pad;
  const int32_t* shp;
};
int frontend_mel_stats(hipStream_t s, const float* audio, const int32_t* audio_lens, int B, int S, const float* fb,
                       const float* window, int n_mels, float preemph, int pad_to, float* feats, int32_t* feat_lens,
                       const void* workspace, size_t workspace_bytes, double* stats, int* n_tiles, int* n_frames,
                       const RaggedFront* rg = nullptr);
int frontend_mel_planned_ragged(hipStream_t s, const float* audio, const int32_t* audio_lens, int B, int S, const float* fb,
                                const float* window, int n_mels, float preemph, int pad_to, float* feats, int32_t* feat_lens,
                                const void* workspace, size_t workspace_bytes, const RaggedFront& rg);
// qasr_decoder.hip: the decoder's 1x1 conv + log_softmax + argmax (+ the encoded lengths) as one launch
bool decoder_fusable(const SepP& p);
int launch_decoder(hipStream_t s, const SepP& p, float* logp, int32_t* tokens, int32_t* lens_out, bool keep_logits,
                   float* frame_score = nullptr);
// qasr_decoder_wide.hip: the same op for 32 < classes <= QASR_DECW_MAX_CLASSES (k_decw_stats + k_decw_out); `ws` is the plan's
// partial-softmax workspace of decoder_wide_ws_bytes(B, Tp) bytes
#define QASR_DECW_MAX_CLASSES 8192
bool decoder_wide_fusable(const SepP& p);
size_t decoder_wide_ws_bytes(int B, int Tp);
int launch_decoder_wide(hipStream_t s, const SepP& p, float* logp, int32_t* tokens, int32_t* lens_out, bool keep_logits,
                        void* ws, size_t ws_bytes, float* frame_score = nullptr);
// qasr_ctc.hip: greedy CTC collapse of a token matrix (k_ctc), one work-group per utterance
// t_act (reserved engines, device): the batch's own frame count; rows keep the pitch T
int launch_ctc(hipStream_t s, const int32_t* tokens, const float* frame_score, const int32_t* lens, int B, int T, int blank,
               const qasr_ctc_out& out, const int32_t* t_act = nullptr);
// qasr_beam.hip: CTC prefix beam search (k_topn, k_beam); the arguments are checked by the callers in qasr_engine.hip
int launch_topn(hipStream_t s, const qasr_ctc_topn_args& a);
size_t beam_workspace_bytes(int B, int T, int W);
int launch_beam(hipStream_t s, const qasr_ctc_beam_args& a);
int launch_beam_lm(hipStream_t s, const qasr_ctc_beam_lm_args& a);      // k_beam_lm: the search with an n-gram model
int launch_beam_boost(hipStream_t s, const qasr_ctc_beam_boost_args& a);      // k_beam_boost (qasr_beam_boost.hip): phrase boosting, with or without a model
// qasr_align.hip: CTC forced alignment and transcript scoring (k_align); the arguments are checked by qasr_ctc_align
size_t align_workspace_bytes(int P, int T, int max_labels);
int launch_align(hipStream_t s, const qasr_ctc_align_args& a);
// qasr_post.hip: CTC posteriors along an alignment (k_post); the arguments are checked by qasr_ctc_post
size_t post_workspace_bytes(int P, int T);
int launch_post(hipStream_t s, const qasr_ctc_post_args& a);
// qasr_align_band.hip: banded CTC alignment of long recordings (k_align_band); the arguments are checked by qasr_ctc_align_band
size_t align_band_workspace_bytes(int P, int T, int band_states);
int launch_align_band(hipStream_t s, const qasr_ctc_align_band_args& a);
// qasr_post_band.hip: CTC posteriors inside the band of a banded alignment (k_post_band); checked by qasr_ctc_post_band
size_t post_band_workspace_bytes(int P, int T);
int launch_post_band(hipStream_t s, const qasr_ctc_post_band_args& a);
// qasr_star.hip: the wildcard's emission plane (k_star); the arguments are checked by qasr_ctc_star
int launch_star(hipStream_t s, const qasr_ctc_star_args& a);
// qasr_spot.hip: keyword spotting (k_spot); the arguments are checked by qasr_ctc_spot
int launch_spot(hipStream_t s, const qasr_ctc_spot_args& a);
// qasr_edit.hip: word and character error counts (k_edit_cut, k_edit, k_edit_totals); checked by qasr_edit_distance
size_t edit_workspace_bytes(long long P, int max_hyp, int max_ref, int mode);
int launch_edit(hipStream_t s, const qasr_edit_args& a);
// the edit path (k_edit_cut, k_edit_trace); checked by qasr_edit_trace
size_t edit_trace_workspace_bytes(long long P, int max_hyp, int max_ref, int mode);
int launch_edit_trace(hipStream_t s, const qasr_edit_trace_args& a);
// k_edit_cut over P n-best rows without reference rows: (units, state) per row into info, in word mode the words into rec [P][HU]
void launch_edit_cut_rows(hipStream_t s, int mode, const int32_t* rows, const int32_t* lens, const int32_t* n_hyps,
                          const uint8_t* is_space, int2* info, int4* rec, long long pitch, long long HU, int P, int K, int C,
                          int width);
// qasr_mbr.hip: minimum Bayes risk re-ranking of n-best rows (k_edit_cut, k_mbr_pair, k_mbr_pick); checked by qasr_ctc_mbr
size_t mbr_workspace_bytes(int B, int K, int max_ids, int mode);
int launch_mbr(hipStream_t s, const qasr_mbr_args& a);
// qasr_resample.hip: rational polyphase resampler (k_resample); the arguments are checked by qasr_resample
int launch_resample(hipStream_t s, const qasr_resample_args& a);
// qasr_longform.hip: windows of long recordings cut (k_cut) and stitched (k_stitch); the arguments are checked by the callers
int launch_longform_cut(hipStream_t s, const qasr_longform_cut_args& a);
int launch_longform_stitch(hipStream_t s, const qasr_longform_stitch_args& a);
// qasr_stream.hip: streaming state, windows and the incremental collapse (k_stream_push / _window / _emit); checked by the callers
size_t stream_state_bytes(int S, int Wl, int C);
int launch_stream_push(hipStream_t s, const qasr_stream_push_args& a);
int launch_stream_window(hipStream_t s, const qasr_stream_window_args& a);
int launch_stream_emit(hipStream_t s, const qasr_stream_emit_args& a);
// qasr_stream_beam.hip: the streaming beam search (k_stream_beam<LM>); checked by qasr_stream_beam
size_t stream_beam_state_bytes(int S, int W, int F);
int launch_stream_beam(hipStream_t s, const qasr_stream_beam_args& a);
// qasr_stream_beam_boost.hip: the streaming beam search with phrase boosting (k_stream_beam_boost<LM>); checked by qasr_stream_beam_boost
size_t stream_beam_boost_state_bytes(int S, int W, int F);
int launch_stream_beam_boost(hipStream_t s, const qasr_stream_beam_boost_args& a);
// qasr_stream_ep.hip: streaming endpointing (k_stream_endpoint); checked by qasr_stream_endpoint
size_t stream_ep_state_bytes(int S);
int launch_stream_endpoint(hipStream_t s, const qasr_stream_endpoint_args& a);
// qasr_stream_spot.hip: streaming keyword spotting (k_stream_spot<NS>); checked by qasr_stream_spot
size_t stream_spot_state_bytes(int S, int K, int max_labels);
int launch_stream_spot(hipStream_t s, const qasr_stream_spot_args& a);
// qasr_stream_beam_ep.hip: the streaming beam search finalised and reset at cuts (k_stream_beam_ep<LM, BOOST>); checked by qasr_stream_beam_ep
int launch_stream_beam_ep(hipStream_t s, const qasr_stream_beam_ep_args& a);
// qasr_stream_rs.hip: streaming at any sample rate (k_stream_rs_append, k_stream_rs_fir); checked by qasr_stream_rs_push
size_t stream_rs_state_bytes(int S, int hcap);
size_t stream_rs_work_bytes(int B);
int launch_stream_rs_push(hipStream_t s, const qasr_stream_rs_push_args& a);
// qasr_ragged.hip: the bucket policy of reserved engines and their one eager launch per call (k_ragged_stage)
#define QASR_RAGGED_TILE 128          /* every bucket edge is a multiple of the largest frame tile */
#define QASR_SHAPE_B 0                /* shape block, i32: rows of the batch, */
#define QASR_SHAPE_S 1                /* its padded sample count (0: feature entry), */
#define QASR_SHAPE_NF 2               /* STFT frames 1 + S / hop, */
#define QASR_SHAPE_DOM 4              /* and from here its frame count per time domain */
#define QASR_SHAPE_MAXDOM 12
#define QASR_SHAPE_WORDS (QASR_SHAPE_DOM + QASR_SHAPE_MAXDOM)
int ragged_bucket(int max_frames, int max_graphs, int T);
struct RaggedStageP {
  const float* src;         // the caller's [B][row] floats (audio: row = S; features: row = n_mels x T as n_rows rows of T)
  float* dst;               // staging
  const int32_t* lens_in;   // [B]
  int32_t* lens_out;        // [max_batch]: rows >= B get 0
  int32_t* shp;             // shape block
  int B, max_batch;
  int row, src_pitch, dst_pitch, n_rows;   // floats per row; n_rows rows per utterance (1 / n_mels)
  int shape[QASR_SHAPE_WORDS];
};
int launch_ragged_stage(hipStream_t s, const RaggedStageP& p);
void launch_lens(hipStream_t s, const int32_t* lens_in, int32_t* lens_all, const qasr_domain_desc* doms,
                 int n_domains, int B);

}  // namespace qasr
