/*
 * qasr.h — C ABI of the MI355X integer-only ASR engine (libqasr_hip.so).
 *
 * The reference (kssteven418/Q-ASR) has no FFI: its boundary for this path is the Python
 * nn.Module API (QuantAct / QuantConv1d / ConvASREncoder / ConvASRDecoder / EncDecCTCModel).
 * This header is the native surface that sits directly under that API; each
 * entry point names the reference interface it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only; the caller owns every device buffer it passes;
 * the engine owns its packed blob copy and scratch arena; every call returns an int status
 * (QASR_OK == 0) and never throws; one engine per device, not thread-safe; work is enqueued on
 * the caller's HIP stream (passed as void*) with no host synchronisation unless stated.
 */
#ifndef QASR_H
#define QASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QASR_OK 0
#define QASR_ERR_ARG 1        /* bad argument / shape */
#define QASR_ERR_BLOB 2       /* malformed packed model */
#define QASR_ERR_HIP 3        /* HIP runtime error (see qasr_last_error) */
#define QASR_ERR_UNSUPPORTED 4

#define QASR_BLOB_MAGIC 0x52534151u /* "QASR" */
#define QASR_BLOB_VERSION 6u

/* ---- packed model ("blob") layout, produced by qasr/pack.py --------------------------------
 * header | tensor table | op table | data (int8 weights, int32 biases, f64 requant multipliers,
 * f32 scales).  All offsets are bytes from the start of the blob; data items are 16-B aligned. */
typedef struct qasr_blob_header {
  uint32_t magic, version;
  uint32_t n_tensors, n_ops;
  uint32_t feat_in;          /* mel bins entering the encoder */
  uint32_t n_classes;        /* decoder outputs incl. blank */
  uint32_t weight_bit, act_bit;
  uint32_t n_domains, reserved;
  uint64_t tensors_off, ops_off, domains_off, data_off, total_bytes;
} qasr_blob_header;

/* A time domain: every tensor of a domain has the same frame count T and per-utterance lengths.
 * Domain 0 is the encoder input; a strided conv opens a new one with
 * len' = (len + 2*padding - dilation*(kernel-1) - 1)/stride + 1   (MaskedConv1d.get_seq_len, jasper.py:170-173). */
typedef struct qasr_domain_desc {
  int32_t parent;              /* -1 for domain 0 */
  uint32_t kernel, stride, dilation, padding;
  uint32_t reserved[3];
} qasr_domain_desc;

/* dtype of an activation tensor stored as [B][C][Tp] (time contiguous, Tp = T rounded up to 64) */
enum { QASR_DT_S8 = 0, QASR_DT_U8 = 1, QASR_DT_F32 = 2, QASR_DT_I32 = 3 };

typedef struct qasr_tensor_desc {
  uint32_t channels;
  uint32_t dtype;
  uint32_t domain;
  uint32_t reserved;
  int32_t producer;          /* op index that writes it, -1 for the network input */
  int32_t last_use;          /* last op index that reads it */
} qasr_tensor_desc;

enum {
  QASR_OP_QUANT_IN = 0,      /* QuantAct first layer: f32 features -> s8 (quant_modules.py:180-184) */
  QASR_OP_DW = 1,            /* depthwise QuantConv1d + next QuantAct requant (jasper.py:569-583) */
  QASR_OP_PW = 2,            /* 1x1 QuantConv1d (+ residual 1x1 convs + res_act) + next QuantAct requant */
  QASR_OP_DENSE = 3,         /* dense k>1 QuantConv1d (Jasper) (+ residual panes) */
  QASR_OP_LOGSOFTMAX = 4,    /* log_softmax + argmax over classes (conv_asr.py:275, ctc_models.py:405) */
  QASR_OP_REQUANT = 5        /* stand-alone QuantAct requant of a stored s8 / i32 value (extra consumers) */
};

enum {
  QASR_F_RELU = 1u << 0,        /* ReLU on the conv output before requantisation (jasper.py:661,687) */
  QASR_F_MASK_OUT = 1u << 1,    /* write 0 for t >= len[b]: the consumer's MaskedConv1d mask (jasper.py:177-181) */
  QASR_F_EXACT_Z = 1u << 2,     /* |acc| may reach 2^22: take z through the float32 round trip (quant_utils.py:187) */
  QASR_F_LOGITS = 1u << 3,      /* decoder: emit f32 logits = fl32(fl32(acc)*s_b) as [B][T][C] */
  QASR_F_RESADD = 1u << 4,      /* res_act: q = clamp(rq(main) + rq(pane) ...) sequentially over panes */
  QASR_F_TAPMAJOR = 1u << 5,    /* DENSE op (stride 1, 'same' padding): weights stored as one MFMA-fragment-ordered
                                   [cout_pad][cin_pad] matrix per tap; runs on the k_sep tile kernel */
  QASR_F_WIDE_RQ = 1u << 6,     /* some |acc * m| of this op may reach 2^30 (a QuantAct calibrated on near-silence): the
                                   requantisation must clamp in the double domain (k_sep), not on the low word (k_sep2) */
  QASR_F_W6PACK = 1u << 7       /* weights of this op and of its panes are stored sub-byte (weight_bit <= 6): 4 two's-
                                   complement 6-bit codes per 3 bytes (b0 = c0 | c1 << 6, b1 = c1 >> 2 | c2 << 4,
                                   b2 = c2 >> 4 | c3 << 2), element order unchanged; DW ops then carry no zero-margined
                                   tap array (m_off = 0).  qasr_engine_create expands them to int8 on the device */
};

#define QASR_MAX_PANES 12
#define QASR_MAX_OUTS 3

typedef struct qasr_pane {     /* one residual 1x1 conv feeding res_act (jasper.py:664-682) */
  int32_t in;                  /* tensor id (u8, already requantised for this conv's QuantAct) */
  uint32_t cin;
  uint64_t w_off;              /* s8, MFMA fragment order like the main 1x1 weights */
  uint64_t bias_off;           /* i32 [cout], includes the +128*sum(W) correction for u8 inputs */
  uint64_t m_off;              /* f64 [cout]: s_b[c] / S  as m*2^-e (batch_frexp) */
  uint64_t sb_off;             /* f32 [cout]: conv output scale (only read with QASR_F_EXACT_Z) */
} qasr_pane;

typedef struct qasr_out {      /* one consumer of the op's integer result */
  int32_t tensor;              /* tensor id, -1 = unused */
  int32_t lo, hi;              /* clamp range of the consumer's QuantAct */
  uint32_t mode;               /* 0: scalar multiplier `m`; 1: per-channel table at m_off (f64[cout]);
                                  2: identity copy of the integer result; 3: raw int32 accumulator */
  uint64_t m_off;
  double m;
} qasr_out;

typedef struct qasr_op_desc {
  uint32_t kind, flags;
  int32_t in;                  /* main input tensor */
  uint32_t cin, cout, kernel, stride, dilation, padding;
  uint32_t n_panes;
  uint64_t w_off;              /* s8 weights: DW [c][kpad4]; PW cout_pad x cin_pad in MFMA fragment order (see
                                  qasr_pw_conv_acc); DENSE [cout_pad][k][cin_pad] */
  uint64_t bias_off;           /* i32 [cout] (0 = none) */
  uint64_t m_off;              /* RESADD: f64 [cout] multiplier of the main accumulator towards S;
                                  DW ops: s8 [cout][kpad4 + 32], the taps again behind 8 zero bytes and followed by zeros
                                  (per-lane pre-shifted tap streams of the MFMA depthwise stage) */
  uint64_t sb_off;             /* f32 [cout] conv output scale s_w[c]*s_x */
  int32_t qlo, qhi;            /* RESADD clamp of res_act */
  float in_inv_scale;          /* QUANT_IN: fl32(1/s) ; int32 range in qlo/qhi */
  uint32_t reserved;
  qasr_out outs[QASR_MAX_OUTS];
  qasr_pane panes[QASR_MAX_PANES];
} qasr_op_desc;

/* Host-only validation of a packed model (no GPU is touched): QASR_OK, or QASR_ERR_BLOB with a message in `err` (may be
 * NULL) when the header, a table entry or any data offset + extent an op refers to falls outside the blob, an index is
 * out of range, an op's output mode does not match its tensor's element size, or operand time domains disagree.  The
 * reference's loader is unchecked (nemo/core/classes/modelPT.py:379-400); here a blob may have travelled over RCCL
 * (qasr/dist.py) and every field ends up in a kernel argument.  qasr_engine_create[_ex] runs it first. */
int qasr_blob_check(const void* blob, size_t blob_bytes, char* err, size_t err_cap);

/* ---- engine -------------------------------------------------------------------------------- */
typedef struct qasr_engine qasr_engine;

/* Build an engine from a packed model.  Replaces model construction + `qm.evaluate(model)` state:
 * EncDecCTCModel.__init__ / encoder.bn_folding / calibrated QuantAct ranges
 * (nemo/collections/asr/models/ctc_models.py:91-147, examples/asr/quantization/inference.py:105-136).
 * `debug` bit 0 keeps every intermediate tensor and int32 accumulator alive for qasr_engine_read_*;
 * bit 1 only records one HIP event per op on the launch stream (qasr_engine_last_op_ms), no other change;
 * bit 2 (round 1's whole-utterance kernels k_utt) is retired: refused with QASR_ERR_UNSUPPORTED;
 * bit 3 makes k_sep use 64-frame tiles (half the weight / halo traffic per frame and half as many work-groups per
 * launch: faster when several steps are in flight on separate streams, slower for a single step);
 * bit 4 replays the forward as a hipGraph: the second forward with the same shape and the same five buffer pointers is
 * captured, later ones are one hipGraphLaunch (a new pointer set or shape starts over; ignored with bits 0/1).
 * This entry keeps qasr_engine_opts.fuse_norm = 0: qasr_engine_forward_audio leaves the normalised log-mel in `feats`, as in
 * rounds 1 / 2 (the fused normalisation is opt-in through qasr_engine_create_ex, whose default has it on). */
int qasr_engine_create(const void* blob, size_t blob_bytes, int device, int debug, qasr_engine** out);
void qasr_engine_destroy(qasr_engine* e);

/* The same with every launch-plan choice spelled out (what the `debug` bits and, before round 3, environment variables
 * selected).  Tri-state fields: -1 = the engine's default, 0 = off, 1 = on.  `struct_size` = sizeof(qasr_engine_opts) of
 * the caller's header (a shorter, older struct is accepted: missing fields take their defaults; a longer one is refused).
 * Two engines in one process are configured independently of each other through this call.
 * Environment variables remain ONLY as A/B overrides for profiling runs of an unmodified caller, read once per create
 * call AFTER the options: QASR_TILE128=0|1 (128-frame tiles when tile_frames >= 64), QASR_RES_TILE128=0|1 (res_tile128),
 * QASR_RES_TILE=32|64|128 (the block-end tile itself, read after QASR_RES_TILE128; 32 has no option value), QASR_DENSE_TILE128,
 * QASR_SEP_GEN=1|2, QASR_PAIR_SPLIT=0|1 (pair_split), QASR_HALF_TILES=0|1 (the unpaired plain layers of a
 * tile_frames == 128 engine as 64-frame launches, qasr_engine_op_halved; no option field: on below 8 hardware queues by the hint
 * res_tile128 reads), QASR_NO_FUSE, QASR_NO_FUSE_STEM, QASR_NO_FUSE_DEC, QASR_WIDE_TILES, QASR_NO_FUSE_NORM; QASR_SEP2_TUNE is a kernel-internal experiment knob (csrc/qasr_sep2_impl.h). */
typedef struct qasr_engine_opts {
  uint32_t struct_size;
  uint32_t debug;              /* bit 0: keep every tensor + int32 accumulators (parity hooks); bit 1: one HIP event per op */
  int32_t tile_frames;         /* frames per work-group of the separable-layer kernels: 0 (= 32), 32, 64 or 128.  32: one
                                  launch of a 32-utterance batch fills the chip (one step in flight); 128: cheapest frame,
                                  B * Tp / 128 work-groups per launch (several steps in flight) */
  int32_t sep_gen;             /* 0 / 2: k_sep2 where it has the shape; 1: round 1's k_sep everywhere */
  int32_t fuse_dw;             /* depthwise conv fused into the following 1x1 conv's launch */
  int32_t fuse_stem;           /* block 0 (lengths, first-layer QuantAct, strided depthwise, 1x1) as one launch */
  int32_t fuse_decoder;        /* decoder conv + log-softmax + argmax + encoded lengths fused: one launch (k_dec) up to 32
                                  classes, two (k_decw) for 33 .. 8192; 0: the generic k_sep logits + k_logsoftmax */
  int32_t graph;               /* replay the forward as one hipGraph launch (second call with the same buffers captures) */
  int32_t retired_whole_utterance; /* round 1's k_utt kernels, removed in round 4: must be <= 0 */
  int32_t res_tile128;         /* block-end (residual) layers of a tile_frames == 128 engine: 1 = on 128-frame tiles too, 0 = on
                                  64-frame tiles.  Default (-1): by the hardware queues of the process, GPU_MAX_HW_QUEUES read
                                  with getenv per create call as a hint (unset or unparsable: 4, HIP's default): 8 or more - a
                                  queue for each of four streams, four launch chains side by side - 128; fewer - streams share
                                  queues, two chains at a time - 64.  The plain layers stay on tile_frames */
  int32_t dense_tile128;       /* Jasper's plain dense convs on 128-frame tiles when tile_frames >= 64 */
  int32_t retired_legacy_pw;   /* round 1's k_pw, removed in round 4: must be <= 0 */
  int32_t retired_persistent;  /* round 3's persistent per-utterance launch (built, bit-exact, measured slower: DESIGN.md closed
                                  routes), removed in round 4: must be <= 0.  The three retired fields keep the struct layout */
  int32_t fuse_norm;           /* qasr_engine_forward_audio with the fused block 0: normalize_batch folded into k_stem from
                                  per-tile sums k_mel writes (no k_norm launch; `feats` then holds the UN-normalised log-mel) */
  int32_t mask_skip;           /* k_sep2's layers run as k_sep2s: a work-group whose frames all lie at or beyond its utterance's
                                  length stores the zero codes and returns (the same bytes, no work).  Default (-1): on for a
                                  reserved engine (qasr_engine_reserve), off otherwise - the never-taken branch costs the
                                  full-length step 0.14 - 0.28 us per launch */
  int32_t pair_split;          /* the plain 512 -> 512 separable layers of a tile_frames == 128 engine on work-group PAIRS (k_sep2p):
                                  each member serves 64 of the tile's 128 frames over all channels with the 64-frame body, the
                                  members exchange nothing (same bytes, labels and launch count).
                                  Default (-1): by the GPU_MAX_HW_QUEUES hint res_tile128 reads - on below 8 queues (two chains
                                  at a time), off from 8.  Never for debug / timing / reserved engines or other tiles.
                                  QASR_PAIR_SPLIT=0|1 is the A/B override */
} qasr_engine_opts;
/* fills `o` with struct_size and the defaults (-1 / 0) */
void qasr_engine_default_opts(qasr_engine_opts* o);
int qasr_engine_create_ex(const void* blob, size_t blob_bytes, int device, const qasr_engine_opts* opts, qasr_engine** out);

/* Encoder + decoder for one batch, replacing ConvASREncoder.forward + ConvASRDecoder.forward + argmax
 * (nemo/collections/asr/modules/conv_asr.py:194-206,270-275; ctc_models.py:403-405).
 * feats   device f32 [B][feat_in][T]   (the preprocessor's output, time contiguous)
 * lens    device i32 [B]               valid frames per utterance
 * logp    device f32 [B][T'][n_classes] log-probabilities (may be NULL)
 * tokens  device i32 [B][T']           greedy argmax (may be NULL)
 * lens_out device i32 [B]              encoded lengths (may be NULL)
 * T' = qasr_engine_out_frames(e, T).
 * Decoder kernels by width (fuse_decoder on, the default): up to 32 classes k_dec, one launch (decoder input channels a
 * multiple of 256, at most 2048); 33 .. 8192 classes (e.g. QuartzNet15x5Base-Zh's 5207) with at most 2048 decoder input
 * channels k_decw, two launches (per-group softmax statistics, then tokens / lengths and, when logp is
 * not NULL, the log-probabilities), its workspace part of the plan; any other shape, or fuse_decoder = 0: k_sep logits + k_logsoftmax
 * (qasr_engine_op_label names the kernel a plan uses).
 * Tokens are the argmax of the same float32 logits on every path; log-probabilities agree to rounding. */
int qasr_engine_forward(qasr_engine* e, void* stream, const float* feats, const int32_t* lens, int B, int T,
                        float* logp, int32_t* tokens, int32_t* lens_out);
/* The same with the mel front-end in front (qasr_frontend_mel_planned into the caller's `feats` [B][n_mels][T_pad] /
 * `feat_lens` [B] buffers, T_pad = qasr_frontend_frames(S, pad_to)): AudioToMelSpectrogramPreprocessor + encoder +
 * decoder of EncDecCTCModel.forward (ctc_models.py:383-406) as ONE call - and, with graph replay on, one hipGraph launch
 * per batch.  `frontend_plan`: a workspace filled by qasr_frontend_plan for this filterbank.
 * `feats` is working storage of the call: with qasr_engine_opts.fuse_norm (default on where block 0 runs as k_stem) it holds
 * the log-mel BEFORE normalize_batch (features.py:53-67 runs inside k_stem); fuse_norm = 0 leaves the normalised features
 * qasr_frontend_mel returns. */
int qasr_engine_forward_audio(qasr_engine* e, void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                              const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                              const void* frontend_plan, size_t plan_bytes, float* feats, int32_t* feat_lens, float* logp,
                              int32_t* tokens, int32_t* lens_out);
int qasr_engine_out_frames(const qasr_engine* e, int T);
int qasr_engine_num_ops(const qasr_engine* e);
/* kernel launches of the last forward with the current plan: encoder + decoder (80 for QuartzNet15x5 with the default
 * options) plus, after qasr_engine_forward_audio, the front-end's (k_mel; + k_norm when fuse_norm is
 * off: 81 / 82), plus one (k_ctc) while a qasr_ctc_out is attached; -1 before the first forward */
int qasr_engine_num_launches(const qasr_engine* e);

/* Parity hooks (debug engines only; synchronise the stream).  acc: int32 [B][cout][T_out] = the
 * value rint(conv_int) of QuantConv1d.int_conv (quant_modules.py:304) for op `op` (pane < 0: main conv). */
int qasr_engine_read_acc(qasr_engine* e, int op, int pane, int32_t* host_out, size_t n_elems);
/* read_tensor also serves a production (non-debug) engine for a tensor whose arena slot no later tensor reused - e.g.
 * the decoder's input, the final encoder codes - and refuses the others.  Every engine refuses a tensor its launch plan
 * never stores (a depthwise output inside the fused layer's launch, k_stem's intermediates, the float logits inside
 * k_dec / k_decw). */
int qasr_engine_read_tensor(qasr_engine* e, int tensor, void* host_out, size_t n_bytes, int* T_out, int* Tp_out);
/* average device time (ms) per op kind over the last forward, measured with HIP events (debug engines) */
int qasr_engine_last_op_ms(qasr_engine* e, float* ms_per_op, int n_ops);
/* Roofline hook: after a forward, replay each op `reps` times back to back between one pair of HIP events on
 * `stream` and return the average duration per launch in ms (synchronises). */
int qasr_engine_time_ops(qasr_engine* e, void* stream, int reps, float* ms_per_launch, int n_ops);
/* Name of the kernel instantiation op `op` is routed to, with its template arguments as rocprofv3 prints them
 * ("k_sep<75, 1, 1, false>", "k_dw", ...); ops executed inside the next op's launch report "(fused ...)". */
int qasr_engine_op_label(qasr_engine* e, int op, char* buf, size_t cap);
/* Re-enqueue a single op of the last forward's plan (diagnostics / profiling of one layer). */
int qasr_engine_run_op(qasr_engine* e, void* stream, int op);

/* ---- calibration helper -------------------------------------------------------- */

/* The two torch.quantile calls of QuantAct's percentile calibration
 * (nemo/quantization/utils/quant_modules.py:121-125: x_min = quantile(x_act, 1 - p/100), x_max = quantile(x_act, p/100))
 * over a flattened float32 device tensor of n elements (16-byte aligned, finite values): exact order statistics by a
 * 4-pass radix select + torch's float32 linear interpolation.  out2[0] = quantile(q_lo), out2[1] = quantile(q_hi);
 * bit-identical to torch.quantile on the CPU; ranks clamp to n - 1 (n > 2^24, where fl32(n - 1) can round up to n:
 * q = 1 is the maximum).  Enqueued on `stream`; `workspace` (device, qasr_quantile_workspace_bytes()
 * bytes) must stay untouched until the stream has finished. */
size_t qasr_quantile_workspace_bytes(void);
int qasr_quantile2(void* stream, const float* x, size_t n, float q_lo, float q_hi, float* out2, void* workspace,
                   size_t workspace_bytes);

/* ---- greedy CTC decoding on the device ---------------------------------------------------------------------------
 * The loop of WER.ctc_decoder_predictions_tensor (nemo/collections/asr/metrics/wer.py: keep p when
 * (p != previous or previous == blank) and p != blank) as one kernel, k_ctc, with what that loop throws away.
 * Input: tokens i32 [B][T]; frame_score f32 [B][T] (optional): the log-probability of each frame's arg-max class; lens
 * i32 [B] (optional).  Per utterance b, over the frames t < lim, lim = min(lens[b], T) (lens NULL: T, the padded row as
 * the reference walks it): a run is a maximal stretch of equal tokens; every run of a non-blank token emits one label.
 * Outputs (caller-owned device buffers, row pitch T):
 *   labels    i32 [B][T]  the emitted ids in order; entries from n_labels[b] on are `blank`
 *   n_labels  i32 [B]
 *   start     i32 [B][T]  first frame of the run;  nframes i32 [B][T] its length;  tails 0        (each optional)
 *   score     f32 [B][T]  the maximum of frame_score over the run's frames (exact); tail 0        (optional)
 *   utt_score f32 [B]     log-probability of the greedy path = sum of frame_score[b][t], t < lim, in this fixed order:
 *                         part[l] = float32 sum, in increasing t, of the frames with t % 64 == l (from 0.0f); result =
 *                         float32 sum of part[0] .. part[63] in increasing l (from 0.0f).  lim == 0: 0.0f  (optional)
 * score / utt_score need frame_score.  Score maxima are taken in the total order of float32 bit patterns (-0 < +0). */
typedef struct qasr_ctc_out {
  uint32_t struct_size;        /* sizeof(qasr_ctc_out) of the caller's header */
  int32_t* labels;
  int32_t* n_labels;
  int32_t* start;
  int32_t* nframes;
  float* score;
  float* utt_score;
} qasr_ctc_out;
/* Stand-alone operator on any token matrix (one launch on `stream`).  QASR_ERR_ARG (nothing launched): B < 1, T < 1, a
 * NULL tokens / out / labels / n_labels, score or utt_score without frame_score, an unknown struct_size. */
int qasr_ctc_collapse(void* stream, const int32_t* tokens, const float* frame_score, const int32_t* lens, int B, int T,
                      int blank, const qasr_ctc_out* out);
/* Sticky attachment: every later qasr_engine_forward / qasr_engine_forward_audio of this engine also writes
 * `frame_score` (f32 [B][T'], if not NULL: one store per frame from the decoder kernel, bit-identical to
 * logp[b][t][tokens[b][t]] of the same run, no extra launch) and, if `out` is not NULL, runs k_ctc on the call's own
 * tokens after the decoder, on the same stream and inside the captured graph (one more launch; `tokens` must then be
 * non-NULL).  blank = the decoder's last class.  use_lens = 1: stop at the encoded length; 0: walk the padded row like
 * the reference.  The struct is copied; the buffers stay the caller's and must fit the B x T' of the forwards that follow.
 * The attachment is part of the graph key: changing it re-captures, keeping it replays.  Both NULL detaches.
 * QASR_ERR_ARG: a blob without a LOGSOFTMAX op, score / utt_score without frame_score, missing labels / n_labels. */
int qasr_engine_attach_ctc(qasr_engine* e, float* frame_score, const qasr_ctc_out* out, int use_lens);

/* ---- CTC prefix beam search on the device (no language model) ---------------------------------------------------------
 * What ctc_beam_search_decoder of ctc_decoders does without a scorer (the reference's BeamSearchDecoderWithLM with
 * lm_path=None, cutoff_prob=1.0), in fixed point: a log-probability x becomes q = rint(x * 2^16) (clamped to +-2^30, NaN:
 * the floor), scores are int64 sums of them, log 0 is the sentinel -2^62 (never an operand), and log-add-exp is
 * max + table[(max - min) >> 6] (max alone from a difference of 16 * 2^16 on) with the 16384-entry u16 table
 * table[i] = rint(log1p(exp(-(64 i) / 2^16)) * 2^16) the caller builds once and passes in device memory.  The rules, the
 * tie order and the prefix hash are stated in qasr/beam.py, which these kernels follow bit for bit.  Prefix identity ("is p + c
 * already in the beam", "which entry is my parent") is a 64-bit hash of the labels together with the length, not the labels
 * themselves: two different prefixes of one length whose hashes collide would be merged.  Two launches:
 *   k_topn: log_probs f32, utterance b / frame t / class c at log_probs[b * pitch_utt + t * pitch_frame + c]  ->
 *           cand_id i32 [B][T][N], cand_q i32 [B][T][N]: per frame the min(N, C) classes of largest value, best first (order
 *           of the float bit patterns, -0 < +0; ties: lower class first) and their q; the other slots, and every frame
 *           t >= min(lens[b], T), hold -1 / INT32_MIN.  lens may be NULL (the padded row).
 *   k_beam: candidates -> per utterance its final beam, best first: labels i32 [B][n_best][T] (tails and unused rows:
 *           blank), n_labels i32 [B][n_best], score i64 [B][n_best] (fixed point; unused rows -2^62), n_hyps i32 [B].
 *           workspace: qasr_ctc_beam_workspace_bytes(B, T, beam_width) bytes the call may overwrite (the prefix trie);
 *           nothing is allocated and no length is read on the host, so both calls can be captured.
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL among the required pointers,
 * B < 1, T < 1 or T > QASR_BEAM_MAX_FRAMES, B * T >= 2^31, C < 1, N outside 1 .. QASR_BEAM_MAX_CANDIDATES, beam_width
 * outside 1 .. QASR_BEAM_MAX_WIDTH, n_best outside 1 .. beam_width, blank < 0, pitch_frame < C,
 * pitch_utt < T * pitch_frame, lae_entries != QASR_BEAM_TABLE_ENTRIES, a workspace smaller than the query says. */
#define QASR_BEAM_MAX_WIDTH 128
#define QASR_BEAM_MAX_CANDIDATES 64
#define QASR_BEAM_MAX_FRAMES 65536
#define QASR_BEAM_TABLE_ENTRIES 16384
typedef struct qasr_ctc_topn_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t B, T, C, N;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional */
  int32_t* cand_id;
  int32_t* cand_q;
} qasr_ctc_topn_args;
int qasr_ctc_topn(void* stream, const qasr_ctc_topn_args* args);
typedef struct qasr_ctc_beam_args {
  uint32_t struct_size;
  int32_t B, T, N, beam_width, n_best, blank;
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  const int32_t* cand_id;
  const int32_t* cand_q;
  const int32_t* lens;         /* optional */
  const uint16_t* lae_table;
  void* workspace;
  size_t workspace_bytes;
  int32_t* labels;
  int32_t* n_labels;
  int64_t* score;
  int32_t* n_hyps;
} qasr_ctc_beam_args;
size_t qasr_ctc_beam_workspace_bytes(int B, int T, int beam_width);
int qasr_ctc_beam(void* stream, const qasr_ctc_beam_args* args);

/* ---- CTC prefix beam search with a back-off n-gram language model --------------------------------------------------------
 * The search above with the shallow fusion of ctc_decoders' Scorer, in fixed point: every extension of a prefix by a label
 * adds term = ((raw * alpha_q + 2^15) >> 16) + beta_q, raw = the model's log-probability of the token that the label
 * completes (character mode: the label itself; word mode, space >= 0: the word that a space ends) in units of 2^-16 nat,
 * walked through the packed model of qasr/ngram.py (context nodes with back-offs, an open-addressed transition table, a
 * word-hash table).  The rules are LM_RULES of qasr/beam.py, which k_beam_lm follows bit for bit.  lm_score i64 [B][n_best]
 * receives each hypothesis' sum of terms (unused rows 0); score includes it.
 * qasr_lm_check validates a packed model ON THE HOST (no GPU is touched): QASR_OK, or QASR_ERR_BLOB (qasr_last_error names
 * the field) for a bad magic, version, size, order (1 .. QASR_LM_MAX_ORDER) or mode, an n_labels other than the caller's, a
 * capacity that is no power of two, a probe bound outside 1 .. QASR_LM_MAX_PROBE, level offsets that do not ascend, a
 * node / word / next index out of range, a value beyond +-2^30, a suffix that does not lie exactly one level below its node,
 * or a stored key that its probe sequence does not reach.  The kernel trusts `lm`: pass only the bytes that passed.
 * qasr_ctc_beam_lm: QASR_ERR_ARG with nothing launched and no output written for everything qasr_ctc_beam refuses, and
 * for a NULL or unaligned (16 bytes) lm, lm_bytes < 128, alpha_q outside 0 .. 16 * 2^16, |beta_q| > 16 * 2^16,
 * space < -1 or space == blank, a NULL lm_score. */
#define QASR_LM_MAX_ORDER 6
#define QASR_LM_MAX_PROBE 1024
#define QASR_LM_MAX_WEIGHT (16 << 16)
int qasr_lm_check(const void* blob, size_t bytes, int n_labels);
typedef struct qasr_ctc_beam_lm_args {
  uint32_t struct_size;
  int32_t B, T, N, beam_width, n_best, blank;
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  const int32_t* cand_id;
  const int32_t* cand_q;
  const int32_t* lens;         /* optional */
  const uint16_t* lae_table;
  void* workspace;             /* qasr_ctc_beam_workspace_bytes(B, T, beam_width) */
  size_t workspace_bytes;
  int32_t* labels;
  int32_t* n_labels;
  int64_t* score;
  int32_t* n_hyps;
  const void* lm;              /* device memory: a packed model that passed qasr_lm_check */
  size_t lm_bytes;
  int32_t alpha_q, beta_q;     /* rint(alpha * 2^16), rint(beta * 2^16) */
  int32_t space;               /* the label that ends a word; -1: character mode (must agree with the model's mode) */
  int32_t reserved;
  int64_t* lm_score;
} qasr_ctc_beam_lm_args;
int qasr_ctc_beam_lm(void* stream, const qasr_ctc_beam_lm_args* args);

/* ---- CTC prefix beam search with phrase boosting ("hot words") -----------------------------------------------------------
 * The search above, with or without the n-gram model, biased towards a caller-supplied list of phrases: every extension of
 * a prefix by a label moves an automaton over the compiled phrases from state s to s' = delta(s, label) and adds
 * pot[s'] - pot[s] + bank[s'] (units of 2^-16 nat) where the model's term goes; after the last frame every entry takes a
 * virtual space (whole words), loses the pot of its unfinished match and the beam is re-ordered once.  The rules are
 * BOOST_RULES of qasr/boost.py, which k_beam_boost follows bit for bit; the packed set (qasr.boost.PhraseSet.pack) is a
 * 128-byte header (magic 'QBS1', version, total bytes, n_nodes, n_labels, start state, whole_words, table capacity, probe
 * bound, zeros), an open-addressed table of (node, label, next, 0) slots, nodes (pot_q, bank_q) and the dense root row.
 * boost_score i64 [B][n_best] receives each hypothesis' sum of boost terms (unused rows 0); score includes it, lm_score
 * stays the model's share alone.
 * qasr_boost_check validates a packed set ON THE HOST (no GPU is touched): QASR_OK, or QASR_ERR_BLOB (qasr_last_error names
 * the field) for a bad magic, version or size, an n_labels other than the caller's, a capacity that is no power of two, a
 * probe bound outside 1 .. QASR_LM_MAX_PROBE, a start state, node, label or next out of range, a pot or bank outside
 * 0 .. 2^30, a non-zero reserved word, or a stored key that its probe sequence does not reach.  The kernel trusts `boost`.
 * qasr_ctc_beam_boost: lm == NULL searches without a model (alpha_q, beta_q and lm_score are then ignored; space is still
 * needed for whole words).  QASR_ERR_ARG with nothing launched and no output written for everything qasr_ctc_beam_lm refuses
 * (the model's own fields only with a model), and for a NULL or unaligned (16 bytes) boost, boost_bytes < 128, a NULL
 * boost_score, whole_words != 0 with space < 0, space < -1 or space == blank.  whole_words must repeat the header's flag (the
 * header lies in device memory, which this call does not read): a disagreement, like a header that does not fit
 * boost_bytes, ends the search empty (n_hyps 0).  Workspace: qasr_ctc_beam_workspace_bytes, unchanged. */
#define QASR_BOOST_MAX_PHRASE 64
int qasr_boost_check(const void* blob, size_t bytes, int n_labels);
typedef struct qasr_ctc_beam_boost_args {
  uint32_t struct_size;
  int32_t B, T, N, beam_width, n_best, blank;
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  const int32_t* cand_id;
  const int32_t* cand_q;
  const int32_t* lens;         /* optional */
  const uint16_t* lae_table;
  void* workspace;             /* qasr_ctc_beam_workspace_bytes(B, T, beam_width) */
  size_t workspace_bytes;
  int32_t* labels;
  int32_t* n_labels;
  int64_t* score;
  int32_t* n_hyps;
  const void* lm;              /* device memory: a packed model that passed qasr_lm_check, or NULL: no model */
  size_t lm_bytes;
  int32_t alpha_q, beta_q;
  int32_t space;               /* the label that ends a word, -1: none (with a model: must agree with its mode) */
  int32_t whole_words;         /* the whole_words flag of the set's header */
  int64_t* lm_score;           /* with a model */
  const void* boost;           /* device memory: a packed phrase set that passed qasr_boost_check */
  size_t boost_bytes;
  int64_t* boost_score;
} qasr_ctc_beam_boost_args;
int qasr_ctc_beam_boost(void* stream, const qasr_ctc_beam_boost_args* args);

/* ---- CTC forced alignment and transcript scoring ---------------------------------------------------------------------
 * For a GIVEN label sequence: its best alignment against the log-probabilities (Viterbi: per label the first frame, the
 * frame count and the best frame log-probability of its run, the outputs of k_ctc for a text instead of the arg-max) and
 * its CTC log-likelihood over all alignments (forward), in the fixed point of the beam search above: q = rint(x * 2^16),
 * int64 sums, log 0 = -2^62, log-add-exp through the caller's table.  The rules (states, predecessors, the tie order
 * stay < s-1 < s-2, the order of the two log-add-exps, the end states) are RULES of qasr/align.py, which k_align follows
 * bit for bit.  Problem p < P aligns targets[p][0 .. target_lens[p]) against utterance p / K (K problems per utterance:
 * the n-best rows of a beam, K = 1 for one transcript each).  max_labels is the row pitch of targets and of the per-label
 * outputs, at most QASR_ALIGN_MAX_LABELS; a longer target is not alignable.
 *   start, nframes i32 [P][max_labels], score f32 [P][max_labels]: the label's run (tails 0); path_score i64 [P]: the best
 *   alignment's score; total i64 [P]: the log-likelihood (both / 2^16 = nats); ok i32 [P].  Every output but ok is optional;
 *   without total the forward pass is skipped and no table is needed.
 * Not alignable - ok 0, the rows 0, path_score = total = -2^62: fewer frames than labels plus adjacent repeats, no frames
 * for a non-empty target, target_lens outside 0 .. max_labels, a label outside [0, C) or equal to blank.  Targets are device
 * data: the kernel checks them itself and reads nothing through a bad label.
 * workspace: qasr_ctc_align_workspace_bytes(P, T, max_labels) bytes the call may overwrite (backpointers, 2 bits per frame
 * and state); nothing is allocated and no length is read on the host, so the call can be captured.
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL among log_probs, targets,
 * target_lens, workspace, ok; B, T, C or K < 1, P != B * K, T > QASR_BEAM_MAX_FRAMES, max_labels outside
 * 1 .. QASR_ALIGN_MAX_LABELS, blank outside [0, C), pitch_frame < C, pitch_utt < T * pitch_frame, total without lae_table, a
 * lae_table with lae_entries != QASR_BEAM_TABLE_ENTRIES, a workspace smaller than the query says, a star_logp with
 * star_pitch < T.
 * star_logp / star_pitch (the wildcard, see qasr_ctc_star below): f32 [B][star_pitch], one row per utterance.  With a plane
 * the label id C is a valid target label whose log-probability at frame t is star_logp[u][t] wherever logp[u][t][c] is read
 * (emission, score); NULL: id C is a label outside [0, C) as before.  struct_size may be the size of the struct without
 * these two fields (QASR_CTC_ALIGN_ARGS_V1_SIZE): they then count as absent and the call is the one it was. */
#define QASR_ALIGN_MAX_LABELS 2048
typedef struct qasr_ctc_align_args {
  uint32_t struct_size;
  int32_t B, T, C, P, K, blank, max_labels;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  const int32_t* targets;      /* [P][max_labels] */
  const int32_t* target_lens;  /* [P] */
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES (with lae_table) */
  uint32_t reserved;
  const uint16_t* lae_table;   /* required only with total */
  void* workspace;
  size_t workspace_bytes;
  int32_t* start;              /* optional */
  int32_t* nframes;            /* optional */
  float* score;                /* optional */
  int64_t* path_score;         /* optional */
  int64_t* total;              /* optional */
  int32_t* ok;
  const float* star_logp;      /* optional [B][star_pitch]: the wildcard's plane */
  int64_t star_pitch;          /* in floats, >= T (with star_logp) */
} qasr_ctc_align_args;
#define QASR_CTC_ALIGN_ARGS_V1_SIZE offsetof(qasr_ctc_align_args, star_logp)
size_t qasr_ctc_align_workspace_bytes(int P, int T, int max_labels);   /* 0 for a shape qasr_ctc_align refuses */
int qasr_ctc_align(void* stream, const qasr_ctc_align_args* args);

/* ---- CTC posteriors along an alignment (forward-backward) -----------------------------------------------------------------
 * How much of the transcript's probability mass agrees with the alignment qasr_ctc_align found: for every frame t < lens the
 * log-posterior g(t) = A(t, s_t) + Bk(t, s_t) - q(t, s_t) - total of the path's state s_t, where A is the forward row of
 * qasr_ctc_align, Bk the backward row over the same lattice and total the log-likelihood, all in the same fixed point and with
 * the same table.  The rules (successors, the order of the two log-add-exps, the path read from start / nframes, what makes a
 * row valid) are POST_RULES of qasr/align.py, which k_post follows bit for bit.  Problems, K, max_labels, the wildcard plane
 * and the checks of the target are those of qasr_ctc_align.
 *   start, nframes i32 [P][max_labels], ok_in i32 [P] (optional: NULL counts as all 1): the outputs of qasr_ctc_align for the
 *   same inputs.  They are device data: the kernel checks that they describe a CTC alignment of the target over lens frames
 *   (runs in order, none empty, a blank frame between equal neighbours, the last run inside lens) and only ever compares them
 *   with frame numbers, so garbage in them reads and writes nothing out of bounds.
 *   frame_post i32 [P][post_pitch]: g(t) clamped to [-2^30, 0] (/ 2^16 = nats) for t < lens, 0 for lens <= t < T (columns
 *   T .. post_pitch are not written); label_post i32 [P][max_labels]: the minimum of frame_post over the label's run (tails 0);
 *   total i64 [P] (optional): equal to qasr_ctc_align's on every byte; ok i32 [P].
 * ok 0 - frame_post and label_post rows 0, total -2^62: ok_in 0, a target qasr_ctc_align does not align, start / nframes that
 * are not an alignment of it.
 * workspace: qasr_ctc_post_workspace_bytes(P, T) = P * T * 8 bytes, 8-byte aligned, that the call may overwrite (the forward
 * score along the path); nothing is allocated and no length is read on the host, so the call can be captured, also right
 * behind the qasr_ctc_align whose outputs it reads.
 * QASR_ERR_ARG with nothing launched and no output written: what qasr_ctc_align refuses (an unknown struct_size, a NULL among
 * log_probs, targets, target_lens, workspace, ok; B, T, C or K < 1, P != B * K, T > QASR_BEAM_MAX_FRAMES, max_labels outside
 * 1 .. QASR_ALIGN_MAX_LABELS, blank outside [0, C), pitch_frame < C, pitch_utt < T * pitch_frame, lae_entries !=
 * QASR_BEAM_TABLE_ENTRIES, a workspace smaller than the query says, a star_logp with star_pitch < T), a NULL among start,
 * nframes, frame_post, label_post, a NULL lae_table, post_pitch < T, a workspace that is not 8-byte aligned. */
typedef struct qasr_ctc_post_args {
  uint32_t struct_size;
  int32_t B, T, C, P, K, blank, max_labels;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  const int32_t* targets;      /* [P][max_labels] */
  const int32_t* target_lens;  /* [P] */
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  uint32_t reserved;
  const uint16_t* lae_table;
  const int32_t* start;        /* [P][max_labels]: qasr_ctc_align's */
  const int32_t* nframes;      /* [P][max_labels]: qasr_ctc_align's */
  const int32_t* ok_in;        /* optional [P]: qasr_ctc_align's ok */
  void* workspace;
  size_t workspace_bytes;
  int32_t* frame_post;         /* [P][post_pitch] */
  int64_t post_pitch;          /* in int32s, >= T */
  int32_t* label_post;         /* [P][max_labels] */
  int64_t* total;              /* optional [P] */
  int32_t* ok;                 /* [P] */
  const float* star_logp;      /* optional [B][star_pitch]: the wildcard's plane */
  int64_t star_pitch;          /* in floats, >= T (with star_logp) */
} qasr_ctc_post_args;
size_t qasr_ctc_post_workspace_bytes(int P, int T);   /* 0 for a shape qasr_ctc_post refuses */
int qasr_ctc_post(void* stream, const qasr_ctc_post_args* args);

/* ---- banded CTC alignment: one long recording against its whole transcript --------------------------------------------
 * k_align above computes every state of every frame and holds 2048 labels and 65 536 frames.  An hour of audio is 180 000
 * frames and some 54 000 characters; k_align_band keeps only a band of band_states = 256, 1024 or 4352 lattice states that
 * follows the alignment (every 32 frames it is re-centred on the lowest state that holds the row's maximum, and never moves
 * back), so the cost is T * band_states cells.  Viterbi only; the fixed point, the predecessors and the tie order are
 * k_align's, the rest is BAND_RULES of qasr/align.py, which the kernel follows bit for bit.  One problem per recording:
 * problem p < B aligns targets[p][0 .. target_lens[p]) against log_probs[p]; max_labels is the row pitch of targets and of the
 * per-label outputs.  While 2 * target_lens[p] + 1 <= band_states the band never moves and every output equals qasr_ctc_align's.
 *   start, nframes i32 [B][max_labels], score f32 [B][max_labels], path_score i64 [B], ok i32 [B]: as in qasr_ctc_align;
 *   frame_logp f32 [B][T]: the log-probability of the path's label at each frame < lens, 0 behind;
 *   band_base i32 [B][ceil(T / 32)]: the lowest state of the band during each 32-frame block (0 behind lens).
 *   Every output but ok is optional.
 * Not alignable - ok 0, the rows and frame_logp 0, path_score -2^62: the reasons of qasr_ctc_align (target_lens above
 * QASR_BAND_MAX_LABELS in place of QASR_ALIGN_MAX_LABELS), or the band lost the path (band_base is kept then).  Targets are device
 * data: the kernel checks them itself and reads nothing through a bad label.
 * workspace: qasr_ctc_align_band_workspace_bytes(B, T, band_states) bytes, 4-byte aligned, that the call may overwrite:
 * per problem ceil(T / 4) * band_states bytes of backpointers and 4 T bytes of path states (an hour at 4352: 197 MB).  Nothing is
 * allocated and no length is read on the host, so the call can be captured.
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL among log_probs, targets,
 * target_lens, workspace, ok; B, T or C < 1, T > QASR_BAND_MAX_FRAMES, max_labels outside 1 .. QASR_BAND_MAX_LABELS, band_states
 * not 256, 1024 or 4352, blank outside [0, C), pitch_frame < C, pitch_utt < T * pitch_frame, a workspace that is not 4-byte
 * aligned or smaller than the query says, a star_logp with star_pitch < T.
 * star_logp / star_pitch: the wildcard's plane f32 [B][star_pitch] exactly as in qasr_ctc_align (frame_logp reads it too);
 * struct_size may be QASR_CTC_ALIGN_BAND_ARGS_V1_SIZE, the struct without the two fields. */
#define QASR_BAND_MAX_LABELS (1 << 20)
#define QASR_BAND_MAX_FRAMES (1 << 22)
typedef struct qasr_ctc_align_band_args {
  uint32_t struct_size;
  int32_t B, T, C, blank, max_labels, band_states;
  uint32_t reserved;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  const int32_t* targets;      /* [B][max_labels] */
  const int32_t* target_lens;  /* [B] */
  void* workspace;
  size_t workspace_bytes;
  int32_t* start;              /* optional */
  int32_t* nframes;            /* optional */
  float* score;                /* optional */
  int64_t* path_score;         /* optional */
  float* frame_logp;           /* optional */
  int32_t* band_base;          /* optional */
  int32_t* ok;
  const float* star_logp;      /* optional [B][star_pitch]: the wildcard's plane */
  int64_t star_pitch;          /* in floats, >= T (with star_logp) */
} qasr_ctc_align_band_args;
#define QASR_CTC_ALIGN_BAND_ARGS_V1_SIZE offsetof(qasr_ctc_align_band_args, star_logp)
size_t qasr_ctc_align_band_workspace_bytes(int B, int T, int band_states);   /* 0 for a shape qasr_ctc_align_band refuses */
int qasr_ctc_align_band(void* stream, const qasr_ctc_align_band_args* args);

/* ---- CTC posteriors along a banded alignment (forward-backward inside the band) --------------------------------------------
 * qasr_ctc_post for recordings that only fit qasr_ctc_align_band: k_post_band runs the forward and the backward pass over the
 * cells the band kept - (t, s) with band_base[p][t / 32] <= s < band_base[p][t / 32] + band_states - and over the edges
 * k_align_band's own step uses (a predecessor below the new base does not count), with k_align_band's circular ownership.
 * Every quantity is the restricted lattice's: total is the log-likelihood of the alignments inside the band, a lower bound
 * on the full lattice's; frame_post and label_post have qasr_ctc_post's meaning and fixed point.  The rules are
 * POST_BAND_RULES of qasr/align.py, which the kernel follows bit for bit.  One problem per recording, as in
 * qasr_ctc_align_band; band_states is the width that call ran with.
 *   start, nframes i32 [B][max_labels], ok_in i32 [B] (optional: NULL counts as all 1), band_base i32 [B][ceil(T / 32)]: the
 *   outputs of qasr_ctc_align_band for the same inputs.  They are device data: the kernel checks that start / nframes are a CTC
 *   alignment of the target over lens frames, that band_base is a trajectory k_align_band can produce (starts at 0, never
 *   decreases, moves by less than band_states / 2 per block, stays in [0, max(0, 2 * target_lens + 1 - band_states)]) and that
 *   the path stays inside the band and on its edges, all by comparisons and before anything is read through them.
 *   frame_post i32 [B][post_pitch], label_post i32 [B][max_labels], total i64 [B] (optional), ok i32 [B]: as in qasr_ctc_post.
 * ok 0 - frame_post and label_post rows 0, total -2^62: ok_in 0, a target qasr_ctc_align_band does not align, start / nframes
 * that are not an alignment of it, a band_base row that is no trajectory, a path outside the band.
 * workspace: qasr_ctc_post_band_workspace_bytes(B, T) = B * T * 8 bytes, 8-byte aligned, that the call may overwrite (the
 * forward score along the path); nothing is allocated and no length is read on the host, so the call can be captured, also
 * right behind the qasr_ctc_align_band whose outputs it reads.
 * QASR_ERR_ARG with nothing launched and no output written: what qasr_ctc_align_band refuses (an unknown struct_size, a NULL
 * among log_probs, targets, target_lens, workspace, ok; B, T or C < 1, T > QASR_BAND_MAX_FRAMES, max_labels outside
 * 1 .. QASR_BAND_MAX_LABELS, band_states not 256, 1024 or 4352, blank outside [0, C), pitch_frame < C, pitch_utt < T *
 * pitch_frame, a workspace smaller than the query says, a star_logp with star_pitch < T), what qasr_ctc_post refuses (a NULL
 * among start, nframes, frame_post, label_post, a NULL lae_table, lae_entries != QASR_BEAM_TABLE_ENTRIES, post_pitch < T, a
 * workspace that is not 8-byte aligned), a NULL band_base. */
typedef struct qasr_ctc_post_band_args {
  uint32_t struct_size;
  int32_t B, T, C, blank, max_labels, band_states;
  uint32_t reserved;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  const int32_t* targets;      /* [B][max_labels] */
  const int32_t* target_lens;  /* [B] */
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  uint32_t reserved2;
  const uint16_t* lae_table;
  const int32_t* start;        /* [B][max_labels]: qasr_ctc_align_band's */
  const int32_t* nframes;      /* [B][max_labels]: qasr_ctc_align_band's */
  const int32_t* ok_in;        /* optional [B]: qasr_ctc_align_band's ok */
  const int32_t* band_base;    /* [B][ceil(T / 32)]: qasr_ctc_align_band's */
  void* workspace;
  size_t workspace_bytes;
  int32_t* frame_post;         /* [B][post_pitch] */
  int64_t post_pitch;          /* in int32s, >= T */
  int32_t* label_post;         /* [B][max_labels] */
  int64_t* total;              /* optional [B] */
  int32_t* ok;                 /* [B] */
  const float* star_logp;      /* optional [B][star_pitch]: the wildcard's plane */
  int64_t star_pitch;          /* in floats, >= T (with star_logp) */
} qasr_ctc_post_band_args;
size_t qasr_ctc_post_band_workspace_bytes(int B, int T);   /* 0 for a shape qasr_ctc_post_band refuses */
int qasr_ctc_post_band(void* stream, const qasr_ctc_post_band_args* args);

/* ---- the wildcard ("star") for audio the transcript does not cover -------------------------------------------------------
 * A transcript that omits part of the audio pushes those frames onto the neighbouring labels.  The wildcard is one more
 * label, id C, that the caller puts into the target where text is missing; its log-probability at frame t is not a column of
 * log_probs but star[u][t] = max over c < C of log_probs[u][t][c] - penalty (the maximum in the order k_ctc and k_align take
 * maxima in, one IEEE float32 subtraction) for t < lens[u], 0 behind: the best class of the frame, less a price per frame that
 * keeps the wildcard from eating its neighbours.  qasr_ctc_star (k_star: one wave per frame, log_probs read once) writes that
 * plane; qasr_ctc_align / qasr_ctc_align_band take it as star_logp.  The rules are STAR_RULES of qasr/align.py, which the
 * kernels follow bit for bit: every output equals the call without a plane on log_probs with star as class C of C + 1.
 * Nothing is allocated and no length is read on the host, so the call can be captured.
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL log_probs or star, B, T or C < 1,
 * pitch_frame < C, pitch_utt < T * pitch_frame, star_pitch < T, a penalty that is not finite or outside
 * 0 .. QASR_STAR_MAX_PENALTY. */
#define QASR_STAR_MAX_PENALTY 16.0f
typedef struct qasr_ctc_star_args {
  uint32_t struct_size;
  int32_t B, T, C;
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  float penalty;               /* nats per frame */
  uint32_t reserved;
  float* star;                 /* [B][star_pitch] */
  int64_t star_pitch;          /* in floats, >= T */
} qasr_ctc_star_args;
int qasr_ctc_star(void* stream, const qasr_ctc_star_args* args);

/* ---- keyword spotting: where each of K phrases occurs, and how well it matches ----------------------------------------------
 * K keywords (label sequences, shared by all utterances) against B utterances: problem p = u * K + k.  Each keyword's CTC
 * lattice (the states of qasr_ctc_align, s = 1 .. 2L - 1) runs over the frames with a FREE start and a FREE end: state 0 is
 * the constant fresh start (value 0, start = the frame being entered) and the final state is 2L - 1 only.  The emission is
 * the likelihood ratio against the frame's best class, e(t, s) = min(q(logp[u][t][lab(s)]) - q(star_logp[u][t]), 0), q =
 * rint(x * 2^16) clamped as in the beam search, star_logp the plane of qasr_ctc_star with penalty 0.  One Viterbi row of pairs
 * (D i64, start i32); at frame t a live final state with n = t - start + 1 <= max_span and D >= threshold_q * n is a candidate;
 * one greedy pass in time order keeps one open hit per problem: an overlapping candidate (start <= open.end) replaces it iff
 * its mean is strictly higher (D * n_open > D_open * n), one that does not overlap closes and emits it.  The rules are
 * SPOT_RULES of qasr/spot.py, which k_spot (one wave per problem, no LDS, no barrier in the frame loop) follows bit for bit.
 *   hit_start, hit_end i32 [B * K][max_hits] (inclusive frames), hit_score i64 [B * K][max_hits] (D; / 2^16 / n = nats per
 *   frame): the first max_hits hits in time order, rows behind them 0; n_hits i32 [B * K]: every emitted hit, stored or not;
 *   ok i32 [B * K]: 0, with no hits, for target_lens outside 1 .. min(max_labels, QASR_SPOT_MAX_LABELS), a label outside [0, C)
 *   or equal to blank (targets are device data: the kernel checks them itself and reads nothing through a bad label).
 *   trace_score i64 / trace_start i32 [B * K][trace_pitch] (optional, both or neither): (D, start) of the final state at every
 *   frame < lens (dead: -2^62 / -1), 0 behind and 0 for ok = 0.
 * No workspace; nothing is allocated and no length is read on the host, so the call can be captured.
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL among log_probs, star_logp, targets,
 * target_lens, hit_start, hit_end, hit_score, n_hits, ok; B, T, C or K < 1, T > QASR_BAND_MAX_FRAMES, B * K above 2^31 - 1,
 * max_labels outside 1 .. QASR_SPOT_MAX_LABELS, blank outside [0, C), star_pitch < T, pitch_frame < C, pitch_utt < T *
 * pitch_frame, threshold_q outside QASR_SPOT_MIN_THRESHOLD_Q .. 0, max_span outside 1 .. QASR_SPOT_MAX_SPAN, max_hits < 1, one
 * trace pointer without the other, trace_pitch < T (with a trace). */
#define QASR_SPOT_MAX_LABELS 127
#define QASR_SPOT_MAX_SPAN 65536
#define QASR_SPOT_MIN_THRESHOLD_Q (-(16 << 16))
typedef struct qasr_ctc_spot_args {
  uint32_t struct_size;
  int32_t B, T, C, K, max_labels, blank;
  int32_t threshold_q;         /* fixed point, nats per frame */
  int32_t max_span;            /* frames */
  int32_t max_hits;            /* row pitch of the hit outputs */
  int64_t pitch_utt, pitch_frame;   /* in floats */
  const float* log_probs;
  const int32_t* lens;         /* optional [B] */
  const float* star_logp;      /* [B][star_pitch]: qasr_ctc_star with penalty 0 */
  int64_t star_pitch;          /* in floats, >= T */
  const int32_t* targets;      /* [K][max_labels] */
  const int32_t* target_lens;  /* [K] */
  int32_t* hit_start;          /* [B * K][max_hits] */
  int32_t* hit_end;            /* [B * K][max_hits] */
  int64_t* hit_score;          /* [B * K][max_hits] */
  int32_t* n_hits;             /* [B * K] */
  int32_t* ok;                 /* [B * K] */
  int64_t* trace_score;        /* optional [B * K][trace_pitch] */
  int32_t* trace_start;        /* optional [B * K][trace_pitch] */
  int64_t trace_pitch;         /* in elements, >= T (with a trace) */
} qasr_ctc_spot_args;
int qasr_ctc_spot(void* stream, const qasr_ctc_spot_args* args);

/* ---- word and character error counts: edit distance over label ids -----------------------------------------------------------
 * What word_error_rate (nemo/collections/asr/metrics/wer.py) computes on the host from strings, over the label rows where they
 * lie on the device: hypothesis rows hyp i32 [B * K][hyp_pitch] (max_hyp ids each; hyp_lens i32 [B * K] or NULL) against
 * reference rows ref i32 [B][ref_pitch] (max_ref ids each; ref_lens i32 [B] or NULL); a NULL length vector means the padded
 * row, every id of it.  Problem p = b * K + k scores hypothesis row p against reference row b (K rows per reference: the beam's
 * n-best layout); n_hyps i32 [B] (optional): rows k >= n_hyps[b] are absent.  mode QASR_EDIT_CHAR: a unit is one id;
 * QASR_EDIT_WORD: a unit is a maximal run of ids c with is_space[c] == 0 (is_space u8 [C], the caller's
 * vocabulary[c].isspace()); two words are equal when their id sequences are equal - length and a 64-bit hash are compared first
 * and the ids are verified on a match.  Unit costs; D[0][j] = j deletions, D[i][0] = i insertions; among predecessors of equal
 * cost the diagonal first, then the deletion (i, j - 1), then the insertion (i - 1, j); every cell carries (cost, S, D) of the
 * path this picks.  The rules are EDIT_RULES of qasr/edit.py, which the kernels follow byte for byte.
 *   rows i32 [B * K][8]: errors, S, D, I, ref_units, hyp_units, ok, 0.  ok = 1 scored; 2 an absent row; 0 a length outside
 *   0 .. max_hyp (max_ref) or an id inside the length outside [0, C), in either row (rows are device data: the kernels check
 *   them before any use).  Rows with ok != 1 hold 0 in every count.
 *   totals i64 [16], which the call ADDS to (the caller zeroes it): [0] errors [1] ref_units [2] S [3] D [4] I [5] hyp_units
 *   [6] rows, each over the rows with ok == 1 and k == 0; [7] the n-best oracle: over b, the smallest errors of b's rows with
 *   ok == 1; [8] the number of rows with ok == 0; [9 .. 15] reserved, left as they are.
 * Three launches on `stream`: k_edit_cut (one wave per row: checks, and in word mode the words as (start, len, hash) in the
 * workspace), k_edit<MODE, NC> (one wave per problem, NC = 1 / 4 / 16 reference units per lane from max_ref, references wider
 * than 64 * 16 units in consecutive strips) and k_edit_totals (one work-group; thread w writes totals[w]).  No atomics, plain
 * vector stores, nothing allocated and nothing read on the host, so the call can be captured behind qasr_ctc_collapse or the
 * beam kernels and replayed.  workspace: 16-byte aligned device memory of qasr_edit_workspace_bytes(B * K, max_hyp, max_ref,
 * mode) bytes (0: a shape the call refuses), one per call in flight.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL among hyp, ref, rows, totals and
 * workspace, a mode other than the two, is_space NULL in word mode, B, K or C < 1, B * K above QASR_EDIT_MAX_PROBLEMS, max_hyp or
 * max_ref outside 1 .. QASR_EDIT_MAX_IDS, hyp_pitch < max_hyp, ref_pitch < max_ref, workspace_bytes below the query, a
 * workspace or rows not 16-byte aligned, totals not 8-byte aligned. */
#define QASR_EDIT_CHAR 0
#define QASR_EDIT_WORD 1
#define QASR_EDIT_MAX_IDS (1 << 20)
#define QASR_EDIT_MAX_PROBLEMS (1 << 24)
#define QASR_EDIT_ROW_WORDS 8
#define QASR_EDIT_TOTAL_WORDS 16
typedef struct qasr_edit_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t mode;                /* QASR_EDIT_CHAR / QASR_EDIT_WORD */
  int32_t B, K, C;             /* references, hypothesis rows per reference, classes */
  int32_t max_hyp, max_ref;    /* ids per row */
  int32_t pad_;
  int64_t hyp_pitch, ref_pitch;   /* in int32 */
  const int32_t* hyp;          /* [B * K][hyp_pitch] */
  const int32_t* hyp_lens;     /* optional [B * K] */
  const int32_t* ref;          /* [B][ref_pitch] */
  const int32_t* ref_lens;     /* optional [B] */
  const int32_t* n_hyps;       /* optional [B] */
  const uint8_t* is_space;     /* [C]; word mode */
  int32_t* rows;               /* [B * K][8] */
  int64_t* totals;             /* [16] */
  void* workspace;
  size_t workspace_bytes;
} qasr_edit_args;
size_t qasr_edit_workspace_bytes(int P, int max_hyp, int max_ref, int mode);
int qasr_edit_distance(void* stream, const qasr_edit_args* args);

/* ---- the edit path: which unit became which ----------------------------------------------------------------------------------
 * qasr_edit_distance's rows, units, validity and recurrence, with the path the recurrence picks written out (TRACE_RULES of
 * qasr/edit.py, which k_edit_trace follows byte for byte).  The path runs from cell (hyp_units, ref_units) back to (0, 0): at
 * i == 0 a deletion, at j == 0 an insertion, otherwise the predecessor the cell took - the diagonal first, the deletion
 * (i, j - 1) only when strictly cheaper, the insertion (i - 1, j) only when strictly cheaper than that.
 *   ops u8 [B * K][ops_pitch], in FORWARD order: 0 hit and 1 substitution (one unit of each row), 2 deletion (a reference
 *   unit), 3 insertion (a hypothesis unit).  n_ops i32 [B * K]; bytes at and behind n_ops[p] are left as they are; rows with
 *   ok != 1 have n_ops = 0 and nothing written.  The numbers of codes 1 / 2 / 3 are rows[p][1 / 2 / 3], that of code 0 is
 *   ref_units - S - D, n_ops = ref_units + I <= hyp_units + ref_units.
 *   rows i32 [B * K][8]: qasr_edit_distance's, byte for byte.  There is no totals block: sum with qasr_edit_distance.
 * Two launches on `stream`: k_edit_cut, as above, and k_edit_trace<MODE, NC> (one wave per problem: k_edit's frame step with
 * the choice of every cell, 2 bits, stored step-major to a plane in the workspace, then the walk by the same wave, which
 * reads the plane in blocks and writes the ops to their forward places).  No atomics, plain vector stores, nothing allocated
 * and nothing read on the host: capturable.  ops_pitch >= HU + RU, the unit bounds of the two widths: max_hyp (max_ref) in
 * char mode, (max_hyp + 1) / 2 in word mode.  workspace: 16-byte aligned device memory of
 * qasr_edit_trace_workspace_bytes(B * K, max_hyp, max_ref, mode) bytes (0: a shape the call refuses) - about HU * RU / 4 bytes
 * per problem (64 HU when RU <= 64) -, one per call in flight.
 * QASR_ERR_ARG with nothing launched and nothing written: what qasr_edit_distance refuses (totals aside), ops or n_ops NULL,
 * ops_pitch < HU + RU. */
typedef struct qasr_edit_trace_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t mode;                /* QASR_EDIT_CHAR / QASR_EDIT_WORD */
  int32_t B, K, C;             /* references, hypothesis rows per reference, classes */
  int32_t max_hyp, max_ref;    /* ids per row */
  int32_t pad_;
  int64_t hyp_pitch, ref_pitch, ops_pitch;   /* in int32, int32, bytes */
  const int32_t* hyp;          /* [B * K][hyp_pitch] */
  const int32_t* hyp_lens;     /* optional [B * K] */
  const int32_t* ref;          /* [B][ref_pitch] */
  const int32_t* ref_lens;     /* optional [B] */
  const int32_t* n_hyps;       /* optional [B] */
  const uint8_t* is_space;     /* [C]; word mode */
  int32_t* rows;               /* [B * K][8], = qasr_edit_distance's */
  uint8_t* ops;                /* [B * K][ops_pitch] */
  int32_t* n_ops;              /* [B * K] */
  void* workspace;
  size_t workspace_bytes;
} qasr_edit_trace_args;
size_t qasr_edit_trace_workspace_bytes(int P, int max_hyp, int max_ref, int mode);
int qasr_edit_trace(void* stream, const qasr_edit_trace_args* args);

/* ---- minimum Bayes risk re-ranking of n-best rows -----------------------------------------------------------------------------
 * Among the K rows the beam kernels leave per utterance - labels i32 [B * K][label_pitch] (max_ids ids each), n_labels i32
 * [B * K], score i64 [B * K] in 2^-16 nat, n_hyps i32 [B] (optional) - the order by expected edit distance to the other rows,
 * those weighted by their posterior (MBR_RULES of qasr/mbr.py, which the kernels follow byte for byte).  mode, is_space, units
 * and the equality of words are qasr_edit_distance's.
 *   ok i32 [B * K]: 2 an absent row (k >= n_hyps[b]); 1 a present row: length in 0 .. max_ids, every id inside it in [0, C)
 *   and score > -2^61; 0 otherwise.  Rows with ok != 1 take no part.
 *   weight i32 [B * K]: with smax the largest score of b's present rows, d = min(smax - score, 2^40),
 *   x = (d * scale_q + 2^15) >> 16: 0 when x >= 16 << 16, else wtab[x >> 6]; wtab u32 [QASR_MBR_TABLE_ENTRIES],
 *   wtab[i] = rint(exp(-(64 i) / 2^16) * 2^24) (qasr.mbr.weight_table), in device memory.  0 for rows with ok != 1.
 *   wsum i64 [B]: the sum of b's weights (0: no present row).
 *   dist i32 [B][K][K] (optional; NULL: the matrix lives in the workspace): the unit-cost edit distance between rows i and j,
 *   0 on the diagonal, -1 wherever either row has ok != 1.
 *   risk i64 [B * K]: sum over present j of weight[j] * dist[i][j]; -1 for rows with ok != 1.
 *   order i32 [B * K]: b's present rows by (risk ascending, score descending, k ascending), then -1.
 * Three launches on `stream`: k_edit_cut over the B * K rows, k_mbr_pair<MODE, NC> (one wave per unordered pair of rows of an
 * utterance, NC = 1 / 4 / 16 units per lane from max_ids, longer rows in strips; none for K = 1) and k_mbr_pick (one work-group
 * per utterance).  No atomics, plain vector stores, nothing allocated and nothing read on the host, so the call can be
 * captured behind qasr_ctc_beam[_lm|_boost] and replayed; every output element is written exactly once per call.
 * workspace: 16-byte aligned device memory of qasr_mbr_workspace_bytes(B, K, max_ids, mode) bytes (0: a shape the call
 * refuses), one per call in flight.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL among labels, n_labels, score, wtab,
 * weight, wsum, risk, order, ok and workspace, a mode other than the two, is_space NULL in word mode, B or C < 1, K outside
 * 1 .. QASR_BEAM_MAX_WIDTH, max_ids outside 1 .. QASR_BEAM_MAX_FRAMES, B * K or B * K * (K - 1) / 2 above
 * QASR_EDIT_MAX_PROBLEMS, scale_q outside 0 .. 16 << 16, wtab_entries != QASR_MBR_TABLE_ENTRIES, label_pitch < max_ids,
 * workspace_bytes below the query, a workspace not 16-byte aligned, wsum or risk not 8-byte aligned, dist, weight, order or ok
 * not 4-byte aligned. */
#define QASR_MBR_TABLE_ENTRIES 16384
#define QASR_MBR_MAX_SCALE_Q (16 << 16)
typedef struct qasr_mbr_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t mode;                /* QASR_EDIT_CHAR / QASR_EDIT_WORD */
  int32_t B, K, C;             /* utterances, rows per utterance, classes */
  int32_t max_ids;             /* ids per row */
  int32_t scale_q;             /* rint(scale * 2^16), 0 .. QASR_MBR_MAX_SCALE_Q */
  uint32_t wtab_entries;       /* QASR_MBR_TABLE_ENTRIES */
  int64_t label_pitch;         /* in int32 */
  const int32_t* labels;       /* [B * K][label_pitch] */
  const int32_t* n_labels;     /* [B * K] */
  const int64_t* score;        /* [B * K] */
  const int32_t* n_hyps;       /* optional [B] */
  const uint8_t* is_space;     /* [C]; word mode */
  const uint32_t* wtab;        /* [wtab_entries] */
  int32_t* dist;               /* optional [B][K][K] */
  int32_t* weight;             /* [B * K] */
  int64_t* wsum;               /* [B] */
  int64_t* risk;               /* [B * K] */
  int32_t* order;              /* [B * K] */
  int32_t* ok;                 /* [B * K] */
  void* workspace;
  size_t workspace_bytes;
} qasr_mbr_args;
size_t qasr_mbr_workspace_bytes(int B, int K, int max_ids, int mode);
int qasr_ctc_mbr(void* stream, const qasr_mbr_args* args);

/* ---- audio at any sample rate: rational polyphase resampler and PCM ingest -----------------------------------------------
 * What AudioSegment.__init__ does on the host with librosa.core.resample when target_sr != sample_rate (parts/segment.py:
 * 57-59), as one kernel, k_resample, in front of the mel front-end: int16 PCM (mono or interleaved channels) or float32 at an
 * integer rate sr_in -> float32 mono at the model's rate, with per-utterance lengths.  g = gcd(sr_in, sr_out), L = sr_out / g,
 * M = sr_in / g; n input frames give ceil(n L / M) outputs; output i reads the 2 W frames around (i M) / L through a Kaiser-
 * windowed sinc evaluated per phase and rounded to 2^-30 (the packed table).  int16 input accumulates exactly in int64 and
 * is rounded twice (one float64 division by channels * 2^45, one conversion to float32); float32 input accumulates in float64,
 * product and sum rounded separately.  Equal rates (L = M = 1) bypass the filter.  The rules are RULES of qasr/resample.py,
 * which the kernel follows byte for byte; parity with librosa's own filter tables is not pinned.
 * The packed table (qasr.resample.ResamplePlan.pack): 32 int32 header words (magic 'QRS1', version, total bytes, L, M, W,
 * sr_in, sr_out, quality, entries = L * 2 W, zeros), then int32 [2 W][L], column r = the slot i mod L of an output.
 * qasr_resample_check validates it ON THE HOST (no GPU is touched): QASR_OK, or QASR_ERR_BLOB (qasr_last_error names the field)
 * for a bad magic, version or size, L, M or W out of range (L, M >= 1 and coprime, W 1 .. QASR_RESAMPLE_MAX_W, L * 2 W <=
 * QASR_RESAMPLE_MAX_ENTRIES), rates that do not reduce to L / M, entries != L * 2 W, a non-zero reserved word, or a column
 * whose sum of |c| * 32768 * QASR_RESAMPLE_MAX_CHANNELS reaches 2^53 (the int64 accumulator would not convert exactly).
 * The kernel trusts `blob`: pass only the bytes that passed.
 * qasr_resample: one launch on `stream`; lengths are device data and nothing is read back, so it can be captured.
 *   in       device int16 or float32 (dtype) [B][in_pitch frames][channels], interleaved
 *   in_lens  device i32 [B]: frames per utterance (clamped to 0 .. in_pitch); a frame at or behind it is never read
 *   out      device f32 [B][out_pitch]: out[b][0 .. out_len) the result, zeros from there to the pitch - a row can be handed
 *            to qasr_engine_forward_audio / qasr_engine_forward_ragged_audio as it is
 *   out_lens device i32 [B]: out_len = min(ceil(n L / M), out_pitch)
 *   L, M, W  repeat the header's fields (the header lies in device memory, which this call does not read): a disagreement
 *            ends every row empty (out_lens 0, zeros)
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL blob / in / in_lens / out /
 * out_lens, an unaligned (16 bytes) blob, blob_bytes != 128 + 4 * L * 2 W, B outside 1 .. 65535, channels outside
 * 1 .. QASR_RESAMPLE_MAX_CHANNELS, an unknown dtype, L, M or W out of range, in_pitch or out_pitch outside
 * 0 .. QASR_RESAMPLE_MAX_PITCH (beyond it i * M leaves 64 bits' safe range and the grid its limit).
 * qasr_resample_out_samples: ceil(in_samples * L / M), or -1 for a negative count, L or M < 1, or a result above 2^31 - 1. */
#define QASR_RESAMPLE_MAX_W 4096
#define QASR_RESAMPLE_MAX_ENTRIES (1 << 20)
#define QASR_RESAMPLE_MAX_CHANNELS 8
#define QASR_RESAMPLE_MAX_PITCH (1ll << 38)
enum { QASR_PCM_S16 = 0, QASR_PCM_F32 = 1 };
int qasr_resample_check(const void* blob, size_t bytes);
typedef struct qasr_resample_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t B, channels, dtype;  /* dtype: QASR_PCM_S16 / QASR_PCM_F32 */
  int32_t L, M, W, reserved;
  const void* blob;            /* device memory: a packed table that passed qasr_resample_check */
  size_t blob_bytes;
  const void* in;
  const int32_t* in_lens;
  int64_t in_pitch;            /* frames per input row */
  float* out;
  int64_t out_pitch;           /* floats per output row */
  int32_t* out_lens;
} qasr_resample_args;
int qasr_resample(void* stream, const qasr_resample_args* args);
int qasr_resample_out_samples(int in_samples, int L, int M);

/* ---- long recordings: overlapped windows cut and stitched on the device --------------------------------------------------
 * A recording is cut into equal windows that overlap (k_cut), the windows run through the engine as a batch, and the
 * per-frame outputs of neighbouring windows are joined at one frame of their overlap, the seam (k_stitch).  The plan and the
 * seam rule are qasr/longform.py (WindowPlan, SEAM_RULES), which both kernels follow byte for byte.  Normalisation is per
 * window: the stitched result is not that of one run over the whole recording.
 *   table    device i32 [Wn][4] = (recording, start_sample, n_samples, first_global_frame), windows of one recording adjacent
 *            and ascending, as WindowPlan lays them out (the kernels trust it up to memory safety: a recording outside
 *            0 .. R - 1 gives an empty window / writes nothing)
 * qasr_longform_cut: audio f32 [R][pitch], lens i32 [R] -> windows f32 [Wn][Wl] (window k = min(n_samples, lens - start)
 *   samples, zeros behind them) and window_lens i32 [Wn].  One launch; can be captured.
 * qasr_longform_stitch: one launch; can be captured.
 *   enc_lens     device i32 [Wn]: encoded frames per window (clamped to 0 .. min(Tw, 2 * hop_frames))
 *   tokens       device i32 [Wn][Tw], frame_score f32 [Wn][Tw] or NULL: what the seam is chosen from
 *   planes       n_planes <= QASR_LONGFORM_MAX_PLANES of (src [Wn][Tw][bytes_per_frame], dst [R][Tmax][bytes_per_frame],
 *                bytes_per_frame a multiple of 4, fill: the 32-bit word written where no window holds a frame and behind
 *                total_frames); tokens / frame_score are stitched only if they are listed as planes too
 *   total_frames device i32 [R] = min(first_global_frame(last) + enc_len(last), Tmax);  seams device i32 [Wn] = the first
 *                global frame window k contributes (0 for a recording's first window)
 *   guard, hop_frames (H / samples_per_frame), blank, seam_mode: the plan's and SEAM_RULES'
 * QASR_ERR_ARG with nothing launched and no output written: an unknown struct_size, a NULL among the required pointers (all
 * but frame_score; every listed plane's src and dst), Wn < 1, R < 1, Wl / Tw / Tmax / hop_frames < 1, pitch < 0, n_planes
 * outside 0 .. QASR_LONGFORM_MAX_PLANES, a bytes_per_frame that is < 4 or no multiple of 4, guard < 0, an unknown seam_mode. */
#define QASR_LONGFORM_MAX_PLANES 6
enum { QASR_SEAM_BLANK = 0, QASR_SEAM_MIDDLE = 1 };
typedef struct qasr_longform_cut_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t R, Wn, Wl;
  const float* audio;
  int64_t pitch;               /* floats per audio row */
  const int32_t* lens;
  const int32_t* table;
  float* windows;
  int32_t* window_lens;
} qasr_longform_cut_args;
int qasr_longform_cut(void* stream, const qasr_longform_cut_args* args);
typedef struct qasr_longform_plane {
  const void* src;
  void* dst;
  int64_t bytes_per_frame;
  uint32_t fill, reserved;
} qasr_longform_plane;
typedef struct qasr_longform_stitch_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t R, Wn, Tw, Tmax, guard, hop_frames, blank, seam_mode, n_planes;
  const int32_t* table;
  const int32_t* enc_lens;
  const int32_t* tokens;
  const float* frame_score;    /* optional */
  int32_t* total_frames;
  int32_t* seams;
  qasr_longform_plane planes[QASR_LONGFORM_MAX_PLANES];
} qasr_longform_stitch_args;
int qasr_longform_stitch(void* stream, const qasr_longform_stitch_args* args);

/* ---- streaming recognition, buffered: per-stream state and chunked decode on the device ---------------------------------
 * The models are not causal and normalise per utterance, so a step re-runs a window [left context L | new chunk C |
 * look-ahead Rr] (Wl = L + C + Rr samples, each a multiple of samples_per_frame) of a stream's latest samples through the
 * engine, and only the chunk's frames become final, one look-ahead late.  The rule, the state layout and the NumPy twins are
 * qasr/stream.py (StreamPlan, STREAM_RULES), which the three kernels follow byte for byte, the state included: what is
 * pinned is that equality and the invariant that the per-step deltas of any sequence of steps over one stream, concatenated,
 * are the outputs of qasr_ctc_collapse over the concatenated final frames on every byte (labels, start, nframes, score, count;
 * the END step's utt_score is qasr_ctc_out.utt_score of that row).  Accuracy on speech is not pinned.
 *   state    device memory of qasr_stream_state_bytes(S, Wl, C) bytes, 16-byte aligned, for S slots: per slot 80 32-bit
 *            words (received i64, frames_done, the open run's token + 1 / first global frame / running maximum in k_ctc's
 *            integer order, n_labels, 64 f32 partial sums of utt_score), then per slot a ring of Wl + C samples (rounded up
 *            to a multiple of 4).  Zeroed memory is S fresh streams.  0 bytes: S, Wl or C < 1, or Wl + C beyond int32.
 *   slots    device i32 [B], distinct, each < S (a slot out of range: its row is skipped / reports status 2)
 *   flags    device i32 [B]: QASR_STREAM_BEGIN (push: forget the slot's history and state first), QASR_STREAM_END (emit:
 *            every frame of the window becomes final, the open run closes, utt_score is summed)
 * qasr_stream_push: chunk f32 or s16 [B][pitch] (s16 as float32(x) / 32768), n_new device i32 [B] (clamped to
 *   0 .. min(pitch, C)) -> the slots' rings and `received`.  One launch; can be captured.
 * qasr_stream_window: -> windows f32 [B][Wl] (the slot's samples [start, received), start = max(0, spf * ceil((received -
 *   Wl) / spf)), zeros behind them), window_lens i32 [B], first_frame i32 [B] = start / spf: local frame j of the window is
 *   global frame first_frame + j.  Reads the state, writes none of it.  One launch; can be captured.
 * qasr_stream_emit: tokens i32 [B][Tw], frame_score f32 [B][Tw], enc_lens i32 [B] (clamped to 0 .. Tw) and first_frame as
 *   the window's forward and qasr_stream_window gave them -> the step's delta, pitch P: labels (tail: blank) / start (global
 *   frames) / nframes / score [B][P] (tails 0) of the runs that CLOSED inside the final range [frames_done, hi), hi =
 *   first_frame + enc_len on END, else min(that, (received - Rr) / spf); the run that reaches hi - 1 stays open in the state.
 *   n_new_labels (<= P), status (0; 1: frames_done < first_frame, frames were lost - nothing final, state untouched; 2: no such
 *   slot), total_frames (= hi), utt_score (END rows; else 0) [B].  tail_labels i32 [B][Ptail] and tail_n i32 [B] (both or
 *   neither): the provisional labels of the look-ahead frames, the open run's first.  One launch; can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL among the required pointers (all but
 * tail_labels / tail_n), B < 1, B > S, B > 65535 (the rows are one dimension of a launch grid), Wl / C < 1, samples_per_frame < 1, Wl, C or Rr no multiple of samples_per_frame, Rr < 0
 * or Rr + C > Wl, state_bytes below qasr_stream_state_bytes(S, Wl, C), an unknown sample format, pitch < 0, Tw / P < 1, Ptail < 1
 * with a tail, one of tail_labels / tail_n without the other. */
enum { QASR_STREAM_BEGIN = 1, QASR_STREAM_END = 2 };
size_t qasr_stream_state_bytes(int S, int Wl, int C);
typedef struct qasr_stream_push_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, samples_per_frame;
  int32_t dtype, reserved;     /* dtype: QASR_PCM_S16 / QASR_PCM_F32 */
  void* state;
  size_t state_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* n_new;
  const void* chunk;
  int64_t pitch;               /* samples per chunk row */
} qasr_stream_push_args;
int qasr_stream_push(void* stream, const qasr_stream_push_args* args);
typedef struct qasr_stream_window_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, samples_per_frame;
  int32_t reserved[2];
  const void* state;
  size_t state_bytes;
  const int32_t* slots;
  float* windows;
  int32_t* window_lens;
  int32_t* first_frame;
} qasr_stream_window_args;
int qasr_stream_window(void* stream, const qasr_stream_window_args* args);
typedef struct qasr_stream_emit_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, Rr, samples_per_frame, Tw, P, Ptail, blank, reserved;
  void* state;
  size_t state_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* tokens;
  const float* frame_score;
  const int32_t* enc_lens;
  const int32_t* first_frame;
  int32_t* labels;
  int32_t* start;
  int32_t* nframes;
  float* score;
  int32_t* n_new_labels;
  int32_t* status;
  int32_t* total_frames;
  float* utt_score;
  int32_t* tail_labels;        /* optional, with tail_n */
  int32_t* tail_n;
} qasr_stream_emit_args;
int qasr_stream_emit(void* stream, const qasr_stream_emit_args* args);

/* ---- streaming beam search: per-stream beam state and fixed-lag commit on the device -------------------------------------
 * The prefix beam search of qasr_ctc_beam / qasr_ctc_beam_lm (lm == NULL: without a model) over the frames that a streaming
 * step makes final, with the beam of every slot kept on the device between steps.  The rule, the state layout and the NumPy
 * twin are qasr/stream_beam.py (STREAM_BEAM_RULES), which k_stream_beam follows byte for byte, state block and ring included.
 * Text becomes final by a fixed-lag commit that prunes: after every GLOBAL frame t with (t + 1) % K == 0 and h = t - Lg >= 0
 * the labels of the best entry whose trie node was created at a frame <= h are committed, and every entry whose labels up to
 * that horizon differ is dropped.  Pinned: the equality with the twin; that the steps of ANY slicing of a stream, concatenated,
 * equal the whole-stream search (lagged_search_host) on every byte; that with Lg >= the stream's length the END rows equal
 * qasr_ctc_beam[_lm] over the same candidates.  Accuracy on speech, and the default lag, are not pinned.
 *   state       the stream state of qasr_stream_push / _emit, READ-ONLY here (frames_done, received): launch this call after
 *               qasr_ctc_topn over the window's log-probabilities and BEFORE qasr_stream_emit, which advances frames_done
 *   beam_state  device memory of qasr_stream_beam_state_bytes(S, beam_width, F) bytes, 16-byte aligned: per slot 16 header
 *               words (live entries, commit_len, frames_done, 1 once stepped), 20 * beam_width words of entries, then a ring of
 *               F rows x beam_width (parent node, label) pairs; node t * beam_width + r lives in row t % F.  Zeroed memory is S
 *               fresh streams.  0 bytes: S < 1, beam_width outside 1 .. QASR_BEAM_MAX_WIDTH, F outside 1 ..
 *               QASR_STREAM_BEAM_MAX_RING.  F >= Lg + K rows keep every live node (StreamBeamPlan derives it).
 *   cand_id, cand_q  i32 [B][Tw][N] of the windows (qasr_ctc_topn); enc_lens, first_frame, slots as for qasr_stream_emit
 *   flags       QASR_STREAM_BEGIN: the slot's beam is reset to the single empty entry first; QASR_STREAM_END: after the last
 *               final frame the unfinished-word term (word-mode models) and the n-best are written
 *   -> labels, frames i32 [B][P]: the step's newly committed labels and the creation frame of each one's node (a free
 *      emission time, NOT an alignment; tails: blank / 0); n_new_labels (<= P), commit_len (all labels committed so far),
 *      n_live, status i32 [B]; tail_labels i32 [B][Ptail] and tail_n i32 [B]: the best entry's uncommitted labels (the first
 *      Ptail; tail_n is their true count; END rows: none); on END rows end_labels i32 [B][n_best][Pend], end_n_labels i32,
 *      end_score i64, end_lm_score i64 (with lm) [B][n_best], n_hyps i32 [B]: the final beam, best first, as suffixes behind
 *      the committed text (unused rows and other steps: blank / 0 / -2^62 / 0 / 0).
 *   status 0; 1: frames were lost (qasr_stream_emit's status 1); 2: no such slot; 3: the beam block's frames_done (0 with
 *      BEGIN) is not the stream block's; 4: the step's node ids would pass 2^31 - 1.  A row with a status leaves its state
 *      alone and writes an empty step.
 * One launch; nothing is read back; the chain qasr_ctc_topn -> qasr_stream_beam -> qasr_stream_emit can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL among the required pointers (all but
 * lm, and end_lm_score without lm), what qasr_stream_emit refuses about S, B, Wl, C, Rr, samples_per_frame, state_bytes and Tw,
 * Tw > QASR_BEAM_MAX_FRAMES, what qasr_ctc_beam refuses about N, beam_width, n_best, blank and lae_entries (and with lm what
 * qasr_ctc_beam_lm refuses about lm, lm_bytes, alpha_q, beta_q, space), Lg < 0, K outside 1 .. QASR_STREAM_BEAM_ROUND,
 * F < Lg + K or F > QASR_STREAM_BEAM_MAX_RING, beam_state_bytes below the query, a state not 16-byte aligned,
 * max_final_frames outside 1 .. Tw, P < F + max_final_frames, Ptail < 1, Pend < F. */
#define QASR_STREAM_BEAM_ROUND 32
#define QASR_STREAM_BEAM_MAX_RING (1 << 20)
size_t qasr_stream_beam_state_bytes(int S, int beam_width, int F);
typedef struct qasr_stream_beam_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, Rr, samples_per_frame, Tw;
  int32_t N, beam_width, n_best, blank;
  int32_t Lg, K, F;            /* the lag and the round period in frames (K: QASR_STREAM_BEAM_ROUND), rows of the ring */
  int32_t max_final_frames;    /* the most frames one step makes final (StreamPlan.max_final_frames) */
  int32_t P, Ptail, Pend;
  uint32_t lae_entries;        /* QASR_BEAM_TABLE_ENTRIES */
  const void* state;
  size_t state_bytes;
  void* beam_state;
  size_t beam_state_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* cand_id;
  const int32_t* cand_q;
  const int32_t* enc_lens;
  const int32_t* first_frame;
  const uint16_t* lae_table;
  int32_t* labels;
  int32_t* frames;
  int32_t* n_new_labels;
  int32_t* commit_len;
  int32_t* n_live;
  int32_t* status;
  int32_t* tail_labels;
  int32_t* tail_n;
  int32_t* end_labels;
  int32_t* end_n_labels;
  int64_t* end_score;
  int32_t* n_hyps;
  const void* lm;              /* device memory: a packed model that passed qasr_lm_check, or NULL: no model */
  size_t lm_bytes;
  int32_t alpha_q, beta_q;
  int32_t space, reserved;
  int64_t* end_lm_score;       /* with lm */
} qasr_stream_beam_args;
int qasr_stream_beam(void* stream, const qasr_stream_beam_args* args);

/* ---- streaming phrase boosting: per-stream hot words in the streaming beam search ---------------------------------------
 * qasr_stream_beam with the phrase boosting of qasr_ctc_beam_boost inside the frame step: every entry of a slot's beam also
 * keeps its automaton state and its running bonus on the device between steps.  The rule, the state layout and the NumPy twin
 * are qasr/stream_beam.py (STREAM_BOOST_RULES, over BOOST_RULES of qasr/boost.py), which k_stream_beam_boost follows byte for
 * byte, state block and ring included.  Pinned: that equality; that the steps of ANY slicing of a stream equal the
 * whole-stream search (lagged_search_host(boost=)); that with Lg >= the stream's length the END rows equal
 * qasr_ctc_beam_boost over the same candidates (labels, score, lm_score, boost_score); that with set 0 or with every weight 0
 * every byte shared with qasr_stream_beam's layout equals it; that end_boost_score is the brute-force sum over the phrase
 * occurrences in the hypothesis' whole text, however much of it was committed early.  Accuracy on speech is not pinned.
 *   beam        the arguments of qasr_stream_beam, every one as documented there (beam.struct_size =
 *               sizeof(qasr_stream_beam_args)), with two differences: beam.beam_state holds
 *               qasr_stream_beam_boost_state_bytes(S, beam_width, F) bytes - per slot 16 header words (word 4: the slot's set +
 *               1, 0: not boosted), 24 * beam_width words of entries (qasr_stream_beam's eight 64-bit arrays, then boost_tot;
 *               its four 32-bit arrays, then the automaton state, then a pad of zeros), then the ring - and beam.space is the
 *               space label of the vocabulary (-1: none) also without lm
 *   n_sets      1 .. QASR_STREAM_BEAM_MAX_SETS phrase sets of this session
 *   sets, set_bytes, whole_words   per set: device memory holding a packed set that passed qasr_boost_check, 16-byte
 *               aligned, its size, and whether it was compiled for whole words (as qasr_ctc_beam_boost's boost, boost_bytes,
 *               whole_words); entries at and behind n_sets are ignored
 *   boost_set   i32 [B] on the device: read on QASR_STREAM_BEGIN rows only - the set the slot uses until its next BEGIN,
 *               -1: none (the stream is searched as qasr_stream_beam searches it)
 *   -> qasr_stream_beam's outputs, end_score including the boosting's share, and end_boost_score i64 [B][n_best]: that share
 *      (unused rows and other steps: 0)
 *   status      qasr_stream_beam's, and 5: a BEGIN row whose boost_set is outside -1 .. n_sets - 1.
 * One launch; nothing is read back; the sets are arguments, not a table on the device, so that this call validates them and
 * the chain qasr_ctc_topn -> qasr_stream_beam_boost -> qasr_stream_emit can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size (of either struct), everything
 * qasr_stream_beam refuses, n_sets outside 1 .. QASR_STREAM_BEAM_MAX_SETS, a NULL or not 16-byte-aligned set or set_bytes
 * outside 128 .. 2^31 - 1, whole_words != 0 with beam.space < 0 (and beam.space < -1 or == blank), a NULL boost_set or
 * end_boost_score, beam_state_bytes below the boosted size. */
#define QASR_STREAM_BEAM_MAX_SETS 8
size_t qasr_stream_beam_boost_state_bytes(int S, int beam_width, int F);
typedef struct qasr_stream_beam_boost_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t n_sets;
  qasr_stream_beam_args beam;
  const void* sets[QASR_STREAM_BEAM_MAX_SETS];
  size_t set_bytes[QASR_STREAM_BEAM_MAX_SETS];
  int32_t whole_words[QASR_STREAM_BEAM_MAX_SETS];
  const int32_t* boost_set;
  int64_t* end_boost_score;
} qasr_stream_beam_boost_args;
int qasr_stream_beam_boost(void* stream, const qasr_stream_beam_boost_args* args);

/* ---- streaming endpointing: utterance boundaries per stream on the device -------------------------------------------------
 * Decoder-driven: no acoustic model, no energy threshold.  The frames that a streaming step makes final say where speech is
 * (blank against non-blank arg-max, and the frame score); integer rules over global frames cut the stream into utterances:
 * SILENCE (1: speech seen and Fsil frames without), TIMEOUT (2: Fstart frames and no speech), MAX (3: Fmax frames, at the next
 * blank frame), HARD (4: Fhard frames, wherever it stands) and END (5: the END row's last utterance, written even when empty).
 * The rule, the state layout and the NumPy twin are qasr/stream_ep.py (EP_RULES), which k_stream_endpoint follows byte for
 * byte, the state block included.  Pinned: that equality; that the records of the steps of ANY slicing of a stream,
 * concatenated, equal the whole-stream pass (endpoints_whole_host) on every byte; that every record's score is the utt_score
 * of its own frames.  Accuracy on speech, and every default of the façade, are not pinned.
 *   state       the stream state of qasr_stream_push / _emit, READ-ONLY here: launch this call AFTER qasr_stream_emit of the same
 *               rows (hi = its frames_done, n_labels = its label count)
 *   ep_state    device memory of qasr_stream_ep_state_bytes(S) bytes, 16-byte aligned: per slot 80 words (frames_done of this
 *               block, utt_index, utt_first, first speech frame + 1, last speech frame + 1, speech frames, labels_done, zeros,
 *               then float32 part[(t - utt_first) % 64]).  Zeroed memory is S fresh streams.  0 bytes: S < 1.
 *   tokens, frame_score, enc_lens, first_frame, slots, flags   what qasr_stream_emit was given; QASR_STREAM_BEGIN zeroes the
 *               slot's block first, QASR_STREAM_END writes the END record
 *   emit_start, emit_nframes i32 [B][P], emit_n_new_labels, emit_status i32 [B]   qasr_stream_emit's outputs of the same step
 *   Fsil, Fstart, Fmax, Fhard   the rules in frames, 1 .. 2^24, Fhard >= Fmax; min_logp: a non-blank frame is speech when its
 *               score >= min_logp in float32 (-inf: every non-blank frame; NaN scores are never speech)
 *   -> records i32 [B][E][10]: index, first, end (global frames, end exclusive), speech_first, speech_last (-1: none),
 *      speech_frames, reason, score (float32 bits: the utt_score of frame_score[first:end]), label_end (the stream's label
 *      count up to and including this utterance: labels whose run a final frame at or before the cut closed), 0; rows behind
 *      n_records hold zeros; n_records (<= E; EndpointPlan.max_records is never exceeded by a session's steps), status i32 [B]
 *   status 0; 1: emit_status of the row is not 0; 2: no such slot; 3: lo > hi, lo < first_frame, or lo < hi and hi beyond
 *      first_frame + enc_len (lo: this block's frames_done, 0 with BEGIN).  A row with a status leaves its state alone.
 * One launch of one wave per row; plain vector stores by the work-group that owns the slot; no atomics; nothing is read back;
 * the chain qasr_stream_emit -> qasr_stream_endpoint can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL pointer (all are required), what
 * qasr_stream_emit refuses about S, B, Wl, C, Rr, samples_per_frame, Tw, P and state_bytes, E < 1, a rule outside 1 .. 2^24
 * frames or Fhard < Fmax, a NaN min_logp, ep_state_bytes below the query, a state not 16-byte aligned. */
#define QASR_STREAM_EP_MAX_FRAMES (1 << 24)
#define QASR_STREAM_EP_RECORD_WORDS 10
size_t qasr_stream_ep_state_bytes(int S);
typedef struct qasr_stream_endpoint_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, Rr, samples_per_frame, Tw;
  int32_t P, E, blank;         /* the delta's row pitch, the records' row pitch (in records), the blank id */
  int32_t Fsil, Fstart, Fmax, Fhard;
  float min_logp;
  const void* state;
  size_t state_bytes;
  void* ep_state;
  size_t ep_state_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* tokens;
  const float* frame_score;
  const int32_t* enc_lens;
  const int32_t* first_frame;
  const int32_t* emit_start;
  const int32_t* emit_nframes;
  const int32_t* emit_n_new_labels;
  const int32_t* emit_status;
  int32_t* records;
  int32_t* n_records;
  int32_t* status;
} qasr_stream_endpoint_args;
int qasr_stream_endpoint(void* stream, const qasr_stream_endpoint_args* args);

/* ---- streaming keyword spotting: per-stream lattice state on the device ------------------------------------------------------
 * qasr_ctc_spot over the frames that a streaming step makes final.  K keywords are shared by all streams of a session; problem
 * p = row * K + k of a step, its state at (slot, k).  A keyword's whole lattice is one Viterbi row of pairs (D i64, start i32),
 * so a stream's state between two steps is that row plus one open hit: a step loads it, walks the frames that became final -
 * the frame step, the candidate rule and the overlap rule are qasr_ctc_spot's on every point, the fresh start (0, t) with t the
 * GLOBAL frame - and stores it back.  An open hit closes when a candidate that does not overlap arrives, at END, and EARLY:
 * after frame t unless some state 1 .. 2L - 1 is live with start <= open.end and (t + 1) - start + 1 <= max_span; no later
 * candidate can overlap a hit closed this way, so the emitted list is qasr_ctc_spot's of the whole stream.  The rule, the state
 * layout and the NumPy twin are qasr/stream_spot.py (STREAM_SPOT_RULES), which k_stream_spot follows byte for byte, the state
 * block included.  Pinned: that equality; that the hits of the steps of ANY slicing of a stream, concatenated, equal spot_host
 * over the concatenated final frames on every byte of start / end / score and in count.  Accuracy on speech, the façade's
 * defaults and how long a final hit trails its end (up to max_span frames on blank-dominated audio) are not pinned.
 *   state       the stream state of qasr_stream_push / _emit, READ-ONLY here: launch this call AFTER qasr_stream_emit of the same
 *               rows (hi = its frames_done)
 *   spot_state  device memory of qasr_stream_spot_state_bytes(S, K, max_labels) bytes, 16-byte aligned: per (slot, keyword) a
 *               block of 8 + 3 SP 32-bit words, SP = 64 NS, NS = 1 / 2 / 4 by 2 max_labels + 1 <= 64 / 128 / 256: frames_done of
 *               this block, stepped (0: fresh), open flag, the open hit's start, end, count (hits emitted since BEGIN), its
 *               score (i64); then D i64 [SP] and start i32 [SP].  A block with stepped == 0 is a fresh stream whatever else it
 *               holds: zeroed memory is S fresh streams.  0 bytes: S or K < 1, max_labels outside 1 .. QASR_SPOT_MAX_LABELS.
 *   log_probs f32 [B][Tw][n_classes] with pitches, star_logp f32 [B][star_pitch] (qasr_ctc_star, penalty 0, lens = enc_lens,
 *               over the same window), enc_lens, first_frame, slots, flags   what the step's forward and qasr_stream_emit were
 *               given; QASR_STREAM_BEGIN makes the slot's blocks fresh first, QASR_STREAM_END closes the open hit
 *   emit_status i32 [B]   qasr_stream_emit's status of the same step
 *   targets i32 [K][max_labels], target_lens i32 [K]   device data: the kernel checks them itself (ok) and reads nothing through
 *               a bad label;  threshold_q, max_span   as for qasr_ctc_spot
 *   max_final_frames   the most frames one step walks (StreamPlan.max_final_frames); PH: the row pitch of the hit outputs (a
 *               frame closes at most two hits and END one more: 2 * max_final_frames + 1 holds every hit of a step)
 *   -> hit_start, hit_end, hit_detect i32 [B * K][PH] (global frames, inclusive; detect: the frame after which the hit closed,
 *      hi - 1 on END), hit_score i64 [B * K][PH]: the hits that closed in this step, in order, tails 0; n_new_hits: every hit
 *      closed, stored or not; n_hits_total: the block's count; open_start, open_end i32, open_score i64 [B * K]: the open hit
 *      after the step (-1 / -1 / 0: none), the provisional detection; ok (the keyword's validity, as qasr_ctc_spot's), status
 *   status 0; 1: emit_status of the row is not 0; 2: no such slot; 3: lo > hi, lo < first_frame, lo < hi and hi beyond
 *      first_frame + enc_len, or hi - lo > max_final_frames (lo: this block's frames_done, 0 when fresh or with BEGIN).  A problem
 *      with a status, or with ok = 0, leaves its block alone and writes an empty step (no hits, counts 0, open -1 / -1 / 0).
 * One launch, one wave per problem; plain vector stores by the wave that owns the block; no LDS, no barrier, no atomics; nothing
 * is read back; the chain qasr_ctc_star -> qasr_stream_spot behind qasr_stream_emit can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL pointer (all are required), what
 * qasr_stream_emit refuses about S, B, Wl, C, Rr, samples_per_frame, state_bytes and Tw, what qasr_ctc_spot refuses about
 * n_classes (its C), K, max_labels, blank, pitch_frame, pitch_utt, star_pitch (with T = Tw), threshold_q and max_span, B * K above
 * 2^31 - 1, PH < 1, max_final_frames outside 1 .. Tw, spot_state_bytes below the query, a state not 16-byte aligned. */
size_t qasr_stream_spot_state_bytes(int S, int K, int max_labels);
typedef struct qasr_stream_spot_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, Rr, samples_per_frame, Tw;    /* C: the chunk in samples, as in qasr_stream_emit_args */
  int32_t n_classes, K, max_labels, blank;
  int32_t threshold_q;         /* fixed point, nats per frame */
  int32_t max_span;            /* frames */
  int32_t PH;                  /* row pitch of the hit outputs */
  int32_t max_final_frames;
  int64_t pitch_utt, pitch_frame;   /* of log_probs, in floats */
  const float* log_probs;
  const float* star_logp;      /* [B][star_pitch] */
  int64_t star_pitch;          /* in floats, >= Tw */
  const void* state;
  size_t state_bytes;
  void* spot_state;
  size_t spot_state_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* enc_lens;
  const int32_t* first_frame;
  const int32_t* emit_status;
  const int32_t* targets;      /* [K][max_labels] */
  const int32_t* target_lens;  /* [K] */
  int32_t* hit_start;          /* [B * K][PH] */
  int32_t* hit_end;
  int32_t* hit_detect;
  int64_t* hit_score;
  int32_t* n_new_hits;         /* [B * K] */
  int32_t* n_hits_total;
  int32_t* open_start;
  int32_t* open_end;
  int64_t* open_score;
  int32_t* ok;
  int32_t* status;
} qasr_stream_spot_args;
int qasr_stream_spot(void* stream, const qasr_stream_spot_args* args);

/* ---- streaming beam endpointing: the per-stream beam finalised and reset at the cuts of qasr_stream_endpoint ---------------
 * qasr_stream_beam / qasr_stream_beam_boost for sessions that are cut into utterances: the same frame step and commit round,
 * and at every record of the step's qasr_stream_endpoint the END pass of those calls, written per cut, after which the slot's
 * beam is the single fresh entry again.  The rule and the NumPy twin are qasr/stream_beam.py (STREAM_BEAM_EP_RULES), which
 * k_stream_beam_ep<LM, BOOST> follows byte for byte, state block and ring included.  Pinned: that equality; that the steps of
 * ANY slicing of a stream equal the whole-stream search (lagged_search_ep_host); that with Lg at or beyond the longest
 * utterance every cut's rows equal qasr_ctc_beam[_lm|_boost] over the utterance's own frames.  Accuracy on speech is not pinned.
 *   boost       the arguments of qasr_stream_beam_boost (boost.struct_size and boost.beam.struct_size as there), with these
 *               differences: this call is launched AFTER qasr_stream_emit and qasr_stream_endpoint of the same rows - lo is
 *               the beam block's own frames_done (0 with BEGIN), hi the stream block's frames_done as emit left it;
 *               boost.n_sets == 0 selects the layout and size of qasr_stream_beam (sets, boost_set ignored), 1 .. 8 that of
 *               qasr_stream_beam_boost; header word 5 of a slot's block counts the cuts done; end_labels, end_n_labels,
 *               end_score, end_lm_score, n_hyps and end_boost_score are ignored (they may be NULL); commit_len and n_live
 *               describe the beam the step leaves behind, tail_labels / tail_n its best entry on every row
 *   E           the records' row pitch (in records) and the most cuts of one row
 *   records, n_records, ep_status   qasr_stream_endpoint's outputs of the same step, read-only: i32 [B][E][10], [B], [B]
 *   -> n_cuts i32 [B] (= n_records); per cut k < n_cuts: cut_n_hyps i32 [B][E], and for the first n_best entries of the beam as
 *      the END pass orders it cut_labels i32 [B][E][n_best][Pend] (the suffix behind commit_len), cut_n_labels i32, cut_score
 *      i64, cut_lm_score i64 (with lm), cut_boost_score i64 (with sets) [B][E][n_best]; cut_delta_end i32 [B][E]: the length of
 *      the step's delta (labels / frames) after cut k, whose last labels are the best entry's suffix.  Unused rows: blank / 0 /
 *      -2^62 / 0 / 0; cut_n_hyps and cut_delta_end 0.
 *   status      qasr_stream_beam_boost's; 3 also covers lo > hi, lo < hi with hi beyond first_frame + enc_len, n_records
 *               outside 0 .. E, record ends that fall or lie outside (lo, hi] (end == lo only with lo == hi), a first record
 *               whose index is not the block's cut count (0 with BEGIN), and ep_status != 0.  A row with a status leaves its
 *               state alone and writes an empty step.
 * One launch of one work-group of 256 threads per row; plain vector stores by the work-group that owns the slot; atomics on
 * LDS only; nothing is read back; the chain qasr_ctc_topn -> qasr_stream_emit -> qasr_stream_endpoint -> qasr_stream_beam_ep
 * can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size (of any of the three structs), what
 * qasr_stream_beam_boost refuses (but for the ignored pointers, and n_sets may be 0), E < 1 or B * E * n_best * Pend >= 2^31,
 * a NULL among records, n_records, ep_status, n_cuts, cut_n_hyps, cut_delta_end, cut_labels, cut_n_labels, cut_score,
 * cut_lm_score with lm, cut_boost_score with sets. */
typedef struct qasr_stream_beam_ep_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t E;
  qasr_stream_beam_boost_args boost;
  const int32_t* records;
  const int32_t* n_records;
  const int32_t* ep_status;
  int32_t* n_cuts;
  int32_t* cut_n_hyps;
  int32_t* cut_delta_end;
  int32_t* cut_labels;
  int32_t* cut_n_labels;
  int64_t* cut_score;
  int64_t* cut_lm_score;       /* with lm */
  int64_t* cut_boost_score;    /* with sets */
} qasr_stream_beam_ep_args;
int qasr_stream_beam_ep(void* stream, const qasr_stream_beam_ep_args* args);

/* ---- streaming at any sample rate: per-stream resampler state on the device -------------------------------------------
 * In front of the sample ring above: PCM at the source's rate (int16 or float32, 1 .. 8 interleaved channels) is appended to a
 * per-slot history of channel sums, and the outputs of the polyphase resampler that have become FINAL are written into the
 * slot's sample ring, where qasr_stream_window / _emit find them as if they had been pushed.  Output i reads the input frames
 * q - W + 1 .. q + W, q = floor(i M / L); once n frames have arrived, the first ready(n) = max(0, ceil((n - W) L / M)) outputs
 * cannot change any more, and they equal qasr_resample over the whole stream on every byte.  A FLUSH row treats the frames
 * behind the last one as zeros (as the end of an utterance does) and produces up to out_len(n) = ceil(n L / M).  Equal rates
 * (L = M = 1, the channel mean only) count as W = 0.  The rule and the NumPy twin: qasr/stream_rs.py (RS_STREAM_RULES).
 *   rs_state device memory of qasr_stream_rs_state_bytes(S, hcap) bytes, 16-byte aligned: per slot 16 32-bit words
 *            (in_received i64, the slot's sample format + 1, zeros), then per slot a history of hcap 8-byte entries; input
 *            frame k lives at entry k % hcap as its channel sum: int64 for int16 input, float64 (channels added in ascending
 *            order) for float32 input.  Zeroed memory is S fresh streams.  0 bytes: S < 1, hcap < 4, no multiple of 4 or
 *            above 2^26.  hcap = StreamResamplePlan.hcap (2 W + the most frames of one append, rounded up to a multiple of 4).
 *   work     device memory of qasr_stream_rs_work_bytes(B) bytes, 16-byte aligned: one record of 8 32-bit words per row
 *            (first output i64, count, sample format, in_received i64, slot, zero), written by the first launch and read by
 *            the second.  0 bytes: B < 1.
 *   blob     the packed table of qasr_resample (it passed qasr_resample_check); L, M, W repeat its header
 *   flags    device i32 [B]: QASR_STREAM_BEGIN (forget the slot's stream block and resampler block first), QASR_STREAM_FLUSH
 *   chunk    device s16 or f32 (dtype) [B][pitch frames][channels]; n_in device i32 [B] frames, clamped to 0 .. min(pitch,
 *            max(1, floor(C M / L))) and then so that no history entry is overwritten that an output at or behind the
 *            stream's `received` still reads (frames at or above floor(received M / L) - W + 1 stay; W = 0: at or above received)
 *   out_limit device i32 [B]: at most this many outputs are produced (and at most C)
 *   -> n_taken, n_out, status device i32 [B]: frames appended, outputs produced, 0 / 1 (frames were dropped because the
 *            history is full) / 2 (no such slot: nothing done) / 3 (the slot holds the other sample format: nothing appended)
 *            / 4 (the table's header disagrees with L, M, W: nothing done)
 * Two launches: k_stream_rs_append (one work-group per row: the history, both counters, the record, the three outputs), then
 * k_stream_rs_fir (tiles of 256 outputs per row: reads the record, the history and the table only, writes the sample ring).
 * Nothing is read back; can be captured.
 * QASR_ERR_ARG with nothing launched and nothing written: an unknown struct_size, a NULL among the pointers, what
 * qasr_stream_push refuses about S, B, Wl, C, samples_per_frame and state_bytes, rs_state_bytes / work_bytes below the two
 * functions, state / rs_state / work / blob not 16-byte aligned, blob_bytes != 128 + 4 * L * 2 W, channels outside
 * 1 .. QASR_RESAMPLE_MAX_CHANNELS, an unknown dtype, L, M or W out of qasr_resample's range, hcap out of range or below 2 W
 * (W = 0 for equal rates), pitch < 0 or above QASR_RESAMPLE_MAX_PITCH. */
enum { QASR_STREAM_FLUSH = 4 };
size_t qasr_stream_rs_state_bytes(int S, int hcap);
size_t qasr_stream_rs_work_bytes(int B);
typedef struct qasr_stream_rs_push_args {
  uint32_t struct_size;        /* sizeof of this struct in the caller's header */
  int32_t S, B, Wl, C, samples_per_frame;
  int32_t dtype, channels;     /* dtype: QASR_PCM_S16 / QASR_PCM_F32 */
  int32_t L, M, W, hcap;
  void* state;                 /* the stream state of qasr_stream_push */
  size_t state_bytes;
  void* rs_state;
  size_t rs_state_bytes;
  void* work;
  size_t work_bytes;
  const void* blob;
  size_t blob_bytes;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* n_in;
  const int32_t* out_limit;
  const void* chunk;
  int64_t pitch;               /* frames per chunk row */
  int32_t* n_taken;
  int32_t* n_out;
  int32_t* status;
} qasr_stream_rs_push_args;
int qasr_stream_rs_push(void* stream, const qasr_stream_rs_push_args* args);

/* ---- reserved engines: ragged batches without allocation, with graph replay ------------------------------------------
 * A data loader pads every batch to its own longest utterance (the reference's collate function), so (B, T) changes on
 * almost every call; qasr_engine_forward[_audio] then rebuilds its plan (device-synchronising frees + allocations) and,
 * with caller-allocated outputs, never replays a graph.  qasr_engine_reserve allocates ONCE for an envelope: the arena,
 * the length tables, every workspace, staging buffers for the input and engine-owned output buffers.  Afterwards
 * qasr_engine_forward_ragged[_audio] run any shape inside the envelope:
 *   - the shape is rounded up to a bucket: all max_batch rows (the added rows have length 0) and
 *     qasr_ragged_bucket_frames() frames; the outputs for rows < B and frames < T' are bit-identical to the exact-shape
 *     forward of an unreserved engine (every conv masks its input with the lengths; the mel front-end reads the batch's
 *     own sample count from a device-resident shape block, so torch.stft's reflect padding folds where it does at the
 *     exact shape);
 *   - one kernel (k_ragged_stage) copies input and lengths into the engine's staging buffers and writes the shape
 *     block; it is launched directly, everything behind it belongs to the bucket's hipGraph: the first call that lands
 *     in a bucket launches kernel by kernel, the second captures, later ones replay.  Graphs are kept per bucket and
 *     share the one arena;
 *   - a shape outside the envelope returns QASR_ERR_ARG (the message names the limit); nothing is reallocated.
 * Debug / timing engines cannot be reserved.  A reserved engine refuses qasr_engine_forward[_audio] (they would rebuild
 * the plan): use a second engine for those.  Graph capture needs a non-default stream, as for qasr_engine_opts.graph. */
typedef struct qasr_reserve_opts {
  uint32_t struct_size;        /* sizeof(qasr_reserve_opts) of the caller's header */
  int32_t max_batch;           /* >= 1 */
  int32_t max_samples;         /* audio entry: longest padded row S (0: audio entry not used) */
  int32_t max_frames;          /* feature entry: most frames T (0: derived from max_samples); the envelope is the larger of
                                  the two, rounded up to a multiple of 128 frames */
  int32_t n_mels;              /* audio entry: rows of the filterbank (0: the blob's feat_in) */
  int32_t pad_to;              /* audio entry: frames are padded to a multiple of it; must divide 128 (0: 16) */
  int32_t want_logp;           /* keep a log-probability buffer [max_batch][T'max][n_classes] */
  int32_t decode;              /* greedy CTC outputs and per-frame scores as qasr_engine_attach_ctc writes them: 1: use_lens = 1
                                  (stop at the encoded lengths); 2: use_lens = 0 (the padded row as the reference walks it -
                                  the batch's own T' frames, not the bucket's) */
  int32_t max_graphs;          /* most buckets, one captured graph each (0: 16; at most 64) */
  int32_t reserved[3];
} qasr_reserve_opts;
/* Engine-owned buffers of the last ragged forward (device pointers; valid until the next call on this engine).  Rows
 * are `*_pitch` ELEMENTS apart; rows < B and frames < out_frames hold the result, the rest is unspecified. */
typedef struct qasr_ragged_out {
  uint32_t struct_size;        /* sizeof(qasr_ragged_out), set by the caller */
  int32_t out_frames;          /* T' of the exact shape: qasr_engine_out_frames(e, T) */
  int32_t bucket_frames;       /* the bucket edge this call ran at (input frames) */
  int32_t row_pitch;           /* frames per row of tokens / frame_score / the CTC outputs */
  int32_t n_classes;
  int32_t* tokens;             /* i32 [max_batch][row_pitch] */
  int32_t* lens_out;           /* i32 [max_batch] encoded lengths */
  float* logp;                 /* f32 [max_batch][row_pitch][n_classes], NULL without want_logp */
  float* frame_score;          /* f32 [max_batch][row_pitch], NULL without decode */
  qasr_ctc_out ctc;            /* NULL members without decode */
  float* feats;                /* audio entry: staging features f32 [max_batch][n_mels][bucket_frames] (see
                                  qasr_engine_forward_audio for what they hold) */
  int32_t* feat_lens;          /* i32 [max_batch] */
} qasr_ragged_out;
typedef struct qasr_ragged_stats {
  uint32_t struct_size;        /* sizeof(qasr_ragged_stats), set by the caller */
  int32_t n_buckets;           /* buckets with at least one call */
  uint64_t device_allocs;      /* hipMalloc calls made by this engine since qasr_engine_create */
  uint64_t device_frees;       /* hipFree calls */
  uint64_t graphs_captured, graph_replays, eager_runs;
  int32_t bucket_frames[64];   /* per bucket that was visited: its edge */
  uint64_t bucket_calls[64];   /* ... and the calls that landed in it */
} qasr_ragged_stats;
int qasr_engine_reserve(qasr_engine* e, const qasr_reserve_opts* opts);
/* As qasr_engine_forward / qasr_engine_forward_audio without the output (and feature) pointers; lens[b] <= T. */
int qasr_engine_forward_ragged(qasr_engine* e, void* stream, const float* feats, const int32_t* lens, int B, int T,
                               qasr_ragged_out* out);
int qasr_engine_forward_ragged_audio(qasr_engine* e, void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                                     const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                                     const void* frontend_plan, size_t plan_bytes, qasr_ragged_out* out);
/* Works on every engine (an unreserved one reports its allocations and zero graphs). */
int qasr_engine_ragged_stats(const qasr_engine* e, qasr_ragged_stats* out);
/* The bucket policy, a pure function (no GPU): max_frames (a multiple of 128) is cut into at most max_graphs equal steps
 * of whole 128-frame tiles; returns the smallest edge >= T, or -1 when T < 1, T > max_frames or an argument is bad.
 * qasr_ragged_envelope_frames: the envelope a qasr_reserve_opts describes (-1: bad arguments). */
int qasr_ragged_bucket_frames(int max_frames, int max_graphs, int T);
int qasr_ragged_envelope_frames(int max_samples, int max_frames, int pad_to);

/* ---- stand-alone operators (same kernels the engine launches; device pointers) -------------- */

/* AudioToMelSpectrogramPreprocessor.forward / FilterbankFeatures.forward
 * (nemo/collections/asr/parts/features.py:334-397): pre-emphasis, STFT(512, hop 160, hann 320),
 * power, mel filterbank, log, per-feature normalisation, mask, pad to a multiple of `pad_to`.
 * audio f32 [B][S]; audio_lens i32 [B] (samples); fb f32 [n_mels][257]; window f32 [320];
 * feats f32 [B][n_mels][T_pad]; feat_lens i32 [B].  T_pad = qasr_frontend_frames(S, pad_to).
 * workspace: device memory of qasr_frontend_workspace_bytes(B, S, n_mels) bytes, 16-byte aligned: tables that depend
 * on the filterbank only (non-zero run of every mel filter, the runs' weights packed back to back, FFT twiddles).
 * qasr_frontend_mel fills them and runs (self-contained, 5 launches).  A caller whose filterbank is fixed — every
 * model is — calls qasr_frontend_plan once and qasr_frontend_mel_planned per batch (2 launches: k_mel, k_norm); the
 * workspace is read-only from then on and may be shared by any number of streams. */
int qasr_frontend_mel(void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                      const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                      float* feats, int32_t* feat_lens, void* workspace, size_t workspace_bytes);
int qasr_frontend_plan(void* stream, const float* fb, int n_mels, void* workspace, size_t workspace_bytes);
int qasr_frontend_mel_planned(void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                              const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                              float* feats, int32_t* feat_lens, const void* workspace, size_t workspace_bytes);
int qasr_frontend_frames(int S, int pad_to);
size_t qasr_frontend_workspace_bytes(int B, int S, int n_mels);

/* QuantConv1d.int_conv accumulator only (quant_modules.py:301-305) for a 1x1 conv:
 * x i8 [B][cin][Tp] (x_unsigned: bytes are u8, and bias must carry +128*sum(W)); bias i32 [cout_pad128] or NULL;
 * w s8, cout_pad128 x cin_pad128 values in MFMA fragment order: byte ((tile*(cin_pad/32) + ks)*64 + lane)*16 + j holds
 * W[32*tile + (lane & 31)][32*ks + 16*(lane >> 5) + j]; acc i32 [B][cout][Tp].  T valid columns. */
int qasr_pw_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias,
                     int B, int cin, int cin_pad, int cout, int T, int Tp, int32_t* acc);
/* depthwise int_conv accumulator: w s8 [c][kpad]; acc i32 [B][c][Tp_out]; bias i32 [c] or NULL (x_unsigned: bytes
 * are u8 and the kernel feeds x - 128, so bias carries 128 * sum(w[c]) to give the accumulator of the u8 codes) */
int qasr_dw_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias, int B, int c,
                     int kernel, int kpad, int stride, int dilation, int padding, int T, int Tp, int T_out, int Tp_out,
                     int32_t* acc);
/* dense (groups = 1) int_conv accumulator for any kernel / stride / dilation (Jasper's convs; quant_modules.py:301-305):
 * w s8 [cout_pad128][kernel][cin_pad128]; bias i32 [cout_pad128] or NULL (x_unsigned: + 128 * sum(W[co]) over all taps);
 * acc i32 [B][cout][Tp_out] */
int qasr_dense_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias, int B, int cin,
                        int cin_pad, int cout, int kernel, int stride, int dilation, int padding, int T, int Tp, int T_out,
                        int Tp_out, int32_t* acc);
/* fixedpoint_mul.forward for one operand (quant_utils.py:187-198,213): q = clamp(rint(acc*m[c]), lo, hi)
 * with m[c] = mantissa*2^-e as f64; exact_z selects the float32 round trip through sb[c]. */
int qasr_requant(void* stream, const int32_t* acc, const double* m, const float* sb, int exact_z, int relu,
                 int B, int c, int Tp, int lo, int hi, int8_t* out);

/* ---- dynamic-quantisation device path (QuantAct.forward with dynamic=True, quant_modules.py:149-194) --------------
 * In dynamic mode every QuantAct takes its range from the batch in front of it, so multipliers, bias integers and
 * output scales are data dependent.  These entries keep the whole derivation on the device (the reference goes through
 * host numpy in batch_frexp, quant_utils.py:121-147); qasr/dynamic.py strings them together with the conv accumulator
 * kernels above into ConvASREncoder / ConvASRDecoder forward passes.  A float tensor is handed over as the integers of
 * its producer times their float32 scales: */
typedef struct qasr_dyn_view {
  const void* data;            /* int32 [B][C][Tp] accumulators, or int8 [B][C][Tp] codes (is_int8) */
  const float* scale;          /* f32 [C] (per_channel) or [1] */
  int32_t is_int8, per_channel;
  /* Optional (both or neither; accumulators only): the reference's conv_int is F.conv1d in double over
   * x_int = fl32(x / pre_sf) (quant_modules.py:301-305), and that float32 quotient is the integer or a float32 neighbour
   * of it - conv_int = integers + sum(w residue), rounded once by .type(torch.float).  residue_lo + 128 residue_hi is that
   * sum in units of 2^-24 (the int_conv accumulators of the two tensors qasr_dyn_residue_codes writes, no bias).  It never
   * changes a code, but it is in the float tensor a dynamic QuantAct ranges over. */
  const int32_t* residue_lo;
  const int32_t* residue_hi;
} qasr_dyn_view;
/* x_act.min() / .max() (quant_modules.py:152-153): x_act = relu?(a) (+ b as the identity), zero where t >= lens[b]
 * (MaskedConv1d's mask, jasper.py:177-181; lens NULL: no mask), over t < T.  xf != NULL: the tensor is the float input
 * itself, [B][C][Tx] (first layer).  minmax: two order-preserving encodings of the float32 min / max. */
int qasr_dyn_range(void* stream, const qasr_dyn_view* a, const qasr_dyn_view* b, const float* xf, int Tx,
                   const int32_t* lens, int relu, int B, int C, int T, int Tp, uint32_t* minmax);
/* The percentile form of the same range (qm.set_percentile in force, quant_modules.py:158-167): minmax =
 * (torch.quantile(x_act, q_lo), torch.quantile(x_act, q_hi)) over ALL B C T elements, masked zeros included, in the
 * encoding of qasr_dyn_range.  x_act: device scratch of B C T floats (the tensor is written out once, then
 * qasr_quantile2 selects on it); workspace as for qasr_quantile2. */
int qasr_dyn_range_percentile(void* stream, const qasr_dyn_view* a, const qasr_dyn_view* b, const float* xf, int Tx,
                              const int32_t* lens, int relu, int B, int C, int T, int Tp, float q_lo, float q_hi,
                              float* x_act, void* workspace, size_t workspace_bytes, uint32_t* minmax);
/* act_scaling_factor = max(|min|, |max|, 1e-8) / (2^(bits-1) - 1) (quant_utils.py:44-54) -> s_out[0]; per channel the
 * fixedpoint_mul multiplier m 2^-e of f64(pre_sf[c]) / f64(act_sf) with (m, e) = batch_frexp (quant_utils.py:121-147,
 * 190-196) as float64 -> Ma[c] (operand a, scales sa) and Mb[c] (operand b, scales sb; NULL: none). */
int qasr_dyn_act_params(void* stream, const uint32_t* minmax, int bits, int C, const float* sa, int a_per_channel,
                        const float* sb, int b_per_channel, float* s_out, double* Ma, double* Mb);
/* fixedpoint_mul.forward (quant_utils.py:163-216): z = round(relu?(view) / pre_sf) through the float32 view, out =
 * clamp(round(z_a Ma) (+ round(z_b Mb)), lo, hi) as int8 / uint8 bytes [B][C][Tp]; columns >= min(lens[b], T) are 0. */
int qasr_dyn_requant(void* stream, const qasr_dyn_view* a, const double* Ma, const qasr_dyn_view* b, const double* Mb,
                     const int32_t* lens, int relu, int B, int C, int T, int Tp, int lo, int hi, int8_t* out);
/* first layer (quant_modules.py:180-184): s_out[0] = act_scaling_factor, out = clamp(round(fl32(1/s) x), -n, n-1) */
int qasr_dyn_quant_in(void* stream, const float* x, int Tx, const uint32_t* minmax, const int32_t* lens, int bits, int B,
                      int C, int T, int Tp, float* s_out, int8_t* out);
/* residue(q) = fl32(fl32(q s_x[0]) / s_x[0]) - q of every code byte (see qasr_dyn_view), in units of 2^-24, as
 * lo + 128 hi with |lo| <= 64, |hi| <= 2: two s8 tensors of n bytes (n a multiple of 16, 16-byte aligned pointers). */
int qasr_dyn_residue_codes(void* stream, const int8_t* codes, int x_unsigned, const float* s_x, size_t n, int8_t* lo,
                           int8_t* hi);
/* the conv that consumes those codes (quant_modules.py:293-299,307): sf_out[c] = s_w[c] s_x, bias[c] =
 * clamp(round(fl32(1/sf_out[c]) bprime[c])) evaluated in float32, saturated to [INT32_MIN, INT32_MAX] (the reference's
 * float32 clamp gives +-2^31: (float)INT32_MAX is its +2^31) (+ wsum128[c] = 128 sum(W[c]) modulo 2^32 when the codes
 * are stored as u8); rows C..C_pad-1: scale 1, bias 0. */
int qasr_dyn_conv_params(void* stream, const float* s_x, const float* s_w, const float* bprime, const int32_t* wsum128,
                         int C, int C_pad, float* sf_out, int32_t* bias);

/* One fused time-channel-separable layer exactly as the engine launches it (k_sep2 / k_sep): depthwise QuantConv1d
 * (K taps, stride 1, 'same' padding) -> QuantAct requant -> 1x1 QuantConv1d [-> residual 1x1 QuantConv1d + res_act] ->
 * ReLU -> the consumers' QuantAct requant (jasper.py:569-600,664-687; quant_modules.py:186-190,301-309).  Every pointer
 * is a device pointer in the blob's layouts (see qasr_op_desc): the parity tests drive the production kernels through
 * this entry with operands of their own making (accumulators beyond 2^22, rounding ties, ragged lengths).
 * K == 0: no depthwise stage (`x` feeds the 1x1 conv).  gen: 2 = k_sep2 where it has the shape, 1 = k_sep, 3 = k_sep2s
 * (k_sep2 with the mask-skip rule, see qasr_engine_opts.mask_skip).
 * tile: 32, 64 or 128 (k_sep2's plain layers; others fall back to 64) frames per work-group.  `label` (optional)
 * receives the kernel instantiation that ran. */
typedef struct qasr_sep_layer_args {
  int32_t B, T, Tp, cin, cout, K, dilation, tile, gen;
  uint32_t flags;              /* QASR_F_RELU | MASK_OUT | EXACT_Z | RESADD */
  const int8_t* x;             /* [B][cin][Tp] depthwise input (1x1 input when K == 0) */
  int32_t x_unsigned, dw_lo, dw_hi, n_outs;
  const int8_t* wdw;           /* s8 [cin][kpad4] */
  const int8_t* wdw2;          /* s8 [cin][kpad4 + 32]: taps behind 8 zero bytes */
  const int32_t* bias_dw;      /* i32 [cin_pad128] (128 * sum(w) for u8 inputs) */
  const double* m_dw;          /* f64 [cin_pad128] */
  const int8_t* w;             /* s8 cout_pad128 x cin_pad128, MFMA fragment order */
  const int32_t* bias;         /* i32 [cout_pad128] */
  const float* sb;             /* f32 [cout_pad128] (EXACT_Z) */
  const double* m_main;        /* f64 [cout_pad128] (RESADD) */
  const int32_t* lens;         /* i32 [B] valid frames */
  const int8_t* rx;            /* RESADD: residual conv input [B][rcin][Tp] */
  const int8_t* rw;            /*         its weights, fragment order */
  const int32_t* rbias;
  const double* rm;
  const float* rsb;
  int32_t rcin, r_unsigned, qlo, qhi;
  struct {
    void* ptr;                 /* i8 [B][cout][Tp] */
    const double* mtab;        /* mode 1 */
    double m;                  /* mode 0 */
    int32_t lo, hi, mode, pad_;
  } outs[QASR_MAX_OUTS];
  int32_t* dw_acc;             /* optional hooks: i32 [B][cin][Tp], [B][cout][Tp], [B][cout][Tp] */
  int32_t* acc;
  int32_t* racc;
  int32_t pair, pad_;          /* 1: the paired form (qasr_engine_opts.pair_split); QASR_ERR_UNSUPPORTED for a shape without one */
  void* pair_ws;               /* ... its workspace: 256-byte aligned device memory of qasr_sep_pair_workspace_bytes(B, Tp) bytes, */
  size_t pair_ws_bytes;        /*     one per launch in flight.  Its head holds the members' completion counters (2 u32 per pair, zeroed
                                      by the call; each member adds 1 at its end, nothing waits for them); the u32 at
                                      qasr_sep_pair_timeout_offset, the time-out word of the former hand-off, is no longer written, and
                                      nothing behind it is touched (the size is kept for callers that sized their buffers by it) */
} qasr_sep_layer_args;
int qasr_sep_layer(void* stream, const qasr_sep_layer_args* a, char* label, size_t label_cap);
size_t qasr_sep_pair_workspace_bytes(int B, int Tp);
size_t qasr_sep_pair_timeout_offset(int B, int Tp);
/* 1 if op `op` of the current plan runs in the paired form, 0 if not, -1 for a bad argument (after a forward) */
int qasr_engine_op_paired(const qasr_engine* e, int op);
/* 1 if op `op` of the current plan runs in the halved form, 0 if not, -1 for a bad argument (after a forward).  Halved: an
 * unpaired plain k_sep2 layer of a 128-frame tile launched as the 64-frame instantiation of the same kernel on grid
 * (B, Tp / 64) - the same bytes, label and launch count.  For a tile_frames == 128 engine below 8 hardware queues (the
 * GPU_MAX_HW_QUEUES hint of res_tile128; QASR_HALF_TILES=0|1 overrides), never for debug / timing / reserved engines, paired
 * ops, block-end layers or rows that 128 does not divide */
int qasr_engine_op_halved(const qasr_engine* e, int op);
/* synchronises the device and reads the time-out word of paired launches.  Kept from the form whose members handed their
 * halves over inside the launch: the members of a pair exchange nothing now, no kernel writes the word, the result is always 0 */
int qasr_engine_pair_timeouts(qasr_engine* e);
/* Diagnostics, read-only: the flag words of the plan's paired ops (2 per work-group pair and op, each op's padded to 256
 * bytes) - completion counters: each member of a pair adds 1 to its own word at its end, nothing waits for them.  Returns how
 * many words the engine has (0: no paired op, -1: error); with `out`, synchronises the device and copies the first
 * min(n, that many) words.  Behind a forward every word of a pair that ran holds 1: each forward zeroes them first. */
int qasr_engine_pair_flag_words(const qasr_engine* e, uint32_t* out, size_t n);

/* Diagnostics: when set to a device buffer of 32 int64, work-group (1,0,0) of every k_sep launch writes s_memtime
 * stamps at its phase boundaries (slot 31 = number of stamps); NULL (default) disables. */
int qasr_debug_prof(void* dev_buf);
/* per-work-group timeline of the k_sep2 launches that follow: dev_buf[4 wg .. 4 wg + 3] = {start, end (100 MHz
 * s_memrealtime), HW_ID | XCC_ID << 32, shader cycles (s_memtime) between the two}, wg = blockIdx.y * gridDim.x +
 * blockIdx.x < capacity_work_groups (dev_buf holds 4 * capacity_work_groups int64; work-groups beyond it write nothing);
 * NULL switches it off.  A forward that would CAPTURE a hipGraph while either diagnostic buffer is set is refused. */
int qasr_debug_timeline(void* dev_buf, size_t capacity_work_groups);

const char* qasr_last_error(void);
const char* qasr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QASR_H */
