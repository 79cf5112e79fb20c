// Host runtime of the integer-only ASR engine: blob parsing, static buffer arena, launch plan, C ABI.
// One engine per device; all work is enqueued on the caller's stream; no host synchronisation on the
// forward path (parity hooks excepted).  See include/qasr.h for the contract.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "qasr_internal.h"

#include <unordered_map>

using namespace qasr;

// ---- sub-byte weight storage (QASR_F_W6PACK): expansion to int8 at load time --------------------------------------
// In-register unpack would cost ~28 VALU instructions per 16-byte MFMA fragment (120 cycles against the MFMA's 32), so
// the packed form is what travels (file, RCCL broadcast) and the kernels keep reading int8 fragments.
__global__ void __launch_bounds__(256) k_unpack6(const uint8_t* __restrict__ in, int8_t* __restrict__ out, size_t n_quads) {
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned w = in[3 * q] | ((unsigned)in[3 * q + 1] << 8) | ((unsigned)in[3 * q + 2] << 16);
    unsigned o = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (int)((w >> (6 * i)) & 0x3f);
      o |= (unsigned)(((c ^ 0x20) - 0x20) & 0xff) << (8 * i);      // sign-extend the 6-bit field
    }
    ((unsigned*)out)[q] = o;
  }
}
// zero-margined tap rows of the MFMA depthwise stage: [c][kp + 32], taps behind 8 zero bytes (pack.py writes them
// into byte-per-code blobs; sub-byte blobs derive them here)
__global__ void __launch_bounds__(256) k_tap_rows(const int8_t* __restrict__ w, int8_t* __restrict__ out, int C, int K, int kp) {
  const int ks = kp + 32;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)C * ks; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / ks), j = (int)(i - (size_t)c * ks) - 8;
    out[i] = (j >= 0 && j < K) ? w[(size_t)c * kp + j] : (int8_t)0;
  }
}

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t _e = (x);                                                                   \
    if (_e != hipSuccess) return fail(QASR_ERR_HIP, "%s: %s", #x, hipGetErrorString(_e)); \
  } while (0)

// How an entry point that takes an args struct opens and closes: the struct is there and of this library's size; the launch
// function's code, then HIP's.  `who` is the entry's name in the message.  (Entries that accept an older, shorter struct and
// those whose text differs keep their own lines.)
template <class A>
static int args_check(const char* who, const A* a) {
  if (!a) return fail(QASR_ERR_ARG, "%s: args is NULL", who);
  if (a->struct_size != sizeof(A)) return fail(QASR_ERR_ARG, "%s: struct_size %u is not %zu", who, a->struct_size, sizeof(A));
  return QASR_OK;
}
static int launched(const char* who, int rc) {
  if (rc) return fail(rc, "%s: launch", who);
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }
static inline size_t dt_size(uint32_t dt) { return (dt == QASR_DT_F32 || dt == QASR_DT_I32) ? 4 : 1; }

struct TensorRT {
  qasr_tensor_desc d;
  int T = 0, Tp = 0;
  size_t bytes = 0;
  void* ptr = nullptr;
  int slot = -1;
};

struct qasr_engine {
  int device = 0;
  bool debug = false;                  // keep every tensor + dump int32 accumulators (parity hooks)
  bool timing = false;                 // per-op HIP events (qasr_engine_last_op_ms)
  std::vector<uint8_t> blob;           // host copy
  uint8_t* dblob = nullptr;            // device copy
  int8_t* dexp = nullptr;              // QASR_F_W6PACK: int8 expansion of every sub-byte weight array (+ derived tap rows)
  std::unordered_map<uint64_t, const int8_t*> wexp, wexp2;   // blob data offset -> expanded array / tap rows
  qasr_blob_header h{};
  const qasr_tensor_desc* tdesc = nullptr;
  const qasr_op_desc* ops = nullptr;
  const qasr_domain_desc* doms = nullptr;
  // shape plan
  int B = 0, T0 = 0;
  std::vector<int> domT;
  std::vector<TensorRT> tens;
  std::vector<void*> slots;            // owned device buffers
  std::vector<size_t> slot_bytes;
  int32_t* lens_all = nullptr;
  int32_t* time_tokens = nullptr;      // scratch token buffer for qasr_engine_time_ops
  std::vector<std::vector<int32_t*>> acc_dbg;   // [op][1 + pane]
  std::vector<hipEvent_t> ev;          // debug timing: n_ops + 1 events
  bool timed = false;
  bool fuse = true;                    // fuse depthwise -> pointwise pairs into k_sep (QASR_NO_FUSE=1 disables)
  std::vector<int> fused_dw;           // per op: index of the DW op fused into this PW op, or -1
  std::vector<char> skip;              // per op: launched as part of the following op
  bool fuse_stem = true;               // block 0 (lengths, first-layer quantisation, strided depthwise, 1x1) in one launch (QASR_NO_FUSE_STEM=1: four)
  bool stem = false;                   // ... and the plan has that shape: ops 0..2 run as k_stem
  bool fuse_norm = true;               // forward_audio: normalize_batch inside k_stem from k_mel's per-tile sums (qasr_engine_opts.fuse_norm)
  double* norm_stats = nullptr;        // [B][tiles][n_mels][2]
  size_t norm_stats_bytes = 0;
  int norm_tiles = 0, norm_frames = 0; // of the forward being enqueued (0: the stem reads normalised features)
  int fe_launches = 0;                 // front-end kernels of the last forward (forward_audio: k_mel [+ k_norm])
  const int32_t* cur_lens = nullptr;   // the caller's lengths of the current / last forward (k_stem derives every domain's from them)
  bool fuse_dec = true;                // decoder conv + log-softmax + argmax in one launch (QASR_NO_FUSE_DEC=1: two launches)
  std::vector<char> rq_skip;           // per op: REQUANT op served by the launch of an earlier REQUANT op of the same stored value
  std::vector<char> dec_skip;          // per op: LOGSOFTMAX op that ran inside the preceding decoder launch
  std::vector<char> dec_wide;          // per op: decoder op that ran as k_decw (two launches)
  void* decw_ws = nullptr;             // k_decw's per-(frame, class group) partials: part of the plan (no allocation in forward)
  size_t decw_ws_bytes = 0;
  bool tile128 = true;                 // tile_frames == 128 (QASR_TILE128=0: k_sep2's plain layers stay on 64-frame tiles, A/B runs)
  int res_tile = 128;                  // frames per work-group of the block-end layers of a tile_frames == 128 engine: 128, 64 or 32
                                       // (qasr_engine_opts.res_tile128; its default goes by res_tile_default())
  bool dense_tile128 = true;           // QASR_DENSE_TILE128=0 keeps Jasper's dense convs on 64-frame tiles (A/B runs)
  bool wide_tiles = false;             // k_sep with 64-frame tiles (throughput mode: bit 3 of `debug`, or QASR_WIDE_TILES=1)
  int mask_skip = -1;                  // k_sep2s (mask-skip rule): -1 = when reserved, 0 = never, 1 = always (qasr_engine_opts.mask_skip)
  int sep_gen = 2;                     // 2: k_sep2 where it has the shape; 1 (QASR_SEP_GEN=1): k_sep everywhere (A/B runs)
  // qasr_engine_opts.pair_split: the plain 512 -> 512 layers of a tile_frames == 128 engine as k_sep2p (two work-groups per tile)
  bool pair_split = false;
  std::vector<char> paired;            // per op: launched in the paired form (empty: none)
  std::vector<size_t> pair_flag_off;   // per op: byte offset of its flag words in pair_flags
  unsigned* pair_flags = nullptr;      // every paired op's flag words: an allocation of their own, zeroed once per forward (by k_stem, or by ONE k_pair_zero node without the fused stem)
  size_t pair_flag_bytes = 0;
  unsigned* pair_tmo = nullptr;        // 256 B: the time-out word of the former hand-off; no kernel writes it, qasr_engine_pair_timeouts reads 0
  // the unpaired plain layers of a tile_frames == 128 engine on 64-frame halves: by half_tiles_default(), QASR_HALF_TILES
  bool half_tiles = false;
  std::vector<char> halved;            // per op: launched in the halved form (empty: none)
  bool in_forward = false;             // launch_op runs inside enqueue_forward (which zeroes the flags: k_pair_zero in front, or k_stem)
  // hipGraph replay (bit 4 of `debug`): the whole forward of one (shape, buffer set) is captured once and re-launched
  // with one call; key = the caller's pointers, which a serving loop keeps stable
  bool forwarded = false;              // a forward has been enqueued with the current plan
  bool use_graph = false;
  hipGraphExec_t gexec = nullptr;
  const void* gkey[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // everything else the captured front-end nodes bake in: S, n_mels, pad_to, preemph (bits), fb, window (a caller that
  // reuses its buffers with another S of equal T_pad, or swaps the filterbank, must not replay the old graph)
  uint64_t gfe[6] = {0, 0, 0, 0, 0, 0};
  int gcalls = 0;                      // forwards seen with the current key (1st: direct launches, 2nd: capture)
  // qasr_engine_attach_ctc: per-frame best-path score from the decoder kernel and / or k_ctc behind it
  float* ctc_fs = nullptr;
  qasr_ctc_out ctc_out{};
  bool ctc_on = false;                 // ctc_out is attached: one more launch
  int ctc_use_lens = 0;
  uint64_t gctc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the attachment a captured graph bakes in
  // qasr_engine_ragged_stats: every hipMalloc / hipFree this engine makes goes through dev_alloc / dev_free
  uint64_t n_allocs = 0, n_frees = 0;
  // qasr_engine_reserve: the plan, staging and output buffers are allocated once for the envelope max_batch x max_frames;
  // qasr_engine_forward_ragged[_audio] re-derive the launch parameters for a bucket shape inside it and never allocate
  struct Bucket {
    int frames = 0;
    uint64_t calls = 0;
    hipGraphExec_t gexec = nullptr;
    uint64_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // what the graph bakes in besides the engine's own buffers (front-end arguments)
  };
  struct Reserved {
    bool on = false;
    int max_batch = 0, max_samples = 0, max_frames = 0, n_mels = 0, pad_to = 16, max_graphs = 16;
    int spitch = 0, out_frames = 0;      // staging pitch of an audio row; T' of max_frames
    bool want_logp = false, decode = false;
    int decode_use_lens = 1;
    float* audio = nullptr;              // [max_batch][spitch]
    int32_t* audio_lens = nullptr;       // [max_batch]
    float* feats = nullptr;              // [max_batch][n_mels or feat_in][max_frames]
    int32_t* feat_lens = nullptr;        // [max_batch]
    int32_t* shp = nullptr;              // shape block, QASR_SHAPE_WORDS i32
    int32_t* tokens = nullptr;
    int32_t* lens_out = nullptr;
    float* logp = nullptr;
    float* fs = nullptr;
    qasr_ctc_out ctc{};
    std::vector<void*> owned;
    std::vector<Bucket> buckets;
    uint64_t captured = 0, replays = 0, eager = 0;
  } rs;
  const int32_t* ctc_t_act = nullptr;  // ragged forward being enqueued: k_ctc walks the batch's own T' (shape block)
};

static hipError_t dev_alloc(qasr_engine* e, void** p, size_t n) {
  hipError_t rc = hipMalloc(p, n);
  if (rc == hipSuccess) e->n_allocs++;
  return rc;
}
static void dev_free(qasr_engine* e, void* p) {
  if (!p) return;
  (void)hipFree(p);
  e->n_frees++;
}

template <class T>
static const T* dev_at(const qasr_engine* e, uint64_t off) {
  return off ? reinterpret_cast<const T*>(e->dblob + e->h.data_off + off) : nullptr;
}
// int8 weight array at blob offset `off`: the blob bytes, or their load-time expansion for sub-byte blobs
static const int8_t* dev_w(const qasr_engine* e, uint64_t off) {
  if (!off) return nullptr;
  auto it = e->wexp.find(off);
  return it != e->wexp.end() ? it->second : dev_at<int8_t>(e, off);
}

static int conv_out_len(int len, const qasr_domain_desc& d) {
  int num = len + 2 * (int)d.padding - (int)d.dilation * ((int)d.kernel - 1) - 1;
  int q = num >= 0 ? num / (int)d.stride : -((-num + (int)d.stride - 1) / (int)d.stride);
  return q + 1;
}

static void free_plan(qasr_engine* e) {
  for (void* p : e->slots) dev_free(e, p);
  e->slots.clear();
  e->slot_bytes.clear();
  dev_free(e, e->lens_all);
  e->lens_all = nullptr;
  dev_free(e, e->time_tokens);
  e->time_tokens = nullptr;
  dev_free(e, e->norm_stats);
  e->norm_stats = nullptr;
  e->norm_stats_bytes = 0;
  e->norm_tiles = e->norm_frames = 0;
  dev_free(e, e->decw_ws);
  e->decw_ws = nullptr;
  e->decw_ws_bytes = 0;
  dev_free(e, e->pair_flags);
  e->pair_flags = nullptr;
  e->pair_flag_bytes = 0;
  dev_free(e, e->pair_tmo);
  e->pair_tmo = nullptr;
  e->paired.clear();
  e->pair_flag_off.clear();
  e->halved.clear();
  for (auto& v : e->acc_dbg)
    for (auto p : v)
      dev_free(e, p);
  e->acc_dbg.clear();
  e->tens.clear();
  e->B = e->T0 = 0;
  e->forwarded = false;
}

static void build_sep(qasr_engine* e, uint32_t oi, SepP& p);

// Launch parameters of a shape: frames per time domain, every tensor's frames / row pitch / bytes, the fusion plan.
// Host only.  Arena slots and pointers a tensor already holds are kept: a reserved engine calls this per bucket.
static int plan_shape(qasr_engine* e, int B, int T0) {
  const auto& h = e->h;
  e->domT.assign(h.n_domains, 0);
  e->domT[0] = T0;
  for (uint32_t d = 1; d < h.n_domains; ++d) e->domT[d] = conv_out_len(e->domT[e->doms[d].parent], e->doms[d]);
  for (uint32_t d = 0; d < h.n_domains; ++d)
    if (e->domT[d] <= 0) return fail(QASR_ERR_ARG, "input of %d frames is too short for domain %u", T0, d);
  e->tens.resize(h.n_tensors);
  for (uint32_t i = 0; i < h.n_tensors; ++i) {
    TensorRT& t = e->tens[i];
    t.d = e->tdesc[i];
    t.T = e->domT[t.d.domain];
    t.Tp = rup(t.T, 64);
    // f32 logits are [B][T][C]; everything else [B][C][Tp]
    t.bytes = (t.d.dtype == QASR_DT_F32) ? (size_t)B * t.T * t.d.channels * 4 : (size_t)B * t.d.channels * t.Tp * dt_size(t.d.dtype);
    t.bytes = (t.bytes + 255) / 256 * 256;
  }
  // fusion plan first: it moves the point where a depthwise input is read to the following launch
  e->fused_dw.assign(h.n_ops, -1);
  e->skip.assign(h.n_ops, 0);
  e->dec_skip.assign(h.n_ops, 0);
  e->dec_wide.assign(h.n_ops, 0);
  e->rq_skip.assign(h.n_ops, 0);
  if (e->fuse)
    for (uint32_t oi = 0; oi + 1 < h.n_ops; ++oi) {
      const qasr_op_desc& d = e->ops[oi];
      const qasr_op_desc& q = e->ops[oi + 1];
      if (d.kind != QASR_OP_DW || q.kind != QASR_OP_PW) continue;
      const uint32_t same_pad = d.dilation > 1 ? (d.dilation * d.kernel) / 2 - 1 : d.kernel / 2;
      if (d.stride != 1 || d.padding != same_pad || !(d.kernel & 1) || !sep_supported((int)d.kernel, (int)d.dilation)) continue;
      if (d.outs[1].tensor >= 0 || d.outs[0].mode != 1 || q.in != d.outs[0].tensor) continue;
      if (e->tdesc[d.outs[0].tensor].last_use != (int)oi + 1 || (d.flags & QASR_F_EXACT_Z)) continue;
      e->fused_dw[oi + 1] = (int)oi;
      e->skip[oi] = 1;
    }
  e->B = B;
  e->T0 = T0;
  return QASR_OK;
}

// Allocates for the shape plan_shape derived last: arena, length tables, workspaces.  A reserved engine calls it once,
// for its maximum; every smaller shape fits the same slots (a tensor's bytes grow with B and T, its lifetime does not move).
static int plan_alloc(qasr_engine* e) {
  const auto& h = e->h;
  const int B = e->B, T0 = e->T0;
  // a production engine's fused wide decoder (k_decw) never stores the float logits [B][T][C] (167 MB at bs32 x 500
  // frames x 5207 classes): that tensor gets no arena slot; launch_op takes the same decision from the same shapes
  std::vector<char> no_slot(h.n_tensors, 0);
  if (e->fuse_dec && !e->debug)
    for (uint32_t oi = 0; oi + 1 < h.n_ops; ++oi) {
      const qasr_op_desc& op = e->ops[oi];
      if (op.kind != QASR_OP_PW || !(op.flags & QASR_F_LOGITS) || e->ops[oi + 1].kind != QASR_OP_LOGSOFTMAX ||
          e->ops[oi + 1].in != op.outs[0].tensor)
        continue;
      SepP p{};
      build_sep(e, oi, p);
      if (!decoder_fusable(p) && decoder_wide_fusable(p)) no_slot[op.outs[0].tensor] = 1;
    }
  // greedy arena: a slot is reused once its tensor's last reader has been enqueued (stream order makes that safe)
  std::vector<int> free_slots;
  auto acquire = [&](TensorRT& t) -> int {
    int best = -1;
    if (!e->debug)
      for (size_t k = 0; k < free_slots.size(); ++k) {
        int s = free_slots[k];
        if (e->slot_bytes[s] >= t.bytes && (best < 0 || e->slot_bytes[s] < e->slot_bytes[free_slots[best]])) best = (int)k;
      }
    int s;
    if (best >= 0) {
      s = free_slots[best];
      free_slots.erase(free_slots.begin() + best);
    } else {
      void* p = nullptr;
      if (dev_alloc(e, &p, t.bytes) != hipSuccess) return -1;
      e->slots.push_back(p);
      e->slot_bytes.push_back(t.bytes);
      s = (int)e->slots.size() - 1;
    }
    t.slot = s;
    t.ptr = e->slots[s];
    return s;
  };
  for (uint32_t oi = 0; oi < h.n_ops; ++oi) {
    for (uint32_t i = 1; i < h.n_tensors; ++i)      // tensor 0 is the caller's feature buffer
      if (e->tens[i].d.producer == (int)oi && !no_slot[i] && acquire(e->tens[i]) < 0) return fail(QASR_ERR_HIP, "hipMalloc failed (arena)");
    for (uint32_t i = 1; i < h.n_tensors; ++i) {
      TensorRT& t = e->tens[i];
      // a depthwise op fused into the next op's launch reads its input THERE: the input must outlive that launch,
      // or the fused kernel's output could be planned into the very buffer its halo reads come from
      int last = std::max(t.d.last_use, t.d.producer);
      if (last >= 0 && last + 1 < (int)h.n_ops && e->skip[last]) last += 1;
      bool dead_after = t.d.producer <= (int)oi && t.slot >= 0 && last == (int)oi;
      if (dead_after && !e->debug) free_slots.push_back(t.slot);
    }
  }
  HIPCHK(dev_alloc(e, (void**)&e->lens_all, sizeof(int32_t) * h.n_domains * B));
  for (uint32_t oi = 0; oi < h.n_ops; ++oi) {                // k_decw's workspace, for a decoder wider than k_dec's 32 classes
    const qasr_op_desc& op = e->ops[oi];
    if (op.kind != QASR_OP_PW || !(op.flags & QASR_F_LOGITS) || op.cout <= 32) continue;
    const size_t need = decoder_wide_ws_bytes(B, e->tens[op.outs[0].tensor].Tp);
    if (need > e->decw_ws_bytes) {
      dev_free(e, e->decw_ws);
      e->decw_ws = nullptr;
      e->decw_ws_bytes = 0;
      HIPCHK(dev_alloc(e, &e->decw_ws, need));
      e->decw_ws_bytes = need;
    }
  }
  HIPCHK(dev_alloc(e, (void**)&e->time_tokens, sizeof(int32_t) * (size_t)B * (T0 + 64)));
  if (e->debug) {
    e->acc_dbg.resize(h.n_ops);
    for (uint32_t oi = 0; oi < h.n_ops; ++oi) {
      const qasr_op_desc& op = e->ops[oi];
      if (op.kind != QASR_OP_DW && op.kind != QASR_OP_PW && op.kind != QASR_OP_DENSE) continue;
      const TensorRT& o = e->tens[op.outs[0].tensor];
      size_t n = (size_t)B * op.cout * rup(o.T, 64);
      for (uint32_t k = 0; k < 1 + op.n_panes; ++k) {
        int32_t* p = nullptr;
        HIPCHK(dev_alloc(e, (void**)&p, n * 4));
        HIPCHK(hipMemset(p, 0, n * 4));
        e->acc_dbg[oi].push_back(p);
      }
    }
  }
  if (e->timing && e->ev.empty()) {
    e->ev.resize(h.n_ops + 1);
    for (auto& v : e->ev) HIPCHK(hipEventCreate(&v));
  }
  return QASR_OK;
}

// Which ops run in the paired form, and their completion words.  Never for debug / timing engines (hooks, per-op events), tiles
// below 128, reserved engines (they do not come through build_plan); sep_pair_ok leaves only the production launches of
// k_sep2<51 | 63 | 75, 4, 0, 2, false, 128, 1>.
static int plan_pairs(qasr_engine* e) {
  const auto& h = e->h;
  if (!e->pair_split || e->debug || e->timing || !e->wide_tiles || !e->tile128 || e->rs.on) return QASR_OK;
  std::vector<char> paired(h.n_ops, 0);
  std::vector<size_t> off(h.n_ops, 0);
  size_t fb = 0;
  for (uint32_t oi = 0; oi < h.n_ops; ++oi) {
    if (e->ops[oi].kind != QASR_OP_PW || e->skip[oi] || e->fused_dw[oi] < 0) continue;
    SepP p{};
    build_sep(e, oi, p);
    if (!sep_pair_ok(p)) continue;
    paired[oi] = 1;
    off[oi] = fb;
    fb += sep_pair_flag_bytes(p.e.B, p.e.Tp);
  }
  if (!fb) return QASR_OK;
  HIPCHK(dev_alloc(e, (void**)&e->pair_flags, fb));
  HIPCHK(dev_alloc(e, (void**)&e->pair_tmo, 256));
  HIPCHK(hipMemset(e->pair_flags, 0, fb));
  HIPCHK(hipMemset(e->pair_tmo, 0, 256));
  e->pair_flag_bytes = fb;
  e->paired.swap(paired);
  e->pair_flag_off.swap(off);
  return QASR_OK;
}

// Which ops run in the halved form (after plan_pairs: a paired op is never halved).  The same engines as plan_pairs; sep_half_ok
// leaves the unpaired plain production launches of 128-frame tiles whose shape class is in sep2_half_shape.
static void plan_halves(qasr_engine* e) {
  const auto& h = e->h;
  if (!e->half_tiles || e->debug || e->timing || !e->wide_tiles || !e->tile128 || e->rs.on) return;
  std::vector<char> halved(h.n_ops, 0);
  bool any = false;
  for (uint32_t oi = 0; oi < h.n_ops; ++oi) {
    if (e->ops[oi].kind != QASR_OP_PW || e->skip[oi] || e->fused_dw[oi] < 0) continue;
    SepP p{};
    build_sep(e, oi, p);
    if (sep_half_ok(p)) halved[oi] = 1, any = true;
  }
  if (any) e->halved.swap(halved);
}

static int build_plan(qasr_engine* e, int B, int T0) {
  free_plan(e);
  int rc = plan_shape(e, B, T0);
  if (rc) {
    e->B = e->T0 = 0;
    return rc;
  }
  rc = plan_alloc(e);
  if (!rc) rc = plan_pairs(e);
  if (!rc) plan_halves(e);
  if (rc) e->B = e->T0 = 0;
  return rc;
}

static void fill_out(const qasr_engine* e, const qasr_out& o, OutP& d) {
  d.ptr = e->tens[o.tensor].ptr;
  d.mtab = dev_at<double>(e, o.m_off);
  d.m = o.m;
  d.lo = o.lo;
  d.hi = o.hi;
  d.mode = (int)o.mode;
  d.pad_ = 0;
}

static int fill_epi(const qasr_engine* e, int oi, const qasr_op_desc& op, EpiP& ep) {
  memset(&ep, 0, sizeof ep);
  int n = 0;
  for (int j = 0; j < QASR_MAX_OUTS; ++j)
    if (op.outs[j].tensor >= 0) fill_out(e, op.outs[j], ep.outs[n++]);
  ep.n_outs = n;
  ep.flags = op.flags;
  ep.sb = dev_at<float>(e, op.sb_off);
  ep.m_main = dev_at<double>(e, op.m_off);
  const TensorRT& o0 = e->tens[op.outs[0].tensor];
  ep.lens = e->lens_all + (size_t)o0.d.domain * e->B;
  ep.acc_dbg = (e->debug && !e->acc_dbg[oi].empty()) ? e->acc_dbg[oi][0] : nullptr;
  ep.qlo = op.qlo;
  ep.qhi = op.qhi;
  ep.T = o0.T;
  ep.Tp = rup(o0.T, 64);
  ep.cout = (int)op.cout;
  ep.B = e->B;
  if (op.flags & QASR_F_LOGITS) {
    ep.logits = (float*)o0.ptr;
    ep.n_outs = 0;
  }
  return QASR_OK;
}

static void fill_panes(const qasr_engine* e, int oi, const qasr_op_desc& op, PaneP* panes) {
  for (uint32_t k = 0; k < op.n_panes; ++k) {
    const qasr_pane& s = op.panes[k];
    PaneP& d = panes[k];
    const TensorRT& t = e->tens[s.in];
    d.x = (const int8_t*)t.ptr;
    d.w = dev_w(e, s.w_off);
    d.bias = dev_at<int32_t>(e, s.bias_off);
    d.m = dev_at<double>(e, s.m_off);
    d.sb = dev_at<float>(e, s.sb_off);
    d.acc_dbg = e->debug ? e->acc_dbg[oi][1 + k] : nullptr;
    d.cin = (int)s.cin;
    d.cin_pad = rup((int)s.cin, 128);
    d.x_unsigned = t.d.dtype == QASR_DT_U8;
    d.pad_ = 0;
  }
}

extern "C" {

const char* qasr_last_error(void) { return g_err.c_str(); }
const char* qasr_version(void) { return "qasr-hip 0.1 (gfx950)"; }

int qasr_debug_prof(void* dev_buf) {
  qasr::g_prof = (long long*)dev_buf;
  qasr::g_prof_mode = 0;
  qasr::g_prof_cap = 0;
  return QASR_OK;
}
int qasr_debug_timeline(void* dev_buf, size_t capacity_work_groups) {
  if (dev_buf && (capacity_work_groups < 1 || capacity_work_groups > (1u << 22))) return fail(QASR_ERR_ARG, "debug_timeline: capacity");
  qasr::g_prof = (long long*)dev_buf;
  qasr::g_prof_mode = dev_buf ? 1 : 0;
  qasr::g_prof_cap = dev_buf ? (int)capacity_work_groups : 0;
  return QASR_OK;
}

void qasr_engine_default_opts(qasr_engine_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->struct_size = (uint32_t)sizeof *o;
  o->fuse_dw = o->fuse_stem = o->fuse_decoder = o->res_tile128 = o->dense_tile128 = o->fuse_norm = o->mask_skip = o->pair_split = -1;
}

// Block-end tile of a tile_frames == 128 engine when the caller leaves qasr_engine_opts.res_tile128 at -1.  What decides is how
// many launch chains run side by side, and the one thing the engine can know about that is the process's hardware queue count:
// HIP spreads a process's streams over GPU_MAX_HW_QUEUES queues (4 when unset), and four streams on fewer than
// QASR_SIDE_BY_SIDE_QUEUES queues run pairwise.  Two chains of 64-work-group launches leave half the CUs without a work-group
// and the step pays each chain's own latency: the block-end layers then take the smaller tile (more, shorter work-groups).
// With a queue per chain four chains fill the chip and the 128-frame tile is the cheaper one.
#define QASR_SIDE_BY_SIDE_QUEUES 8      /* smallest tested count (4, 8) at which four streams' chains ran side by side */
#define QASR_RES_TILE_FEW_CHAINS 64     /* two chains in flight, ms/step: 128 frames 0.584, 64 frames 0.543 - 0.550, 32 frames 0.551 - 0.558 */
static long hw_queues_hint() {
  long q = 4;                                               // HIP's own default
  if (const char* g = getenv("GPU_MAX_HW_QUEUES")) {
    char* end = nullptr;
    const long v = strtol(g, &end, 10);
    if (end != g && v >= 1) q = v;
  }
  return q;
}
static int res_tile_default() { return hw_queues_hint() >= QASR_SIDE_BY_SIDE_QUEUES ? 128 : QASR_RES_TILE_FEW_CHAINS; }
// qasr_engine_opts.pair_split at -1, by the same hint: two chains at a time leave half the CUs idle behind the 64-work-group
// launches of the plain 512 -> 512 layers, and a tile on two work-groups halves their span; with four chains
// side by side the chip is full and the plan stays as it is.
static bool pair_split_default() { return hw_queues_hint() < QASR_SIDE_BY_SIDE_QUEUES; }
// The unpaired plain layers' 128-frame tiles as two 64-frame work-groups, by the same hint: with two chains at a time their 64
// work-groups become 128, one chain's plus the other's fill the 256 CUs, and a shorter work-group shortens the chain
// (DESIGN.md 5.10); from QASR_SIDE_BY_SIDE_QUEUES queues the plan stays as it is.  No option field: QASR_HALF_TILES=0|1 overrides.
static bool half_tiles_default() { return hw_queues_hint() < QASR_SIDE_BY_SIDE_QUEUES; }

// the `debug` bits of round 1 / 2 callers, as options
int qasr_engine_create(const void* blob, size_t n, int device, int debug, qasr_engine** out) {
  qasr_engine_opts o;
  qasr_engine_default_opts(&o);
  o.debug = (uint32_t)debug & 3u;
  if (debug & 4) return fail(QASR_ERR_UNSUPPORTED, "qasr_engine_create: bit 2 (k_utt) was retired in round 4");
  o.tile_frames = (debug & 8) ? 128 : 32;
  o.graph = (debug & 16) != 0;
  o.fuse_norm = 0;       // callers of this entry read `feats` of qasr_engine_forward_audio as the NORMALISED log-mel (rounds 1 / 2)
  return qasr_engine_create_ex(blob, n, device, &o, out);
}

int qasr_engine_create_ex(const void* blob, size_t n, int device, const qasr_engine_opts* opts, qasr_engine** out) {
  if (!blob || !out || n < sizeof(qasr_blob_header)) return fail(QASR_ERR_ARG, "null / short blob");
  qasr_engine_opts o;
  qasr_engine_default_opts(&o);
  if (opts) {
    if (opts->struct_size < 8 || opts->struct_size > sizeof o) return fail(QASR_ERR_ARG, "qasr_engine_opts.struct_size %u (this library: %zu)", opts->struct_size, sizeof o);
    memcpy(&o, opts, opts->struct_size);                     // an older, shorter struct keeps the defaults of the newer fields
    o.struct_size = (uint32_t)sizeof o;
  }
  if (o.tile_frames != 0 && o.tile_frames != 32 && o.tile_frames != 64 && o.tile_frames != 128)
    return fail(QASR_ERR_ARG, "qasr_engine_opts.tile_frames %d (0, 32, 64 or 128)", o.tile_frames);
  if (o.sep_gen < 0 || o.sep_gen > 2) return fail(QASR_ERR_ARG, "qasr_engine_opts.sep_gen %d (0, 1 or 2)", o.sep_gen);
  if (o.retired_whole_utterance > 0 || o.retired_legacy_pw > 0 || o.retired_persistent > 0)
    return fail(QASR_ERR_UNSUPPORTED, "qasr_engine_opts: whole_utterance / legacy_pw / persistent were retired in round 4 (include/qasr.h)");
  const int debug = (int)o.debug;
  {                                                          // every offset / index / shape of the blob, before any HIP call
    char why[256];
    if (qasr_blob_check(blob, n, why, sizeof why) != QASR_OK) return fail(QASR_ERR_BLOB, "%s", why);
  }
  qasr_blob_header h;
  memcpy(&h, blob, sizeof h);
  HIPCHK(hipSetDevice(device));
  qasr_engine* e = new qasr_engine();
  e->device = device;
  e->debug = (debug & 1) != 0;
  e->timing = (debug & 3) != 0;
  auto tri = [](int32_t v, bool dflt) { return v < 0 ? dflt : v != 0; };
  e->fuse = tri(o.fuse_dw, true);
  e->fuse_stem = tri(o.fuse_stem, true);
  e->fuse_dec = tri(o.fuse_decoder, true);
  e->fuse_norm = tri(o.fuse_norm, true);
  e->wide_tiles = o.tile_frames >= 64;
  e->tile128 = o.tile_frames == 128;
  e->res_tile = o.res_tile128 < 0 ? res_tile_default() : (o.res_tile128 ? 128 : 64);
  e->dense_tile128 = tri(o.dense_tile128, true);
  e->sep_gen = o.sep_gen == 1 ? 1 : 2;
  e->mask_skip = o.mask_skip < 0 ? -1 : (o.mask_skip != 0);
  e->pair_split = o.pair_split < 0 ? pair_split_default() : o.pair_split != 0;
  e->half_tiles = half_tiles_default();
  e->use_graph = o.graph > 0;
  // environment: A/B overrides for profiling runs of an unmodified caller (include/qasr.h lists them), read per create call
  if (getenv("QASR_NO_FUSE")) e->fuse = false;
  if (getenv("QASR_WIDE_TILES")) { e->wide_tiles = true; e->tile128 = true; }
  if (const char* g = getenv("QASR_TILE128")) e->tile128 = atoi(g) != 0;
  if (const char* g = getenv("QASR_RES_TILE128")) e->res_tile = atoi(g) != 0 ? 128 : 64;
  if (const char* g = getenv("QASR_RES_TILE")) {
    const int v = atoi(g);
    if (v == 32 || v == 64 || v == 128) e->res_tile = v;
  }
  if (const char* g = getenv("QASR_NO_FUSE_DEC")) e->fuse_dec = atoi(g) == 0;
  if (const char* g = getenv("QASR_NO_FUSE_STEM")) e->fuse_stem = atoi(g) == 0;
  if (const char* g = getenv("QASR_NO_FUSE_NORM")) e->fuse_norm = atoi(g) == 0;
  if (const char* g = getenv("QASR_DENSE_TILE128")) e->dense_tile128 = atoi(g) != 0;
  if (const char* g = getenv("QASR_SEP_GEN")) e->sep_gen = atoi(g) == 1 ? 1 : 2;
  if (const char* g = getenv("QASR_PAIR_SPLIT")) e->pair_split = atoi(g) != 0;
  if (const char* g = getenv("QASR_HALF_TILES")) e->half_tiles = atoi(g) != 0;
  e->blob.assign((const uint8_t*)blob, (const uint8_t*)blob + n);
  e->h = h;
  e->tdesc = (const qasr_tensor_desc*)(e->blob.data() + h.tensors_off);
  e->ops = (const qasr_op_desc*)(e->blob.data() + h.ops_off);
  e->doms = (const qasr_domain_desc*)(e->blob.data() + h.domains_off);
  if (dev_alloc(e, (void**)&e->dblob, n + 256) != hipSuccess ||      // slack: 16-byte granule copies may overrun an array's tail
      hipMemcpy(e->dblob, blob, n, hipMemcpyHostToDevice) != hipSuccess) {
    delete e;
    return fail(QASR_ERR_HIP, "blob upload failed");
  }
  // sub-byte blobs: expand every packed weight array (and derive the depthwise tap rows) once, on the device
  {
    struct Job { uint64_t off; size_t packed, expanded; int C, K, kp; };
    std::vector<Job> jobs;
    size_t total = 0;
    auto add = [&](uint64_t off, size_t expanded, int C = 0, int K = 0, int kp = 0) {
      if (!off || e->wexp.count(off)) return;
      e->wexp[off] = nullptr;
      jobs.push_back({off, expanded / 4 * 3, expanded, C, K, kp});
      total += (expanded + 255) / 256 * 256;
      if (C) total += ((size_t)C * (kp + 32) + 64 + 255) / 256 * 256;
    };
    for (uint32_t i = 0; i < h.n_ops; ++i) {
      const qasr_op_desc& op = e->ops[i];
      if (!(op.flags & QASR_F_W6PACK)) continue;
      const size_t cp = rup((int)op.cout, 128), cinp = rup((int)op.cin, 128);
      if (op.kind == QASR_OP_DW) add(op.w_off, (size_t)op.cout * rup((int)op.kernel, 4), (int)op.cout, (int)op.kernel, rup((int)op.kernel, 4));
      else add(op.w_off, cp * cinp * (op.kind == QASR_OP_DENSE ? op.kernel : 1));
      for (uint32_t k = 0; k < op.n_panes; ++k) add(op.panes[k].w_off, cp * (size_t)rup((int)op.panes[k].cin, 128));
    }
    if (!jobs.empty()) {
      if (dev_alloc(e, (void**)&e->dexp, total) != hipSuccess) {
        qasr_engine_destroy(e);
        return fail(QASR_ERR_HIP, "weight expansion buffer (%zu bytes)", total);
      }
      size_t pos = 0;
      for (const Job& j : jobs) {
        if (h.data_off + j.off + j.packed > n) {
          qasr_engine_destroy(e);
          return fail(QASR_ERR_BLOB, "packed weight array out of range");
        }
        int8_t* dst = e->dexp + pos;
        pos += (j.expanded + 255) / 256 * 256;
        hipLaunchKernelGGL(k_unpack6, dim3(1024), dim3(256), 0, 0, e->dblob + h.data_off + j.off, dst, j.expanded / 4);
        e->wexp[j.off] = dst;
        if (j.C) {
          int8_t* rows = e->dexp + pos;
          pos += ((size_t)j.C * (j.kp + 32) + 64 + 255) / 256 * 256;
          (void)hipMemsetAsync(rows, 0, (size_t)j.C * (j.kp + 32) + 64, 0);
          hipLaunchKernelGGL(k_tap_rows, dim3(256), dim3(256), 0, 0, dst, rows, j.C, j.K, j.kp);
          e->wexp2[j.off] = rows;
        }
      }
      if (hipDeviceSynchronize() != hipSuccess) {
        qasr_engine_destroy(e);
        return fail(QASR_ERR_HIP, "weight expansion failed");
      }
    }
  }
  *out = e;
  return QASR_OK;
}

void qasr_engine_destroy(qasr_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
  for (auto& bk : e->rs.buckets)
    if (bk.gexec) (void)hipGraphExecDestroy(bk.gexec);
  for (void* p : e->rs.owned) dev_free(e, p);
  free_plan(e);
  for (auto v : e->ev) (void)hipEventDestroy(v);
  dev_free(e, e->dblob);
  dev_free(e, e->dexp);
  delete e;
}

int qasr_engine_num_ops(const qasr_engine* e) { return e ? (int)e->h.n_ops : -1; }

int qasr_engine_num_launches(const qasr_engine* e) {
  if (!e || !e->B || !e->forwarded) return -1;
  int n = (e->stem ? 0 : 1) + e->fe_launches;               // (k_lens, which the stem absorbs; front-end of forward_audio)
  for (uint32_t oi = 0; oi < e->h.n_ops; ++oi) {
    if (e->skip[oi] || e->dec_skip[oi] || e->rq_skip[oi] || (e->stem && oi >= 1 && oi <= 2)) continue;
    n += e->dec_wide[oi] ? 2 : 1;                            // k_decw: statistics + output launches
  }
  return n + (e->ctc_on ? 1 : 0);                            // k_ctc behind the decoder
}

int qasr_engine_out_frames(const qasr_engine* e, int T) {
  if (!e) return -1;
  std::vector<int> dT(e->h.n_domains);
  dT[0] = T;
  for (uint32_t d = 1; d < e->h.n_domains; ++d) dT[d] = conv_out_len(dT[e->doms[d].parent], e->doms[d]);
  const qasr_op_desc& last = e->ops[e->h.n_ops - 1];
  return dT[e->tdesc[last.in].domain];
}

// parameter block of the fused separable-layer kernels (k_sep2 / k_sep / k_dense2) for PW op `oi`
static void build_sep(qasr_engine* e, uint32_t oi, SepP& p) {
  const qasr_op_desc& op = e->ops[oi];
  const TensorRT& tin = e->tens[op.in];
  p.w = dev_w(e, op.w_off);
  p.bias = dev_at<int32_t>(e, op.bias_off);
  p.cin = (int)op.cin;
  p.cin_pad = rup(p.cin, 128);
  p.n_panes = (int)op.n_panes;
  p.tile = e->wide_tiles ? (e->tile128 ? 128 : 64) : 32;   // 128: k_sep2's separable layers only (sep2_tile), everything else 64
  p.etile = p.tile;
  // block-end layers: the engine's own tile (32 only for the separable form: dense and bare 1x1 block ends have 64 as their smallest)
  if (p.tile == 128 && (op.flags & QASR_F_RESADD)) p.tile = (e->res_tile == 32 && e->fused_dw[oi] < 0) ? 64 : e->res_tile;
  p.gen = e->sep_gen;
  p.mask_skip = e->mask_skip < 0 ? e->rs.on : e->mask_skip != 0;
  if (!e->paired.empty() && e->paired[oi]) {
    p.pair = 1;
    p.pair_flags = (unsigned*)((unsigned char*)e->pair_flags + e->pair_flag_off[oi]);
  }
  if (!e->halved.empty() && e->halved[oi]) p.half = 1;
  fill_panes(e, oi, op, p.panes);
  fill_epi(e, oi, op, p.e);
  const int di = e->fused_dw[oi];
  if (di >= 0) {
    const qasr_op_desc& d = e->ops[di];
    const TensorRT& din = e->tens[d.in];
    p.x = (const int8_t*)din.ptr;
    p.wdw = dev_w(e, d.w_off);
    {                                                       // zero-margined tap rows: in the blob (m_off), or derived on load
      auto it = e->wexp2.find(d.w_off);
      p.wdw2 = it != e->wexp2.end() ? it->second : dev_at<int8_t>(e, d.m_off);
    }
    p.bias_dw = dev_at<int32_t>(e, d.bias_off);
    p.m_dw = dev_at<double>(e, d.outs[0].m_off);
    p.dw_acc_dbg = (e->debug && !e->acc_dbg[di].empty()) ? e->acc_dbg[di][0] : nullptr;
    p.dw_lo = d.outs[0].lo;
    p.dw_hi = d.outs[0].hi;
    p.K = (int)d.kernel;
    p.dilation = (int)d.dilation;
    p.x_unsigned = din.d.dtype == QASR_DT_U8;
    p.pw_unsigned = 0;
    if (d.flags & QASR_F_WIDE_RQ) p.gen = 1;                // k_sep2 clamps on the low word of the rounded product
  } else {
    p.x = (const int8_t*)tin.ptr;
    p.K = 0;
    p.dilation = 1;
    p.pw_unsigned = tin.d.dtype == QASR_DT_U8;
    if (op.kind == QASR_OP_DENSE) {
      p.dense_k = (int)op.kernel;
      p.dilation = (int)op.dilation;
      // the window of all input channels must fit the LDS next to the residual operand and the staging tiles
      const int halo = ((p.dense_k - 1) * p.dilation / 2 + 3) & ~3;
      size_t xr = 0;
      for (int k = 0; k < p.n_panes; ++k) xr = std::max(xr, (size_t)64 * (p.panes[k].cin_pad + 16));
      if (p.tile > 64) p.tile = 64;
      if ((size_t)(64 + 2 * halo) * (p.cin_pad + 16) + xr + 37 * 1024 > 160 * 1024) p.tile = 32;
      // plain dense convs in throughput mode: 128-frame tiles (every weight fragment feeds four frame tiles; a launch
      // then has B * Tp / 128 work-groups and two launches of different steps share the chip) where the window fits
      const TensorRT& o0 = e->tens[op.outs[0].tensor];
      if (e->wide_tiles && e->dense_tile128 && p.n_panes == 0 && rup(o0.T, 64) % 128 == 0 &&
          (size_t)(128 + 2 * halo) * (p.cin_pad + 16) + 37 * 1024 <= 160 * 1024)
        p.tile = 128;
    }
  }
}

static void build_quant_in(const qasr_engine* e, uint32_t oi, QuantInP& p) {
  const qasr_op_desc& op = e->ops[oi];
  const TensorRT& tin = e->tens[op.in];
  const TensorRT& to = e->tens[op.outs[0].tensor];
  p.x = (const float*)tin.ptr;
  p.out = (int8_t*)to.ptr;
  p.lens = e->lens_all + (size_t)to.d.domain * e->B;
  p.inv_scale = op.in_inv_scale;
  p.lo = op.qlo;
  p.hi = op.qhi;
  p.C = (int)op.cin;
  p.T = tin.T;
  p.Tp = to.Tp;
  p.B = e->B;
}
static void build_dw(qasr_engine* e, uint32_t oi, DwP& p) {
  const qasr_op_desc& op = e->ops[oi];
  const TensorRT& tin = e->tens[op.in];
  p.x = (const int8_t*)tin.ptr;
  p.w = dev_w(e, op.w_off);
  p.bias = dev_at<int32_t>(e, op.bias_off);
  p.C = (int)op.cin;
  p.K = (int)op.kernel;
  p.kpad = rup(p.K, 4);
  p.stride = (int)op.stride;
  p.dilation = (int)op.dilation;
  p.padding = (int)op.padding;
  p.T_in = tin.T;
  p.Tp_in = tin.Tp;
  p.x_unsigned = tin.d.dtype == QASR_DT_U8;
  fill_epi(e, oi, op, p.e);
}
// ops 0..2 = [first-layer QuantAct, strided depthwise conv, 1x1 conv], each feeding only the next: the stem k_stem runs
static bool stem_shape(qasr_engine* e) {
  if (e->h.n_ops < 3) return false;
  const qasr_op_desc &a = e->ops[0], &b = e->ops[1], &c = e->ops[2];
  if (a.kind != QASR_OP_QUANT_IN || b.kind != QASR_OP_DW || c.kind != QASR_OP_PW || e->skip[1] || e->fused_dw[2] >= 0) return false;
  if (b.in != a.outs[0].tensor || c.in != b.outs[0].tensor || a.outs[1].tensor >= 0 || b.outs[1].tensor >= 0) return false;
  for (uint32_t oi = 3; oi < e->h.n_ops; ++oi) {             // nobody else reads the two intermediate tensors
    const qasr_op_desc& q = e->ops[oi];
    if (q.in == a.outs[0].tensor || q.in == b.outs[0].tensor) return false;
    for (uint32_t k = 0; k < q.n_panes; ++k)
      if (q.panes[k].in == a.outs[0].tensor || q.panes[k].in == b.outs[0].tensor) return false;
  }
  QuantInP qi{};
  DwP dw{};
  SepP pw{};
  build_quant_in(e, 0, qi);
  build_dw(e, 1, dw);
  build_sep(e, 2, pw);
  return stem_supported(qi, dw, pw);
}
static int stem_launch(qasr_engine* e, hipStream_t s) {
  QuantInP qi{};
  DwP dw{};
  SepP pw{};
  build_quant_in(e, 0, qi);
  build_dw(e, 1, dw);
  build_sep(e, 2, pw);
  // inside a forward the stem zeroes the flag words of every paired op (enqueue_forward enqueues no k_pair_zero then); run_op
  // and time_ops reach here outside one, and their paired ops zero their own words
  const bool zero = e->in_forward && e->pair_flags;
  int rc = launch_stem(s, qi, dw, pw, (const qasr_domain_desc*)(e->dblob + e->h.domains_off), (int)e->h.n_domains, e->cur_lens,
                       e->lens_all, e->norm_tiles ? e->norm_stats : nullptr, e->norm_tiles, e->norm_frames,
                       zero ? e->pair_flags : nullptr, zero ? e->pair_flag_bytes : 0);
  return rc ? fail(rc, "k_stem launch") : QASR_OK;
}

static int launch_op(qasr_engine* e, hipStream_t s, uint32_t oi, float* logp, int32_t* tokens, int32_t* lens_out) {
  const qasr_op_desc& op = e->ops[oi];
  const int B = e->B;
  if (e->skip[oi]) return QASR_OK;        // runs inside the next op's k_sep launch
  if (e->stem && oi <= 2) return oi == 0 ? stem_launch(e, s) : QASR_OK;   // block 0 as one launch
  const TensorRT& tin = e->tens[op.in];
  switch (op.kind) {
    case QASR_OP_QUANT_IN: {
      QuantInP p{};
      build_quant_in(e, oi, p);
      launch_quant_in(s, p);
      break;
    }
    case QASR_OP_DW: {
      DwP p{};
      build_dw(e, oi, p);
      launch_dw(s, p);
      break;
    }
    case QASR_OP_PW: {
      SepP p{};
      build_sep(e, oi, p);
      if (e->fuse_dec && (op.flags & QASR_F_LOGITS) && oi + 1 < e->h.n_ops && e->ops[oi + 1].kind == QASR_OP_LOGSOFTMAX &&
          e->ops[oi + 1].in == op.outs[0].tensor && decoder_fusable(p)) {
        int rc = launch_decoder(s, p, logp, tokens, lens_out, e->debug, e->ctc_fs);
        if (rc) return fail(rc, "op %u: decoder launch", oi);
        e->dec_skip[oi + 1] = 1;
        break;
      }
      if (e->fuse_dec && (op.flags & QASR_F_LOGITS) && oi + 1 < e->h.n_ops && e->ops[oi + 1].kind == QASR_OP_LOGSOFTMAX &&
          e->ops[oi + 1].in == op.outs[0].tensor && decoder_wide_fusable(p)) {
        int rc = launch_decoder_wide(s, p, logp, tokens, lens_out, e->debug, e->decw_ws, e->decw_ws_bytes, e->ctc_fs);
        if (rc) return fail(rc, "op %u: wide decoder launch", oi);
        e->dec_skip[oi + 1] = 1;
        e->dec_wide[oi] = 1;
        break;
      }
      // a paired op outside a forward (run_op, time_ops): its flag words are zeroed here, as the forward's memset does for all
      if (p.pair && !e->in_forward && launch_pair_zero(s, p.pair_flags, sep_pair_flag_bytes(p.e.B, p.e.Tp))) return fail(QASR_ERR_ARG, "op %u: k_pair_zero", oi);
      int rc = launch_sep(s, p);
      if (rc) return fail(rc, "op %u: no k_sep instantiation for K=%d dilation=%d (or bad launch shape)", oi, p.K, p.dilation);
      break;
    }
    case QASR_OP_DENSE: {
      if (op.flags & QASR_F_TAPMAJOR) {                     // stride-1 'same' dense conv: taps shifted 1x1 GEMMs on the tile kernel
        SepP p{};
        build_sep(e, oi, p);
        int rc = launch_sep(s, p);
        if (rc) return fail(rc, "op %u: dense conv has no k_sep launch shape", oi);
        break;
      }
      DenseP p{};
      p.x = (const int8_t*)tin.ptr;
      p.w = dev_w(e, op.w_off);
      p.bias = dev_at<int32_t>(e, op.bias_off);
      p.cin = (int)op.cin;
      p.cin_pad = rup(p.cin, 128);
      p.K = (int)op.kernel;
      p.stride = (int)op.stride;
      p.dilation = (int)op.dilation;
      p.padding = (int)op.padding;
      p.T_in = tin.T;
      p.Tp_in = tin.Tp;
      p.x_unsigned = tin.d.dtype == QASR_DT_U8;
      p.n_panes = (int)op.n_panes;
      fill_panes(e, oi, op, p.panes);
      fill_epi(e, oi, op, p.e);
      launch_dense(s, p);
      break;
    }
    case QASR_OP_REQUANT: {
      if (e->rq_skip[oi]) break;                             // served by an earlier launch on the same stored value
      const TensorRT& to = e->tens[op.outs[0].tensor];
      RequantP p{};
      p.in = tin.ptr;
      p.in_is_i32 = tin.d.dtype == QASR_DT_I32;
      fill_out(e, op.outs[0], p.outs[0]);
      p.n_outs = 1;
      // the packer emits the REQUANT ops of one stored value back to back: one launch serves up to QASR_RQ_MAX of them
      for (uint32_t oj = oi + 1; oj < e->h.n_ops && p.n_outs < QASR_RQ_MAX; ++oj) {
        const qasr_op_desc& q = e->ops[oj];
        if (q.kind != QASR_OP_REQUANT || q.in != op.in || q.flags != op.flags || q.sb_off != op.sb_off || q.cin != op.cin ||
            e->tens[q.outs[0].tensor].d.domain != to.d.domain)
          break;
        fill_out(e, q.outs[0], p.outs[p.n_outs++]);
        e->rq_skip[oj] = 1;
      }
      p.sb = dev_at<float>(e, op.sb_off);
      p.lens = e->lens_all + (size_t)to.d.domain * B;
      p.flags = op.flags & QASR_F_MASK_OUT;   // the stored value is already ReLU'd / round-tripped z
      p.C = (int)op.cin;
      p.T = to.T;
      p.Tp = to.Tp;
      p.B = B;
      launch_requant(s, p);
      break;
    }
    case QASR_OP_LOGSOFTMAX: {
      if (e->dec_skip[oi]) break;                            // ran inside the decoder's launch (k_dec / k_decw), lengths included
      launch_logsoftmax(s, (const float*)tin.ptr, logp, tokens, e->ctc_fs, B * tin.T, (int)op.cin);
      if (lens_out)
        HIPCHK(hipMemcpyAsync(lens_out, e->lens_all + (size_t)tin.d.domain * B, sizeof(int32_t) * B,
                              hipMemcpyDeviceToDevice, s));
      break;
    }
    default:
      return fail(QASR_ERR_UNSUPPORTED, "op kind %u", op.kind);
  }
  return QASR_OK;
}

// index of the plan's LOGSOFTMAX op (the decoder's output stage), or -1
static int logsoftmax_op(const qasr_engine* e) {
  for (uint32_t oi = 0; oi < e->h.n_ops; ++oi)
    if (e->ops[oi].kind == QASR_OP_LOGSOFTMAX) return (int)oi;
  return -1;
}

// front-end of a forward_audio call (nullptr: the caller's features are the input)
struct FrontArgs {
  const float* audio;
  const int32_t* audio_lens;
  int S;
  const float* fb;
  const float* window;
  int n_mels;
  float preemph;
  int pad_to;
  const void* plan;
  size_t plan_bytes;
  const RaggedFront* rg;               // reserved engines: staging pitch, bucket frames, shape block (nullptr otherwise)
};

// every launch of one forward, in order: front-end, lengths, ops, k_ctc (directly, or inside a stream capture)
static int enqueue_forward(qasr_engine* e, hipStream_t s, const FrontArgs* fe, bool norm_in_stem, float* feats, int32_t* lens,
                           float* logp, int32_t* tokens, int32_t* lens_out) {
  const auto& h = e->h;
  const int B = e->B;
  // the flag words of every paired op, zero before the first kernel: one node per forward.  A kernel, not hipMemsetAsync: as a
  // memset node of the captured graph the zeroing was not in place for every paired launch of back-to-back replays (a few
  // tokens differed from the serial result, no spin timed out: flags of the previous replay were still seen set)
  // With the fused stem there is no node of its own: k_stem, the first kernel of the ops, zeroes them (stem_launch)
  if (e->pair_flags && !e->stem && launch_pair_zero(s, e->pair_flags, e->pair_flag_bytes)) return fail(QASR_ERR_ARG, "forward: k_pair_zero");
  struct InForward {
    qasr_engine* e;
    explicit InForward(qasr_engine* e_) : e(e_) { e->in_forward = true; }
    ~InForward() { e->in_forward = false; }
  } in_forward(e);
  if (fe && norm_in_stem) {
    int nt = 0, nf = 0;
    int rc = frontend_mel_stats(s, fe->audio, fe->audio_lens, B, fe->S, fe->fb, fe->window, fe->n_mels, fe->preemph, fe->pad_to,
                                feats, lens, fe->plan, fe->plan_bytes, e->norm_stats, &nt, &nf, fe->rg);
    if (rc || nt != e->norm_tiles || nf != e->norm_frames) return fail(rc ? rc : QASR_ERR_ARG, "forward_audio: front-end (k_mel with statistics)");
  } else if (fe) {                                           // mel front-end into the caller's feature / length buffers
    int rc = fe->rg ? frontend_mel_planned_ragged(s, fe->audio, fe->audio_lens, B, fe->S, fe->fb, fe->window, fe->n_mels,
                                                  fe->preemph, fe->pad_to, feats, lens, fe->plan, fe->plan_bytes, *fe->rg)
                    : qasr_frontend_mel_planned(s, fe->audio, fe->audio_lens, B, fe->S, fe->fb, fe->window, fe->n_mels, fe->preemph,
                                                fe->pad_to, feats, lens, fe->plan, fe->plan_bytes);
    if (rc) return fail(rc, "forward_audio: front-end");
  }
  const qasr_domain_desc* ddoms = (const qasr_domain_desc*)(e->dblob + h.domains_off);
  if (!e->stem) launch_lens(s, lens, e->lens_all, ddoms, (int)h.n_domains, B);   // (k_stem derives them itself)
  for (uint32_t oi = 0; oi < h.n_ops; ++oi) {
    if (e->timing) HIPCHK(hipEventRecord(e->ev[oi], s));
    int rc = launch_op(e, s, oi, logp, tokens, lens_out);
    if (rc) return rc;
  }
  if (e->ctc_on) {                                           // greedy collapse of this call's tokens, behind the decoder
    const qasr_op_desc& ls = e->ops[logsoftmax_op(e)];
    const TensorRT& tl = e->tens[ls.in];
    int rc = launch_ctc(s, tokens, e->ctc_fs, e->ctc_use_lens ? e->lens_all + (size_t)tl.d.domain * B : nullptr, B, tl.T,
                        (int)ls.cin - 1, e->ctc_out, e->ctc_t_act);
    if (rc) return fail(rc, "k_ctc launch");
  }
  return QASR_OK;
}

static int forward_impl(qasr_engine* e, hipStream_t s, const FrontArgs* fe, float* feats, int32_t* lens, int B, int T,
                        float* logp, int32_t* tokens, int32_t* lens_out) {
  if (e->rs.on) return fail(QASR_ERR_ARG, "forward: this engine is reserved (qasr_engine_reserve): use qasr_engine_forward_ragged[_audio], or a second engine");
  if (B != e->B || T != e->T0) {
    int rc = build_plan(e, B, T);
    if (rc) return rc;
    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    e->gexec = nullptr;
    e->gkey[0] = nullptr;
  }
  if (e->ctc_on && !tokens) return fail(QASR_ERR_ARG, "forward: a qasr_ctc_out is attached, tokens must not be NULL");
  const auto& h = e->h;
  e->tens[0].ptr = (void*)feats;
  e->cur_lens = lens;
  e->stem = e->fuse_stem && stem_shape(e);
  // normalize_batch inside k_stem: k_mel leaves per-tile sums, no k_norm launch
  const bool norm_in_stem = fe && e->stem && e->fuse_norm && fe->n_mels == (int)h.feat_in;
  e->norm_tiles = e->norm_frames = 0;                        // (a forward on features hands k_stem normalised input)
  e->fe_launches = fe ? (norm_in_stem ? 1 : 2) : 0;
  if (norm_in_stem) {
    e->norm_frames = 1 + fe->S / 160;
    e->norm_tiles = (e->norm_frames + QASR_MEL_TILE - 1) / QASR_MEL_TILE;
    const size_t need = frontend_stats_bytes(B, fe->S, fe->n_mels);
    if (need > e->norm_stats_bytes) {                        // (a captured graph holds the old pointer)
      if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
      e->gexec = nullptr;
      e->gkey[0] = nullptr;
      dev_free(e, e->norm_stats);
      e->norm_stats = nullptr;
      e->norm_stats_bytes = 0;
      HIPCHK(dev_alloc(e, (void**)&e->norm_stats, need));
      e->norm_stats_bytes = need;
    }
  }
  auto enqueue = [&]() -> int { return enqueue_forward(e, s, fe, norm_in_stem, feats, lens, logp, tokens, lens_out); };
  e->forwarded = true;
  if (e->use_graph && s != nullptr && !e->timing && !e->debug) {   // the legacy default stream cannot be captured
    const void* key[8] = {feats, lens, logp, tokens, lens_out, fe ? fe->audio : nullptr, fe ? fe->audio_lens : nullptr,
                          fe ? fe->plan : nullptr};
    uint64_t fkey[6] = {0, 0, 0, 0, 0, 0};
    if (fe) {
      uint32_t pre_bits;
      memcpy(&pre_bits, &fe->preemph, 4);
      fkey[0] = (uint64_t)fe->S; fkey[1] = (uint64_t)fe->n_mels; fkey[2] = (uint64_t)fe->pad_to; fkey[3] = pre_bits;
      fkey[4] = (uint64_t)(uintptr_t)fe->fb; fkey[5] = (uint64_t)(uintptr_t)fe->window;
    }
    bool same = true;
    for (int i = 0; i < 8; ++i) same = same && key[i] == e->gkey[i];
    for (int i = 0; i < 6; ++i) same = same && fkey[i] == e->gfe[i];
    const uint64_t ckey[8] = {(uint64_t)(uintptr_t)e->ctc_fs, (uint64_t)(uintptr_t)e->ctc_out.labels, (uint64_t)(uintptr_t)e->ctc_out.n_labels,
                              (uint64_t)(uintptr_t)e->ctc_out.start, (uint64_t)(uintptr_t)e->ctc_out.nframes, (uint64_t)(uintptr_t)e->ctc_out.score,
                              (uint64_t)(uintptr_t)e->ctc_out.utt_score, (uint64_t)(e->ctc_on ? 1 : 0) | (uint64_t)(e->ctc_use_lens ? 2 : 0)};
    for (int i = 0; i < 8; ++i) same = same && ckey[i] == e->gctc[i];
    if (!same) {                                             // new buffer set / front-end arguments: drop the old graph, start over
      if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
      e->gexec = nullptr;
      e->gcalls = 0;
      for (int i = 0; i < 8; ++i) e->gkey[i] = key[i];
      for (int i = 0; i < 6; ++i) e->gfe[i] = fkey[i];
      for (int i = 0; i < 8; ++i) e->gctc[i] = ckey[i];
    }
    if (e->gexec) {
      HIPCHK(hipGraphLaunch(e->gexec, s));
      return QASR_OK;
    }
    if (e->gcalls++ >= 1) {                                  // second call with this key: capture (the first one ran every
      hipGraph_t g = nullptr;                                // kernel's one-time attribute setup outside a capture)
      if (g_prof) return fail(QASR_ERR_ARG, "graph capture while qasr_debug_prof / qasr_debug_timeline is set: the buffer would be baked into the graph");
      HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      int rc = enqueue();
      hipError_t ce = hipStreamEndCapture(s, &g);
      if (rc) {                                              // an enqueue error inside the capture: nothing is kept
        if (g) (void)hipGraphDestroy(g);
        e->gcalls = 0;
        return rc;
      }
      if (ce != hipSuccess || !g) return fail(QASR_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
      hipError_t ie = hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (ie != hipSuccess) return fail(QASR_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
      HIPCHK(hipGraphLaunch(e->gexec, s));
      return QASR_OK;
    }
  }
  {
    int rc = enqueue();
    if (rc) return rc;
  }
  if (e->timing) {
    HIPCHK(hipEventRecord(e->ev[h.n_ops], s));
    e->timed = true;
  }
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

// the caller's qasr_ctc_out, checked; an older (shorter) struct is not known yet: sizes must match
static int ctc_out_check(const qasr_ctc_out* out, bool have_fs, const char* who) {
  if (out->struct_size != sizeof(qasr_ctc_out)) return fail(QASR_ERR_ARG, "%s: qasr_ctc_out.struct_size %u is not %zu", who, out->struct_size, sizeof(qasr_ctc_out));
  if (!out->labels || !out->n_labels) return fail(QASR_ERR_ARG, "%s: labels and n_labels are required", who);
  if ((out->score || out->utt_score) && !have_fs) return fail(QASR_ERR_ARG, "%s: score / utt_score need frame_score", who);
  return QASR_OK;
}

int qasr_ctc_collapse(void* stream, const int32_t* tokens, const float* frame_score, const int32_t* lens, int B, int T,
                      int blank, const qasr_ctc_out* out) {
  if (!tokens || !out || B < 1 || T < 1) return fail(QASR_ERR_ARG, "ctc_collapse: tokens / out NULL or B, T < 1");
  int rc = ctc_out_check(out, frame_score != nullptr, "ctc_collapse");
  if (rc) return rc;
  return launched("ctc_collapse", launch_ctc((hipStream_t)stream, tokens, frame_score, lens, B, T, blank, *out));
}

int qasr_ctc_topn(void* stream, const qasr_ctc_topn_args* a) {
  if (int rc = args_check("ctc_topn", a)) return rc;
  if (!a->log_probs || !a->cand_id || !a->cand_q) return fail(QASR_ERR_ARG, "ctc_topn: log_probs, cand_id and cand_q are required");
  if (a->B < 1 || a->T < 1 || a->T > QASR_BEAM_MAX_FRAMES || a->C < 1 || (int64_t)a->B * a->T >= (1ll << 31))
    return fail(QASR_ERR_ARG, "ctc_topn: B %d, T %d (1 .. %d), C %d out of range", a->B, a->T, QASR_BEAM_MAX_FRAMES, a->C);
  if (a->N < 1 || a->N > QASR_BEAM_MAX_CANDIDATES)
    return fail(QASR_ERR_ARG, "ctc_topn: N %d is outside 1 .. %d", a->N, QASR_BEAM_MAX_CANDIDATES);
  if (a->pitch_frame < a->C || a->pitch_utt < (int64_t)a->T * a->pitch_frame)
    return fail(QASR_ERR_ARG, "ctc_topn: pitch_frame %lld < C or pitch_utt %lld < T * pitch_frame", (long long)a->pitch_frame,
                (long long)a->pitch_utt);
  return launched("ctc_topn", launch_topn((hipStream_t)stream, *a));
}

static int beam_shape_ok(int B, int T, int W) {
  return B >= 1 && T >= 1 && T <= QASR_BEAM_MAX_FRAMES && W >= 1 && W <= QASR_BEAM_MAX_WIDTH && (int64_t)B * T < (1ll << 31);
}

size_t qasr_ctc_beam_workspace_bytes(int B, int T, int beam_width) {
  return beam_shape_ok(B, T, beam_width) ? beam_workspace_bytes(B, T, beam_width) : 0;
}

// ---- the checks the beam entry points share, offline and streaming, with the entry's name in the message; 0 or the error's code.
// qasr_ctc_beam, _lm and _boost: their structs open with the same fields but are three types, hence the templates.  Each entry
// words its own pointer refusal (what is optional differs).
static int beam_cand_check(const char* who, int N, int n_best, int beam_width, int blank, uint32_t lae_entries) {
  if (N < 1 || N > QASR_BEAM_MAX_CANDIDATES) return fail(QASR_ERR_ARG, "%s: N %d is outside 1 .. %d", who, N, QASR_BEAM_MAX_CANDIDATES);
  if (n_best < 1 || n_best > beam_width || blank < 0)
    return fail(QASR_ERR_ARG, "%s: n_best %d is outside 1 .. beam_width, or blank %d < 0", who, n_best, blank);
  if (lae_entries != QASR_BEAM_TABLE_ENTRIES) return fail(QASR_ERR_ARG, "%s: lae_entries %u is not %d", who, lae_entries, QASR_BEAM_TABLE_ENTRIES);
  return 0;
}
extern "C++" {                                                               // (templates: not inside the extern "C" block around them)
template <class A>
static bool beam_ptrs_ok(const A* a) {
  return a->cand_id && a->cand_q && a->lae_table && a->workspace && a->labels && a->n_labels && a->score && a->n_hyps;
}
template <class A>
static int beam_shape_check(const char* who, const A* a) {                 // shape, N, n_best / blank, table, workspace
  if (!beam_shape_ok(a->B, a->T, a->beam_width))
    return fail(QASR_ERR_ARG, "%s: B %d, T %d (1 .. %d) or beam_width %d (1 .. %d) out of range", who, a->B, a->T, QASR_BEAM_MAX_FRAMES,
                a->beam_width, QASR_BEAM_MAX_WIDTH);
  if (int rc = beam_cand_check(who, a->N, a->n_best, a->beam_width, a->blank, a->lae_entries)) return rc;
  const size_t need = beam_workspace_bytes(a->B, a->T, a->beam_width);
  if (a->workspace_bytes < need) return fail(QASR_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", who, a->workspace_bytes, need);
  return 0;
}
}
static int beam_blob_check(const char* who, const char* what, const void* blob, size_t bytes) {     // a packed model (`lm`) or phrase set (`boost`)
  if (((uintptr_t)blob & 15) != 0 || bytes < 128 || bytes > (size_t)INT32_MAX)
    return fail(QASR_ERR_ARG, "%s: %s must be 16-byte aligned and 128 .. 2^31 - 1 bytes, got %zu", who, what, bytes);
  return 0;
}
static int beam_lm_check(const char* who, const void* lm, size_t lm_bytes, int alpha_q, int beta_q) {
  if (int rc = beam_blob_check(who, "lm", lm, lm_bytes)) return rc;
  if (alpha_q < 0 || alpha_q > QASR_LM_MAX_WEIGHT || beta_q < -QASR_LM_MAX_WEIGHT || beta_q > QASR_LM_MAX_WEIGHT)
    return fail(QASR_ERR_ARG, "%s: alpha_q %d outside 0 .. 16 * 2^16 or |beta_q| %d above it", who, alpha_q, beta_q);
  return 0;
}
static int beam_space_check(const char* who, int space, int blank) {
  return space < -1 || space == blank ? fail(QASR_ERR_ARG, "%s: space %d must be a label other than blank, or -1", who, space) : 0;
}

int qasr_ctc_beam(void* stream, const qasr_ctc_beam_args* a) {
  if (int rc = args_check("ctc_beam", a)) return rc;
  if (!beam_ptrs_ok(a)) return fail(QASR_ERR_ARG, "ctc_beam: a required pointer is NULL (only lens is optional)");
  if (int rc = beam_shape_check("ctc_beam", a)) return rc;
  return launched("ctc_beam", launch_beam((hipStream_t)stream, *a));
}

// Host-only validation of a packed n-gram model (qasr/ngram.py states the layout); k_beam_lm trusts what passes here.
int qasr_lm_check(const void* blob, size_t bytes, int n_labels) {
  enum { HDR = 32 };
  const int32_t LIM = 1 << 30;
  if (!blob) return fail(QASR_ERR_BLOB, "lm_check: blob is NULL");
  if (bytes < HDR * 4 || bytes > (size_t)INT32_MAX) return fail(QASR_ERR_BLOB, "lm_check: %zu bytes is no model", bytes);
  if (((uintptr_t)blob & 3) != 0) return fail(QASR_ERR_BLOB, "lm_check: blob is not 4-byte aligned");
  const int32_t* h = (const int32_t*)blob;
  if (h[0] != 0x314D4C51 || h[1] != 1) return fail(QASR_ERR_BLOB, "lm_check: magic %#x / version %d", (unsigned)h[0], h[1]);
  const int order = h[2], mode = h[3], n_nodes = h[4], start = h[5], tcap = h[6], tprobe = h[7], wcap = h[9], wprobe = h[10];
  const int n_words = h[11];
  const int32_t* level = h + 13;
  if (order < 1 || order > QASR_LM_MAX_ORDER || (mode != 0 && mode != 1)) return fail(QASR_ERR_BLOB, "lm_check: order %d / mode %d", order, mode);
  if (h[8] != n_labels || n_labels < 1) return fail(QASR_ERR_BLOB, "lm_check: packed for %d labels, asked for %d", h[8], n_labels);
  if (n_nodes < 1 || n_words < 1 || start < 0 || start >= n_nodes)
    return fail(QASR_ERR_BLOB, "lm_check: n_nodes %d, n_words %d or start %d out of range", n_nodes, n_words, start);
  if (tcap < 1 || (tcap & (tcap - 1)) || wcap < 1 || (wcap & (wcap - 1)))
    return fail(QASR_ERR_BLOB, "lm_check: capacities %d / %d are not powers of two", tcap, wcap);
  if (tprobe < 1 || tprobe > QASR_LM_MAX_PROBE || tprobe > tcap || wprobe < 1 || wprobe > QASR_LM_MAX_PROBE || wprobe > wcap)
    return fail(QASR_ERR_BLOB, "lm_check: probe bounds %d / %d outside 1 .. %d (or above the capacity)", tprobe, wprobe, QASR_LM_MAX_PROBE);
  const uint64_t total = 4ull * HDR + 16ull * (uint64_t)tcap + 16ull * (uint64_t)wcap + 8ull * (uint64_t)n_nodes + 4ull * (uint64_t)n_labels;
  if (total != (uint64_t)bytes || h[12] != (int32_t)bytes) return fail(QASR_ERR_BLOB, "lm_check: %zu bytes, the header describes %llu (total field %d)", bytes, (unsigned long long)total, h[12]);
  for (int i = 21; i < HDR; ++i)
    if (h[i] != 0) return fail(QASR_ERR_BLOB, "lm_check: reserved header word %d is %d", i, h[i]);
  if (level[0] != 0 || level[1] != 1) return fail(QASR_ERR_BLOB, "lm_check: level[0 .. 1] = %d, %d", level[0], level[1]);
  for (int k = 1; k < 8; ++k)
    if (level[k] < level[k - 1] || level[k] > n_nodes || (k >= order && level[k] != n_nodes))
      return fail(QASR_ERR_BLOB, "lm_check: level[%d] = %d does not ascend to n_nodes %d", k, level[k], n_nodes);
  const int32_t* trans = h + HDR;
  const int32_t* words = trans + 4 * (size_t)tcap;
  const int32_t* nodes = words + 4 * (size_t)wcap;
  const int32_t* l2w = nodes + 2 * (size_t)n_nodes;
  int lv = 0;
  for (int i = 0; i < n_nodes; ++i) {
    while (lv < 7 && i >= level[lv + 1]) ++lv;                // node i has lv words
    const int bo = nodes[2 * i], sf = nodes[2 * i + 1];
    if (bo < -LIM || bo > LIM) return fail(QASR_ERR_BLOB, "lm_check: back-off %d of node %d beyond 2^30", bo, i);
    const bool ok = lv == 0 ? sf == 0 : (sf >= level[lv - 1] && sf < level[lv]);
    if (!ok) return fail(QASR_ERR_BLOB, "lm_check: suffix %d of node %d (level %d) is not one level down", sf, i, lv);
  }
  for (int s = 0; s < tcap; ++s) {
    const int32_t* e = trans + 4 * (size_t)s;
    if (e[0] == -1) continue;
    if (e[0] < 0 || e[0] >= n_nodes || e[1] < 0 || e[1] >= n_words || e[3] < 0 || e[3] >= n_nodes || e[2] < -LIM || e[2] > LIM)
      return fail(QASR_ERR_BLOB, "lm_check: transition slot %d (%d, %d, %d, %d) out of range", s, e[0], e[1], e[2], e[3]);
    uint64_t x = (((uint64_t)(uint32_t)e[0] << 32) | (uint32_t)e[1]) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    const int home = (int)((uint32_t)x & (uint32_t)(tcap - 1)), dist = (s - home) & (tcap - 1);
    if (dist >= tprobe) return fail(QASR_ERR_BLOB, "lm_check: transition slot %d lies %d probes from its home, the bound is %d", s, dist + 1, tprobe);
    for (int d = 0; d < dist; ++d)
      if (trans[4 * (size_t)((home + d) & (tcap - 1))] == -1) return fail(QASR_ERR_BLOB, "lm_check: transition slot %d is cut off from its home", s);
  }
  for (int s = 0; s < wcap; ++s) {
    const int32_t* e = words + 4 * (size_t)s;
    if (e[2] == -1) continue;
    if (e[2] < 0 || e[2] >= n_words) return fail(QASR_ERR_BLOB, "lm_check: word slot %d holds id %d", s, e[2]);
    const int home = (int)((uint32_t)e[0] & (uint32_t)(wcap - 1)), dist = (s - home) & (wcap - 1);
    if (dist >= wprobe) return fail(QASR_ERR_BLOB, "lm_check: word slot %d lies %d probes from its home, the bound is %d", s, dist + 1, wprobe);
    for (int d = 0; d < dist; ++d)
      if (words[4 * (size_t)((home + d) & (wcap - 1)) + 2] == -1) return fail(QASR_ERR_BLOB, "lm_check: word slot %d is cut off from its home", s);
  }
  for (int i = 0; i < n_labels; ++i)
    if (l2w[i] < -1 || l2w[i] >= n_words) return fail(QASR_ERR_BLOB, "lm_check: label %d maps to word %d", i, l2w[i]);
  return QASR_OK;
}

int qasr_ctc_beam_lm(void* stream, const qasr_ctc_beam_lm_args* a) {
  if (int rc = args_check("ctc_beam_lm", a)) return rc;
  if (!beam_ptrs_ok(a) || !a->lm || !a->lm_score) return fail(QASR_ERR_ARG, "ctc_beam_lm: a required pointer is NULL (only lens is optional)");
  if (int rc = beam_shape_check("ctc_beam_lm", a)) return rc;
  if (int rc = beam_lm_check("ctc_beam_lm", a->lm, a->lm_bytes, a->alpha_q, a->beta_q)) return rc;
  if (int rc = beam_space_check("ctc_beam_lm", a->space, a->blank)) return rc;
  return launched("ctc_beam_lm", launch_beam_lm((hipStream_t)stream, *a));
}

// Host-only validation of a packed phrase set (qasr/boost.py states the layout); k_beam_boost trusts what passes here.
int qasr_boost_check(const void* blob, size_t bytes, int n_labels) {
  enum { HDR = 32 };
  const int32_t LIM = 1 << 30;
  if (!blob) return fail(QASR_ERR_BLOB, "boost_check: blob is NULL");
  if (bytes < HDR * 4 || bytes > (size_t)INT32_MAX) return fail(QASR_ERR_BLOB, "boost_check: %zu bytes is no phrase set", bytes);
  if (((uintptr_t)blob & 3) != 0) return fail(QASR_ERR_BLOB, "boost_check: blob is not 4-byte aligned");
  const int32_t* h = (const int32_t*)blob;
  if (h[0] != 0x31534251 || h[1] != 1) return fail(QASR_ERR_BLOB, "boost_check: magic %#x / version %d", (unsigned)h[0], h[1]);
  const int n_nodes = h[3], start = h[5], whole = h[6], cap = h[7], probe = h[8];
  if (h[4] != n_labels || n_labels < 1) return fail(QASR_ERR_BLOB, "boost_check: packed for %d labels, asked for %d", h[4], n_labels);
  if (n_nodes < 1) return fail(QASR_ERR_BLOB, "boost_check: n_nodes %d", n_nodes);
  if (start < 0 || start >= n_nodes) return fail(QASR_ERR_BLOB, "boost_check: start state %d outside the %d nodes", start, n_nodes);
  if (whole != 0 && whole != 1) return fail(QASR_ERR_BLOB, "boost_check: whole_words %d", whole);
  if (cap < 1 || (cap & (cap - 1))) return fail(QASR_ERR_BLOB, "boost_check: capacity %d is no power of two", cap);
  if (probe < 1 || probe > QASR_LM_MAX_PROBE || probe > cap)
    return fail(QASR_ERR_BLOB, "boost_check: probe bound %d outside 1 .. %d (or above the capacity)", probe, QASR_LM_MAX_PROBE);
  const uint64_t total = 4ull * HDR + 16ull * (uint64_t)cap + 8ull * (uint64_t)n_nodes + 4ull * (uint64_t)n_labels;
  if (total != (uint64_t)bytes || h[2] != (int32_t)bytes)
    return fail(QASR_ERR_BLOB, "boost_check: %zu bytes, the header describes %llu (total field %d)", bytes, (unsigned long long)total, h[2]);
  for (int i = 9; i < HDR; ++i)
    if (h[i] != 0) return fail(QASR_ERR_BLOB, "boost_check: reserved header word %d is %d", i, h[i]);
  const int32_t* table = h + HDR;
  const int32_t* nodes = table + 4 * (size_t)cap;
  const int32_t* root_next = nodes + 2 * (size_t)n_nodes;
  for (int i = 0; i < n_nodes; ++i) {
    if (nodes[2 * i] < 0 || nodes[2 * i] > LIM) return fail(QASR_ERR_BLOB, "boost_check: pot %d of node %d outside 0 .. 2^30", nodes[2 * i], i);
    if (nodes[2 * i + 1] < 0 || nodes[2 * i + 1] > LIM) return fail(QASR_ERR_BLOB, "boost_check: bank %d of node %d outside 0 .. 2^30", nodes[2 * i + 1], i);
  }
  for (int i = 0; i < n_labels; ++i)
    if (root_next[i] < 0 || root_next[i] >= n_nodes) return fail(QASR_ERR_BLOB, "boost_check: root_next[%d] = %d outside the %d nodes", i, root_next[i], n_nodes);
  for (int s = 0; s < cap; ++s) {
    const int32_t* e = table + 4 * (size_t)s;
    if (e[0] == -1) continue;
    if (e[0] < 1 || e[0] >= n_nodes || e[1] < 0 || e[1] >= n_labels || e[2] < 0 || e[2] >= n_nodes || e[3] != 0)
      return fail(QASR_ERR_BLOB, "boost_check: table slot %d (node %d, label %d, next %d, %d) out of range", s, e[0], e[1], e[2], e[3]);
    uint64_t x = (((uint64_t)(uint32_t)e[0] << 32) | (uint32_t)e[1]) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    const int home = (int)((uint32_t)x & (uint32_t)(cap - 1)), dist = (s - home) & (cap - 1);
    if (dist >= probe) return fail(QASR_ERR_BLOB, "boost_check: table slot %d lies %d probes from its home, the probe bound is %d", s, dist + 1, probe);
    for (int d = 0; d < dist; ++d)
      if (table[4 * (size_t)((home + d) & (cap - 1))] == -1) return fail(QASR_ERR_BLOB, "boost_check: table slot %d is cut off from its home", s);
  }
  return QASR_OK;
}

int qasr_ctc_beam_boost(void* stream, const qasr_ctc_beam_boost_args* a) {
  if (int rc = args_check("ctc_beam_boost", a)) return rc;
  if (!beam_ptrs_ok(a) || !a->boost || !a->boost_score || (a->lm && !a->lm_score))
    return fail(QASR_ERR_ARG, "ctc_beam_boost: a required pointer is NULL (only lens and lm are optional; lm needs lm_score)");
  if (int rc = beam_shape_check("ctc_beam_boost", a)) return rc;
  if (a->lm)
    if (int rc = beam_lm_check("ctc_beam_boost", a->lm, a->lm_bytes, a->alpha_q, a->beta_q)) return rc;
  if (int rc = beam_blob_check("ctc_beam_boost", "boost", a->boost, a->boost_bytes)) return rc;
  if (int rc = beam_space_check("ctc_beam_boost", a->space, a->blank)) return rc;
  if (a->whole_words != 0 && a->space < 0)
    return fail(QASR_ERR_ARG, "ctc_beam_boost: whole words need the space label, got %d", a->space);
  return launched("ctc_beam_boost", launch_beam_boost((hipStream_t)stream, *a));
}

// ---- the checks the CTC lattice entry points below share, with the entry's name in the message; 0 or the error's code.  The
// templates run over structs that hold the same fields but are distinct types (no casts); what one entry asks differently stays in it.
extern "C++" {                                                               // (templates, as above)
static int ctc_blank_check(const char* who, int blank, int C) {
  return blank < 0 || blank >= C ? fail(QASR_ERR_ARG, "%s: blank %d is outside [0, %d)", who, blank, C) : 0;
}
static int ctc_pitch_check(const char* who, int T, int C, int64_t pitch_frame, int64_t pitch_utt) {
  if (pitch_frame < C || pitch_utt < (int64_t)T * pitch_frame)
    return fail(QASR_ERR_ARG, "%s: pitch_frame %lld < C or pitch_utt %lld < T * pitch_frame", who, (long long)pitch_frame, (long long)pitch_utt);
  return 0;
}
static int ctc_star_pitch_check(const char* who, int64_t star_pitch, int T) {
  return star_pitch < T ? fail(QASR_ERR_ARG, "%s: star_pitch %lld < T %d", who, (long long)star_pitch, T) : 0;
}
template <class A>
static int ctc_workspace_plane_check(const char* who, const A* a, size_t need) {   // how the four alignment entries' checks end
  if (a->workspace_bytes < need) return fail(QASR_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", who, a->workspace_bytes, need);
  return a->star_logp ? ctc_star_pitch_check(who, a->star_pitch, a->T) : 0;                // the plane is optional
}
static int ctc_max_labels_check(const char* who, int max_labels, int cap) {
  return max_labels < 1 || max_labels > cap ? fail(QASR_ERR_ARG, "%s: max_labels %d is outside 1 .. %d", who, max_labels, cap) : 0;
}
template <class A>
static int ctc_targets_check(const char* who, const A* a, int max_labels_cap) {   // of the four alignment entries
  if (int rc = ctc_max_labels_check(who, a->max_labels, max_labels_cap)) return rc;
  if (int rc = ctc_blank_check(who, a->blank, a->C)) return rc;
  return ctc_pitch_check(who, a->T, a->C, a->pitch_frame, a->pitch_utt);
}
// ctc_align and ctc_align_band take their struct in two sizes: `full`, zeroed by the caller, receives what was given (the
// shorter struct: no wildcard plane)
template <class A>
static int ctc_two_size_args(const char* who, const A* given, size_t v1_size, A* full) {
  if (!given) return fail(QASR_ERR_ARG, "%s: args is NULL", who);
  if (given->struct_size != sizeof(A) && given->struct_size != v1_size)
    return fail(QASR_ERR_ARG, "%s: struct_size %u is neither %zu nor %zu", who, given->struct_size, sizeof(A), v1_size);
  memcpy(full, given, given->struct_size);
  return 0;
}
template <class A>
static int ctc_five_ptrs_check(const char* who, const A* a) {
  if (!a->log_probs || !a->targets || !a->target_lens || !a->workspace || !a->ok)
    return fail(QASR_ERR_ARG, "%s: log_probs, targets, target_lens, workspace and ok are required", who);
  return 0;
}
template <class A>
static int ctc_problems_check(const char* who, const A* a) {         // ctc_align and ctc_post: K problems per utterance, their rows
  if (a->B < 1 || a->T < 1 || a->T > QASR_BEAM_MAX_FRAMES || a->C < 1 || a->K < 1)
    return fail(QASR_ERR_ARG, "%s: B %d, T %d (1 .. %d), C %d or K %d out of range", who, a->B, a->T, QASR_BEAM_MAX_FRAMES, a->C, a->K);
  if ((long long)a->P != (long long)a->B * a->K) return fail(QASR_ERR_ARG, "%s: P %d is not B %d * K %d", who, a->P, a->B, a->K);
  return ctc_targets_check(who, a, QASR_ALIGN_MAX_LABELS);
}
static bool band_states_ok(int band_states) { return band_states == 256 || band_states == 1024 || band_states == 4352; }
template <class A>
static int ctc_band_check(const char* who, const A* a) {             // the banded entries: one problem per recording, its rows
  if (!band_states_ok(a->band_states)) return fail(QASR_ERR_ARG, "%s: band_states %d is not 256, 1024 or 4352", who, a->band_states);
  if (a->B < 1 || a->T < 1 || a->T > QASR_BAND_MAX_FRAMES || a->C < 1)
    return fail(QASR_ERR_ARG, "%s: B %d, T %d (1 .. %d) or C %d out of range", who, a->B, a->T, QASR_BAND_MAX_FRAMES, a->C);
  return ctc_targets_check(who, a, QASR_BAND_MAX_LABELS);
}
template <class A>
static int ctc_post_tail_check(const char* who, const A* a, size_t need) {   // the posterior entries: table (required) .. plane
  if (!a->lae_table || a->lae_entries != QASR_BEAM_TABLE_ENTRIES)
    return fail(QASR_ERR_ARG, "%s: lae_table is required and lae_entries %u must be %d", who, a->lae_entries, QASR_BEAM_TABLE_ENTRIES);
  if (a->post_pitch < a->T) return fail(QASR_ERR_ARG, "%s: post_pitch %lld < T %d", who, (long long)a->post_pitch, a->T);
  if (((uintptr_t)a->workspace & 7) != 0) return fail(QASR_ERR_ARG, "%s: workspace is not 8-byte aligned", who);
  return ctc_workspace_plane_check(who, a, need);
}
// what ctc_spot and stream_spot ask of the keywords and of the planes they run over: T frames (the window's Tw) of C classes
template <class A>
static int spot_keywords_check(const char* who, const A* a, int T, int C) {
  if ((long long)a->B * a->K > INT_MAX) return fail(QASR_ERR_ARG, "%s: B %d * K %d is above 2^31 - 1", who, a->B, a->K);
  if (int rc = ctc_max_labels_check(who, a->max_labels, QASR_SPOT_MAX_LABELS)) return rc;
  if (int rc = ctc_blank_check(who, a->blank, C)) return rc;
  if (int rc = ctc_star_pitch_check(who, a->star_pitch, T)) return rc;
  if (int rc = ctc_pitch_check(who, T, C, a->pitch_frame, a->pitch_utt)) return rc;
  if (a->threshold_q < QASR_SPOT_MIN_THRESHOLD_Q || a->threshold_q > 0)
    return fail(QASR_ERR_ARG, "%s: threshold_q %d is outside %d .. 0", who, a->threshold_q, QASR_SPOT_MIN_THRESHOLD_Q);
  if (a->max_span < 1 || a->max_span > QASR_SPOT_MAX_SPAN)
    return fail(QASR_ERR_ARG, "%s: max_span %d is outside 1 .. %d", who, a->max_span, QASR_SPOT_MAX_SPAN);
  return 0;
}
}

// ---- CTC forced alignment (k_align, qasr_align.hip): the checks of include/qasr.h, then one launch
static int align_shape_ok(int P, int T, int max_labels) {
  return P >= 1 && T >= 1 && T <= QASR_BEAM_MAX_FRAMES && max_labels >= 1 && max_labels <= QASR_ALIGN_MAX_LABELS;
}

size_t qasr_ctc_align_workspace_bytes(int P, int T, int max_labels) {
  return align_shape_ok(P, T, max_labels) ? align_workspace_bytes(P, T, max_labels) : 0;
}

int qasr_ctc_align(void* stream, const qasr_ctc_align_args* given) {
  const char* const who = "ctc_align";
  qasr_ctc_align_args full{};
  const qasr_ctc_align_args* const a = &full;
  if (int rc = ctc_two_size_args(who, given, QASR_CTC_ALIGN_ARGS_V1_SIZE, &full)) return rc;
  if (int rc = ctc_five_ptrs_check(who, a)) return rc;
  if (int rc = ctc_problems_check(who, a)) return rc;
  if (a->total && !a->lae_table) return fail(QASR_ERR_ARG, "ctc_align: total needs lae_table");     // the table is optional here
  if (a->lae_table && a->lae_entries != QASR_BEAM_TABLE_ENTRIES)
    return fail(QASR_ERR_ARG, "ctc_align: lae_entries %u is not %d", a->lae_entries, QASR_BEAM_TABLE_ENTRIES);
  if (int rc = ctc_workspace_plane_check(who, a, align_workspace_bytes(a->P, a->T, a->max_labels))) return rc;
  return launched(who, launch_align((hipStream_t)stream, *a));
}

// ---- CTC posteriors along an alignment (k_post, qasr_post.hip): the checks of include/qasr.h, then one launch
size_t qasr_ctc_post_workspace_bytes(int P, int T) {
  return P >= 1 && T >= 1 && T <= QASR_BEAM_MAX_FRAMES ? post_workspace_bytes(P, T) : 0;
}

int qasr_ctc_post(void* stream, const qasr_ctc_post_args* a) {
  const char* const who = "ctc_post";
  if (int rc = args_check(who, a)) return rc;
  if (int rc = ctc_five_ptrs_check(who, a)) return rc;
  if (!a->start || !a->nframes || !a->frame_post || !a->label_post)
    return fail(QASR_ERR_ARG, "ctc_post: start, nframes, frame_post and label_post are required");
  if (int rc = ctc_problems_check(who, a)) return rc;
  if (int rc = ctc_post_tail_check(who, a, post_workspace_bytes(a->P, a->T))) return rc;
  return launched(who, launch_post((hipStream_t)stream, *a));
}

// ---- banded CTC alignment (k_align_band, qasr_align_band.hip): the checks of include/qasr.h, then one launch
static int band_shape_ok(int B, int T, int band_states) {
  return B >= 1 && T >= 1 && T <= QASR_BAND_MAX_FRAMES && band_states_ok(band_states);
}

size_t qasr_ctc_align_band_workspace_bytes(int B, int T, int band_states) {
  return band_shape_ok(B, T, band_states) ? align_band_workspace_bytes(B, T, band_states) : 0;
}

int qasr_ctc_align_band(void* stream, const qasr_ctc_align_band_args* given) {
  const char* const who = "ctc_align_band";
  qasr_ctc_align_band_args full{};
  const qasr_ctc_align_band_args* const a = &full;
  if (int rc = ctc_two_size_args(who, given, QASR_CTC_ALIGN_BAND_ARGS_V1_SIZE, &full)) return rc;
  if (int rc = ctc_five_ptrs_check(who, a)) return rc;
  if (int rc = ctc_band_check(who, a)) return rc;
  if (((uintptr_t)a->workspace & 3) != 0) return fail(QASR_ERR_ARG, "ctc_align_band: workspace is not 4-byte aligned");
  if (int rc = ctc_workspace_plane_check(who, a, align_band_workspace_bytes(a->B, a->T, a->band_states))) return rc;
  return launched(who, launch_align_band((hipStream_t)stream, *a));
}

// ---- CTC posteriors inside the band (k_post_band, qasr_post_band.hip): the checks of include/qasr.h, then one launch
size_t qasr_ctc_post_band_workspace_bytes(int B, int T) {
  return B >= 1 && T >= 1 && T <= QASR_BAND_MAX_FRAMES ? post_band_workspace_bytes(B, T) : 0;
}

int qasr_ctc_post_band(void* stream, const qasr_ctc_post_band_args* a) {
  const char* const who = "ctc_post_band";
  if (int rc = args_check(who, a)) return rc;
  if (int rc = ctc_five_ptrs_check(who, a)) return rc;
  if (!a->start || !a->nframes || !a->band_base || !a->frame_post || !a->label_post)
    return fail(QASR_ERR_ARG, "ctc_post_band: start, nframes, band_base, frame_post and label_post are required");
  if (int rc = ctc_band_check(who, a)) return rc;
  if (int rc = ctc_post_tail_check(who, a, post_band_workspace_bytes(a->B, a->T))) return rc;
  return launched(who, launch_post_band((hipStream_t)stream, *a));
}

// ---- the wildcard's emission plane (k_star, qasr_star.hip): the checks of include/qasr.h, then one launch
int qasr_ctc_star(void* stream, const qasr_ctc_star_args* a) {
  if (int rc = args_check("ctc_star", a)) return rc;
  if (!a->log_probs || !a->star) return fail(QASR_ERR_ARG, "ctc_star: log_probs and star are required");
  if (a->B < 1 || a->T < 1 || a->C < 1) return fail(QASR_ERR_ARG, "ctc_star: B %d, T %d or C %d out of range", a->B, a->T, a->C);
  if (int rc = ctc_pitch_check("ctc_star", a->T, a->C, a->pitch_frame, a->pitch_utt)) return rc;
  if (int rc = ctc_star_pitch_check("ctc_star", a->star_pitch, a->T)) return rc;
  if (!(a->penalty >= 0.f && a->penalty <= QASR_STAR_MAX_PENALTY))   // (a NaN fails both comparisons)
    return fail(QASR_ERR_ARG, "ctc_star: penalty %g is not a finite number in 0 .. %g", (double)a->penalty, (double)QASR_STAR_MAX_PENALTY);
  int rc = launch_star((hipStream_t)stream, *a);
  if (rc) return fail(rc, "ctc_star: launch (B * T above 2^33)");
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

// ---- keyword spotting (k_spot, qasr_spot.hip): the checks of include/qasr.h, then one launch
int qasr_ctc_spot(void* stream, const qasr_ctc_spot_args* a) {
  if (int rc = args_check("ctc_spot", a)) return rc;
  if (!a->log_probs || !a->star_logp || !a->targets || !a->target_lens)
    return fail(QASR_ERR_ARG, "ctc_spot: log_probs, star_logp, targets and target_lens are required");
  if (!a->hit_start || !a->hit_end || !a->hit_score || !a->n_hits || !a->ok)
    return fail(QASR_ERR_ARG, "ctc_spot: hit_start, hit_end, hit_score, n_hits and ok are required");
  if (a->B < 1 || a->T < 1 || a->T > QASR_BAND_MAX_FRAMES || a->C < 1 || a->K < 1)
    return fail(QASR_ERR_ARG, "ctc_spot: B %d, T %d (1 .. %d), C %d or K %d out of range", a->B, a->T, QASR_BAND_MAX_FRAMES, a->C, a->K);
  if (int rc = spot_keywords_check("ctc_spot", a, a->T, a->C)) return rc;
  if (a->max_hits < 1) return fail(QASR_ERR_ARG, "ctc_spot: max_hits %d < 1", a->max_hits);
  if (!a->trace_score != !a->trace_start) return fail(QASR_ERR_ARG, "ctc_spot: trace_score and trace_start go together");
  if (a->trace_score && a->trace_pitch < a->T)
    return fail(QASR_ERR_ARG, "ctc_spot: trace_pitch %lld < T %d", (long long)a->trace_pitch, a->T);
  return launched("ctc_spot", launch_spot((hipStream_t)stream, *a));
}

// ---- word and character error counts (k_edit_cut, k_edit, k_edit_totals, qasr_edit.hip) and the edit path (k_edit_cut,
// k_edit_trace): the checks of include/qasr.h, stated once for the two entry points, then the launches
static bool edit_shape_ok(long long P, int max_hyp, int max_ref, int mode) {
  return P >= 1 && P <= QASR_EDIT_MAX_PROBLEMS && max_hyp >= 1 && max_hyp <= QASR_EDIT_MAX_IDS && max_ref >= 1 &&
         max_ref <= QASR_EDIT_MAX_IDS && (mode == QASR_EDIT_CHAR || mode == QASR_EDIT_WORD);
}
size_t qasr_edit_workspace_bytes(int P, int max_hyp, int max_ref, int mode) {
  return edit_shape_ok(P, max_hyp, max_ref, mode) ? edit_workspace_bytes(P, max_hyp, max_ref, mode) : 0;
}
size_t qasr_edit_trace_workspace_bytes(int P, int max_hyp, int max_ref, int mode) {
  return edit_shape_ok(P, max_hyp, max_ref, mode) ? edit_trace_workspace_bytes(P, max_hyp, max_ref, mode) : 0;
}
// what the two args structs share: the struct itself, the rows, the mode, the shape, the pitches, the workspace (`need`: the
// entry's own query) and the alignment of workspace and rows; `extra`: the entry's further required pointers, named in `names`
extern "C++" {
template <class A>
static int edit_check(const char* who, const A* a, bool extra, const char* names, size_t (*need_of)(long long, int, int, int)) {
  if (int rc = args_check(who, a)) return rc;
  if (!a->hyp || !a->ref || !a->rows || !extra || !a->workspace) return fail(QASR_ERR_ARG, "%s: %s and workspace are required", who, names);
  if (a->mode != QASR_EDIT_CHAR && a->mode != QASR_EDIT_WORD)
    return fail(QASR_ERR_ARG, "%s: mode %d is neither QASR_EDIT_CHAR nor QASR_EDIT_WORD", who, a->mode);
  if (a->mode == QASR_EDIT_WORD && !a->is_space) return fail(QASR_ERR_ARG, "%s: word mode needs is_space", who);
  const long long P = (long long)a->B * a->K;
  if (a->B < 1 || a->K < 1 || a->C < 1 || P > QASR_EDIT_MAX_PROBLEMS)
    return fail(QASR_ERR_ARG, "%s: B %d, K %d or C %d < 1, or B * K above %d", who, a->B, a->K, a->C, QASR_EDIT_MAX_PROBLEMS);
  if (!edit_shape_ok(P, a->max_hyp, a->max_ref, a->mode))
    return fail(QASR_ERR_ARG, "%s: max_hyp %d or max_ref %d is outside 1 .. %d", who, a->max_hyp, a->max_ref, QASR_EDIT_MAX_IDS);
  if (a->hyp_pitch < a->max_hyp || a->ref_pitch < a->max_ref)
    return fail(QASR_ERR_ARG, "%s: hyp_pitch %lld < max_hyp %d or ref_pitch %lld < max_ref %d", who, (long long)a->hyp_pitch,
                a->max_hyp, (long long)a->ref_pitch, a->max_ref);
  const size_t need = need_of(P, a->max_hyp, a->max_ref, a->mode);
  if (a->workspace_bytes < need) return fail(QASR_ERR_ARG, "%s: workspace_bytes %zu < %zu", who, a->workspace_bytes, need);
  if (((uintptr_t)a->workspace | (uintptr_t)a->rows) & 15) return fail(QASR_ERR_ARG, "%s: workspace and rows must be 16-byte aligned", who);
  return QASR_OK;
}
}  // extern "C++"
int qasr_edit_distance(void* stream, const qasr_edit_args* a) {
  if (int rc = edit_check("edit_distance", a, a && a->totals, "hyp, ref, rows, totals", edit_workspace_bytes)) return rc;
  if ((uintptr_t)a->totals & 7) return fail(QASR_ERR_ARG, "edit_distance: totals must be 8-byte aligned");
  return launched("edit_distance", launch_edit((hipStream_t)stream, *a));
}
int qasr_edit_trace(void* stream, const qasr_edit_trace_args* a) {
  if (int rc = edit_check("edit_trace", a, a && a->ops && a->n_ops, "hyp, ref, rows, ops, n_ops", edit_trace_workspace_bytes)) return rc;
  const long long units = (a->mode == QASR_EDIT_WORD ? ((long long)a->max_hyp + 1) / 2 + ((long long)a->max_ref + 1) / 2
                                                     : (long long)a->max_hyp + a->max_ref);
  if (a->ops_pitch < units) return fail(QASR_ERR_ARG, "edit_trace: ops_pitch %lld < %lld units of the two rows", (long long)a->ops_pitch, units);
  if ((uintptr_t)a->n_ops & 3) return fail(QASR_ERR_ARG, "edit_trace: n_ops must be 4-byte aligned");
  return launched("edit_trace", launch_edit_trace((hipStream_t)stream, *a));
}

// ---- minimum Bayes risk re-ranking of n-best rows (k_edit_cut, k_mbr_pair, k_mbr_pick, qasr_mbr.hip): the checks of
// include/qasr.h, then the launches
static bool mbr_shape_ok(int B, int K, int max_ids, int mode) {
  return B >= 1 && K >= 1 && K <= QASR_BEAM_MAX_WIDTH && max_ids >= 1 && max_ids <= QASR_BEAM_MAX_FRAMES &&
         (long long)B * K <= QASR_EDIT_MAX_PROBLEMS && (long long)B * K * (K - 1) / 2 <= QASR_EDIT_MAX_PROBLEMS &&
         (mode == QASR_EDIT_CHAR || mode == QASR_EDIT_WORD);
}
size_t qasr_mbr_workspace_bytes(int B, int K, int max_ids, int mode) {
  return mbr_shape_ok(B, K, max_ids, mode) ? mbr_workspace_bytes(B, K, max_ids, mode) : 0;
}
int qasr_ctc_mbr(void* stream, const qasr_mbr_args* a) {
  const char* const who = "ctc_mbr";
  if (int rc = args_check(who, a)) return rc;
  if (!a->labels || !a->n_labels || !a->score || !a->wtab || !a->weight || !a->wsum || !a->risk || !a->order || !a->ok || !a->workspace)
    return fail(QASR_ERR_ARG, "%s: labels, n_labels, score, wtab, weight, wsum, risk, order, ok and workspace are required", who);
  if (a->mode != QASR_EDIT_CHAR && a->mode != QASR_EDIT_WORD)
    return fail(QASR_ERR_ARG, "%s: mode %d is neither QASR_EDIT_CHAR nor QASR_EDIT_WORD", who, a->mode);
  if (a->mode == QASR_EDIT_WORD && !a->is_space) return fail(QASR_ERR_ARG, "%s: word mode needs is_space", who);
  if (a->C < 1 || !mbr_shape_ok(a->B, a->K, a->max_ids, a->mode))
    return fail(QASR_ERR_ARG, "%s: B %d or C %d < 1, K %d outside 1 .. %d, max_ids %d outside 1 .. %d, or more than %d rows or pairs",
                who, a->B, a->C, a->K, QASR_BEAM_MAX_WIDTH, a->max_ids, QASR_BEAM_MAX_FRAMES, QASR_EDIT_MAX_PROBLEMS);
  if (a->scale_q < 0 || a->scale_q > QASR_MBR_MAX_SCALE_Q)
    return fail(QASR_ERR_ARG, "%s: scale_q %d is outside 0 .. %d", who, a->scale_q, QASR_MBR_MAX_SCALE_Q);
  if (a->wtab_entries != QASR_MBR_TABLE_ENTRIES)
    return fail(QASR_ERR_ARG, "%s: wtab_entries %u is not %d", who, a->wtab_entries, QASR_MBR_TABLE_ENTRIES);
  if (a->label_pitch < a->max_ids) return fail(QASR_ERR_ARG, "%s: label_pitch %lld < max_ids %d", who, (long long)a->label_pitch, a->max_ids);
  const size_t need = mbr_workspace_bytes(a->B, a->K, a->max_ids, a->mode);
  if (a->workspace_bytes < need) return fail(QASR_ERR_ARG, "%s: workspace_bytes %zu < %zu", who, a->workspace_bytes, need);
  if ((uintptr_t)a->workspace & 15) return fail(QASR_ERR_ARG, "%s: workspace must be 16-byte aligned", who);
  if (((uintptr_t)a->wsum | (uintptr_t)a->risk) & 7) return fail(QASR_ERR_ARG, "%s: wsum and risk must be 8-byte aligned", who);
  if (((uintptr_t)a->dist | (uintptr_t)a->weight | (uintptr_t)a->order | (uintptr_t)a->ok) & 3)
    return fail(QASR_ERR_ARG, "%s: dist, weight, order and ok must be 4-byte aligned", who);
  return launched(who, launch_mbr((hipStream_t)stream, *a));
}

// ---- polyphase resampler (k_resample, qasr_resample.hip): host-only validation of a packed table (qasr/resample.py states
// the layout), then the checks of include/qasr.h and one launch
static long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b, b = t;
  }
  return a;
}

static int resample_ratio_ok(int L, int M, int W) {
  return L >= 1 && M >= 1 && W >= 1 && W <= QASR_RESAMPLE_MAX_W && (long long)L * 2 * W <= QASR_RESAMPLE_MAX_ENTRIES &&
         gcd_ll(L, M) == 1;
}

int qasr_resample_check(const void* blob, size_t bytes) {
  enum { HDR = 32 };
  if (!blob) return fail(QASR_ERR_BLOB, "resample_check: blob is NULL");
  if (bytes < HDR * 4 || bytes > (size_t)INT32_MAX) return fail(QASR_ERR_BLOB, "resample_check: %zu bytes is no resampling table", bytes);
  if (((uintptr_t)blob & 3) != 0) return fail(QASR_ERR_BLOB, "resample_check: blob is not 4-byte aligned");
  const int32_t* h = (const int32_t*)blob;
  if (h[0] != 0x31535251 || h[1] != 1) return fail(QASR_ERR_BLOB, "resample_check: magic %#x / version %d", (unsigned)h[0], h[1]);
  const int L = h[3], M = h[4], W = h[5], sr_in = h[6], sr_out = h[7], quality = h[8], entries = h[9];
  if (!resample_ratio_ok(L, M, W))
    return fail(QASR_ERR_BLOB, "resample_check: L %d / M %d (coprime, >= 1), W %d (1 .. %d) or L * 2 W (<= %d) out of range", L, M, W,
                QASR_RESAMPLE_MAX_W, QASR_RESAMPLE_MAX_ENTRIES);
  if (sr_in < 1 || sr_out < 1 || (long long)sr_in * L != (long long)sr_out * M)
    return fail(QASR_ERR_BLOB, "resample_check: %d Hz -> %d Hz does not reduce to L / M = %d / %d", sr_in, sr_out, L, M);
  if (quality != 0 && quality != 1) return fail(QASR_ERR_BLOB, "resample_check: quality %d", quality);
  if (entries != L * 2 * W) return fail(QASR_ERR_BLOB, "resample_check: table of %d entries, L * 2 W = %d", entries, L * 2 * W);
  const uint64_t total = 4ull * HDR + 4ull * (uint64_t)entries;
  if (total != (uint64_t)bytes || h[2] != (int32_t)bytes)
    return fail(QASR_ERR_BLOB, "resample_check: %zu bytes, the header describes %llu (total field %d)", bytes, (unsigned long long)total, h[2]);
  for (int i = 10; i < HDR; ++i)
    if (h[i] != 0) return fail(QASR_ERR_BLOB, "resample_check: reserved header word %d is %d", i, h[i]);
  const int32_t* tab = h + HDR;
  const int64_t limit = (int64_t)1 << 53;
  for (int r = 0; r < L; ++r) {                                       // the accumulator bound, recomputed from the table
    int64_t sum = 0;
    for (int j = 0; j < 2 * W; ++j) {
      const int64_t c = tab[(size_t)j * L + r];
      sum += c < 0 ? -c : c;
    }
    if (sum * 32768 * QASR_RESAMPLE_MAX_CHANNELS >= limit)
      return fail(QASR_ERR_BLOB, "resample_check: column %d sums to %lld: %d channels of int16 would pass 2^53 in the accumulator", r,
                  (long long)sum, QASR_RESAMPLE_MAX_CHANNELS);
  }
  return QASR_OK;
}

int qasr_resample_out_samples(int in_samples, int L, int M) {
  if (in_samples < 0 || L < 1 || M < 1) return -1;
  const long long n = ((long long)in_samples * L + M - 1) / M;
  return n > (long long)INT32_MAX ? -1 : (int)n;
}

int qasr_resample(void* stream, const qasr_resample_args* a) {
  if (int rc = args_check("resample", a)) return rc;
  if (!a->blob || !a->in || !a->in_lens || !a->out || !a->out_lens)
    return fail(QASR_ERR_ARG, "resample: blob, in, in_lens, out and out_lens are required");
  if (a->B < 1 || a->B > 65535) return fail(QASR_ERR_ARG, "resample: B %d is outside 1 .. 65535", a->B);
  if (a->channels < 1 || a->channels > QASR_RESAMPLE_MAX_CHANNELS)
    return fail(QASR_ERR_ARG, "resample: channels %d is outside 1 .. %d", a->channels, QASR_RESAMPLE_MAX_CHANNELS);
  if (a->dtype != QASR_PCM_S16 && a->dtype != QASR_PCM_F32) return fail(QASR_ERR_ARG, "resample: dtype %d is neither int16 nor float32", a->dtype);
  if (!resample_ratio_ok(a->L, a->M, a->W))
    return fail(QASR_ERR_ARG, "resample: L %d / M %d, W %d (1 .. %d) or L * 2 W (<= %d) out of range", a->L, a->M, a->W, QASR_RESAMPLE_MAX_W,
                QASR_RESAMPLE_MAX_ENTRIES);
  if (((uintptr_t)a->blob & 15) != 0 || a->blob_bytes != 128 + 8 * (size_t)a->L * (size_t)a->W)
    return fail(QASR_ERR_ARG, "resample: blob must be 16-byte aligned and 128 + 4 * L * 2 W = %zu bytes, got %zu",
                128 + 8 * (size_t)a->L * (size_t)a->W, a->blob_bytes);
  if (a->in_pitch < 0 || a->in_pitch > QASR_RESAMPLE_MAX_PITCH || a->out_pitch < 0 || a->out_pitch > QASR_RESAMPLE_MAX_PITCH)
    return fail(QASR_ERR_ARG, "resample: in_pitch %lld or out_pitch %lld is outside 0 .. 2^38", (long long)a->in_pitch, (long long)a->out_pitch);
  return launched("resample", launch_resample((hipStream_t)stream, *a));
}

// ---- long recordings (k_cut, k_stitch, qasr_longform.hip): the checks of include/qasr.h and one launch each
int qasr_longform_cut(void* stream, const qasr_longform_cut_args* a) {
  if (int rc = args_check("longform_cut", a)) return rc;
  if (!a->audio || !a->lens || !a->table || !a->windows || !a->window_lens)
    return fail(QASR_ERR_ARG, "longform_cut: audio, lens, table, windows and window_lens are required");
  if (a->Wn < 1 || a->Wn > 65535) return fail(QASR_ERR_ARG, "longform_cut: Wn %d is outside 1 .. 65535", a->Wn);
  if (a->R < 1 || a->Wl < 1 || a->pitch < 0)
    return fail(QASR_ERR_ARG, "longform_cut: R %d, Wl %d (both >= 1) or pitch %lld (>= 0) out of range", a->R, a->Wl, (long long)a->pitch);
  return launched("longform_cut", launch_longform_cut((hipStream_t)stream, *a));
}

int qasr_longform_stitch(void* stream, const qasr_longform_stitch_args* a) {
  if (int rc = args_check("longform_stitch", a)) return rc;
  if (!a->table || !a->enc_lens || !a->tokens || !a->total_frames || !a->seams)
    return fail(QASR_ERR_ARG, "longform_stitch: table, enc_lens, tokens, total_frames and seams are required");
  if (a->Wn < 1) return fail(QASR_ERR_ARG, "longform_stitch: Wn %d < 1", a->Wn);
  if (a->R < 1 || a->Tw < 1 || a->Tmax < 1 || a->hop_frames < 1)
    return fail(QASR_ERR_ARG, "longform_stitch: R %d, Tw %d, Tmax %d or hop_frames %d < 1", a->R, a->Tw, a->Tmax, a->hop_frames);
  if (a->guard < 0) return fail(QASR_ERR_ARG, "longform_stitch: guard %d < 0", a->guard);
  if (a->seam_mode != QASR_SEAM_BLANK && a->seam_mode != QASR_SEAM_MIDDLE)
    return fail(QASR_ERR_ARG, "longform_stitch: seam_mode %d is neither blank nor middle", a->seam_mode);
  if (a->n_planes < 0 || a->n_planes > QASR_LONGFORM_MAX_PLANES)
    return fail(QASR_ERR_ARG, "longform_stitch: %d planes, at most %d", a->n_planes, QASR_LONGFORM_MAX_PLANES);
  for (int k = 0; k < a->n_planes; ++k) {
    const qasr_longform_plane& q = a->planes[k];
    if (!q.src || !q.dst) return fail(QASR_ERR_ARG, "longform_stitch: plane %d has a NULL src or dst", k);
    if (q.bytes_per_frame < 4 || q.bytes_per_frame % 4 != 0)
      return fail(QASR_ERR_ARG, "longform_stitch: plane %d: bytes_per_frame %lld is not a positive multiple of 4", k, (long long)q.bytes_per_frame);
    if ((((uintptr_t)q.src | (uintptr_t)q.dst) & 3) != 0) return fail(QASR_ERR_ARG, "longform_stitch: plane %d is not 4-byte aligned", k);
  }
  return launched("longform_stitch", launch_longform_stitch((hipStream_t)stream, *a));
}

// ---- streaming (k_stream_push / _window / _emit, qasr_stream.hip): the checks of include/qasr.h and one launch each
size_t qasr_stream_state_bytes(int S, int Wl, int C) { return stream_state_bytes(S, Wl, C); }

static int stream_geometry(const char* who, int S, int B, int Wl, int C, int Rr, int spf, size_t state_bytes) {
  if (S < 1 || B < 1 || B > S || B > 65535) return fail(QASR_ERR_ARG, "%s: B %d must lie in 1 .. min(S = %d, 65535)", who, B, S);
  if (Wl < 1 || C < 1 || spf < 1) return fail(QASR_ERR_ARG, "%s: Wl %d, C %d and samples_per_frame %d must be at least 1", who, Wl, C, spf);
  if (Wl % spf || C % spf || Rr % spf)
    return fail(QASR_ERR_ARG, "%s: Wl %d, C %d and Rr %d must be multiples of samples_per_frame %d", who, Wl, C, Rr, spf);
  if (Rr < 0 || (long long)Rr + C > Wl) return fail(QASR_ERR_ARG, "%s: Rr %d must lie in 0 .. Wl - C = %d", who, Rr, Wl - C);
  const size_t need = stream_state_bytes(S, Wl, C);
  if (!need || state_bytes < need) return fail(QASR_ERR_ARG, "%s: state_bytes %zu, qasr_stream_state_bytes gives %zu", who, state_bytes, need);
  return QASR_OK;
}

int qasr_stream_push(void* stream, const qasr_stream_push_args* a) {
  if (int rc = args_check("stream_push", a)) return rc;
  if (!a->state || !a->slots || !a->flags || !a->n_new || !a->chunk)
    return fail(QASR_ERR_ARG, "stream_push: state, slots, flags, n_new and chunk are required");
  int rc = stream_geometry("stream_push", a->S, a->B, a->Wl, a->C, 0, a->samples_per_frame, a->state_bytes);
  if (rc) return rc;
  if (a->dtype != QASR_PCM_S16 && a->dtype != QASR_PCM_F32) return fail(QASR_ERR_ARG, "stream_push: dtype %d is neither s16 nor f32", a->dtype);
  if (a->pitch < 0) return fail(QASR_ERR_ARG, "stream_push: pitch %lld < 0", (long long)a->pitch);
  if ((uintptr_t)a->state & 15) return fail(QASR_ERR_ARG, "stream_push: state is not 16-byte aligned");
  return launched("stream_push", launch_stream_push((hipStream_t)stream, *a));
}

int qasr_stream_window(void* stream, const qasr_stream_window_args* a) {
  if (int rc = args_check("stream_window", a)) return rc;
  if (!a->state || !a->slots || !a->windows || !a->window_lens || !a->first_frame)
    return fail(QASR_ERR_ARG, "stream_window: state, slots, windows, window_lens and first_frame are required");
  int rc = stream_geometry("stream_window", a->S, a->B, a->Wl, a->C, 0, a->samples_per_frame, a->state_bytes);
  if (rc) return rc;
  if ((uintptr_t)a->state & 15) return fail(QASR_ERR_ARG, "stream_window: state is not 16-byte aligned");
  return launched("stream_window", launch_stream_window((hipStream_t)stream, *a));
}

int qasr_stream_emit(void* stream, const qasr_stream_emit_args* a) {
  if (int rc = args_check("stream_emit", a)) return rc;
  if (!a->state || !a->slots || !a->flags || !a->tokens || !a->frame_score || !a->enc_lens || !a->first_frame || !a->labels ||
      !a->start || !a->nframes || !a->score || !a->n_new_labels || !a->status || !a->total_frames || !a->utt_score)
    return fail(QASR_ERR_ARG, "stream_emit: every pointer but tail_labels / tail_n is required");
  int rc = stream_geometry("stream_emit", a->S, a->B, a->Wl, a->C, a->Rr, a->samples_per_frame, a->state_bytes);
  if (rc) return rc;
  if (a->Tw < 1 || a->P < 1) return fail(QASR_ERR_ARG, "stream_emit: Tw %d and P %d must be at least 1", a->Tw, a->P);
  if ((a->tail_labels == nullptr) != (a->tail_n == nullptr)) return fail(QASR_ERR_ARG, "stream_emit: tail_labels and tail_n come together");
  if (a->tail_labels && a->Ptail < 1) return fail(QASR_ERR_ARG, "stream_emit: Ptail %d < 1", a->Ptail);
  if ((uintptr_t)a->state & 15) return fail(QASR_ERR_ARG, "stream_emit: state is not 16-byte aligned");
  return launched("stream_emit", launch_stream_emit((hipStream_t)stream, *a));
}

// ---- streaming beam search (k_stream_beam, qasr_stream_beam.hip): the checks of include/qasr.h and one launch
size_t qasr_stream_beam_state_bytes(int S, int beam_width, int F) { return stream_beam_state_bytes(S, beam_width, F); }

// What qasr_stream_beam, _boost and _ep ask of the embedded qasr_stream_beam_args, in the order they ask it: the pointers (the
// entry words that refusal: _ep does not want the END outputs), stream_geometry, the ranges Tw .. F, then the tail from the beam
// state's size (`need` bytes, by the query that `query` names) to the pitches, then the model.
static bool stream_beam_step_ptrs(const qasr_stream_beam_args* a) {
  return a->state && a->beam_state && a->slots && a->flags && a->cand_id && a->cand_q && a->enc_lens && a->first_frame && a->lae_table &&
         a->labels && a->frames && a->n_new_labels && a->commit_len && a->n_live && a->status && a->tail_labels && a->tail_n;
}
static int stream_beam_width_check(const char* who, int W) {
  return W < 1 || W > QASR_BEAM_MAX_WIDTH ? fail(QASR_ERR_ARG, "%s: beam_width %d is outside 1 .. %d", who, W, QASR_BEAM_MAX_WIDTH) : 0;
}
static int stream_beam_range_check(const char* who, const qasr_stream_beam_args* a) {
  if (a->Tw < 1 || a->Tw > QASR_BEAM_MAX_FRAMES || (int64_t)a->B * a->Tw >= (1ll << 31))
    return fail(QASR_ERR_ARG, "%s: Tw %d is outside 1 .. %d (or B * Tw >= 2^31)", who, a->Tw, QASR_BEAM_MAX_FRAMES);
  if (int rc = stream_beam_width_check(who, a->beam_width)) return rc;
  if (int rc = beam_cand_check(who, a->N, a->n_best, a->beam_width, a->blank, a->lae_entries)) return rc;
  if (a->Lg < 0 || a->K < 1 || a->K > QASR_STREAM_BEAM_ROUND)
    return fail(QASR_ERR_ARG, "%s: Lg %d < 0 or K %d outside 1 .. %d", who, a->Lg, a->K, QASR_STREAM_BEAM_ROUND);
  if (a->F > QASR_STREAM_BEAM_MAX_RING || (int64_t)a->F < (int64_t)a->Lg + a->K)
    return fail(QASR_ERR_ARG, "%s: F %d must lie in Lg + K = %lld .. %d", who, a->F, (long long)a->Lg + a->K, QASR_STREAM_BEAM_MAX_RING);
  return 0;
}
static int stream_beam_tail_check(const char* who, const qasr_stream_beam_args* a, size_t need, const char* query) {
  if (!need || a->beam_state_bytes < need)
    return fail(QASR_ERR_ARG, "%s: beam_state_bytes %zu, %s gives %zu", who, a->beam_state_bytes, query, need);
  if (((uintptr_t)a->state | (uintptr_t)a->beam_state) & 15) return fail(QASR_ERR_ARG, "%s: state or beam_state is not 16-byte aligned", who);
  if (a->max_final_frames < 1 || a->max_final_frames > a->Tw)
    return fail(QASR_ERR_ARG, "%s: max_final_frames %d is outside 1 .. Tw", who, a->max_final_frames);
  if ((int64_t)a->P < (int64_t)a->F + a->max_final_frames || a->Ptail < 1 || a->Pend < a->F)
    return fail(QASR_ERR_ARG, "%s: P %d < F + max_final_frames = %lld, Ptail %d < 1 or Pend %d < F = %d", who, a->P,
                (long long)a->F + a->max_final_frames, a->Ptail, a->Pend, a->F);
  return 0;
}
static int stream_beam_lm_check(const char* who, const qasr_stream_beam_args* a, const void* lm_score, const char* lm_score_name) {
  if (!a->lm) return 0;
  if (!lm_score) return fail(QASR_ERR_ARG, "%s: %s is required with lm", who, lm_score_name);
  return beam_lm_check(who, a->lm, a->lm_bytes, a->alpha_q, a->beta_q);
}
static size_t stream_beam_need(const qasr_stream_beam_args* a, bool boosted) {
  return boosted ? stream_beam_boost_state_bytes(a->S, a->beam_width, a->F) : stream_beam_state_bytes(a->S, a->beam_width, a->F);
}
// all of it for the two calls that write the END outputs
static int stream_beam_checks(const char* who, const qasr_stream_beam_args* a, bool boosted) {
  if (int rc = args_check(who, a)) return rc;
  if (!stream_beam_step_ptrs(a) || !a->end_labels || !a->end_n_labels || !a->end_score || !a->n_hyps)
    return fail(QASR_ERR_ARG, "%s: every pointer but lm (and end_lm_score without lm) is required", who);
  if (int rc = stream_geometry(who, a->S, a->B, a->Wl, a->C, a->Rr, a->samples_per_frame, a->state_bytes)) return rc;
  if (int rc = stream_beam_range_check(who, a)) return rc;
  if (int rc = stream_beam_tail_check(who, a, stream_beam_need(a, boosted), boosted ? "qasr_stream_beam_boost_state_bytes" : "qasr_stream_beam_state_bytes"))
    return rc;
  if (int rc = stream_beam_lm_check(who, a, a->end_lm_score, "end_lm_score")) return rc;
  return a->lm ? beam_space_check(who, a->space, a->blank) : 0;
}
// the phrase sets of qasr_stream_beam_boost and _ep
static int stream_beam_sets_check(const char* who, const qasr_stream_beam_boost_args* q) {
  for (int g = 0; g < q->n_sets; ++g) {
    if (!q->sets[g] || ((uintptr_t)q->sets[g] & 15) != 0 || q->set_bytes[g] < 128 || q->set_bytes[g] > (size_t)INT32_MAX)
      return fail(QASR_ERR_ARG, "%s: set %d must be 16-byte aligned and 128 .. 2^31 - 1 bytes, got %zu", who, g, q->set_bytes[g]);
    if (q->whole_words[g] != 0 && q->beam.space < 0)
      return fail(QASR_ERR_ARG, "%s: set %d: whole words need the space label, got %d", who, g, q->beam.space);
  }
  return 0;
}

int qasr_stream_beam(void* stream, const qasr_stream_beam_args* a) {
  if (int rc = stream_beam_checks("stream_beam", a, false)) return rc;
  return launched("stream_beam", launch_stream_beam((hipStream_t)stream, *a));
}

// ---- streaming phrase boosting (k_stream_beam_boost, qasr_stream_beam_boost.hip): qasr_stream_beam's checks under this call's
// name and against its own state query, the sets' checks and one launch.  beam_width is asked about first here, as it always
// was, and space a second time for the sets' sake (a call without lm has not been asked yet).
size_t qasr_stream_beam_boost_state_bytes(int S, int beam_width, int F) { return stream_beam_boost_state_bytes(S, beam_width, F); }

int qasr_stream_beam_boost(void* stream, const qasr_stream_beam_boost_args* q) {
  const char* const who = "stream_beam_boost";
  if (int rc = args_check(who, q)) return rc;
  const qasr_stream_beam_args* a = &q->beam;
  if (int rc = stream_beam_width_check(who, a->beam_width)) return rc;
  if (int rc = stream_beam_checks(who, a, true)) return rc;
  if (q->n_sets < 1 || q->n_sets > QASR_STREAM_BEAM_MAX_SETS)
    return fail(QASR_ERR_ARG, "%s: n_sets %d is outside 1 .. %d", who, q->n_sets, QASR_STREAM_BEAM_MAX_SETS);
  if (!q->boost_set || !q->end_boost_score) return fail(QASR_ERR_ARG, "%s: boost_set and end_boost_score are required", who);
  if (int rc = beam_space_check(who, a->space, a->blank)) return rc;
  if (int rc = stream_beam_sets_check(who, q)) return rc;
  return launched(who, launch_stream_beam_boost((hipStream_t)stream, *q));
}

// ---- streaming beam endpointing (k_stream_beam_ep, qasr_stream_beam_ep.hip): the same blocks under this call's name, without
// the END outputs it ignores; n_sets (0 allowed) is asked between F and the state's size because it picks the query; space once,
// for the model or the sets; then the records' and the cut outputs' checks, and one launch
int qasr_stream_beam_ep(void* stream, const qasr_stream_beam_ep_args* x) {
  const char* const who = "stream_beam_ep";
  if (int rc = args_check(who, x)) return rc;
  const qasr_stream_beam_boost_args* q = &x->boost;
  const qasr_stream_beam_args* a = &q->beam;
  if (q->struct_size != sizeof(qasr_stream_beam_boost_args) || a->struct_size != sizeof(qasr_stream_beam_args))
    return fail(QASR_ERR_ARG, "stream_beam_ep: boost.struct_size %u is not %zu or boost.beam.struct_size %u is not %zu", q->struct_size,
                sizeof(qasr_stream_beam_boost_args), a->struct_size, sizeof(qasr_stream_beam_args));
  if (!stream_beam_step_ptrs(a)) return fail(QASR_ERR_ARG, "stream_beam_ep: every pointer of the step but lm and the END outputs is required");
  if (int rc = stream_geometry(who, a->S, a->B, a->Wl, a->C, a->Rr, a->samples_per_frame, a->state_bytes)) return rc;
  if (int rc = stream_beam_range_check(who, a)) return rc;
  if (q->n_sets < 0 || q->n_sets > QASR_STREAM_BEAM_MAX_SETS)
    return fail(QASR_ERR_ARG, "stream_beam_ep: n_sets %d is outside 0 .. %d", q->n_sets, QASR_STREAM_BEAM_MAX_SETS);
  char query[48];
  snprintf(query, sizeof query, "the state query for %d sets", q->n_sets);
  if (int rc = stream_beam_tail_check(who, a, stream_beam_need(a, q->n_sets != 0), query)) return rc;
  if (int rc = stream_beam_lm_check(who, a, x->cut_lm_score, "cut_lm_score")) return rc;
  if (a->lm || q->n_sets)
    if (int rc = beam_space_check(who, a->space, a->blank)) return rc;
  if (q->n_sets) {
    if (!q->boost_set || !x->cut_boost_score) return fail(QASR_ERR_ARG, "stream_beam_ep: boost_set and cut_boost_score are required with sets");
    if (int rc = stream_beam_sets_check(who, q)) return rc;
  }
  const int64_t cuts = (int64_t)a->B * x->E, per_cut = (int64_t)a->n_best * a->Pend;      // each below 2^62: no overflow below
  if (x->E < 1 || cuts >= (1ll << 31) / QASR_STREAM_EP_RECORD_WORDS || per_cut >= (1ll << 31) || cuts * per_cut >= (1ll << 31))
    return fail(QASR_ERR_ARG, "stream_beam_ep: E %d must be at least 1 (and B * E * n_best * Pend below 2^31)", x->E);
  if (!x->records || !x->n_records || !x->ep_status || !x->n_cuts || !x->cut_n_hyps || !x->cut_delta_end || !x->cut_labels ||
      !x->cut_n_labels || !x->cut_score)
    return fail(QASR_ERR_ARG, "stream_beam_ep: records, n_records, ep_status and every cut output (cut_lm_score with lm, cut_boost_score with sets) are required");
  return launched(who, launch_stream_beam_ep((hipStream_t)stream, *x));
}

// ---- streaming endpointing (k_stream_endpoint, qasr_stream_ep.hip): the checks of include/qasr.h and one launch
size_t qasr_stream_ep_state_bytes(int S) { return stream_ep_state_bytes(S); }

int qasr_stream_endpoint(void* stream, const qasr_stream_endpoint_args* a) {
  if (int rc = args_check("stream_endpoint", a)) return rc;
  if (!a->state || !a->ep_state || !a->slots || !a->flags || !a->tokens || !a->frame_score || !a->enc_lens || !a->first_frame ||
      !a->emit_start || !a->emit_nframes || !a->emit_n_new_labels || !a->emit_status || !a->records || !a->n_records || !a->status)
    return fail(QASR_ERR_ARG, "stream_endpoint: every pointer is required");
  int rc = stream_geometry("stream_endpoint", a->S, a->B, a->Wl, a->C, a->Rr, a->samples_per_frame, a->state_bytes);
  if (rc) return rc;
  if (a->Tw < 1 || a->P < 1) return fail(QASR_ERR_ARG, "stream_endpoint: Tw %d and P %d must be at least 1", a->Tw, a->P);
  if (a->E < 1 || (int64_t)a->B * a->E * QASR_STREAM_EP_RECORD_WORDS >= (1ll << 31))
    return fail(QASR_ERR_ARG, "stream_endpoint: E %d must be at least 1 (and B * E * 10 below 2^31)", a->E);
  if (a->Fsil < 1 || a->Fstart < 1 || a->Fmax < 1 || a->Fhard < a->Fmax || a->Fsil > QASR_STREAM_EP_MAX_FRAMES ||
      a->Fstart > QASR_STREAM_EP_MAX_FRAMES || a->Fhard > QASR_STREAM_EP_MAX_FRAMES)
    return fail(QASR_ERR_ARG, "stream_endpoint: Fsil %d, Fstart %d, Fmax %d must lie in 1 .. 2^24 and Fhard %d in Fmax .. 2^24", a->Fsil,
                a->Fstart, a->Fmax, a->Fhard);
  if (a->min_logp != a->min_logp) return fail(QASR_ERR_ARG, "stream_endpoint: min_logp is NaN");
  const size_t need = stream_ep_state_bytes(a->S);
  if (!need || a->ep_state_bytes < need)
    return fail(QASR_ERR_ARG, "stream_endpoint: ep_state_bytes %zu, qasr_stream_ep_state_bytes gives %zu", a->ep_state_bytes, need);
  if (((uintptr_t)a->state | (uintptr_t)a->ep_state) & 15) return fail(QASR_ERR_ARG, "stream_endpoint: state or ep_state is not 16-byte aligned");
  return launched("stream_endpoint", launch_stream_endpoint((hipStream_t)stream, *a));
}

// ---- streaming keyword spotting (k_stream_spot, qasr_stream_spot.hip): qasr_stream_emit's checks of the session's geometry,
// qasr_ctc_spot's of the keywords and the window's planes (spot_keywords_check with T = Tw), the spot state's, and one launch
size_t qasr_stream_spot_state_bytes(int S, int K, int max_labels) { return stream_spot_state_bytes(S, K, max_labels); }

int qasr_stream_spot(void* stream, const qasr_stream_spot_args* a) {
  const char* const who = "stream_spot";
  if (int rc = args_check(who, a)) return rc;
  if (!a->state || !a->spot_state || !a->slots || !a->flags || !a->log_probs || !a->star_logp || !a->enc_lens || !a->first_frame ||
      !a->emit_status || !a->targets || !a->target_lens)
    return fail(QASR_ERR_ARG, "stream_spot: state, spot_state, slots, flags, log_probs, star_logp, enc_lens, first_frame, emit_status, targets and target_lens are required");
  if (!a->hit_start || !a->hit_end || !a->hit_detect || !a->hit_score || !a->n_new_hits || !a->n_hits_total || !a->open_start ||
      !a->open_end || !a->open_score || !a->ok || !a->status)
    return fail(QASR_ERR_ARG, "stream_spot: every output pointer is required");
  if (int rc = stream_geometry(who, a->S, a->B, a->Wl, a->C, a->Rr, a->samples_per_frame, a->state_bytes)) return rc;
  if (a->Tw < 1 || a->n_classes < 1 || a->K < 1)
    return fail(QASR_ERR_ARG, "stream_spot: Tw %d, n_classes %d and K %d must be at least 1", a->Tw, a->n_classes, a->K);
  if (int rc = spot_keywords_check(who, a, a->Tw, a->n_classes)) return rc;
  if (a->PH < 1) return fail(QASR_ERR_ARG, "stream_spot: PH %d < 1", a->PH);
  if (a->max_final_frames < 1 || a->max_final_frames > a->Tw)
    return fail(QASR_ERR_ARG, "stream_spot: max_final_frames %d is outside 1 .. Tw = %d", a->max_final_frames, a->Tw);
  const size_t need = stream_spot_state_bytes(a->S, a->K, a->max_labels);
  if (!need || a->spot_state_bytes < need)
    return fail(QASR_ERR_ARG, "stream_spot: spot_state_bytes %zu, qasr_stream_spot_state_bytes gives %zu", a->spot_state_bytes, need);
  if (((uintptr_t)a->state | (uintptr_t)a->spot_state) & 15) return fail(QASR_ERR_ARG, "stream_spot: state or spot_state is not 16-byte aligned");
  return launched(who, launch_stream_spot((hipStream_t)stream, *a));
}

// ---- streaming at any sample rate (k_stream_rs_append / _fir, qasr_stream_rs.hip): the checks of include/qasr.h, two launches
size_t qasr_stream_rs_state_bytes(int S, int hcap) { return stream_rs_state_bytes(S, hcap); }
size_t qasr_stream_rs_work_bytes(int B) { return stream_rs_work_bytes(B); }

int qasr_stream_rs_push(void* stream, const qasr_stream_rs_push_args* a) {
  if (int rc = args_check("stream_rs_push", a)) return rc;
  if (!a->state || !a->rs_state || !a->work || !a->blob || !a->slots || !a->flags || !a->n_in || !a->out_limit || !a->chunk ||
      !a->n_taken || !a->n_out || !a->status)
    return fail(QASR_ERR_ARG, "stream_rs_push: every pointer is required");
  int rc = stream_geometry("stream_rs_push", a->S, a->B, a->Wl, a->C, 0, a->samples_per_frame, a->state_bytes);
  if (rc) return rc;
  if (a->channels < 1 || a->channels > QASR_RESAMPLE_MAX_CHANNELS)
    return fail(QASR_ERR_ARG, "stream_rs_push: channels %d is outside 1 .. %d", a->channels, QASR_RESAMPLE_MAX_CHANNELS);
  if (a->dtype != QASR_PCM_S16 && a->dtype != QASR_PCM_F32) return fail(QASR_ERR_ARG, "stream_rs_push: dtype %d is neither s16 nor f32", a->dtype);
  if (!resample_ratio_ok(a->L, a->M, a->W))
    return fail(QASR_ERR_ARG, "stream_rs_push: L %d / M %d, W %d (1 .. %d) or L * 2 W (<= %d) out of range", a->L, a->M, a->W,
                QASR_RESAMPLE_MAX_W, QASR_RESAMPLE_MAX_ENTRIES);
  const int Wf = (a->L == 1 && a->M == 1) ? 0 : a->W;
  const size_t need_rs = stream_rs_state_bytes(a->S, a->hcap), need_work = stream_rs_work_bytes(a->B);
  if (!need_rs || a->hcap < 2 * Wf)
    return fail(QASR_ERR_ARG, "stream_rs_push: hcap %d must be a multiple of 4 in max(4, 2 W = %d) .. 2^26", a->hcap, 2 * Wf);
  if (a->rs_state_bytes < need_rs)
    return fail(QASR_ERR_ARG, "stream_rs_push: rs_state_bytes %zu, qasr_stream_rs_state_bytes gives %zu", a->rs_state_bytes, need_rs);
  if (a->work_bytes < need_work)
    return fail(QASR_ERR_ARG, "stream_rs_push: work_bytes %zu, qasr_stream_rs_work_bytes gives %zu", a->work_bytes, need_work);
  if ((((uintptr_t)a->state | (uintptr_t)a->rs_state | (uintptr_t)a->work | (uintptr_t)a->blob) & 15) != 0)
    return fail(QASR_ERR_ARG, "stream_rs_push: state, rs_state, work and blob must be 16-byte aligned");
  if (a->blob_bytes != 128 + 8 * (size_t)a->L * (size_t)a->W)
    return fail(QASR_ERR_ARG, "stream_rs_push: blob must be 128 + 4 * L * 2 W = %zu bytes, got %zu", 128 + 8 * (size_t)a->L * (size_t)a->W,
                a->blob_bytes);
  if (a->pitch < 0 || a->pitch > QASR_RESAMPLE_MAX_PITCH)
    return fail(QASR_ERR_ARG, "stream_rs_push: pitch %lld is outside 0 .. 2^38", (long long)a->pitch);
  return launched("stream_rs_push", launch_stream_rs_push((hipStream_t)stream, *a));
}

int qasr_engine_attach_ctc(qasr_engine* e, float* frame_score, const qasr_ctc_out* out, int use_lens) {
  if (!e) return fail(QASR_ERR_ARG, "attach_ctc: engine is NULL");
  if (frame_score || out) {
    if (logsoftmax_op(e) < 0) return fail(QASR_ERR_ARG, "attach_ctc: the model has no LOGSOFTMAX op (no CTC decoder)");
    if (out) {
      int rc = ctc_out_check(out, frame_score != nullptr, "attach_ctc");
      if (rc) return rc;
    }
  }
  e->ctc_fs = frame_score;
  e->ctc_on = out != nullptr;
  e->ctc_out = out ? *out : qasr_ctc_out{};
  e->ctc_use_lens = (out && use_lens) ? 1 : 0;
  return QASR_OK;
}

int qasr_engine_forward(qasr_engine* e, void* stream, const float* feats, const int32_t* lens, int B, int T,
                        float* logp, int32_t* tokens, int32_t* lens_out) {
  if (!e || !feats || !lens || B <= 0 || T <= 0) return fail(QASR_ERR_ARG, "bad forward arguments");
  return forward_impl(e, (hipStream_t)stream, nullptr, (float*)feats, (int32_t*)lens, B, T, logp, tokens, lens_out);
}

int qasr_engine_forward_audio(qasr_engine* e, void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                              const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                              const void* frontend_plan, size_t plan_bytes, float* feats, int32_t* feat_lens, float* logp,
                              int32_t* tokens, int32_t* lens_out) {
  if (!e || !audio || !audio_lens || !fb || !window || !frontend_plan || !feats || !feat_lens || B <= 0 || S <= 0)
    return fail(QASR_ERR_ARG, "bad forward_audio arguments");
  FrontArgs fe{audio, audio_lens, S, fb, window, n_mels, preemph, pad_to, frontend_plan, plan_bytes, nullptr};
  return forward_impl(e, (hipStream_t)stream, &fe, feats, feat_lens, B, qasr_frontend_frames(S, pad_to), logp, tokens, lens_out);
}

// ---------------------------------------------------------------------------------- reserved engines (ragged batches)
int qasr_ragged_bucket_frames(int max_frames, int max_graphs, int T) { return ragged_bucket(max_frames, max_graphs, T); }

int qasr_ragged_envelope_frames(int max_samples, int max_frames, int pad_to) {
  if (pad_to == 0) pad_to = 16;
  if (pad_to < 1 || QASR_RAGGED_TILE % pad_to || max_samples < 0 || max_frames < 0 || (max_samples == 0 && max_frames == 0)) return -1;
  if (max_samples > (1 << 28) || max_frames > (1 << 24)) return -1;
  int m = max_frames;
  if (max_samples > 0) m = std::max(m, qasr_frontend_frames(max_samples, pad_to));
  return rup(m, QASR_RAGGED_TILE);
}

int qasr_engine_reserve(qasr_engine* e, const qasr_reserve_opts* opts) {
  // the options first: refused without an engine and without touching the device
  if (!opts) return fail(QASR_ERR_ARG, "reserve: opts is NULL");
  if (opts->struct_size != sizeof(qasr_reserve_opts))
    return fail(QASR_ERR_ARG, "reserve: qasr_reserve_opts.struct_size %u is not %zu", opts->struct_size, sizeof(qasr_reserve_opts));
  const qasr_reserve_opts o = *opts;
  if (o.max_batch < 1 || o.max_batch > 4096) return fail(QASR_ERR_ARG, "reserve: max_batch %d (1 .. 4096)", o.max_batch);
  if (o.max_samples <= 0 && o.max_frames <= 0) return fail(QASR_ERR_ARG, "reserve: max_samples and max_frames are both 0: nothing to reserve");
  if (o.max_samples > 0 && o.max_samples <= 256) return fail(QASR_ERR_ARG, "reserve: max_samples %d (the front-end needs more than 256 samples)", o.max_samples);
  const int pad_to = o.pad_to ? o.pad_to : 16, max_graphs = o.max_graphs ? o.max_graphs : 16;
  if (max_graphs < 1 || max_graphs > 64) return fail(QASR_ERR_ARG, "reserve: max_graphs %d (1 .. 64)", o.max_graphs);
  if (o.decode < 0 || o.decode > 2) return fail(QASR_ERR_ARG, "reserve: decode %d (0, 1 or 2)", o.decode);
  const int M = qasr_ragged_envelope_frames(std::max(o.max_samples, 0), std::max(o.max_frames, 0), pad_to);
  if (M < 0) return fail(QASR_ERR_ARG, "reserve: pad_to %d must divide %d; max_samples / max_frames out of range", pad_to, QASR_RAGGED_TILE);
  if (!e) return fail(QASR_ERR_ARG, "reserve: engine is NULL");
  if (e->debug || e->timing) return fail(QASR_ERR_ARG, "reserve: debug / timing engines keep per-shape hook buffers and cannot be reserved");
  if (e->rs.on) return fail(QASR_ERR_ARG, "reserve: this engine is reserved already");
  if (e->h.n_domains > QASR_SHAPE_MAXDOM) return fail(QASR_ERR_UNSUPPORTED, "reserve: %u time domains (the shape block holds %d)", e->h.n_domains, QASR_SHAPE_MAXDOM);
  const int ls = logsoftmax_op(e);
  if (ls < 0) return fail(QASR_ERR_ARG, "reserve: the model has no LOGSOFTMAX op (no CTC decoder)");
  HIPCHK(hipSetDevice(e->device));
  if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
  e->gexec = nullptr;
  e->gkey[0] = nullptr;
  free_plan(e);
  int rc = plan_shape(e, o.max_batch, M);
  if (!rc) rc = plan_alloc(e);
  if (rc) {
    free_plan(e);
    return rc;
  }
  auto& r = e->rs;
  r.max_batch = o.max_batch;
  r.max_samples = std::max(o.max_samples, 0);
  r.max_frames = M;
  r.n_mels = o.n_mels > 0 ? o.n_mels : (int)e->h.feat_in;
  r.pad_to = pad_to;
  r.max_graphs = max_graphs;
  r.want_logp = o.want_logp != 0;
  r.decode = o.decode != 0;
  r.decode_use_lens = o.decode == 2 ? 0 : 1;
  r.spitch = rup(std::max(r.max_samples, 4), 4);
  r.out_frames = e->tens[e->ops[ls].in].T;
  const int ncls = (int)e->ops[ls].cin;
  const size_t Bm = (size_t)o.max_batch, rows = Bm * (size_t)r.out_frames;
  bool ok = true;
  auto take = [&](auto** p, size_t bytes) {
    void* q = nullptr;
    if (!ok || dev_alloc(e, &q, bytes) != hipSuccess || hipMemset(q, 0, bytes) != hipSuccess) {
      ok = false;
      if (q) r.owned.push_back(q);
      return;
    }
    r.owned.push_back(q);
    *p = reinterpret_cast<std::remove_reference_t<decltype(*p)>>(q);
  };
  take(&r.shp, sizeof(int32_t) * QASR_SHAPE_WORDS);
  if (r.max_samples > 0) {
    take(&r.audio, sizeof(float) * Bm * r.spitch);
    take(&r.audio_lens, sizeof(int32_t) * Bm);
    const size_t need = Bm * (size_t)(M / QASR_MEL_TILE) * r.n_mels * 2 * sizeof(double);   // k_mel's per-tile statistics
    if (ok && dev_alloc(e, (void**)&e->norm_stats, need) == hipSuccess) e->norm_stats_bytes = need;
    else ok = false;
  }
  take(&r.feats, sizeof(float) * Bm * std::max(r.n_mels, (int)e->h.feat_in) * M);
  take(&r.feat_lens, sizeof(int32_t) * Bm);
  take(&r.tokens, sizeof(int32_t) * rows);
  take(&r.lens_out, sizeof(int32_t) * Bm);
  if (r.want_logp) take(&r.logp, sizeof(float) * rows * ncls);
  r.ctc = qasr_ctc_out{};
  if (r.decode) {
    r.ctc.struct_size = (uint32_t)sizeof(qasr_ctc_out);
    take(&r.fs, sizeof(float) * rows);
    take(&r.ctc.labels, sizeof(int32_t) * rows);
    take(&r.ctc.n_labels, sizeof(int32_t) * Bm);
    take(&r.ctc.start, sizeof(int32_t) * rows);
    take(&r.ctc.nframes, sizeof(int32_t) * rows);
    take(&r.ctc.score, sizeof(float) * rows);
    take(&r.ctc.utt_score, sizeof(float) * Bm);
  }
  if (!ok || hipDeviceSynchronize() != hipSuccess) {
    for (void* p : r.owned) dev_free(e, p);
    r = qasr_engine::Reserved{};
    free_plan(e);
    return fail(QASR_ERR_HIP, "reserve: allocation for %d x %d frames failed", o.max_batch, M);
  }
  r.buckets.reserve((size_t)max_graphs);
  r.on = true;
  return QASR_OK;
}

// one ragged forward: fe == nullptr: `src` = features [B][feat_in][X]; else audio [B][X] samples
static int ragged_impl(qasr_engine* e, hipStream_t s, const FrontArgs* fe, const float* src, const int32_t* lens, int B, int X,
                       qasr_ragged_out* out) {
  const char* who = fe ? "forward_ragged_audio" : "forward_ragged";
  if (!e || !src || !lens || !out || B <= 0 || X <= 0) return fail(QASR_ERR_ARG, "%s: bad arguments", who);
  if (out->struct_size != sizeof(qasr_ragged_out)) return fail(QASR_ERR_ARG, "%s: qasr_ragged_out.struct_size %u is not %zu", who, out->struct_size, sizeof(qasr_ragged_out));
  auto& r = e->rs;
  if (!r.on) return fail(QASR_ERR_ARG, "%s: call qasr_engine_reserve first", who);
  if (B > r.max_batch) return fail(QASR_ERR_ARG, "%s: batch %d is outside the reserved envelope (max_batch %d)", who, B, r.max_batch);
  if (fe) {
    if (!r.audio) return fail(QASR_ERR_ARG, "%s: the engine was reserved without max_samples", who);
    if (X > r.max_samples) return fail(QASR_ERR_ARG, "%s: %d samples are outside the reserved envelope (max_samples %d)", who, X, r.max_samples);
    if (X <= 256) return fail(QASR_ERR_ARG, "%s: %d samples (the front-end needs more than 256)", who, X);
    if (fe->n_mels != r.n_mels || fe->pad_to != r.pad_to)
      return fail(QASR_ERR_ARG, "%s: n_mels %d / pad_to %d differ from the reservation (%d / %d)", who, fe->n_mels, fe->pad_to, r.n_mels, r.pad_to);
  }
  const int T = fe ? qasr_frontend_frames(X, r.pad_to) : X;
  if (T > r.max_frames) return fail(QASR_ERR_ARG, "%s: %d frames are outside the reserved envelope (max_frames %d)", who, T, r.max_frames);
  const auto& h = e->h;
  RaggedStageP sp{};
  sp.shape[QASR_SHAPE_B] = B;
  sp.shape[QASR_SHAPE_S] = fe ? X : 0;
  sp.shape[QASR_SHAPE_NF] = fe ? 1 + X / 160 : T;
  sp.shape[QASR_SHAPE_DOM] = T;
  for (uint32_t d = 1; d < h.n_domains; ++d)
    sp.shape[QASR_SHAPE_DOM + d] = conv_out_len(sp.shape[QASR_SHAPE_DOM + e->doms[d].parent], e->doms[d]);
  for (uint32_t d = 0; d < h.n_domains; ++d)
    if (sp.shape[QASR_SHAPE_DOM + d] <= 0) return fail(QASR_ERR_ARG, "input of %d frames is too short for domain %u", T, d);
  const int Tb = ragged_bucket(r.max_frames, r.max_graphs, T);
  if (Tb < T) return fail(QASR_ERR_ARG, "%s: no bucket for %d frames", who, T);
  qasr_engine::Bucket* bk = nullptr;
  for (auto& q : r.buckets)
    if (q.frames == Tb) bk = &q;
  if (!bk) {
    r.buckets.emplace_back();
    bk = &r.buckets.back();
    bk->frames = Tb;
  }
  HIPCHK(hipSetDevice(e->device));
  if (e->T0 != Tb || e->B != r.max_batch) {                  // launch parameters of the bucket: host arithmetic only
    int rc = plan_shape(e, r.max_batch, Tb);
    if (rc) return rc;
  }
  const int ls = logsoftmax_op(e);
  const TensorRT& tl = e->tens[e->ops[ls].in];
  e->tens[0].ptr = (void*)r.feats;
  e->cur_lens = r.feat_lens;
  e->stem = e->fuse_stem && stem_shape(e);
  const bool norm_in_stem = fe && e->stem && e->fuse_norm && fe->n_mels == (int)h.feat_in;
  e->norm_tiles = e->norm_frames = 0;
  e->fe_launches = fe ? (norm_in_stem ? 1 : 2) : 0;
  if (norm_in_stem) {                                        // the grid covers the bucket; tiles beyond the batch's frames hold zeros
    e->norm_frames = Tb;
    e->norm_tiles = Tb / QASR_MEL_TILE;
  }
  // ---- the one eager launch: input + lengths into staging, shape block
  sp.src = src;
  sp.lens_in = lens;
  sp.shp = r.shp;
  sp.B = B;
  sp.max_batch = r.max_batch;
  if (fe) {
    sp.dst = r.audio, sp.lens_out = r.audio_lens;
    sp.row = X, sp.src_pitch = X, sp.dst_pitch = r.spitch, sp.n_rows = 1;
  } else {
    sp.dst = r.feats, sp.lens_out = r.feat_lens;
    sp.row = T, sp.src_pitch = T, sp.dst_pitch = Tb, sp.n_rows = (int)h.feat_in;
  }
  {
    int rc = launch_ragged_stage(s, sp);
    if (rc) return fail(rc, "%s: k_ragged_stage launch", who);
  }
  // ---- everything else runs on the engine's own buffers: the bucket's graph
  RaggedFront rg{r.spitch, Tb, r.shp};
  FrontArgs f2{};
  if (fe) {
    f2 = *fe;
    f2.audio = r.audio, f2.audio_lens = r.audio_lens, f2.S = X, f2.rg = &rg;
  }
  struct CtcSwap {                                           // the reservation's own CTC outputs for the duration of the call
    qasr_engine* e;
    float* fs; qasr_ctc_out out; bool on; int use_lens;
    ~CtcSwap() { e->ctc_fs = fs, e->ctc_out = out, e->ctc_on = on, e->ctc_use_lens = use_lens, e->ctc_t_act = nullptr; }
  } swap{e, e->ctc_fs, e->ctc_out, e->ctc_on, e->ctc_use_lens};
  e->ctc_fs = r.decode ? r.fs : nullptr;
  e->ctc_out = r.ctc;
  e->ctc_on = r.decode;
  e->ctc_use_lens = r.decode ? r.decode_use_lens : 0;
  e->ctc_t_act = r.shp + QASR_SHAPE_DOM + tl.d.domain;
  auto enqueue = [&]() -> int {
    return enqueue_forward(e, s, fe ? &f2 : nullptr, norm_in_stem, r.feats, r.feat_lens, r.logp, r.tokens, r.lens_out);
  };
  out->out_frames = sp.shape[QASR_SHAPE_DOM + tl.d.domain];
  out->bucket_frames = Tb;
  out->row_pitch = tl.T;
  out->n_classes = (int)e->ops[ls].cin;
  out->tokens = r.tokens, out->lens_out = r.lens_out, out->logp = r.logp, out->frame_score = r.fs, out->ctc = r.ctc;
  out->feats = r.feats, out->feat_lens = r.feat_lens;
  e->forwarded = true;
  uint64_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (fe) {
    uint32_t pre_bits;
    memcpy(&pre_bits, &fe->preemph, 4);
    key[0] = 1, key[1] = (uint64_t)(uintptr_t)fe->fb, key[2] = (uint64_t)(uintptr_t)fe->window, key[3] = (uint64_t)(uintptr_t)fe->plan;
    key[4] = pre_bits, key[5] = (uint64_t)fe->plan_bytes;
  }
  if (memcmp(key, bk->key, sizeof key)) {                    // another entry / filterbank: this bucket starts over
    if (bk->gexec) (void)hipGraphExecDestroy(bk->gexec);
    bk->gexec = nullptr;
    bk->calls = 0;
    memcpy(bk->key, key, sizeof key);
  }
  const uint64_t seen = bk->calls++;
  if (bk->gexec) {
    HIPCHK(hipGraphLaunch(bk->gexec, s));
    r.replays++;
    return QASR_OK;
  }
  if (seen >= 1 && s != nullptr) {                           // second visit: capture (the first ran every kernel's one-time setup)
    if (g_prof) return fail(QASR_ERR_ARG, "graph capture while qasr_debug_prof / qasr_debug_timeline is set: the buffer would be baked into the graph");
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = enqueue();
    hipError_t ce = hipStreamEndCapture(s, &g);
    if (rc) {
      if (g) (void)hipGraphDestroy(g);
      bk->calls = 0;
      return rc;
    }
    if (ce != hipSuccess || !g) return fail(QASR_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
    hipError_t ie = hipGraphInstantiate(&bk->gexec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) {
      bk->gexec = nullptr;
      return fail(QASR_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
    }
    r.captured++;
    HIPCHK(hipGraphLaunch(bk->gexec, s));
    r.replays++;
    return QASR_OK;
  }
  int rc = enqueue();
  if (rc) return rc;
  r.eager++;
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

int qasr_engine_forward_ragged(qasr_engine* e, void* stream, const float* feats, const int32_t* lens, int B, int T,
                               qasr_ragged_out* out) {
  return ragged_impl(e, (hipStream_t)stream, nullptr, feats, lens, B, T, out);
}

int qasr_engine_forward_ragged_audio(qasr_engine* e, void* stream, const float* audio, const int32_t* audio_lens, int B, int S,
                                     const float* fb, const float* window, int n_mels, float preemph, int pad_to,
                                     const void* frontend_plan, size_t plan_bytes, qasr_ragged_out* out) {
  if (!fb || !window || !frontend_plan) return fail(QASR_ERR_ARG, "forward_ragged_audio: bad arguments");
  FrontArgs fe{audio, audio_lens, S, fb, window, n_mels, preemph, pad_to, frontend_plan, plan_bytes, nullptr};
  return ragged_impl(e, (hipStream_t)stream, &fe, audio, audio_lens, B, S, out);
}

int qasr_engine_ragged_stats(const qasr_engine* e, qasr_ragged_stats* out) {
  if (!e || !out) return fail(QASR_ERR_ARG, "ragged_stats: NULL argument");
  if (out->struct_size != sizeof(qasr_ragged_stats)) return fail(QASR_ERR_ARG, "ragged_stats: qasr_ragged_stats.struct_size %u is not %zu", out->struct_size, sizeof(qasr_ragged_stats));
  memset(out, 0, sizeof *out);
  out->struct_size = (uint32_t)sizeof *out;
  out->device_allocs = e->n_allocs;
  out->device_frees = e->n_frees;
  out->graphs_captured = e->rs.captured;
  out->graph_replays = e->rs.replays;
  out->eager_runs = e->rs.eager;
  for (const auto& b : e->rs.buckets) {
    if (out->n_buckets >= 64) break;
    out->bucket_frames[out->n_buckets] = b.frames;
    out->bucket_calls[out->n_buckets] = b.calls;
    out->n_buckets++;
  }
  return QASR_OK;
}

// Replays every op `reps` times back to back between ONE pair of HIP events on `stream` and returns the
// average duration per launch (ms).  The buffers hold the activations of the last forward, so operands are
// real data; each op reads its inputs and rewrites its own outputs, which makes the replay idempotent.
int qasr_engine_time_ops(qasr_engine* e, void* stream, int reps, float* ms_per_launch, int n_ops) {
  if (!e || !e->B || reps <= 0 || n_ops != (int)e->h.n_ops || !ms_per_launch) return fail(QASR_ERR_ARG, "time_ops: run a forward first");
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  for (uint32_t oi = 0; oi < e->h.n_ops; ++oi) {
    int rc = launch_op(e, s, oi, nullptr, e->time_tokens, nullptr);      // warm
    if (rc) return rc;
    HIPCHK(hipEventRecord(a, s));
    for (int r = 0; r < reps; ++r) launch_op(e, s, oi, nullptr, e->time_tokens, nullptr);
    HIPCHK(hipEventRecord(b, s));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    ms_per_launch[oi] = ms / reps;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return QASR_OK;
}

int qasr_engine_op_label(qasr_engine* e, int op, char* buf, size_t cap) {
  if (!e || !buf || cap < 8 || op < 0 || op >= (int)e->h.n_ops) return fail(QASR_ERR_ARG, "op_label: bad argument");
  const qasr_op_desc& d = e->ops[op];
  const char* name = "?";
  if (e->skip[op]) name = "(fused into the next op)";
  else if (e->dec_skip[op]) name = "(fused into the previous op)";
  else if (e->rq_skip[op]) name = "(served by the previous k_requant launch)";
  else if (e->stem && op <= 2) name = op == 0 ? "k_stem" : "(fused into the first op)";
  else switch (d.kind) {
    case QASR_OP_QUANT_IN: name = "k_quant_in"; break;
    case QASR_OP_DW: name = "k_dw"; break;
    case QASR_OP_DENSE:
      if (d.flags & QASR_F_TAPMAJOR) {
        SepP p{};
        build_sep(e, (uint32_t)op, p);
        sep_kernel_label(p, buf, cap);
        return QASR_OK;
      }
      name = "k_dense";
      break;
    case QASR_OP_LOGSOFTMAX: name = "k_logsoftmax"; break;
    case QASR_OP_REQUANT: name = "k_requant"; break;
    case QASR_OP_PW:
      {
        SepP p{};
        build_sep(e, (uint32_t)op, p);
        if (e->fuse_dec && (d.flags & QASR_F_LOGITS) && op + 1 < (int)e->h.n_ops && e->dec_skip[op + 1]) {
          name = e->dec_wide[op] ? "k_decw" : "k_dec";
          break;
        }
        sep_kernel_label(p, buf, cap);
        return QASR_OK;
      }
    default: break;
  }
  snprintf(buf, cap, "%s", name);
  return QASR_OK;
}

int qasr_engine_op_paired(const qasr_engine* e, int op) {
  if (!e || op < 0 || op >= (int)e->h.n_ops) return -1;
  return (!e->paired.empty() && e->paired[op]) ? 1 : 0;
}

int qasr_engine_op_halved(const qasr_engine* e, int op) {
  if (!e || op < 0 || op >= (int)e->h.n_ops) return -1;
  return (!e->halved.empty() && e->halved[op]) ? 1 : 0;
}

int qasr_engine_pair_timeouts(qasr_engine* e) {
  if (!e) return -1;
  if (!e->pair_tmo) return 0;
  unsigned v = 0;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&v, e->pair_tmo, sizeof v, hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemset(e->pair_tmo, 0, sizeof v));
  return (int)std::min(v, 0x7fffffffu);
}

int qasr_engine_pair_flag_words(const qasr_engine* e, uint32_t* out, size_t n) {
  if (!e) return -1;
  const size_t have = e->pair_flags ? e->pair_flag_bytes / sizeof(uint32_t) : 0;
  if (!out || n == 0 || have == 0) return (int)std::min(have, (size_t)0x7fffffff);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, e->pair_flags, std::min(n, have) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return (int)std::min(have, (size_t)0x7fffffff);
}

size_t qasr_sep_pair_workspace_bytes(int B, int Tp) {
  if (B < 1 || Tp < 128 || Tp % 128) return 0;
  return sep_pair_flag_bytes(B, Tp) + 256 + sep_pair_x_bytes(B, Tp);
}
size_t qasr_sep_pair_timeout_offset(int B, int Tp) { return (B < 1 || Tp < 128 || Tp % 128) ? 0 : sep_pair_flag_bytes(B, Tp); }

int qasr_engine_run_op(qasr_engine* e, void* stream, int op) {
  if (!e || !e->B || op < 0 || op >= (int)e->h.n_ops) return fail(QASR_ERR_ARG, "run_op: run a forward first");
  return launch_op(e, (hipStream_t)stream, (uint32_t)op, nullptr, e->time_tokens, nullptr);
}

int qasr_engine_read_acc(qasr_engine* e, int op, int pane, int32_t* host_out, size_t n_elems) {
  if (!e || !e->debug || op < 0 || op >= (int)e->h.n_ops || e->acc_dbg.empty()) return fail(QASR_ERR_ARG, "read_acc: not a debug engine / bad op");
  const auto& v = e->acc_dbg[op];
  int k = pane < 0 ? 0 : 1 + pane;
  if (k >= (int)v.size()) return fail(QASR_ERR_ARG, "read_acc: op %d has no accumulator %d", op, k);
  const qasr_op_desc& d = e->ops[op];
  const TensorRT& o = e->tens[d.outs[0].tensor];
  size_t n = (size_t)e->B * d.cout * rup(o.T, 64);
  if (n_elems != n) return fail(QASR_ERR_ARG, "read_acc: expected %zu elements", n);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, v[k], n * 4, hipMemcpyDeviceToHost));
  return QASR_OK;
}

int qasr_engine_read_tensor(qasr_engine* e, int tensor, void* host_out, size_t n_bytes, int* T_out, int* Tp_out) {
  if (!e || tensor <= 0 || tensor >= (int)e->tens.size()) return fail(QASR_ERR_ARG, "read_tensor: bad tensor / no forward yet");
  const TensorRT& t = e->tens[tensor];
  {                                                          // a tensor the launch plan never stores has no bytes to serve
    const int pr = t.d.producer;
    const bool in_launch = pr >= 0 && pr < (int)e->skip.size() && e->skip[pr];           // depthwise output inside the fused layer's launch
    const bool in_stem = e->stem && pr >= 0 && pr <= 1;                                    // k_stem's intermediates
    const bool in_dec = !e->debug && pr >= 0 && pr + 1 < (int)e->dec_skip.size() && e->dec_skip[pr + 1] &&
                        (e->ops[pr].flags & QASR_F_LOGITS);                                // float logits inside k_dec / k_decw
    if (in_launch || in_stem || in_dec || !t.ptr)
      return fail(QASR_ERR_ARG, "read_tensor: tensor %d is never materialised by this plan (its producer, op %d, runs fused inside another launch)", tensor, pr);
  }
  if (!e->debug) {                                           // production engines reuse arena slots: only a tensor nobody overwrote
    for (size_t i = 1; i < e->tens.size(); ++i)
      if ((int)i != tensor && e->tens[i].slot == t.slot && e->tens[i].d.producer > t.d.producer)
        return fail(QASR_ERR_ARG, "read_tensor: the arena slot of tensor %d was reused by tensor %zu (debug engines keep every tensor)", tensor, i);
  }
  if (T_out) *T_out = t.T;
  if (Tp_out) *Tp_out = t.Tp;
  size_t want = (t.d.dtype == QASR_DT_F32) ? (size_t)e->B * t.T * t.d.channels * 4 : (size_t)e->B * t.d.channels * t.Tp * dt_size(t.d.dtype);
  if (!host_out) return QASR_OK;
  if (n_bytes != want) return fail(QASR_ERR_ARG, "read_tensor: expected %zu bytes", want);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, t.ptr, want, hipMemcpyDeviceToHost));
  return QASR_OK;
}

int qasr_engine_last_op_ms(qasr_engine* e, float* ms, int n_ops) {
  if (!e || !e->timing || !e->timed || n_ops != (int)e->h.n_ops) return fail(QASR_ERR_ARG, "last_op_ms: no timed forward");
  HIPCHK(hipEventSynchronize(e->ev[n_ops]));
  for (int i = 0; i < n_ops; ++i) HIPCHK(hipEventElapsedTime(&ms[i], e->ev[i], e->ev[i + 1]));
  return QASR_OK;
}

// ---------------------------------------------------------------------------------- stand-alone operators
static void* g_zero = nullptr;
static const size_t kZeroBytes = 1 << 20;
static int zero_buf(void** p) {
  if (!g_zero) {
    HIPCHK(hipMalloc(&g_zero, kZeroBytes));
    HIPCHK(hipMemset(g_zero, 0, kZeroBytes));
  }
  *p = g_zero;
  return QASR_OK;
}

int qasr_pw_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias, int B,
                     int cin, int cin_pad, int cout, int T, int Tp, int32_t* acc) {
  if (!x || !w || !acc || cin_pad % 128 || Tp % 64 || T > Tp) return fail(QASR_ERR_ARG, "pw_conv_acc: bad arguments");
  void* z;
  int rc = zero_buf(&z);
  if (rc) return rc;
  if ((size_t)rup(cout, 128) * 8 > kZeroBytes) return fail(QASR_ERR_ARG, "cout too large");
  SepP p{};                            // the production 1x1 kernel (k_sep<0>) with no consumers: accumulators only
  p.x = x;
  p.w = w;
  p.bias = bias ? bias : (const int32_t*)z;
  p.cin = cin;
  p.cin_pad = cin_pad;
  p.pw_unsigned = x_unsigned;
  p.K = 0;
  p.dilation = 1;
  p.e.sb = (const float*)z;
  p.e.acc_dbg = acc;
  p.e.T = T;
  p.e.Tp = Tp;
  p.e.cout = cout;
  p.e.B = B;
  p.e.lens = (const int32_t*)z;
  int lrc = launch_sep((hipStream_t)stream, p);
  if (lrc) return fail(lrc, "pw_conv_acc: launch rejected");
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

int qasr_dw_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias, int B, int c,
                     int kernel, int kpad, int stride, int dilation, int padding, int T, int Tp, int T_out, int Tp_out,
                     int32_t* acc) {
  if (!x || !w || !acc || kpad % 4 || kpad < kernel || Tp % 64 || Tp_out % 64) return fail(QASR_ERR_ARG, "dw_conv_acc: bad arguments");
  void* z;
  int rc = zero_buf(&z);
  if (rc) return rc;
  DwP p{};
  p.x = x;
  p.w = w;
  p.bias = bias ? bias : (const int32_t*)z;   // u8 data: the caller's bias carries 128 * sum(w)
  p.C = c;
  p.K = kernel;
  p.kpad = kpad;
  p.stride = stride;
  p.dilation = dilation;
  p.padding = padding;
  p.T_in = T;
  p.Tp_in = Tp;
  p.x_unsigned = x_unsigned;
  p.e.sb = (const float*)z;
  p.e.acc_dbg = acc;
  p.e.T = T_out;
  p.e.Tp = Tp_out;
  p.e.cout = c;
  p.e.B = B;
  p.e.lens = (const int32_t*)z;
  launch_dw((hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

int qasr_dense_conv_acc(void* stream, const int8_t* x, int x_unsigned, const int8_t* w, const int32_t* bias, int B, int cin,
                        int cin_pad, int cout, int kernel, int stride, int dilation, int padding, int T, int Tp, int T_out,
                        int Tp_out, int32_t* acc) {
  if (!x || !w || !acc || cin_pad % 128 || cin > cin_pad || Tp % 64 || Tp_out % 64 || T > Tp || T_out > Tp_out || kernel < 1 ||
      stride < 1 || dilation < 1 || B < 1 || cout < 1)
    return fail(QASR_ERR_ARG, "dense_conv_acc: bad arguments");
  void* z;
  int rc = zero_buf(&z);
  if (rc) return rc;
  if ((size_t)rup(cout, 128) * 8 > kZeroBytes) return fail(QASR_ERR_ARG, "cout too large");
  DenseP p{};                          // the generic dense conv kernel (k_dense) with no consumers: accumulators only
  p.x = x;
  p.w = w;
  p.bias = bias ? bias : (const int32_t*)z;
  p.cin = cin;
  p.cin_pad = cin_pad;
  p.K = kernel;
  p.stride = stride;
  p.dilation = dilation;
  p.padding = padding;
  p.T_in = T;
  p.Tp_in = Tp;
  p.x_unsigned = x_unsigned;
  p.e.sb = (const float*)z;
  p.e.acc_dbg = acc;
  p.e.T = T_out;
  p.e.Tp = Tp_out;
  p.e.cout = cout;
  p.e.B = B;
  p.e.lens = (const int32_t*)z;
  launch_dense((hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

int qasr_sep_layer(void* stream, const qasr_sep_layer_args* a, char* label, size_t label_cap) {
  if (!a || !a->x || !a->w || !a->bias || !a->lens || a->B < 1 || a->cin < 1 || a->cout < 1 || a->Tp % 64 || a->T > a->Tp ||
      a->n_outs < 0 || a->n_outs > QASR_MAX_OUTS || (a->tile != 32 && a->tile != 64 && a->tile != 128))
    return fail(QASR_ERR_ARG, "sep_layer: bad arguments");
  SepP p{};
  p.x = a->x;
  p.wdw = a->wdw;
  p.wdw2 = a->wdw2;
  p.bias_dw = a->bias_dw;
  p.m_dw = a->m_dw;
  p.dw_acc_dbg = a->dw_acc;
  p.dw_lo = a->dw_lo;
  p.dw_hi = a->dw_hi;
  p.K = a->K;
  p.x_unsigned = a->K > 0 ? a->x_unsigned : 0;
  p.pw_unsigned = a->K > 0 ? 0 : a->x_unsigned;
  p.dilation = a->K > 0 ? a->dilation : 1;
  p.tile = a->tile;
  p.gen = a->gen == 3 ? 2 : a->gen;
  p.mask_skip = a->gen == 3;
  p.pair = a->pair != 0;
  p.w = a->w;
  p.bias = a->bias;
  p.cin = a->cin;
  p.cin_pad = rup(a->cin, 128);
  if (a->flags & QASR_F_RESADD) {
    if (!a->rx || !a->rw || !a->rbias || !a->rm || !a->m_main || a->rcin < 1) return fail(QASR_ERR_ARG, "sep_layer: residual operands missing");
    p.n_panes = 1;
    PaneP& d = p.panes[0];
    d.x = a->rx;
    d.w = a->rw;
    d.bias = a->rbias;
    d.m = a->rm;
    d.sb = a->rsb;
    d.acc_dbg = a->racc;
    d.cin = a->rcin;
    d.cin_pad = rup(a->rcin, 128);
    d.x_unsigned = a->r_unsigned;
  }
  EpiP& e = p.e;
  e.n_outs = a->n_outs;
  for (int j = 0; j < a->n_outs; ++j) {
    e.outs[j].ptr = a->outs[j].ptr;
    e.outs[j].mtab = a->outs[j].mtab;
    e.outs[j].m = a->outs[j].m;
    e.outs[j].lo = a->outs[j].lo;
    e.outs[j].hi = a->outs[j].hi;
    e.outs[j].mode = a->outs[j].mode;
    if (!a->outs[j].ptr || (a->outs[j].mode == 1 && !a->outs[j].mtab)) return fail(QASR_ERR_ARG, "sep_layer: consumer %d incomplete", j);
  }
  e.flags = a->flags & (QASR_F_RELU | QASR_F_MASK_OUT | QASR_F_EXACT_Z | QASR_F_RESADD);
  if ((e.flags & QASR_F_EXACT_Z) && !a->sb) return fail(QASR_ERR_ARG, "sep_layer: EXACT_Z needs the conv output scales");
  e.sb = a->sb;
  e.m_main = a->m_main;
  e.lens = a->lens;
  e.acc_dbg = a->acc;
  e.qlo = a->qlo;
  e.qhi = a->qhi;
  e.T = a->T;
  e.Tp = a->Tp;
  e.cout = a->cout;
  e.B = a->B;
  if (p.pair) {
    // hooks are debug instantiations; everything but k_sep2<51 | 63 | 75, 4, 0, 2, false, 128, 1> has no paired form
    if (a->dw_acc || a->acc || a->racc || !sep_pair_ok(p)) return fail(QASR_ERR_UNSUPPORTED, "sep_layer: no paired form for this shape / with hooks");
    const size_t fb = sep_pair_flag_bytes(e.B, e.Tp);
    if (!a->pair_ws || ((uintptr_t)a->pair_ws & 255) || a->pair_ws_bytes < qasr_sep_pair_workspace_bytes(e.B, e.Tp))
      return fail(QASR_ERR_ARG, "sep_layer: pair_ws (256-byte aligned, qasr_sep_pair_workspace_bytes)");
    p.pair_flags = (unsigned*)a->pair_ws;
    if (launch_pair_zero((hipStream_t)stream, p.pair_flags, fb)) return fail(QASR_ERR_ARG, "sep_layer: k_pair_zero");   // flag words: zero before every launch
  }
  if (label && label_cap >= 8) sep_kernel_label(p, label, label_cap);
  int rc = launch_sep((hipStream_t)stream, p);
  if (rc) return fail(rc, "sep_layer: no kernel instantiation for K=%d dilation=%d (or bad launch shape)", p.K, p.dilation);
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

int qasr_requant(void* stream, const int32_t* acc, const double* m, const float* sb, int exact_z, int relu, int B, int c,
                 int Tp, int lo, int hi, int8_t* out) {
  if (!acc || !m || !out || (exact_z && !sb)) return fail(QASR_ERR_ARG, "requant: bad arguments");
  RequantP p{};
  p.in = acc;
  p.in_is_i32 = 1;
  p.n_outs = 1;
  p.outs[0].ptr = out;
  p.outs[0].mtab = m;
  p.outs[0].lo = lo;
  p.outs[0].hi = hi;
  p.outs[0].mode = 1;
  p.sb = sb;
  p.flags = (exact_z ? QASR_F_EXACT_Z : 0) | (relu ? QASR_F_RELU : 0);
  p.C = c;
  p.T = Tp;
  p.Tp = Tp;
  p.B = B;
  launch_requant((hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return QASR_OK;
}

}  // extern "C"
