// Fused CTC decoder for wide vocabularies (32 < classes <= 8192, e.g. QuartzNet15x5Base-Zh: 5206 labels + blank):
// ConvASRDecoder.forward (conv_asr.py:270-275) - the 1x1 QuantConv1d with bias, its float view - then log_softmax and
// the greedy argmax of EncDecCTCModel.forward (ctc_models.py:405), in two launches.  k_dec's design (one 32 x 32 output
// tile per work-group, one lane per frame walking every class) does not stretch to thousands of classes, and the generic
// path (k_sep logits in HBM + k_logsoftmax, one lane per frame walking 5207 classes three times) is what this replaces.
//
//   k_decw_stats  grid (G class groups, B * Tp / 64 frame tiles); the class group is the fastest grid index, so with
//                 G = 8 every XCD walks one eighth of the weight matrix and keeps it in its own L2.  Work-group = 4 waves
//                 x one utterance x 64 frames.  The int8 tile [cin][64 frames] is staged once in LDS as two [channel][32
//                 frame] images (k_sep2's layout, A fragments through ds_read_b64_tr_b8); each wave walks the 32-class
//                 tiles g_lo + wave, g_lo + wave + 4, ... of its group with v_mfma_i32_32x32x32_i8 over the full K, forms
//                 z = fl32(fl32(acc + bias) * s_b[c]) exactly as k_dec / the generic epilogue do, and folds every z into a
//                 per-lane running (max, first argmax, sum exp(z - max)) of its frames (online rescaling).  The 128 lane
//                 partials of a frame are combined through LDS in a fixed order, and one partial per (frame, group) goes to
//                 the plan's workspace.
//   k_decw_out    combines the G partials of a frame in group order (equal maxima: the lower class wins, torch.argmax's
//                 first maximum), writes tokens and lengths; with log-probs requested it recomputes its group's z (same
//                 grid as the stats pass) and stores logp = (z - M) - log S.  Tokens only: one work-group per frame tile,
//                 no GEMM.
// z is bit-identical to the generic path's logits, so tokens are too; log S is summed in another order than
// k_logsoftmax's sequential walk (rounding-level differences in the log-probs).
#include <cmath>

#include "qasr_sep2_impl.h"

namespace qasr {

#define DECW_NT 256
#define DECW_FT 64                       /* frames per work-group: two 32-frame MFMA tiles */
#define DECW_MT (DECW_FT / 32)
#define DECW_G 8                         /* class groups (one per XCD) */

struct DecwP {
  const int8_t* x;          // [B][cin][Tp] codes of the decoder's QuantAct
  const int8_t* w;          // fragment-ordered [cout_pad128][cin_pad]
  const int32_t* bias;      // [cout_pad128] (+ 128 sum(W) for u8 codes)
  const float* sb;          // [cout_pad128] conv output scales
  const int32_t* lens;      // [B] encoded lengths (copied to lens_out)
  int32_t* lens_out;        // optional
  int32_t* acc_dbg;         // optional i32 [B][ncls][Tp]
  float* logits;            // optional f32 [B][T][ncls]
  float* logp;              // optional f32 [B][T][ncls]
  int32_t* tokens;          // optional i32 [B][T]
  float* frame_score;       // optional f32 [B][T]: log-prob of the frame's argmax class, the bits of logp[b][t][tokens[b][t]]
  float4* part;             // workspace [B][Tp][G] {max, sum exp, argmax (bits), 0}
  int cin, cin_pad, x_unsigned, B, T, Tp, ncls, G, n_ct;
};

struct Stat {
  float m, s;
  int a;
};
// fold value z of class c, classes arriving in increasing order
__device__ __forceinline__ void stat_add(Stat& st, float z, int c) {
  if (z > st.m) {
    st.s = st.s * __expf(st.m - z) + 1.f;
    st.m = z;
    st.a = c;
  } else {
    st.s += __expf(z - st.m);
  }
}
// st <- st (+) o; equal maxima keep the lower class; an empty partial (s == 0) changes nothing
__device__ __forceinline__ void stat_merge(Stat& st, const Stat& o) {
  if (o.s == 0.f) return;
  if (st.s == 0.f) { st = o; return; }
  const float M = fmaxf(st.m, o.m);
  st.s = st.s * __expf(st.m - M) + o.s * __expf(o.m - M);
  st.a = o.m > st.m ? o.a : (o.m < st.m ? st.a : min(st.a, o.a));
  st.m = M;
}

// the work-group's [cin][64] codes as two [channel][32 frame] images; rows >= cin are zero
__device__ __forceinline__ void decw_stage(const DecwP& p, lds_u8* Xd, int b, int t0) {
  const unsigned flip = p.x_unsigned ? 0x80808080u : 0u;                  // u8 codes are fed as x - 128 (bias carries 128 sum(W))
  const int ng = 4 * p.cin_pad;                                          // 16-byte granules: [channel][4 x 16 frames]
  for (int base = threadIdx.x; base < ng; base += 4 * DECW_NT) {
    v4i r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = min(base + u * DECW_NT, ng - 1), c = min(g >> 2, p.cin - 1);
      r[u] = *(const v4i*)(p.x + ((size_t)b * p.cin + c) * p.Tp + t0 + 16 * (g & 3));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = base + u * DECW_NT;
      if (g < ng) {
        const int c = g >> 2, q = g & 3;
        v4i v = r[u];
        v[0] ^= flip, v[1] ^= flip, v[2] ^= flip, v[3] ^= flip;
        if (c >= p.cin) v = (v4i){0, 0, 0, 0};
        *(lds_v4i*)(Xd + (q >> 1) * (p.cin_pad * 32) + c * 32 + 16 * (q & 1)) = v;
      }
    }
  }
}

// Walks this wave's class tiles of group g: acc = the 1x1 conv of the 64 frames, then epi(tile, acc) per tile.  Weight
// fragments are double-buffered in registers four K steps at a time, the next chunk (possibly the next tile's first)
// requested before the current one is multiplied.
template <class Epi>
__device__ __forceinline__ void decw_gemm(const DecwP& p, const lds_u8* Xd, int g, int wave, Epi&& epi) {
  const int lane = threadIdx.x & 63;
  const int lo = g * p.n_ct / p.G, hi = (g + 1) * p.n_ct / p.G;
  const int nkc = p.cin_pad >> 7;                                        // chunks of 4 K steps (cin_pad % 128 == 0)
  const lds_u8* const xd_lane = Xd + sep2_a_lane_off(lane);
  if (lo + wave >= hi) return;
  v4i wb[4], wn[4];
  {
    const v4i* wp = w_frag(p.w, p.cin_pad, 32 * (lo + wave), 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) wb[u] = wp[64 * u];                       // consecutive K steps are 1 KiB apart
  }
  for (int tile = lo + wave; tile < hi; tile += 4) {
    v16i acc[DECW_MT];
#pragma unroll
    for (int mt = 0; mt < DECW_MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][r] = 0;
    for (int kc = 0; kc < nkc; ++kc) {
      const int ntile = kc + 1 < nkc ? tile : tile + 4, nkc_ = kc + 1 < nkc ? kc + 1 : 0;
      if (ntile < hi) {
        const v4i* wp = w_frag(p.w, p.cin_pad, 32 * ntile, 4 * nkc_);
#pragma unroll
        for (int u = 0; u < 4; ++u) wn[u] = wp[64 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mt = 0; mt < DECW_MT; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(sep2_a_frag(xd_lane + mt * (p.cin_pad * 32), 4 * kc + u), wb[u], acc[mt], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) wb[u] = wn[u];
    }
    epi(tile, acc);
  }
}

__global__ void __launch_bounds__(DECW_NT) k_decw_stats(DecwP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x, tpu = p.Tp / DECW_FT, b = blockIdx.y / tpu, t0 = (blockIdx.y % tpu) * DECW_FT;
  lds_u8* const Xd = (lds_u8*)smem;
  decw_stage(p, Xd, b, t0);
  __syncthreads();
  Stat st[DECW_MT][16];
#pragma unroll
  for (int mt = 0; mt < DECW_MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[mt][r] = Stat{-INFINITY, 0.f, 0};
  decw_gemm(p, Xd, g, wave, [&](int tile, v16i (&acc)[DECW_MT]) {
    // C layout: lane & 31 = class, register r of half h = frame mfma32_row(r, h) of MFMA tile mt
    const int c = 32 * tile + (lane & 31);
    if (c >= p.ncls) return;
    const int bias = p.bias[c];
    const float sb = p.sb[c];
#pragma unroll
    for (int mt = 0; mt < DECW_MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int a = acc[mt][r] + bias;
        const float z = mul_f32_unfused((float)a, sb);                  // conv_int.float() * scale (quant_modules.py:305-308)
        stat_add(st[mt][r], z, c);
        if (p.acc_dbg || p.logits) {
          const int t = t0 + 32 * mt + mfma32_row(r, h);
          if (t < p.T) {
            if (p.acc_dbg) p.acc_dbg[((size_t)b * p.ncls + c) * p.Tp + t] = a;
            if (p.logits) p.logits[((size_t)b * p.T + t) * p.ncls + c] = z;
          }
        }
      }
  });
  __syncthreads();                                                       // the A images are dead: the LDS holds the partials now
  // ---- 128 lane partials per frame -> 1: wave by wave through LDS [32 lanes][64 frames], thread (q, f) folds lanes 8q..8q+7
  Stat* const lp = (Stat*)smem;
  const int f = tid & 63, q = tid >> 6;
  Stat mine{-INFINITY, 0.f, 0};
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int mt = 0; mt < DECW_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) lp[(lane & 31) * DECW_FT + 32 * mt + mfma32_row(r, h)] = st[mt][r];
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 8; ++l) stat_merge(mine, lp[(8 * q + l) * DECW_FT + f]);
    __syncthreads();
  }
  lp[q * DECW_FT + f] = mine;
  __syncthreads();
  if (tid < DECW_FT) {
    Stat s = lp[f];
#pragma unroll
    for (int k = 1; k < 4; ++k) stat_merge(s, lp[k * DECW_FT + f]);
    p.part[((size_t)b * p.Tp + t0 + f) * p.G + g] = make_float4(s.m, s.s, __int_as_float(s.a), 0.f);
  }
}

__global__ void __launch_bounds__(DECW_NT) k_decw_out(DecwP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x, tpu = p.Tp / DECW_FT, b = blockIdx.y / tpu, t0 = (blockIdx.y % tpu) * DECW_FT;
  float* const Mf = (float*)smem;                                         // [64] max, [64] log sum
  float* const Lf = Mf + DECW_FT;
  lds_u8* const Xd = (lds_u8*)(smem + 2 * DECW_FT * sizeof(float));
  if (p.logp) decw_stage(p, Xd, b, t0);
  if (tid < DECW_FT) {
    const float4* pp = p.part + ((size_t)b * p.Tp + t0 + tid) * p.G;
    Stat s{-INFINITY, 0.f, 0};
    for (int k = 0; k < p.G; ++k) {
      const float4 v = pp[k];
      stat_merge(s, Stat{v.x, v.y, __float_as_int(v.z)});
    }
    Mf[tid] = s.m;
    Lf[tid] = logf(s.s);
    const int t = t0 + tid;
    if (g == 0 && t < p.T && p.tokens) p.tokens[(size_t)b * p.T + t] = s.a;
    // z[argmax] == M bit for bit (the maximum is one of the z values): (z - M) - log S of that class
    if (g == 0 && t < p.T && p.frame_score) p.frame_score[(size_t)b * p.T + t] = 0.0f - Lf[tid];
  }
  if (g == 0 && t0 == 0 && tid == 0 && p.lens_out) p.lens_out[b] = p.lens[b];
  if (!p.logp) return;
  __syncthreads();
  decw_gemm(p, Xd, g, wave, [&](int tile, v16i (&acc)[DECW_MT]) {
    const int c = 32 * tile + (lane & 31);
    if (c >= p.ncls) return;
    const int bias = p.bias[c];
    const float sb = p.sb[c];
#pragma unroll
    for (int mt = 0; mt < DECW_MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int f = 32 * mt + mfma32_row(r, h), t = t0 + f;
        const float z = mul_f32_unfused((float)(acc[mt][r] + bias), sb);
        // one row of 32 consecutive classes per half-wave: 128-byte runs along the class axis
        if (t < p.T) p.logp[((size_t)b * p.T + t) * p.ncls + c] = (z - Mf[f]) - Lf[f];
      }
  });
}

static int decw_groups(int n_ct) { return std::min(DECW_G, n_ct); }

bool decoder_wide_fusable(const SepP& p) {
  return p.K == 0 && p.dense_k <= 1 && p.n_panes == 0 && (p.e.flags & QASR_F_LOGITS) && p.e.cout > 32 &&
         p.e.cout <= QASR_DECW_MAX_CLASSES && p.cin_pad % 128 == 0 && p.cin_pad <= 2048 && p.e.Tp % DECW_FT == 0;
}

size_t decoder_wide_ws_bytes(int B, int Tp) { return (size_t)B * Tp * DECW_G * sizeof(float4); }

int launch_decoder_wide(hipStream_t s, const SepP& q, float* logp, int32_t* tokens, int32_t* lens_out, bool keep_logits,
                        void* ws, size_t ws_bytes, float* frame_score) {
  if (!decoder_wide_fusable(q) || !q.x || !q.w || !q.bias || !q.e.sb || !q.e.lens || q.e.B < 1 || q.e.T > q.e.Tp || !ws ||
      ws_bytes < decoder_wide_ws_bytes(q.e.B, q.e.Tp))
    return QASR_ERR_ARG;
  DecwP p{};
  p.x = q.x, p.w = q.w, p.bias = q.bias, p.sb = q.e.sb, p.lens = q.e.lens, p.lens_out = lens_out;
  p.acc_dbg = q.e.acc_dbg;
  p.logits = keep_logits ? q.e.logits : nullptr;
  p.logp = logp, p.tokens = tokens, p.frame_score = frame_score;
  p.part = (float4*)ws;
  p.cin = q.cin, p.cin_pad = q.cin_pad, p.x_unsigned = q.pw_unsigned;
  p.B = q.e.B, p.T = q.e.T, p.Tp = q.e.Tp, p.ncls = q.e.cout;
  p.n_ct = (p.ncls + 31) / 32;
  p.G = decw_groups(p.n_ct);
  const size_t img = (size_t)DECW_FT * p.cin_pad;
  const size_t smem_stats = std::max(img, (size_t)32 * DECW_FT * sizeof(Stat));
  const size_t smem_out = 2 * DECW_FT * sizeof(float) + (logp ? img : 0);
  static int attr_dev = -1;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (attr_dev != dev) {
    (void)hipFuncSetAttribute((const void*)k_decw_stats, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)k_decw_out, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_dev = dev;
  }
  const int tiles = p.B * (p.Tp / DECW_FT);
  hipLaunchKernelGGL(k_decw_stats, dim3(p.G, tiles), dim3(DECW_NT), smem_stats, s, p);
  hipLaunchKernelGGL(k_decw_out, dim3(logp ? p.G : 1, tiles), dim3(DECW_NT), smem_out, s, p);
  return QASR_OK;
}

}  // namespace qasr
