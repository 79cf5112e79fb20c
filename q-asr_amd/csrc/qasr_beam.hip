// CTC prefix beam search in fixed point, without a language model (k_beam) and with one (k_beam_lm, at the end of the file);
// the host statement is qasr/beam.py, and this file follows it bit for bit: k_topn picks each frame's N best classes out of float32 log-probabilities, k_beam runs the
// search over those candidates.  Scores are int64 sums of q = rint(logp * 2^16); the only non-linear step is a look-up in
// the log-add-exp table the caller passes in (16384 x u16, LDS resident), so neither kernel calls exp or log and the
// results do not depend on thread order.
//
// k_topn: one wave (= one work-group) per frame.  Keys are the order-preserving integer image of the float bits (as k_ctc
// uses it).  An MSB-first radix select (4 passes of 8 bits, LDS histogram) finds the key of the N-th largest class and how
// many classes of exactly that key belong to the N; a compaction in class order collects them (lower id first among equal
// keys), and one rank-by-counting sort in the wave orders the <= 64 survivors.
//
// k_beam: one work-group per utterance, sequential over frames.  The beam (<= 128 entries: pb, pnb, score, prefix hash,
// parent hash, length, last label, trie node) is double-buffered in LDS.  Per frame: every entry computes its own
// successor by gathering its (at most two) contributions; new prefixes are scored on the fly as q + base, never stored.
// The best W of the <= W (N + 1) candidates are found by a radix select on r = max score - score (as many 8-bit passes as
// the frame's score range needs; a tie at the cut is settled by a second select on the candidate index, the tie rule),
// then sorted by counting.  A slot's candidates belong to a fixed group of threads that keep the slot's state in registers.
// Prefixes are nodes (parent, label) in the caller's workspace: the node of the entry that lands in slot s at frame t is
// t * W + s, so nothing is counted or allocated.  LDS atomics only (histogram, winner slots); global memory sees plain
// vector stores.  Every loop is bounded by T, W, N or a constant.
// The constants, log-add-exp, the model's view and walks and the selection itself are qasr_beam_dev.h's, shared with
// k_beam_boost and the streaming kernels.
#include "qasr_beam_dev.h"

namespace qasr {

#define BEAM_EMPTY_Q INT_MIN

// ------------------------------------------------------------------------------------------------------------ k_topn
struct TopnP {
  const float* logp;
  const int32_t* lens;      // optional [B]
  int32_t* cand_id;         // [B][T][N]
  int32_t* cand_q;          // [B][T][N]
  long long pitch_b, pitch_t;
  int B, T, C, N;
};

#define TOPN_UNROLL 8

__global__ void __launch_bounds__(64) k_topn(TopnP p) {
  __shared__ unsigned sm_hist[256];
  __shared__ unsigned sm_key[64];
  __shared__ int sm_id[64];
  const int lane = threadIdx.x;
  const int frame = blockIdx.x;                  // < B * T
  const int b = frame / p.T, t = frame - b * p.T;
  const int lim = p.lens ? min(max(p.lens[b], 0), p.T) : p.T;
  int32_t* const oid = p.cand_id + (size_t)frame * p.N;
  int32_t* const oq = p.cand_q + (size_t)frame * p.N;
  if (t >= lim) {
    if (lane < p.N) oid[lane] = -1, oq[lane] = BEAM_EMPTY_Q;
    return;
  }
  const float* const row = p.logp + (long long)b * p.pitch_b + (long long)t * p.pitch_t;
  const int C = p.C, ne = min(p.N, C);
  // radix select: the key of the ne-th largest class
  unsigned prefix = 0;
  int k = ne;                                    // still to take, counted from the top
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = pass * 8;
    for (int i = lane; i < 256; i += 64) sm_hist[i] = 0;      // no barrier before this: the work-group is ONE wave, whose
    __syncthreads();                                          // LDS reads of the previous pass are behind it in program order
    for (int c0 = lane; c0 < C; c0 += 64 * TOPN_UNROLL) {        // TOPN_UNROLL independent loads in flight per lane
      int bits[TOPN_UNROLL];
#pragma unroll
      for (int j = 0; j < TOPN_UNROLL; ++j) bits[j] = c0 + j * 64 < C ? __float_as_int(row[c0 + j * 64]) : 0;
#pragma unroll
      for (int j = 0; j < TOPN_UNROLL; ++j) {
        const unsigned key = (unsigned)fx_key(bits[j]) ^ 0x80000000u;
        if (c0 + j * 64 < C && (pass == 3 || (key >> (shift + 8)) == prefix)) atomicAdd(&sm_hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    unsigned h[4];
    unsigned tl = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = sm_hist[lane * 4 + j], tl += h[j];
    unsigned suf = tl;                           // inclusive suffix sum over lanes: classes in this lane's bins and above
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_down(suf, d);
      if (lane + d < 64) suf += o;
    }
    const unsigned above = suf - tl;
    const bool mine = above < (unsigned)k && (unsigned)k <= suf;
    int bin = 0, kk = 0;
    if (mine) {
      unsigned acc = above;
      bin = lane * 4;
      kk = k - (int)acc;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (acc + h[j] >= (unsigned)k) { bin = lane * 4 + j; kk = k - (int)acc; break; }
        acc += h[j];
      }
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;      // exactly one lane (the counts add up to >= k)
    bin = __shfl(bin, src);
    k = __shfl(kk, src);
    prefix = (prefix << 8) | (unsigned)bin;
  }
  // prefix: the cut key; k of the classes with exactly that key belong to the ne (lowest ids first)
  int n_out = 0, n_eq = 0;
  for (int cb = 0; cb < C; cb += 64 * TOPN_UNROLL) {
    int bits[TOPN_UNROLL];
#pragma unroll
    for (int j = 0; j < TOPN_UNROLL; ++j) bits[j] = cb + j * 64 + lane < C ? __float_as_int(row[cb + j * 64 + lane]) : 0;
#pragma unroll
    for (int j = 0; j < TOPN_UNROLL; ++j) {                      // class order: chunk by chunk, lane by lane
      const int c = cb + j * 64 + lane;
      const unsigned key = (unsigned)fx_key(bits[j]) ^ 0x80000000u;
      const bool gt = c < C && key > prefix, eq = c < C && key == prefix;
      const unsigned long long below = (1ull << lane) - 1ull;
      const unsigned long long em = __ballot(eq);
      const bool take = gt || (eq && n_eq + __popcll(em & below) < k);
      const unsigned long long tm = __ballot(take);
      if (take) {
        const int pos = n_out + __popcll(tm & below);
        if (pos < 64) sm_key[pos] = key, sm_id[pos] = c;
      }
      n_out += __popcll(tm);
      n_eq += __popcll(em);
    }
  }
  __syncthreads();
  n_out = min(n_out, ne);
  if (lane < n_out) {
    const unsigned key = sm_key[lane];
    const int id = sm_id[lane];
    int rank = 0;
    for (int j = 0; j < n_out; ++j) {
      const unsigned kj = sm_key[j];
      rank += (kj > key || (kj == key && sm_id[j] < id)) ? 1 : 0;
    }
    oid[rank] = id;
    oq[rank] = fx_quantize(__int_as_float(fx_key((int)(key ^ 0x80000000u))));
  } else if (lane < p.N) {
    oid[lane] = -1, oq[lane] = BEAM_EMPTY_Q;
  }
}

int launch_topn(hipStream_t s, const qasr_ctc_topn_args& a) {
  TopnP p{};
  p.logp = a.log_probs, p.lens = a.lens, p.cand_id = a.cand_id, p.cand_q = a.cand_q;
  p.pitch_b = a.pitch_utt, p.pitch_t = a.pitch_frame;
  p.B = a.B, p.T = a.T, p.C = a.C, p.N = a.N;
  hipLaunchKernelGGL(k_topn, dim3((unsigned)(a.B * a.T)), dim3(64), 0, s, p);
  return QASR_OK;
}

// ------------------------------------------------------------------------------------------------------------ k_beam
struct BeamLds {
  uint16_t tab[BEAM_TAB];
  BeamState st[2];
  long long k_pb[BEAM_W], k_pnb[BEAM_W], k_sc[BEAM_W];     // the entries' own successors
  unsigned long long sel_r[BEAM_W];
  int sel_idx[BEAM_W];
  unsigned long long child[BEAM_W];                        // bit n of slot i: its extension by candidate n is an entry of the beam
  int cid[BEAM_N], cq[BEAM_N];
  unsigned hist[256];
  long long red_max[BEAM_NWAVE], red_min[BEAM_NWAVE];
  int red_cnt[BEAM_NWAVE], red_a[BEAM_NWAVE], red_b[BEAM_NWAVE];
  int bin, kk, n_at, n_sel;
};

__global__ void __launch_bounds__(BEAM_NT) k_beam(BeamP p) {
  __shared__ BeamLds L;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, T = p.T, N = p.N, W = p.W, N1 = N + 1, blank = p.blank;
  const int lim = p.lens ? min(max(p.lens[b], 0), T) : T;
  int2* const nodes = p.nodes + (size_t)b * T * W;
  const int n_nodes = T * W;
  for (int i = tid; i < BEAM_TAB; i += BEAM_NT) L.tab[i] = p.tab[i];
  if (tid == 0) {
    BeamState& S = L.st[0];
    S.pb[0] = 0, S.pnb[0] = BEAM_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.len[0] = 0, S.last[0] = -1, S.node[0] = -1;
  }
  const int32_t* const gid = p.cand_id + (size_t)b * T * N;
  const int32_t* const gq = p.cand_q + (size_t)b * T * N;
  int pf_id = -1, pf_q = 0;
  if (tid < N && lim > 0) pf_id = gid[tid], pf_q = gq[tid];
  int nb = 1, cur = 0;
  __syncthreads();
  for (int t = 0; t < lim && nb > 0; ++t) {
    const BeamState& S = L.st[cur];
    BeamState& D = L.st[cur ^ 1];
    if (tid < N) {
      L.cid[tid] = pf_id, L.cq[tid] = pf_q;
      if (t + 1 < lim) pf_id = gid[(size_t)(t + 1) * N + tid], pf_q = gq[(size_t)(t + 1) * N + tid];
    }
    if (tid < nb) L.child[tid] = 0;
    if (tid == 0) L.n_sel = 0;
    __syncthreads();
    // ---- the entries themselves
    if (tid < nb) {
      const int j = tid, c = S.last[j], lj = S.len[j];
      int nl = -1, nbk = -1;
      for (int n = 0; n < N; ++n) {
        const int id = L.cid[n];
        if (id >= 0) {
          if (id == blank && nbk < 0) nbk = n;
          if (id == c && nl < 0) nl = n;
        }
      }
      int ps = -1;
      if (lj > 0) {
        const unsigned long long ph = S.phash[j];
        for (int i = nb - 1; i >= 0; --i)            // no early exit (the loads pipeline); the first matching slot counts
          ps = (S.hash[i] == ph && S.len[i] + 1 == lj) ? i : ps;
      }
      const long long pbn = nbk >= 0 ? S.sc[j] + (long long)L.cq[nbk] : BEAM_NEG;
      long long a = BEAM_NEG, e = BEAM_NEG;
      if (nl >= 0) {
        const long long ql = (long long)L.cq[nl];
        if (S.pnb[j] != BEAM_NEG) a = ql + S.pnb[j];
        if (ps >= 0) {
          const long long base = S.last[ps] == c ? S.pb[ps] : S.sc[ps];
          if (base != BEAM_NEG) e = ql + base;
          atomicOr(&L.child[ps], 1ull << nl);
        }
      }
      const long long pnbn = fx_lae(a, e, L.tab);
      L.k_pb[j] = pbn, L.k_pnb[j] = pnbn, L.k_sc[j] = fx_lae(pbn, pnbn, L.tab);
    }
    __syncthreads();
    // ---- the candidates: idx = i * (N + 1) + k, k == 0 the entry in slot i itself, else its extension by candidate k - 1.
    // A row of candidates (one slot) belongs to 256 / rows threads, rows = nb rounded up to a power of two, so a thread
    // keeps its slot's state in registers and scores a candidate with one add.
    const int lg = nb > 1 ? 32 - __clz(nb - 1) : 0;            // rows = 1 << lg <= 128
    const int tpr_lg = 8 - lg, tpr = 1 << tpr_lg;               // BEAM_NT == 256
    const int my_i = tid >> tpr_lg, my_sub = tid & (tpr - 1);
    const bool active = my_i < nb;
    const int r_last = active ? S.last[my_i] : -1;
    const long long r_pb = active ? S.pb[my_i] : BEAM_NEG, r_sc = active ? S.sc[my_i] : BEAM_NEG;
    const long long r_ksc = active ? L.k_sc[my_i] : BEAM_NEG;
    const unsigned long long r_child = active ? L.child[my_i] : 0ull;
    auto cand = [&](int k) -> long long {
      if (k == 0) return r_ksc;
      const int n = k - 1, id = L.cid[n];
      if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return BEAM_NEG;
      const long long base = id == r_last ? r_pb : r_sc;
      return base == BEAM_NEG ? BEAM_NEG : base + (long long)L.cq[n];
    };
    const int k_end = active ? N1 : 0;
    long long mx;
    if (!beam_select(L, cand, my_i, my_sub, tpr, k_end, nb, N1, W, mx)) { nb = 0; break; }      // uniform
    const int ns = min(L.n_sel, W);
    // ---- order them (score descending = r ascending, then candidate index) and write the next beam
    if (tid < ns) {
      const unsigned long long r = L.sel_r[tid];
      const int idx = L.sel_idx[tid];
      int rank = 0;
      for (int m = 0; m < ns; ++m) {
        const unsigned long long rm = L.sel_r[m];
        rank += (rm < r || (rm == r && L.sel_idx[m] < idx)) ? 1 : 0;
      }
      const int i = idx / N1, k = idx - i * N1;
      if (k == 0) {
        D.pb[rank] = L.k_pb[i], D.pnb[rank] = L.k_pnb[i], D.sc[rank] = L.k_sc[i];
        D.hash[rank] = S.hash[i], D.phash[rank] = S.phash[i], D.len[rank] = S.len[i], D.last[rank] = S.last[i];
        D.node[rank] = S.node[i];
      } else {
        const int c = L.cid[k - 1];
        const long long v = mx - (long long)r;
        unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
        x ^= x >> 32;
        D.pb[rank] = BEAM_NEG, D.pnb[rank] = v, D.sc[rank] = v;
        D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
        const int nd = t * W + rank;                // < T * W
        D.node[rank] = nd;
        nodes[nd] = make_int2(S.node[i], c);
      }
    }
    __syncthreads();
    nb = ns, cur ^= 1;
  }
  __syncthreads();
  // ---- the final beam, best first
  const BeamState& S = L.st[cur];
  const int nh = min(nb, p.n_best);
  int32_t* const lab = p.labels + (size_t)b * p.n_best * T;
  for (int i = tid; i < p.n_best * T; i += BEAM_NT) lab[i] = blank;
  if (tid == 0) p.n_hyps[b] = nh;
  __syncthreads();                                  // the fill above and every node store of this work-group are visible
  if (tid < p.n_best) {
    const int h = tid;
    int len = 0;
    long long sc = BEAM_NEG;
    if (h < nh) {
      len = min(S.len[h], T), sc = S.sc[h];
      int nd = S.node[h];
      for (int k = len - 1; k >= 0; --k) {          // bounded by T; a node outside the pool ends the walk
        if (nd < 0 || nd >= n_nodes) break;
        const int2 e = nodes[nd];
        lab[(size_t)h * T + k] = e.y;
        nd = e.x;
      }
    }
    p.n_labels[(size_t)b * p.n_best + h] = len;
    p.score[(size_t)b * p.n_best + h] = sc;
  }
}

size_t beam_workspace_bytes(int B, int T, int W) { return (size_t)B * (size_t)T * (size_t)W * sizeof(int2); }

int launch_beam(hipStream_t s, const qasr_ctc_beam_args& a) {
  BeamP p{};
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.lens = a.lens, p.tab = a.lae_table;
  p.nodes = (int2*)a.workspace;
  p.labels = a.labels, p.n_labels = a.n_labels, p.score = (long long*)a.score, p.n_hyps = a.n_hyps;
  p.B = a.B, p.T = a.T, p.N = a.N, p.W = a.beam_width, p.n_best = a.n_best, p.blank = a.blank;
  hipLaunchKernelGGL(k_beam, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, p);
  return QASR_OK;
}


// --------------------------------------------------------------------------------------------------------- k_beam_lm
// k_beam with the shallow fusion of a back-off n-gram model (LM_RULES of qasr/beam.py; the packed model is qasr/ngram.py's).
// What differs from k_beam above: an entry also keeps its context node, the hash
// of its current word, the term of its own creation (the E path reuses it) and the running sum of its terms; the frame's
// terms are evaluated ONCE, before the selection - thread (slot, sub) walks the model for the candidates it scores anyway and
// leaves raw in L.raw[slot][n] (character mode: up to W x N walks; word mode: the space candidate of each slot, <= W) - and
// cand() adds ((raw * alpha_q + 2^15) >> 16) + beta_q.  A winner repeats its one walk for the next context.  The model stays
// in global memory and is read with plain vector loads (one 16-byte slot per probe); every walk is bounded by the order and
// the header's probe bounds.  After the last frame, word mode scores the unfinished word of every entry and re-orders.
// With the table and raw[128][64] the state is about 93 KB of static LDS: gfx950 gives one work-group up to 160 KB.
struct BeamLmP {
  BeamP b;
  const int* lm;
  long long lm_bytes, alpha_q, beta_q;
  long long* lm_score;      // [B][n_best]
  int space;
};

struct BeamLmState {
  BeamState s;
  long long own[BEAM_W], lmt[BEAM_W];
  unsigned long long wh[BEAM_W];
  int ctx[BEAM_W];
};

struct BeamLmLds {
  uint16_t tab[BEAM_TAB];
  BeamLmState st[2];
  long long k_pb[BEAM_W], k_pnb[BEAM_W], k_sc[BEAM_W];
  unsigned long long sel_r[BEAM_W];
  int sel_idx[BEAM_W];
  unsigned long long child[BEAM_W];
  int cid[BEAM_N], cq[BEAM_N];
  unsigned hist[256];
  long long red_max[BEAM_NWAVE], red_min[BEAM_NWAVE];
  int red_cnt[BEAM_NWAVE], red_a[BEAM_NWAVE], red_b[BEAM_NWAVE];
  int bin, kk, n_at, n_sel;
  int raw[BEAM_W * BEAM_N];
};

__global__ void __launch_bounds__(BEAM_NT) k_beam_lm(BeamLmP q) {
  __shared__ BeamLmLds L;
  const BeamP& p = q.b;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, T = p.T, N = p.N, W = p.W, N1 = N + 1, blank = p.blank;
  const int lim = p.lens ? min(max(p.lens[b], 0), T) : T;
  int2* const nodes = p.nodes + (size_t)b * T * W;
  const int n_nodes = T * W;
  // the model (validated on the host by qasr_lm_check); a header that does not fit the bytes given ends the search empty
  LmView m;
  const int space = q.space;
  const bool model_ok = lm_view(m, q.lm, q.lm_bytes, q.alpha_q, q.beta_q, space);
  const bool word_mode = m.word_mode;
  for (int i = tid; i < BEAM_TAB; i += BEAM_NT) L.tab[i] = p.tab[i];
  if (tid == 0) {
    BeamLmState& S0 = L.st[0];
    BeamState& S = S0.s;
    S.pb[0] = 0, S.pnb[0] = BEAM_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.len[0] = 0, S.last[0] = -1, S.node[0] = -1;
    S0.own[0] = 0, S0.lmt[0] = 0, S0.wh[0] = 0, S0.ctx[0] = m.start;
  }
  const int32_t* const gid = p.cand_id + (size_t)b * T * N;
  const int32_t* const gq = p.cand_q + (size_t)b * T * N;
  int pf_id = -1, pf_q = 0;
  if (tid < N && lim > 0) pf_id = gid[tid], pf_q = gq[tid];
  int nb = model_ok ? 1 : 0, cur = 0;
  __syncthreads();
  for (int t = 0; t < lim && nb > 0; ++t) {
    const BeamLmState& SL = L.st[cur];
    BeamLmState& DL = L.st[cur ^ 1];
    const BeamState& S = SL.s;
    BeamState& D = DL.s;
    if (tid < N) {
      L.cid[tid] = pf_id, L.cq[tid] = pf_q;
      if (t + 1 < lim) pf_id = gid[(size_t)(t + 1) * N + tid], pf_q = gq[(size_t)(t + 1) * N + tid];
    }
    if (tid < nb) L.child[tid] = 0;
    if (tid == 0) L.n_sel = 0;
    __syncthreads();
    // ---- the entries themselves (the E path adds the entry's own term)
    if (tid < nb) {
      const int j = tid, c = S.last[j], lj = S.len[j];
      int nl = -1, nbk = -1;
      for (int n = 0; n < N; ++n) {
        const int id = L.cid[n];
        if (id >= 0) {
          if (id == blank && nbk < 0) nbk = n;
          if (id == c && nl < 0) nl = n;
        }
      }
      int ps = -1;
      if (lj > 0) {
        const unsigned long long ph = S.phash[j];
        for (int i = nb - 1; i >= 0; --i)
          ps = (S.hash[i] == ph && S.len[i] + 1 == lj) ? i : ps;
      }
      const long long pbn = nbk >= 0 ? S.sc[j] + (long long)L.cq[nbk] : BEAM_NEG;
      long long a = BEAM_NEG, e = BEAM_NEG;
      if (nl >= 0) {
        const long long ql = (long long)L.cq[nl];
        if (S.pnb[j] != BEAM_NEG) a = ql + S.pnb[j];
        if (ps >= 0) {
          const long long base = S.last[ps] == c ? S.pb[ps] : S.sc[ps];
          if (base != BEAM_NEG) e = ql + base + SL.own[j];
          atomicOr(&L.child[ps], 1ull << nl);
        }
      }
      const long long pnbn = fx_lae(a, e, L.tab);
      L.k_pb[j] = pbn, L.k_pnb[j] = pnbn, L.k_sc[j] = fx_lae(pbn, pnbn, L.tab);
    }
    __syncthreads();
    const int lg = nb > 1 ? 32 - __clz(nb - 1) : 0;
    const int tpr_lg = 8 - lg, tpr = 1 << tpr_lg;
    const int my_i = tid >> tpr_lg, my_sub = tid & (tpr - 1);
    const bool active = my_i < nb;
    const int r_last = active ? S.last[my_i] : -1;
    const long long r_pb = active ? S.pb[my_i] : BEAM_NEG, r_sc = active ? S.sc[my_i] : BEAM_NEG;
    const long long r_ksc = active ? L.k_sc[my_i] : BEAM_NEG;
    const unsigned long long r_child = active ? L.child[my_i] : 0ull;
    const int k_end = active ? N1 : 0;
    int* const my_raw = L.raw + my_i * N;             // my_i < 128: inside raw[BEAM_W * BEAM_N] since N <= BEAM_N
    // ---- this frame's terms, once: the thread that scores candidate (my_i, n) below walks the model for it here
    {
      const int r_ctx = active ? SL.ctx[my_i] : 0;
      const unsigned long long r_wh = active ? SL.wh[my_i] : 0ull;
      const bool inword = r_last >= 0 && r_last != space;
      for (int k = my_sub; k < k_end; k += tpr) {
        if (k == 0) continue;
        const int n = k - 1, id = L.cid[n];
        int r = BEAM_LM_NOTERM, nx;
        if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
          if (!word_mode) r = lm_walk(m, r_ctx, id < m.n_labels ? m.l2w[id] : -1, nx);
          else if (id == space && inword) r = lm_walk(m, r_ctx, lm_word(m, r_wh), nx);
        }
        my_raw[n] = r;
      }
    }
    auto cand = [&](int k) -> long long {
      if (k == 0) return r_ksc;
      const int n = k - 1, id = L.cid[n];
      if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return BEAM_NEG;
      const long long base = id == r_last ? r_pb : r_sc;
      return base == BEAM_NEG ? BEAM_NEG : base + (long long)L.cq[n] + lm_term(m, my_raw[n]);
    };
    long long mx;
    if (!beam_select(L, cand, my_i, my_sub, tpr, k_end, nb, N1, W, mx)) { nb = 0; break; }
    const int ns = min(L.n_sel, W);
    if (tid < ns) {
      const unsigned long long r = L.sel_r[tid];
      const int idx = L.sel_idx[tid];
      int rank = 0;
      for (int mm = 0; mm < ns; ++mm) {
        const unsigned long long rm = L.sel_r[mm];
        rank += (rm < r || (rm == r && L.sel_idx[mm] < idx)) ? 1 : 0;
      }
      const int i = idx / N1, k = idx - i * N1;
      if (k == 0) {
        D.pb[rank] = L.k_pb[i], D.pnb[rank] = L.k_pnb[i], D.sc[rank] = L.k_sc[i];
        D.hash[rank] = S.hash[i], D.phash[rank] = S.phash[i], D.len[rank] = S.len[i], D.last[rank] = S.last[i];
        D.node[rank] = S.node[i];
        DL.own[rank] = SL.own[i], DL.lmt[rank] = SL.lmt[i], DL.wh[rank] = SL.wh[i], DL.ctx[rank] = SL.ctx[i];
      } else {
        const int c = L.cid[k - 1];
        const long long v = mx - (long long)r;
        unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
        x ^= x >> 32;
        D.pb[rank] = BEAM_NEG, D.pnb[rank] = v, D.sc[rank] = v;
        D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
        const int nd = t * W + rank;
        D.node[rank] = nd;
        nodes[nd] = make_int2(S.node[i], c);
        const int raw = L.raw[i * N + k - 1];         // written before the barriers of the selection
        const long long tm = lm_term(m, raw);
        int ctx = SL.ctx[i];
        unsigned long long wh = 0;
        if (word_mode && c != space) {
          wh = (SL.wh[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
          wh ^= wh >> 32;
        } else if (raw != BEAM_LM_NOTERM) {             // the token was scored: the one walk again, for its context
          const int w = word_mode ? lm_word(m, SL.wh[i]) : (c < m.n_labels ? m.l2w[c] : -1);
          lm_walk(m, SL.ctx[i], w, ctx);
        }
        DL.own[rank] = tm, DL.lmt[rank] = SL.lmt[i] + tm, DL.wh[rank] = wh, DL.ctx[rank] = ctx;
      }
    }
    __syncthreads();
    nb = ns, cur ^= 1;
  }
  __syncthreads();
  // ---- word mode: the unfinished word of every entry, then the order (score descending, ties by the previous rank)
  if (word_mode && nb > 0) {
    const BeamLmState& SL = L.st[cur];
    BeamLmState& DL = L.st[cur ^ 1];
    long long sc = BEAM_NEG, lmt = 0;
    if (tid < nb) {
      sc = SL.s.sc[tid], lmt = SL.lmt[tid];
      const int last = SL.s.last[tid];
      if (last >= 0 && last != space) {
        int nx;
        const long long tm = lm_term(m, lm_walk(m, SL.ctx[tid], lm_word(m, SL.wh[tid]), nx));
        sc += tm, lmt += tm;
      }
      L.k_sc[tid] = sc;
    }
    __syncthreads();
    if (tid < nb) {
      int rank = 0;
      for (int mm = 0; mm < nb; ++mm) {
        const long long sm = L.k_sc[mm];
        rank += (sm > sc || (sm == sc && mm < tid)) ? 1 : 0;
      }
      DL.s.sc[rank] = sc, DL.lmt[rank] = lmt, DL.s.len[rank] = SL.s.len[tid], DL.s.node[rank] = SL.s.node[tid];
    }
    __syncthreads();
    cur ^= 1;
  }
  // ---- the final beam, best first
  const BeamLmState& SL = L.st[cur];
  const BeamState& S = SL.s;
  const int nh = min(nb, p.n_best);
  int32_t* const lab = p.labels + (size_t)b * p.n_best * T;
  for (int i = tid; i < p.n_best * T; i += BEAM_NT) lab[i] = blank;
  if (tid == 0) p.n_hyps[b] = nh;
  __syncthreads();
  if (tid < p.n_best) {
    const int h = tid;
    int len = 0;
    long long sc = BEAM_NEG, lmt = 0;
    if (h < nh) {
      len = min(S.len[h], T), sc = S.sc[h], lmt = SL.lmt[h];
      int nd = S.node[h];
      for (int k = len - 1; k >= 0; --k) {
        if (nd < 0 || nd >= n_nodes) break;
        const int2 e = nodes[nd];
        lab[(size_t)h * T + k] = e.y;
        nd = e.x;
      }
    }
    p.n_labels[(size_t)b * p.n_best + h] = len;
    p.score[(size_t)b * p.n_best + h] = sc;
    q.lm_score[(size_t)b * p.n_best + h] = lmt;
  }
}

int launch_beam_lm(hipStream_t s, const qasr_ctc_beam_lm_args& a) {
  BeamLmP q{};
  BeamP& p = q.b;
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.lens = a.lens, p.tab = a.lae_table;
  p.nodes = (int2*)a.workspace;
  p.labels = a.labels, p.n_labels = a.n_labels, p.score = (long long*)a.score, p.n_hyps = a.n_hyps;
  p.B = a.B, p.T = a.T, p.N = a.N, p.W = a.beam_width, p.n_best = a.n_best, p.blank = a.blank;
  q.lm = (const int*)a.lm, q.lm_bytes = (long long)a.lm_bytes, q.alpha_q = a.alpha_q, q.beta_q = a.beta_q;
  q.lm_score = (long long*)a.lm_score, q.space = a.space;
  static_assert(sizeof(BeamLmLds) <= 160 * 1024, "k_beam_lm: the LDS of one gfx950 CU");
  hipLaunchKernelGGL(k_beam_lm, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, q);
  return QASR_OK;
}

}  // namespace qasr
