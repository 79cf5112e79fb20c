// CTC prefix beam search with phrase boosting ("hot words"): k_beam_boost, with an n-gram model (LM = true) and without
// (LM = false: no model state is carried).  The rules are BOOST_RULES of qasr/boost.py (with LM_RULES of qasr/beam.py for
// the model), which this kernel follows bit for bit; the packed phrase set is qasr/boost.py's.  A file of its own, so that
// k_beam and k_beam_lm (qasr_beam.hip) stay as they are: the selection machinery below is theirs, line for line.  What
// differs from k_beam_lm: an entry also keeps its automaton state, the pot of that state and the running sum boost_tot;
// `own` holds the summed term (model + boost).  The frame's boost terms are evaluated ONCE, before the selection: the
// thread that scores candidate (slot, n) looks up s' = delta(state[slot], label n) - an entry in the root state reads the
// dense root row only (one load, no probe), any other makes one bounded probe sequence and falls back to the root row on
// a miss, so no fail link is ever walked - then loads (pot, bank)[s'] and leaves pot[s'] - pot[s] + bank[s'] in
// L.bterm[slot][n], biased by 2^30 into an unsigned (0 <= pot, bank <= 2^30, so the term lies in [-2^30, 2^31]).  A winner
// repeats its one look-up for its next state.  The set stays in global memory and is read with plain vector loads.  After the
// last frame every entry takes the virtual space (whole words), loses its unfinished pot and - with a word-mode model -
// receives its unfinished word's term, then ONE re-ordering.  No exp or log, no allocation, LDS atomics only.
#include <climits>

#include "qasr_internal.h"

namespace qasr {
namespace {                 // the helpers of qasr_beam.hip, repeated here so that that file's code does not change

#define BEAM_NEG (-(1ll << 62))
#define BEAM_QFLOOR (-1073741824.f)
#define BEAM_QCEIL (1073741824.f)
#define BEAM_EMPTY_Q INT_MIN
#define BEAM_DMAX (16ll << 16)
#define BEAM_HMUL 0x9E3779B97F4A7C15ull

#define BEAM_NT 256
#define BEAM_NWAVE (BEAM_NT / 64)
#define BEAM_W QASR_BEAM_MAX_WIDTH
#define BEAM_N QASR_BEAM_MAX_CANDIDATES
#define BEAM_TAB QASR_BEAM_TABLE_ENTRIES

struct BeamP {
  const int32_t* cand_id;   // [B][T][N]
  const int32_t* cand_q;
  const int32_t* lens;      // optional [B]
  const uint16_t* tab;      // [BEAM_TAB]
  int2* nodes;              // [B][T * W] (parent node, label)
  int32_t* labels;          // [B][n_best][T]
  int32_t* n_labels;        // [B][n_best]
  long long* score;         // [B][n_best]
  int32_t* n_hyps;          // [B]
  int B, T, N, W, n_best, blank;
};

struct BeamState {          // one side of the double buffer
  long long pb[BEAM_W], pnb[BEAM_W], sc[BEAM_W];
  unsigned long long hash[BEAM_W], phash[BEAM_W];
  int len[BEAM_W], last[BEAM_W], node[BEAM_W];
};

__device__ __forceinline__ long long beam_lae(long long a, long long b, const uint16_t* tab) {
  const long long m = a > b ? a : b, n = a > b ? b : a;
  if (n == BEAM_NEG) return m;
  const long long d = m - n;
  if (d >= BEAM_DMAX) return m;
  return m + (long long)tab[d >> 6];
}

#define BEAM_LM_MAGIC 0x314D4C51
#define BEAM_LM_OOV (-1000 * 65536)
#define BEAM_LM_RAWLIM 2147483647ll
#define BEAM_LM_NOTERM INT_MIN

struct LmView {
  const int4* trans;        // [tmask + 1] node, word, prob_q, next
  const int4* words;        // [wmask + 1] hash lo, hash hi, word id, 0
  const int2* nodes;        // [n_nodes] backoff_q, suffix
  const int* l2w;           // [n_labels]
  int order, tprobe, wprobe, n_labels;
  unsigned tmask, wmask;
};

// raw(ctx, w) and the context it leaves
__device__ __forceinline__ int lm_walk(const LmView& m, int ctx, int w, int& next) {
  next = 0;
  if (w < 0) return BEAM_LM_OOV;
  long long acc = 0;
  int node = ctx;
  for (int it = 0; it < m.order; ++it) {
    unsigned long long x = (((unsigned long long)(unsigned)node << 32) | (unsigned long long)(unsigned)w) * BEAM_HMUL;
    x ^= x >> 32;
    unsigned s = (unsigned)x & m.tmask;
    bool hit = false;
    for (int pr = 0; pr < m.tprobe; ++pr) {
      const int4 e = m.trans[s];
      if (e.x == node && e.y == w) { acc += e.z; next = e.w; hit = true; break; }
      if (e.x < 0) break;
      s = (s + 1) & m.tmask;
    }
    if (hit) break;
    const int2 nd = m.nodes[node];
    acc += nd.x, node = nd.y;
  }
  acc = acc > BEAM_LM_RAWLIM ? BEAM_LM_RAWLIM : acc;
  acc = acc < -BEAM_LM_RAWLIM ? -BEAM_LM_RAWLIM : acc;
  return (int)acc;
}

// the word id of a label hash, -1: none
__device__ __forceinline__ int lm_word(const LmView& m, unsigned long long h) {
  unsigned s = (unsigned)h & m.wmask;
  for (int pr = 0; pr < m.wprobe; ++pr) {
    const int4 e = m.words[s];
    if (e.z < 0) return -1;
    if ((unsigned)e.x == (unsigned)h && (unsigned)e.y == (unsigned)(h >> 32)) return e.z;
    s = (s + 1) & m.wmask;
  }
  return -1;
}

// ------------------------------------------------------------------------------------------------------ k_beam_boost
#define BOOST_MAGIC 0x31534251
#define BOOST_BIAS (1ll << 30)

struct BoostView {
  const int4* table;        // [mask + 1] node, label, next, 0
  const int2* nodes;        // [n_nodes] pot_q, bank_q
  const int* root_next;     // [n_labels]
  int probe, n_labels;
  unsigned mask;
};

struct BoostP {
  BeamP b;
  const int* lm;            // LM only
  long long lm_bytes, alpha_q, beta_q;
  long long* lm_score;      // [B][n_best], LM only
  const int* boost;
  long long boost_bytes;
  long long* boost_score;   // [B][n_best]
  int space, whole_words;
};

template <bool LM>
struct BoostState {
  BeamState s;
  long long own[BEAM_W], bt[BEAM_W];
  int bst[BEAM_W], bpot[BEAM_W];
  long long lmt[LM ? BEAM_W : 1];
  unsigned long long wh[LM ? BEAM_W : 1];
  int ctx[LM ? BEAM_W : 1];
};

template <bool LM>
struct BoostLds {
  uint16_t tab[BEAM_TAB];
  BoostState<LM> st[2];
  long long k_pb[BEAM_W], k_pnb[BEAM_W], k_sc[BEAM_W];
  unsigned long long sel_r[BEAM_W];
  int sel_idx[BEAM_W];
  unsigned long long child[BEAM_W];
  int cid[BEAM_N], cq[BEAM_N];
  unsigned hist[256];
  long long red_max[BEAM_NWAVE], red_min[BEAM_NWAVE];
  int red_cnt[BEAM_NWAVE], red_a[BEAM_NWAVE], red_b[BEAM_NWAVE];
  int bin, kk, n_at, n_sel;
  unsigned bterm[BEAM_W * BEAM_N];
  int raw[LM ? BEAM_W * BEAM_N : 1];
};

// delta(s, c): one bounded probe sequence, a miss is the root's row; the root itself reads its row only
__device__ __forceinline__ int boost_next(const BoostView& v, int s, int c) {
  if (c < 0 || c >= v.n_labels) return 0;
  const int rn = v.root_next[c];
  if (s == 0) return rn;
  unsigned long long x = (((unsigned long long)(unsigned)s << 32) | (unsigned long long)(unsigned)c) * BEAM_HMUL;
  x ^= x >> 32;
  unsigned k = (unsigned)x & v.mask;
  for (int pr = 0; pr < v.probe; ++pr) {
    const int4 e = v.table[k];
    if (e.x == s && e.y == c) return e.z;
    if (e.x < 0) break;
    k = (k + 1) & v.mask;
  }
  return rn;
}

template <bool LM>
__global__ void __launch_bounds__(BEAM_NT) k_beam_boost(BoostP q) {
  __shared__ BoostLds<LM> L;
  const BeamP& p = q.b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, T = p.T, N = p.N, W = p.W, N1 = N + 1, blank = p.blank;
  const int lim = p.lens ? min(max(p.lens[b], 0), T) : T;
  int2* const nodes = p.nodes + (size_t)b * T * W;
  const int n_nodes = T * W;
  const int space = q.space;
  // the phrase set (validated on the host by qasr_boost_check); a header that does not fit the bytes given ends the search empty
  const int* const bh = q.boost;
  BoostView v;
  const int b_nodes = bh[3], b_cap = bh[7], b_start = bh[5];
  v.n_labels = bh[4], v.probe = bh[8], v.mask = (unsigned)b_cap - 1u;
  v.table = reinterpret_cast<const int4*>(bh + 32);
  v.nodes = reinterpret_cast<const int2*>(v.table + (size_t)(b_cap > 0 ? b_cap : 0));
  v.root_next = reinterpret_cast<const int*>(v.nodes + (size_t)(b_nodes > 0 ? b_nodes : 0));
  const bool whole = bh[6] != 0;
  bool ok = bh[0] == BOOST_MAGIC && bh[1] == 1 && (long long)bh[2] == q.boost_bytes && b_nodes >= 1 && v.n_labels >= 1 &&
            b_cap >= 1 && (b_cap & (b_cap - 1)) == 0 && v.probe >= 1 && v.probe <= b_cap && b_start >= 0 && b_start < b_nodes &&
            128ll + 16ll * b_cap + 8ll * b_nodes + 4ll * v.n_labels == q.boost_bytes &&
            whole == (q.whole_words != 0) && (!whole || (space >= 0 && space < v.n_labels));
  // the model, as k_beam_lm reads it
  LmView m{};
  bool word_mode = false;
  long long alpha_q = 0, beta_q = 0;
  int lm_start = 0;
  if constexpr (LM) {
    const int* const hdr = q.lm;
    m.order = hdr[2], m.tprobe = hdr[7], m.wprobe = hdr[10], m.n_labels = hdr[8];
    m.tmask = (unsigned)hdr[6] - 1u, m.wmask = (unsigned)hdr[9] - 1u;
    m.trans = reinterpret_cast<const int4*>(hdr + 32);
    m.words = m.trans + (size_t)hdr[6];
    m.nodes = reinterpret_cast<const int2*>(m.words + (size_t)hdr[9]);
    m.l2w = reinterpret_cast<const int*>(m.nodes + (size_t)hdr[4]);
    word_mode = hdr[3] != 0;
    alpha_q = q.alpha_q, beta_q = q.beta_q;
    lm_start = hdr[5];
    ok = ok && hdr[0] == BEAM_LM_MAGIC && (long long)hdr[12] == q.lm_bytes && word_mode == (space >= 0) &&
         hdr[5] >= 0 && hdr[5] < hdr[4] && m.order >= 1 && m.order <= 6;
  }
  auto lm_term = [&](int raw) -> long long {
    return raw == BEAM_LM_NOTERM ? 0ll : ((((long long)raw * alpha_q + 32768ll) >> 16) + beta_q);
  };
  for (int i = tid; i < BEAM_TAB; i += BEAM_NT) L.tab[i] = p.tab[i];
  if (tid == 0) {
    BoostState<LM>& S0 = L.st[0];
    BeamState& S = S0.s;
    S.pb[0] = 0, S.pnb[0] = BEAM_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.len[0] = 0, S.last[0] = -1, S.node[0] = -1;
    const int s0 = ok ? b_start : 0;
    S0.own[0] = 0, S0.bt[0] = 0, S0.bst[0] = s0, S0.bpot[0] = ok ? v.nodes[s0].x : 0;
    if constexpr (LM) S0.lmt[0] = 0, S0.wh[0] = 0, S0.ctx[0] = ok ? lm_start : 0;
  }
  const int32_t* const gid = p.cand_id + (size_t)b * T * N;
  const int32_t* const gq = p.cand_q + (size_t)b * T * N;
  int pf_id = -1, pf_q = 0;
  if (tid < N && lim > 0) pf_id = gid[tid], pf_q = gq[tid];
  int nb = ok ? 1 : 0, cur = 0;
  __syncthreads();
  for (int t = 0; t < lim && nb > 0; ++t) {
    const BoostState<LM>& SL = L.st[cur];
    BoostState<LM>& DL = L.st[cur ^ 1];
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
      const long long pnbn = beam_lae(a, e, L.tab);
      L.k_pb[j] = pbn, L.k_pnb[j] = pnbn, L.k_sc[j] = beam_lae(pbn, pnbn, L.tab);
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
    unsigned* const my_bterm = L.bterm + my_i * N;     // my_i < 128: inside bterm[BEAM_W * BEAM_N] since N <= BEAM_N
    int* const my_raw = LM ? L.raw + my_i * N : L.raw;
    // ---- this frame's terms, once: the thread that scores candidate (my_i, n) below evaluates them here
    {
      const int r_bst = active ? SL.bst[my_i] : 0, r_bpot = active ? SL.bpot[my_i] : 0;
      int r_ctx = 0;
      unsigned long long r_wh = 0ull;
      if constexpr (LM) r_ctx = active ? SL.ctx[my_i] : 0, r_wh = active ? SL.wh[my_i] : 0ull;
      const bool inword = r_last >= 0 && r_last != space;
      for (int k = my_sub; k < k_end; k += tpr) {
        if (k == 0) continue;
        const int n = k - 1, id = L.cid[n];
        const bool scored = id >= 0 && id != blank && !((r_child >> n) & 1ull);
        long long bt = 0;
        if (scored) {
          const int2 nd = v.nodes[boost_next(v, r_bst, id)];
          bt = (long long)nd.x - (long long)r_bpot + (long long)nd.y;
        }
        my_bterm[n] = (unsigned)(bt + BOOST_BIAS);
        if constexpr (LM) {
          int r = BEAM_LM_NOTERM, nx;
          if (scored) {
            if (!word_mode) r = lm_walk(m, r_ctx, id < m.n_labels ? m.l2w[id] : -1, nx);
            else if (id == space && inword) r = lm_walk(m, r_ctx, lm_word(m, r_wh), nx);
          }
          my_raw[n] = r;
        }
      }
    }
    auto cand = [&](int k) -> long long {
      if (k == 0) return r_ksc;
      const int n = k - 1, id = L.cid[n];
      if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return BEAM_NEG;
      const long long base = id == r_last ? r_pb : r_sc;
      if (base == BEAM_NEG) return BEAM_NEG;
      long long v0 = base + (long long)L.cq[n] + ((long long)my_bterm[n] - BOOST_BIAS);
      if constexpr (LM) v0 += lm_term(my_raw[n]);
      return v0;
    };
    long long mx = LLONG_MIN, mn = LLONG_MAX;
    int cnt = 0;
    for (int k = my_sub; k < k_end; k += tpr) {
      const long long vv = cand(k);
      if (vv != BEAM_NEG) { ++cnt; mx = vv > mx ? vv : mx; mn = vv < mn ? vv : mn; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const long long omx = __shfl_xor(mx, d), omn = __shfl_xor(mn, d);
      cnt += __shfl_xor(cnt, d);
      mx = omx > mx ? omx : mx, mn = omn < mn ? omn : mn;
    }
    if (lane == 0) L.red_max[wave] = mx, L.red_min[wave] = mn, L.red_cnt[wave] = cnt;
    __syncthreads();
    mx = L.red_max[0], mn = L.red_min[0], cnt = L.red_cnt[0];
#pragma unroll
    for (int w = 1; w < BEAM_NWAVE; ++w) {
      mx = L.red_max[w] > mx ? L.red_max[w] : mx, mn = L.red_min[w] < mn ? L.red_min[w] : mn;
      cnt += L.red_cnt[w];
    }
    if (cnt == 0) { nb = 0; break; }
    auto radix_select = [&](auto keyfn, int nbits, int& kk, int& n_at) -> unsigned long long {
      const int passes = (nbits + 7) >> 3;
      unsigned long long prefix = 0;
      for (int pass = passes - 1; pass >= 0; --pass) {
        const int shift = pass * 8;
        __syncthreads();
        L.hist[tid] = 0;
        __syncthreads();
        for (int k = my_sub; k < k_end; k += tpr) {
          unsigned long long key;
          if (keyfn(k, key) && (shift + 8 >= 64 || (key >> (shift + 8)) == prefix))
            atomicAdd(&L.hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const int mine = (int)L.hist[tid];
        int inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int o = __shfl_up(inc, d);
          if (lane >= d) inc += o;
        }
        if (lane == 63) L.red_a[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += L.red_a[w];
        const int exc = inc - mine;
        if (exc < kk && kk <= inc) L.bin = tid, L.kk = kk - exc, L.n_at = mine;
        __syncthreads();
        prefix = (prefix << 8) | (unsigned long long)L.bin;
        kk = L.kk, n_at = L.n_at;
      }
      return prefix;
    };
    unsigned long long rth = ~0ull;
    int ith = INT_MAX;
    if (cnt > W) {
      const unsigned long long range = (unsigned long long)(mx - mn);
      int need = W, n_at = cnt;
      rth = radix_select([&](int k, unsigned long long& key) {
        const long long vv = cand(k);
        key = (unsigned long long)(mx - vv);
        return vv != BEAM_NEG;
      }, range ? 64 - __clzll((long long)range) : 0, need, n_at);
      if (n_at > need) {
        const int M = nb * N1;
        ith = (int)radix_select([&](int k, unsigned long long& key) {
          const long long vv = cand(k);
          key = (unsigned long long)(my_i * N1 + k);
          return vv != BEAM_NEG && (unsigned long long)(mx - vv) == rth;
        }, 32 - __clz(M), need, n_at);
      }
    }
    for (int k = my_sub; k < k_end; k += tpr) {
      const long long vv = cand(k);
      if (vv != BEAM_NEG) {
        const unsigned long long r = (unsigned long long)(mx - vv);
        const int idx = my_i * N1 + k;
        if (r < rth || (r == rth && idx <= ith)) {
          const int at = atomicAdd(&L.n_sel, 1);
          if (at < BEAM_W) L.sel_r[at] = r, L.sel_idx[at] = idx;
        }
      }
    }
    __syncthreads();
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
        DL.own[rank] = SL.own[i], DL.bt[rank] = SL.bt[i], DL.bst[rank] = SL.bst[i], DL.bpot[rank] = SL.bpot[i];
        if constexpr (LM) DL.lmt[rank] = SL.lmt[i], DL.wh[rank] = SL.wh[i], DL.ctx[rank] = SL.ctx[i];
      } else {
        const int c = L.cid[k - 1];
        const long long vv = mx - (long long)r;
        unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
        x ^= x >> 32;
        D.pb[rank] = BEAM_NEG, D.pnb[rank] = vv, D.sc[rank] = vv;
        D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
        const int nd = t * W + rank;
        D.node[rank] = nd;
        nodes[nd] = make_int2(S.node[i], c);
        const long long btm = (long long)L.bterm[i * N + k - 1] - BOOST_BIAS;      // written before the barriers of the selection
        const int s2 = boost_next(v, SL.bst[i], c);     // the one look-up again, for the next state
        long long own = btm;
        if constexpr (LM) {
          const int raw = L.raw[i * N + k - 1];
          const long long tm = lm_term(raw);
          int ctx = SL.ctx[i];
          unsigned long long wh = 0;
          if (word_mode && c != space) {
            wh = (SL.wh[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
            wh ^= wh >> 32;
          } else if (raw != BEAM_LM_NOTERM) {
            const int w = word_mode ? lm_word(m, SL.wh[i]) : (c < m.n_labels ? m.l2w[c] : -1);
            lm_walk(m, SL.ctx[i], w, ctx);
          }
          own += tm;
          DL.lmt[rank] = SL.lmt[i] + tm, DL.wh[rank] = wh, DL.ctx[rank] = ctx;
        }
        DL.own[rank] = own, DL.bt[rank] = SL.bt[i] + btm, DL.bst[rank] = s2, DL.bpot[rank] = v.nodes[s2].x;
      }
    }
    __syncthreads();
    nb = ns, cur ^= 1;
  }
  __syncthreads();
  // ---- after the last frame: the virtual space (whole words), the unfinished pot, the model's unfinished word; then the
  // order (score descending, ties by the previous rank)
  if (nb > 0) {
    const BoostState<LM>& SL = L.st[cur];
    BoostState<LM>& DL = L.st[cur ^ 1];
    long long sc = BEAM_NEG, lmt = 0, bt = 0;
    if (tid < nb) {
      sc = SL.s.sc[tid], bt = SL.bt[tid];
      if constexpr (LM) {
        lmt = SL.lmt[tid];
        const int last = SL.s.last[tid];
        if (word_mode && last >= 0 && last != space) {
          int nx;
          const long long tm = lm_term(lm_walk(m, SL.ctx[tid], lm_word(m, SL.wh[tid]), nx));
          sc += tm, lmt += tm;
        }
      }
      long long pot = (long long)SL.bpot[tid];
      if (whole) {
        const int2 nd = v.nodes[boost_next(v, SL.bst[tid], space)];
        const long long tm = (long long)nd.x - pot + (long long)nd.y;
        sc += tm, bt += tm, pot = (long long)nd.x;
      }
      sc -= pot, bt -= pot;
      L.k_sc[tid] = sc;
    }
    __syncthreads();
    if (tid < nb) {
      int rank = 0;
      for (int mm = 0; mm < nb; ++mm) {
        const long long sm = L.k_sc[mm];
        rank += (sm > sc || (sm == sc && mm < tid)) ? 1 : 0;
      }
      DL.s.sc[rank] = sc, DL.bt[rank] = bt, DL.s.len[rank] = SL.s.len[tid], DL.s.node[rank] = SL.s.node[tid];
      if constexpr (LM) DL.lmt[rank] = lmt;
    }
    __syncthreads();
    cur ^= 1;
  }
  // ---- the final beam, best first
  const BoostState<LM>& SL = L.st[cur];
  const BeamState& S = SL.s;
  const int nh = min(nb, p.n_best);
  int32_t* const lab = p.labels + (size_t)b * p.n_best * T;
  for (int i = tid; i < p.n_best * T; i += BEAM_NT) lab[i] = blank;
  if (tid == 0) p.n_hyps[b] = nh;
  __syncthreads();
  if (tid < p.n_best) {
    const int h = tid;
    int len = 0;
    long long sc = BEAM_NEG, lmt = 0, bt = 0;
    if (h < nh) {
      len = min(S.len[h], T), sc = S.sc[h], bt = SL.bt[h];
      if constexpr (LM) lmt = SL.lmt[h];
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
    q.boost_score[(size_t)b * p.n_best + h] = bt;
    if constexpr (LM) q.lm_score[(size_t)b * p.n_best + h] = lmt;
  }
}

}  // namespace

int launch_beam_boost(hipStream_t s, const qasr_ctc_beam_boost_args& a) {
  BoostP q{};
  BeamP& p = q.b;
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.lens = a.lens, p.tab = a.lae_table;
  p.nodes = (int2*)a.workspace;
  p.labels = a.labels, p.n_labels = a.n_labels, p.score = (long long*)a.score, p.n_hyps = a.n_hyps;
  p.B = a.B, p.T = a.T, p.N = a.N, p.W = a.beam_width, p.n_best = a.n_best, p.blank = a.blank;
  q.lm = (const int*)a.lm, q.lm_bytes = (long long)a.lm_bytes, q.alpha_q = a.alpha_q, q.beta_q = a.beta_q;
  q.lm_score = (long long*)a.lm_score, q.space = a.space, q.whole_words = a.whole_words;
  q.boost = (const int*)a.boost, q.boost_bytes = (long long)a.boost_bytes, q.boost_score = (long long*)a.boost_score;
  static_assert(sizeof(BoostLds<true>) <= 160 * 1024, "k_beam_boost: the LDS of one gfx950 CU");
  static_assert(sizeof(BoostLds<false>) <= sizeof(BoostLds<true>), "k_beam_boost: the form without a model carries no model state");
  if (a.lm) hipLaunchKernelGGL(k_beam_boost<true>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, q);
  else hipLaunchKernelGGL(k_beam_boost<false>, dim3((unsigned)a.B), dim3(BEAM_NT), 0, s, q);
  return QASR_OK;
}

}  // namespace qasr
