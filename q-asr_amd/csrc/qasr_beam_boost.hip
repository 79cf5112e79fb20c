// CTC prefix beam search with phrase boosting ("hot words"): k_beam_boost, with an n-gram model (LM = true) and without
// (LM = false: no model state is carried).  The rules are BOOST_RULES of qasr/boost.py (with LM_RULES of qasr/beam.py for
// the model), which this kernel follows bit for bit; the packed phrase set is qasr/boost.py's.  The selection, the
// views of the model and of the set, the walks and the look-up are qasr_beam_dev.h's, shared with qasr_beam.hip.  What
// differs from k_beam_lm: an entry also keeps its automaton state, the pot of that state and the running sum boost_tot;
// `own` holds the summed term (model + boost).  The frame's boost terms are evaluated ONCE, before the selection: the
// thread that scores candidate (slot, n) looks up s' = delta(state[slot], label n) - an entry in the root state reads the
// dense root row only (one load, no probe), any other makes one bounded probe sequence and falls back to the root row on
// a miss, so no fail link is ever walked - then loads (pot, bank)[s'] and leaves pot[s'] - pot[s] + bank[s'] in
// L.bterm[slot][n], biased by 2^30 into an unsigned (0 <= pot, bank <= 2^30, so the term lies in [-2^30, 2^31]).  A winner
// repeats its one look-up for its next state.  The set stays in global memory and is read with plain vector loads.  After the
// last frame every entry takes the virtual space (whole words), loses its unfinished pot and - with a word-mode model -
// receives its unfinished word's term, then ONE re-ordering.  No exp or log, no allocation, LDS atomics only.
#include "qasr_beam_dev.h"

namespace qasr {
namespace {

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

template <bool LM>
__global__ void __launch_bounds__(BEAM_NT) k_beam_boost(BoostP q) {
  __shared__ BoostLds<LM> L;
  const BeamP& p = q.b;
  const int tid = threadIdx.x;
  const int b = blockIdx.x, T = p.T, N = p.N, W = p.W, N1 = N + 1, blank = p.blank;
  const int lim = p.lens ? min(max(p.lens[b], 0), T) : T;
  int2* const nodes = p.nodes + (size_t)b * T * W;
  const int n_nodes = T * W;
  const int space = q.space;
  // the phrase set (validated on the host by qasr_boost_check); a header that does not fit the bytes given ends the search empty
  BoostView v;
  bool ok = boost_view(v, q.boost, q.boost_bytes, q.whole_words, space);
  const bool whole = v.whole;
  // the model, as k_beam_lm reads it
  LmView m{};
  if constexpr (LM) ok = lm_view(m, q.lm, q.lm_bytes, q.alpha_q, q.beta_q, space) && ok;
  const bool word_mode = m.word_mode;
  for (int i = tid; i < BEAM_TAB; i += BEAM_NT) L.tab[i] = p.tab[i];
  if (tid == 0) {
    BoostState<LM>& S0 = L.st[0];
    BeamState& S = S0.s;
    S.pb[0] = 0, S.pnb[0] = BEAM_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.len[0] = 0, S.last[0] = -1, S.node[0] = -1;
    const int s0 = ok ? v.start : 0;
    S0.own[0] = 0, S0.bt[0] = 0, S0.bst[0] = s0, S0.bpot[0] = ok ? v.nodes[s0].x : 0;
    if constexpr (LM) S0.lmt[0] = 0, S0.wh[0] = 0, S0.ctx[0] = ok ? m.start : 0;
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
          const int2 nd = v.nodes[boost_next<false>(v, r_bst, id)];
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
      if constexpr (LM) v0 += lm_term(m, my_raw[n]);
      return v0;
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
        const int s2 = boost_next<false>(v, SL.bst[i], c);     // the one look-up again, for the next state
        long long own = btm;
        if constexpr (LM) {
          const int raw = L.raw[i * N + k - 1];
          const long long tm = lm_term(m, raw);
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
          const long long tm = lm_term(m, lm_walk(m, SL.ctx[tid], lm_word(m, SL.wh[tid]), nx));
          sc += tm, lmt += tm;
        }
      }
      long long pot = (long long)SL.bpot[tid];
      if (whole) {
        const int2 nd = v.nodes[boost_next<false>(v, SL.bst[tid], space)];
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
