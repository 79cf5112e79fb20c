// Streaming CTC prefix beam search with phrase boosting (k_stream_beam_boost_boost<LM>): k_stream_beam_boost (qasr_stream_beam.hip) with
// k_beam_boost's look-up (qasr_beam_boost.hip) in the candidate evaluation, the automaton state `bst` and the running bonus
// `boost_tot` of every entry kept in the slot's block between steps.  The host statement is qasr/stream_beam.py
// (STREAM_BOOST_RULES, with BOOST_RULES of qasr/boost.py for the automaton), and this file follows it byte for byte, the state
// block and the ring included.  A kernel of its own, as the house pattern has it: qasr_stream_beam.hip, qasr_beam.hip and
// qasr_beam_boost.hip stay as they are, and the helpers they keep to themselves are repeated here under sbb_ names, so that no
// existing kernel's code object changes.
//
// One work-group of 256 threads per row: k_stream_beam_boost's load / frame loop / commit round / store.  What differs:
//   * a slot's block is 16 + 24 W words: nine 64-bit arrays (k_stream_beam_boost's eight, then boost_tot), six 32-bit arrays (its
//     four, then bst, then a pad of zeros that keeps every slot's 64-bit arrays 8-byte aligned for odd W), then the ring;
//   * header word 4 holds the slot's phrase set + 1: a BEGIN row stores boost_set[row] + 1, later rows read it.  The sets
//     themselves are kernel arguments (up to 8 (pointer, bytes, whole_words) triples that the host call validated), picked
//     by a chain of compares on constant indices; the packed set stays in global memory and is read with plain vector loads;
//   * the frame's boost terms are evaluated ONCE, before the selection, by the thread that scores candidate (entry, n): one
//     bounded probe sequence of the set's hash table (an entry in the root state reads the dense root row only), then
//     (pot, bank)[s'] - the term pot[s'] - pot[s] + bank[s'] is left in L.bterm biased by 2^30.  A winner repeats its one
//     look-up for its next state.  A row whose set is 0 makes no look-up at all;
//   * the commit round moves bst and boost_tot with the survivors and settles nothing; END takes the virtual space (whole
//     words), subtracts the unfinished pot, adds the model's unfinished-word term (word mode) and re-orders ONCE, on the
//     outputs only; END rows also write end_boost_score.
// Bounds.  Every loop is bounded as in k_stream_beam_boost (W, N, F = Lg + K, the step's frames, 256) plus the set's probe bound
// (header word 8, <= the capacity).  Ring indices are (f % F) * W + r with r < W: inside the ring for any node value >= 0.
// A set is used only if its header describes exactly the bytes the host passed (128 + 16 cap + 8 nodes + 4 labels == bytes,
// cap a power of two); table indices are masked by cap - 1, root-row indices are checked against n_labels, and EVERY
// automaton state - loaded from the block, read from the table or from the root row - is clamped to 0 .. n_nodes - 1 before
// it indexes (pot, bank)[]: a corrupt block or blob can give wrong text but no access outside the slot or the blob.  A set
// word outside 0 .. n_sets reads as 0.  Global memory sees plain vector stores only, by the one work-group that owns the
// slot; LDS atomics only.
#include <climits>

#include "qasr_internal.h"

namespace qasr {

#define SBB_NEG (-(1ll << 62))
#define SBB_DMAX (16ll << 16)
#define SBB_HMUL 0x9E3779B97F4A7C15ull
#define SBB_NT 256
#define SBB_NWAVE (SBB_NT / 64)
#define SBB_W QASR_BEAM_MAX_WIDTH
#define SBB_N QASR_BEAM_MAX_CANDIDATES
#define SBB_TAB QASR_BEAM_TABLE_ENTRIES
#define SBB_K QASR_STREAM_BEAM_ROUND
#define SBB_HDR 16                // header words of a slot's block
#define SBB_ENT 24                // words per entry of a slot's block (9 x 64-bit, 6 x 32-bit)
#define SBB_SETS QASR_STREAM_BEAM_MAX_SETS
#define SBB_BOOST_MAGIC 0x31534251
#define SBB_BIAS (1ll << 30)
#define SBB_LM_MAGIC 0x314D4C51
#define SBB_LM_OOV (-1000 * 65536)
#define SBB_LM_RAWLIM 2147483647ll
#define SBB_LM_NOTERM INT_MIN
// the stream block of qasr_stream.hip (read-only here)
#define SBB_ST_WORDS 80
#define SBB_ST_RECV 0
#define SBB_ST_DONE 2

struct SbbP {
  int32_t* bstate;
  const int32_t* sstate;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* cand_id;     // [B][Tw][N]
  const int32_t* cand_q;
  const int32_t* enc_lens;
  const int32_t* first_frame;
  const uint16_t* tab;
  int32_t* labels;            // [B][P]
  int32_t* frames;
  int32_t* n_new_labels;      // [B]
  int32_t* commit_len;
  int32_t* n_live;
  int32_t* status;
  int32_t* tail_labels;       // [B][Ptail]
  int32_t* tail_n;
  int32_t* end_labels;        // [B][n_best][Pend]
  int32_t* end_n_labels;      // [B][n_best]
  long long* end_score;
  long long* end_lm_score;    // with a model
  int32_t* n_hyps;
  const int* lm;
  long long lm_bytes, alpha_q, beta_q;
  long long slot_words;
  int space;
  int S, Tw, N, W, F, Lg, K, n_best, blank, P, Ptail, Pend, Rr, spf;
  const int32_t* boost_set;   // [B]
  long long* end_boost_score; // [B][n_best]
  const int* set[SBB_SETS];
  long long set_bytes[SBB_SETS];
  int set_whole[SBB_SETS];
  int n_sets;
};

struct SbbState {            // one side of the double buffer
  long long pb[SBB_W], pnb[SBB_W], sc[SBB_W];
  unsigned long long hash[SBB_W], phash[SBB_W];
  long long own[SBB_W], lmt[SBB_W];
  unsigned long long wh[SBB_W];
  int len[SBB_W], last[SBB_W], node[SBB_W], ctx[SBB_W];
  long long bt[SBB_W];        // boost_tot
  int bst[SBB_W];
};

template <bool LM>
struct SbbLds {
  uint16_t tab[SBB_TAB];
  SbbState st[2];
  long long k_pb[SBB_W], k_pnb[SBB_W], k_sc[SBB_W];
  unsigned long long sel_r[SBB_W];
  int sel_idx[SBB_W];
  unsigned long long child[SBB_W];
  int cid[SBB_N], cq[SBB_N];
  unsigned hist[256];
  long long red_max[SBB_NWAVE], red_min[SBB_NWAVE];
  int red_cnt[SBB_NWAVE], red_a[SBB_NWAVE];
  int bin, kk, n_at, n_sel;
  int old[SBB_W * SBB_K];       // a round: entry e's labels created at or before h, newest first
  int old_fr[SBB_K];           // entry 0's creation frames
  int old_m[SBB_W];
  int raw[LM ? SBB_W * SBB_N : 1];
  unsigned bterm[SBB_W * SBB_N];
};

struct SbbBoostView {
  const int4* table;        // [mask + 1] node, label, next, 0
  const int2* nodes;        // [n_nodes] pot_q, bank_q
  const int* root_next;     // [n_labels]
  int probe, n_labels, n_nodes;
  unsigned mask;
};

struct SbbLmView {
  const int4* trans;
  const int4* words;
  const int2* nodes;
  const int* l2w;
  int order, tprobe, wprobe, n_labels;
  unsigned tmask, wmask;
};

__device__ __forceinline__ long long sbb_lae(long long a, long long b, const uint16_t* tab) {
  const long long m = a > b ? a : b, n = a > b ? b : a;
  if (n == SBB_NEG) return m;
  const long long d = m - n;
  if (d >= SBB_DMAX) return m;
  return m + (long long)tab[d >> 6];
}

__device__ __forceinline__ int sbb_lm_walk(const SbbLmView& m, int ctx, int w, int& next) {
  next = 0;
  if (w < 0) return SBB_LM_OOV;
  long long acc = 0;
  int node = ctx;
  for (int it = 0; it < m.order; ++it) {
    unsigned long long x = (((unsigned long long)(unsigned)node << 32) | (unsigned long long)(unsigned)w) * SBB_HMUL;
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
  acc = acc > SBB_LM_RAWLIM ? SBB_LM_RAWLIM : acc;
  acc = acc < -SBB_LM_RAWLIM ? -SBB_LM_RAWLIM : acc;
  return (int)acc;
}

__device__ __forceinline__ int sbb_lm_word(const SbbLmView& m, unsigned long long h) {
  unsigned s = (unsigned)h & m.wmask;
  for (int pr = 0; pr < m.wprobe; ++pr) {
    const int4 e = m.words[s];
    if (e.z < 0) return -1;
    if ((unsigned)e.x == (unsigned)h && (unsigned)e.y == (unsigned)(h >> 32)) return e.z;
    s = (s + 1) & m.wmask;
  }
  return -1;
}

// delta(s, c) as k_beam_boost's boost_next, the result clamped into the nodes
__device__ __forceinline__ int sbb_next(const SbbBoostView& v, int s, int c) {
  if (c < 0 || c >= v.n_labels) return 0;
  int rn = v.root_next[c];
  rn = (unsigned)rn < (unsigned)v.n_nodes ? rn : 0;
  if (s == 0) return rn;
  unsigned long long x = (((unsigned long long)(unsigned)s << 32) | (unsigned long long)(unsigned)c) * SBB_HMUL;
  x ^= x >> 32;
  unsigned k = (unsigned)x & v.mask;
  for (int pr = 0; pr < v.probe; ++pr) {
    const int4 e = v.table[k];
    if (e.x == s && e.y == c) return (unsigned)e.z < (unsigned)v.n_nodes ? e.z : 0;
    if (e.x < 0) break;
    k = (k + 1) & v.mask;
  }
  return rn;
}

template <bool LM>
__global__ void __launch_bounds__(SBB_NT) k_stream_beam_boost(SbbP p) {
  __shared__ SbbLds<LM> L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, N = p.N, W = p.W, N1 = N + 1, blank = p.blank, F = p.F, P = p.P;
  const size_t row = (size_t)b * P;
  const int slot = p.slots[b];
  const bool slot_ok = slot >= 0 && slot < p.S;
  const int32_t* const sblk = p.sstate + (long long)(slot_ok ? slot : 0) * SBB_ST_WORDS;
  int32_t* const bblk = p.bstate + (long long)(slot_ok ? slot : 0) * p.slot_words;
  int2* const ring = reinterpret_cast<int2*>(bblk + SBB_HDR + SBB_ENT * W);   // [F][W]
  const int fl = p.flags[b];
  const bool begin = (fl & QASR_STREAM_BEGIN) != 0, end = (fl & QASR_STREAM_END) != 0;
  long long r = *(const long long*)(sblk + SBB_ST_RECV);
  r = r < 0 ? 0 : r;
  const int first = p.first_frame[b];
  const int e_len = min(max(p.enc_lens[b], 0), p.Tw);
  const int lo = sblk[SBB_ST_DONE];
  const long long top = (long long)first + e_len;
  const long long lim = r >= p.Rr ? (r - p.Rr) / p.spf : -1;
  const long long hi64 = end ? max((long long)lo, top) : max((long long)lo, min(top, lim));
  const int hi = (int)min(hi64, (long long)INT_MAX);
  const int nb0 = bblk[0], commit0 = bblk[1], done0 = bblk[2], started = bblk[3];
  int status = 0;
  if (!slot_ok) status = 2;
  else if (lo < first || first < 0) status = 1;
  else if ((begin ? 0 : done0) != lo) status = 3;
  else if ((long long)hi * W > (long long)INT_MAX) status = 4;
  else if (begin && (p.boost_set[b] < -1 || p.boost_set[b] >= p.n_sets)) status = 5;
  const int nbest = p.n_best;
  int32_t* const elab = p.end_labels + (size_t)b * nbest * p.Pend;
  // END rows of a step that is none, and of hypotheses that do not exist
  auto end_rows_empty = [&](int from) {
    for (int i = from * p.Pend + tid; i < nbest * p.Pend; i += SBB_NT) elab[i] = blank;
    for (int h = from + tid; h < nbest; h += SBB_NT) {
      p.end_n_labels[(size_t)b * nbest + h] = 0;
      p.end_score[(size_t)b * nbest + h] = SBB_NEG;
      if (LM) p.end_lm_score[(size_t)b * nbest + h] = 0;
      p.end_boost_score[(size_t)b * nbest + h] = 0;
    }
  };
  if (status != 0) {                                  // an empty step, the state untouched (uniform: every thread read the same)
    for (int i = tid; i < P; i += SBB_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    for (int i = tid; i < p.Ptail; i += SBB_NT) p.tail_labels[(size_t)b * p.Ptail + i] = blank;
    end_rows_empty(0);
    if (tid == 0) {
      p.n_new_labels[b] = 0, p.commit_len[b] = 0, p.n_live[b] = 0, p.status[b] = status, p.tail_n[b] = 0, p.n_hyps[b] = 0;
    }
    return;
  }
  // the model (validated on the host by qasr_lm_check), as k_beam_lm reads it
  SbbLmView m{};
  bool word_mode = false, model_ok = true;
  const int space = p.space;
  const long long alpha_q = p.alpha_q, beta_q = p.beta_q;
  int lm_start = 0;
  if (LM) {
    const int* const hdr = p.lm;
    m.order = hdr[2], m.tprobe = hdr[7], m.wprobe = hdr[10], m.n_labels = hdr[8];
    m.tmask = (unsigned)hdr[6] - 1u, m.wmask = (unsigned)hdr[9] - 1u;
    m.trans = reinterpret_cast<const int4*>(hdr + 32);
    m.words = m.trans + (size_t)hdr[6];
    m.nodes = reinterpret_cast<const int2*>(m.words + (size_t)hdr[9]);
    m.l2w = reinterpret_cast<const int*>(m.nodes + (size_t)hdr[4]);
    word_mode = hdr[3] != 0;
    model_ok = hdr[0] == SBB_LM_MAGIC && (long long)hdr[12] == p.lm_bytes && word_mode == (space >= 0) &&
               hdr[5] >= 0 && hdr[5] < hdr[4] && m.order >= 1 && m.order <= 6;
    lm_start = model_ok ? hdr[5] : 0;
  }
  auto lm_term = [&](int raw) -> long long {
    return raw == SBB_LM_NOTERM ? 0ll : ((((long long)raw * alpha_q + 32768ll) >> 16) + beta_q);
  };
  // the slot's phrase set: header word 4 (a BEGIN row: the input), 0 or a word out of range: no boosting
  int gset = begin ? p.boost_set[b] + 1 : bblk[4];
  gset = gset >= 0 && gset <= p.n_sets ? gset : 0;
  SbbBoostView bv{};
  bool whole = false;
  int b_start = 0;
  if (gset > 0) {
    const int* bh = p.set[0];
    long long bbytes = p.set_bytes[0];
    int bwhole = p.set_whole[0];
#pragma unroll
    for (int g = 1; g < SBB_SETS; ++g)
      if (g == gset - 1) bh = p.set[g], bbytes = p.set_bytes[g], bwhole = p.set_whole[g];
    const int b_nodes = bh[3], b_cap = bh[7];
    b_start = bh[5];
    bv.n_labels = bh[4], bv.probe = bh[8], bv.mask = (unsigned)b_cap - 1u, bv.n_nodes = b_nodes;
    bv.table = reinterpret_cast<const int4*>(bh + 32);
    bv.nodes = reinterpret_cast<const int2*>(bv.table + (size_t)(b_cap > 0 ? b_cap : 0));
    bv.root_next = reinterpret_cast<const int*>(bv.nodes + (size_t)(b_nodes > 0 ? b_nodes : 0));
    whole = bh[6] != 0;
    // a header that does not fit the bytes given ends the search empty, as in k_beam_boost
    model_ok = model_ok && bh[0] == SBB_BOOST_MAGIC && bh[1] == 1 && (long long)bh[2] == bbytes && b_nodes >= 1 &&
               bv.n_labels >= 1 && b_cap >= 1 && (b_cap & (b_cap - 1)) == 0 && bv.probe >= 1 && bv.probe <= b_cap &&
               b_start >= 0 && b_start < b_nodes &&
               128ll + 16ll * b_cap + 8ll * b_nodes + 4ll * bv.n_labels == bbytes && whole == (bwhole != 0) &&
               (!whole || (space >= 0 && space < bv.n_labels));
    if (!model_ok) gset = 0, b_start = 0;
  }
  const bool bo = gset > 0;
  auto st_clamp = [&](int s) -> int { return bo && (unsigned)s < (unsigned)bv.n_nodes ? s : 0; };
  for (int i = tid; i < SBB_TAB; i += SBB_NT) L.tab[i] = p.tab[i];
  // ---- the slot's beam into LDS
  const bool fresh = begin || !started;
  int nb = fresh ? 1 : min(max(nb0, 0), W);
  int commit = fresh ? 0 : max(commit0, 0);
  if (!model_ok) nb = 0;
  {
    SbbState& S = L.st[0];
    const long long* const a64 = reinterpret_cast<const long long*>(bblk + SBB_HDR);
    const int32_t* const a32 = bblk + SBB_HDR + 18 * W;
    if (fresh) {
      if (tid == 0) {
        S.pb[0] = 0, S.pnb[0] = SBB_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.own[0] = 0, S.lmt[0] = 0, S.wh[0] = 0;
        S.len[0] = 0, S.last[0] = -1, S.node[0] = -1, S.ctx[0] = lm_start;
        S.bt[0] = 0, S.bst[0] = b_start;
      }
    } else if (tid < nb) {
      S.pb[tid] = a64[tid], S.pnb[tid] = a64[W + tid], S.sc[tid] = a64[2 * W + tid];
      S.hash[tid] = (unsigned long long)a64[3 * W + tid], S.phash[tid] = (unsigned long long)a64[4 * W + tid];
      S.own[tid] = a64[5 * W + tid], S.lmt[tid] = a64[6 * W + tid], S.wh[tid] = (unsigned long long)a64[7 * W + tid];
      S.len[tid] = a32[tid], S.last[tid] = a32[W + tid], S.node[tid] = a32[2 * W + tid], S.ctx[tid] = a32[3 * W + tid];
      S.bt[tid] = a64[8 * W + tid], S.bst[tid] = st_clamp(a32[4 * W + tid]);
    }
  }
  const int32_t* const gid = p.cand_id + ((size_t)b * p.Tw) * N;             // row t - first: lo >= first, hi <= first + Tw
  const int32_t* const gq = p.cand_q + ((size_t)b * p.Tw) * N;
  int pf_id = -1, pf_q = 0;
  if (tid < N && hi > lo) pf_id = gid[(size_t)(lo - first) * N + tid], pf_q = gq[(size_t)(lo - first) * N + tid];
  int cur = 0, n_new = 0;
  __syncthreads();                                    // the block has been read; the beam and the table are in LDS
  for (int t = lo; t < hi && nb > 0; ++t) {
    {
      const SbbState& S = L.st[cur];
      SbbState& D = L.st[cur ^ 1];
      if (tid < N) {
        L.cid[tid] = pf_id, L.cq[tid] = pf_q;
        if (t + 1 < hi) pf_id = gid[(size_t)(t + 1 - first) * N + tid], pf_q = gq[(size_t)(t + 1 - first) * N + tid];
      }
      if (tid < nb) L.child[tid] = 0;
      if (tid == 0) L.n_sel = 0;
      __syncthreads();
      // ---- the entries themselves (the E path adds the entry's own term: 0 without a model)
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
        const long long pbn = nbk >= 0 ? S.sc[j] + (long long)L.cq[nbk] : SBB_NEG;
        long long a = SBB_NEG, e = SBB_NEG;
        if (nl >= 0) {
          const long long ql = (long long)L.cq[nl];
          if (S.pnb[j] != SBB_NEG) a = ql + S.pnb[j];
          if (ps >= 0) {
            const long long base = S.last[ps] == c ? S.pb[ps] : S.sc[ps];
            if (base != SBB_NEG) e = ql + base + S.own[j];      // the model's term and the boost's; 0 without both
            atomicOr(&L.child[ps], 1ull << nl);
          }
        }
        const long long pnbn = sbb_lae(a, e, L.tab);
        L.k_pb[j] = pbn, L.k_pnb[j] = pnbn, L.k_sc[j] = sbb_lae(pbn, pnbn, L.tab);
      }
      __syncthreads();
      const int lg = nb > 1 ? 32 - __clz(nb - 1) : 0;
      const int tpr_lg = 8 - lg, tpr = 1 << tpr_lg;
      const int my_i = tid >> tpr_lg, my_sub = tid & (tpr - 1);
      const bool active = my_i < nb;
      const int r_last = active ? S.last[my_i] : -1;
      const long long r_pb = active ? S.pb[my_i] : SBB_NEG, r_sc = active ? S.sc[my_i] : SBB_NEG;
      const long long r_ksc = active ? L.k_sc[my_i] : SBB_NEG;
      const unsigned long long r_child = active ? L.child[my_i] : 0ull;
      const int k_end = active ? N1 : 0;
      int* const my_raw = L.raw + (LM ? my_i * N : 0);            // my_i < 128: inside raw[SBB_W * SBB_N] since N <= SBB_N
      unsigned* const my_bterm = L.bterm + my_i * N;              // (likewise)
      if (bo) {                                                   // this frame's boost terms, once (k_beam_boost)
        const int r_bst = active ? S.bst[my_i] : 0;
        const long long r_bpot = active ? (long long)bv.nodes[r_bst].x : 0ll;
        for (int k = my_sub; k < k_end; k += tpr) {
          if (k == 0) continue;
          const int n = k - 1, id = L.cid[n];
          long long bt = 0;
          if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
            const int2 nd = bv.nodes[sbb_next(bv, r_bst, id)];
            bt = (long long)nd.x - r_bpot + (long long)nd.y;
          }
          my_bterm[n] = (unsigned)(bt + SBB_BIAS);
        }
      }
      if (LM) {                                                   // this frame's terms, once (k_beam_lm)
        const int r_ctx = active ? S.ctx[my_i] : 0;
        const unsigned long long r_wh = active ? S.wh[my_i] : 0ull;
        const bool inword = r_last >= 0 && r_last != space;
        for (int k = my_sub; k < k_end; k += tpr) {
          if (k == 0) continue;
          const int n = k - 1, id = L.cid[n];
          int rw = SBB_LM_NOTERM, nx;
          if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
            if (!word_mode) rw = sbb_lm_walk(m, r_ctx, id < m.n_labels ? m.l2w[id] : -1, nx);
            else if (id == space && inword) rw = sbb_lm_walk(m, r_ctx, sbb_lm_word(m, r_wh), nx);
          }
          my_raw[n] = rw;
        }
      }
      auto cand = [&](int k) -> long long {
        if (k == 0) return r_ksc;
        const int n = k - 1, id = L.cid[n];
        if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return SBB_NEG;
        const long long base = id == r_last ? r_pb : r_sc;
        if (base == SBB_NEG) return SBB_NEG;
        return base + (long long)L.cq[n] + (LM ? lm_term(my_raw[n]) : 0ll) + (bo ? (long long)my_bterm[n] - SBB_BIAS : 0ll);
      };
      long long mx = LLONG_MIN, mn = LLONG_MAX;
      int cnt = 0;
      for (int k = my_sub; k < k_end; k += tpr) {
        const long long v = cand(k);
        if (v != SBB_NEG) { ++cnt; mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
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
      for (int w = 1; w < SBB_NWAVE; ++w) {
        mx = L.red_max[w] > mx ? L.red_max[w] : mx, mn = L.red_min[w] < mn ? L.red_min[w] : mn;
        cnt += L.red_cnt[w];
      }
      if (cnt == 0) { nb = 0; break; }               // uniform: the beam died and stays dead
      auto radix_select = [&](auto keyfn, int nbits, int& kk, int& n_at) -> unsigned long long {
        const int passes = (nbits + 7) >> 3;          // <= 8
        unsigned long long prefix = 0;
        for (int pass = passes - 1; pass >= 0; --pass) {
          const int shift = pass * 8;
          __syncthreads();
          L.hist[tid] = 0;                            // SBB_NT == 256 bins
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
          if (exc < kk && kk <= inc) L.bin = tid, L.kk = kk - exc, L.n_at = mine;      // exactly one thread
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
          const long long v = cand(k);
          key = (unsigned long long)(mx - v);
          return v != SBB_NEG;
        }, range ? 64 - __clzll((long long)range) : 0, need, n_at);
        if (n_at > need) {
          const int M = nb * N1;
          ith = (int)radix_select([&](int k, unsigned long long& key) {
            const long long v = cand(k);
            key = (unsigned long long)(my_i * N1 + k);
            return v != SBB_NEG && (unsigned long long)(mx - v) == rth;
          }, 32 - __clz(M), need, n_at);
        }
      }
      for (int k = my_sub; k < k_end; k += tpr) {
        const long long v = cand(k);
        if (v != SBB_NEG) {
          const unsigned long long rr = (unsigned long long)(mx - v);
          const int idx = my_i * N1 + k;
          if (rr < rth || (rr == rth && idx <= ith)) {
            const int at = atomicAdd(&L.n_sel, 1);
            if (at < SBB_W) L.sel_r[at] = rr, L.sel_idx[at] = idx;
          }
        }
      }
      __syncthreads();
      const int ns = min(L.n_sel, W);
      if (tid < ns) {
        const unsigned long long rr = L.sel_r[tid];
        const int idx = L.sel_idx[tid];
        int rank = 0;
        for (int mm = 0; mm < ns; ++mm) {
          const unsigned long long rm = L.sel_r[mm];
          rank += (rm < rr || (rm == rr && L.sel_idx[mm] < idx)) ? 1 : 0;
        }
        const int i = idx / N1, k = idx - i * N1;
        if (k == 0) {
          D.pb[rank] = L.k_pb[i], D.pnb[rank] = L.k_pnb[i], D.sc[rank] = L.k_sc[i];
          D.hash[rank] = S.hash[i], D.phash[rank] = S.phash[i], D.len[rank] = S.len[i], D.last[rank] = S.last[i];
          D.node[rank] = S.node[i];
          D.own[rank] = S.own[i], D.lmt[rank] = S.lmt[i], D.wh[rank] = S.wh[i], D.ctx[rank] = S.ctx[i];
          D.bt[rank] = S.bt[i], D.bst[rank] = S.bst[i];
        } else {
          const int c = L.cid[k - 1];
          const long long v = mx - (long long)rr;
          unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * SBB_HMUL;
          x ^= x >> 32;
          D.pb[rank] = SBB_NEG, D.pnb[rank] = v, D.sc[rank] = v;
          D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
          D.node[rank] = t * W + rank;                // <= hi * W - 1 <= INT_MAX - 1 (status 4 otherwise)
          ring[(size_t)(t % F) * W + rank] = make_int2(S.node[i], c);
          if (LM) {
            const int raw = L.raw[i * N + k - 1];
            const long long tm = lm_term(raw);
            int ctx = S.ctx[i];
            unsigned long long wh = 0;
            if (word_mode && c != space) {
              wh = (S.wh[i] ^ ((unsigned long long)(long long)c + 1ull)) * SBB_HMUL;
              wh ^= wh >> 32;
            } else if (raw != SBB_LM_NOTERM) {
              const int w = word_mode ? sbb_lm_word(m, S.wh[i]) : (c < m.n_labels ? m.l2w[c] : -1);
              sbb_lm_walk(m, S.ctx[i], w, ctx);
            }
            D.own[rank] = tm, D.lmt[rank] = S.lmt[i] + tm, D.wh[rank] = wh, D.ctx[rank] = ctx;
          } else {
            D.own[rank] = 0, D.lmt[rank] = 0, D.wh[rank] = 0, D.ctx[rank] = 0;
          }
          if (bo) {                                   // written before the barriers of the selection
            const long long btm = (long long)L.bterm[i * N + k - 1] - SBB_BIAS;
            D.own[rank] += btm, D.bt[rank] = S.bt[i] + btm;
            D.bst[rank] = sbb_next(bv, S.bst[i], c);   // the one look-up again, for the next state
          } else {
            D.bt[rank] = 0, D.bst[rank] = 0;
          }
        }
      }
      __syncthreads();                                // the next beam and this frame's ring row are visible to the work-group
      nb = ns, cur ^= 1;
    }
    // ---- the commit round
    if ((t + 1) % p.K == 0 && t >= p.Lg) {
      const SbbState& S = L.st[cur];
      SbbState& D = L.st[cur ^ 1];
      const int h = t - p.Lg;
      if (tid < nb) {
        int nd = S.node[tid], mo = 0;
        const int u = min(max(S.len[tid] - commit, 0), F);      // uncommitted labels: at most F (the plan)
        for (int k = 0; k < u && nd >= 0; ++k) {
          const int f = nd / W, rk = nd - f * W;
          const int2 e = ring[(size_t)(f % F) * W + rk];
          if (f <= h) {
            if (mo < SBB_K) {
              L.old[tid * SBB_K + mo] = e.y;
              if (tid == 0) L.old_fr[mo] = f;
            }
            ++mo;
          }
          nd = e.x;
        }
        L.old_m[tid] = mo;
      }
      __syncthreads();
      const int m0 = min(L.old_m[0], SBB_K);           // at most K by the plan
      bool keep = false;
      if (tid < nb) {
        keep = L.old_m[tid] == m0;
        for (int k = 0; k < m0; ++k) keep = keep && L.old[tid * SBB_K + k] == L.old[k];
        keep = keep || tid == 0;
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) L.red_a[wave] = __popcll(bal);
      __syncthreads();
      int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < SBB_NWAVE; ++w) {
        pos += w < wave ? L.red_a[w] : 0;
        total += L.red_a[w];
      }
      if (keep) {
        D.pb[pos] = S.pb[tid], D.pnb[pos] = S.pnb[tid], D.sc[pos] = S.sc[tid], D.hash[pos] = S.hash[tid];
        D.phash[pos] = S.phash[tid], D.own[pos] = S.own[tid], D.lmt[pos] = S.lmt[tid], D.wh[pos] = S.wh[tid];
        D.len[pos] = S.len[tid], D.last[pos] = S.last[tid], D.node[pos] = S.node[tid], D.ctx[pos] = S.ctx[tid];
        D.bt[pos] = S.bt[tid], D.bst[pos] = S.bst[tid];
      }
      if (tid < m0) {                                 // the delta, oldest first
        const int at = n_new + (m0 - 1 - tid);
        if (at < P) p.labels[row + at] = L.old[tid], p.frames[row + at] = L.old_fr[tid];
      }
      __syncthreads();
      nb = total, cur ^= 1, commit += m0, n_new += m0;
    }
  }
  __syncthreads();
  // ---- the beam back into the slot's block (before END re-orders it)
  {
    const SbbState& S = L.st[cur];
    long long* const a64 = reinterpret_cast<long long*>(bblk + SBB_HDR);
    int32_t* const a32 = bblk + SBB_HDR + 18 * W;
    if (tid < W) {
      const bool lv = tid < nb;
      a64[tid] = lv ? S.pb[tid] : 0, a64[W + tid] = lv ? S.pnb[tid] : 0, a64[2 * W + tid] = lv ? S.sc[tid] : 0;
      a64[3 * W + tid] = lv ? (long long)S.hash[tid] : 0, a64[4 * W + tid] = lv ? (long long)S.phash[tid] : 0;
      a64[5 * W + tid] = lv ? S.own[tid] : 0, a64[6 * W + tid] = lv ? S.lmt[tid] : 0;
      a64[7 * W + tid] = lv ? (long long)S.wh[tid] : 0;
      a32[tid] = lv ? S.len[tid] : 0, a32[W + tid] = lv ? S.last[tid] : 0, a32[2 * W + tid] = lv ? S.node[tid] : 0;
      a32[3 * W + tid] = lv ? S.ctx[tid] : 0;
      a64[8 * W + tid] = lv ? S.bt[tid] : 0, a32[4 * W + tid] = lv ? S.bst[tid] : 0, a32[5 * W + tid] = 0;
    }
    if (tid < SBB_HDR) bblk[tid] = tid == 0 ? nb : tid == 1 ? commit : tid == 2 ? hi : tid == 3 ? 1 : tid == 4 ? gset : 0;
  }
  int32_t* const tl = p.tail_labels + (size_t)b * p.Ptail;
  if (!end) {
    // ---- the provisional tail: the best entry's uncommitted labels, oldest first
    const SbbState& S = L.st[cur];
    const int u = nb > 0 ? min(max(S.len[0] - commit, 0), F) : 0;
    if (tid == 0) {
      int nd = nb > 0 ? S.node[0] : -1;
      for (int k = 0; k < u && nd >= 0; ++k) {
        const int f = nd / W, rk = nd - f * W;
        const int2 e = ring[(size_t)(f % F) * W + rk];
        const int at = u - 1 - k;
        if (at < p.Ptail) tl[at] = e.y;
        nd = e.x;
      }
      p.tail_n[b] = u;
    }
    for (int i = min(u, p.Ptail) + tid; i < p.Ptail; i += SBB_NT) tl[i] = blank;
    end_rows_empty(0);
    for (int i = min(n_new, P) + tid; i < P; i += SBB_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    if (tid == 0) {
      p.n_new_labels[b] = min(n_new, P), p.commit_len[b] = commit, p.n_live[b] = nb, p.status[b] = 0, p.n_hyps[b] = 0;
    }
    return;
  }
  // ---- END: word mode scores the unfinished word of every entry, a boosted slot takes the virtual space (whole words) and
  // loses its unfinished pot; then ONE re-ordering (score descending, ties by the previous rank)
  const int n_live = nb;
  if (((LM && word_mode) || bo) && nb > 0) {
    const SbbState& S = L.st[cur];
    SbbState& D = L.st[cur ^ 1];
    long long sc = SBB_NEG, lmt = 0, bt = 0;
    if (tid < nb) {
      sc = S.sc[tid], lmt = S.lmt[tid], bt = S.bt[tid];
      const int last = S.last[tid];
      if (LM && word_mode && last >= 0 && last != space) {
        int nx;
        const long long tm = lm_term(sbb_lm_walk(m, S.ctx[tid], sbb_lm_word(m, S.wh[tid]), nx));
        sc += tm, lmt += tm;
      }
      if (bo) {
        long long pot = (long long)bv.nodes[S.bst[tid]].x;
        if (whole) {
          const int2 nd = bv.nodes[sbb_next(bv, S.bst[tid], space)];
          const long long tm = (long long)nd.x - pot + (long long)nd.y;
          sc += tm, bt += tm, pot = (long long)nd.x;
        }
        sc -= pot, bt -= pot;
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
      D.sc[rank] = sc, D.lmt[rank] = lmt, D.bt[rank] = bt, D.len[rank] = S.len[tid], D.node[rank] = S.node[tid];
    }
    __syncthreads();
    cur ^= 1;
  }
  {
    const SbbState& S = L.st[cur];
    const int nh = min(nb, nbest);
    const int u0 = nh > 0 ? min(max(S.len[0] - commit, 0), F) : 0;
    for (int i = tid; i < nh * p.Pend; i += SBB_NT) elab[i] = blank;
    end_rows_empty(nh);
    for (int i = tid; i < p.Ptail; i += SBB_NT) tl[i] = blank;
    for (int i = min(n_new + u0, P) + tid; i < P; i += SBB_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    __syncthreads();                                  // the fills above are behind every walk's stores
    if (tid < nh) {
      const int hh = tid;
      const int u = min(max(S.len[hh] - commit, 0), F);
      int nd = S.node[hh];
      for (int k = 0; k < u && nd >= 0; ++k) {
        const int f = nd / W, rk = nd - f * W;
        const int2 e = ring[(size_t)(f % F) * W + rk];
        const int at = u - 1 - k;
        if (at < p.Pend) elab[(size_t)hh * p.Pend + at] = e.y;
        if (hh == 0 && n_new + at < P) p.labels[row + n_new + at] = e.y, p.frames[row + n_new + at] = f;
        nd = e.x;
      }
      p.end_n_labels[(size_t)b * nbest + hh] = u;
      p.end_score[(size_t)b * nbest + hh] = S.sc[hh];
      if (LM) p.end_lm_score[(size_t)b * nbest + hh] = S.lmt[hh];
      p.end_boost_score[(size_t)b * nbest + hh] = S.bt[hh];
    }
    if (tid == 0) {
      p.n_new_labels[b] = min(n_new + u0, P), p.commit_len[b] = commit + u0, p.n_live[b] = n_live, p.status[b] = 0;
      p.tail_n[b] = 0, p.n_hyps[b] = nh;
    }
  }
}

size_t stream_beam_boost_state_bytes(int S, int W, int F) {
  if (S < 1 || W < 1 || W > QASR_BEAM_MAX_WIDTH || F < 1 || F > QASR_STREAM_BEAM_MAX_RING) return 0;
  return (size_t)S * 4 * ((size_t)SBB_HDR + SBB_ENT * (size_t)W + 2 * (size_t)F * (size_t)W);
}

int launch_stream_beam_boost(hipStream_t s, const qasr_stream_beam_boost_args& q) {
  const qasr_stream_beam_args& a = q.beam;
  SbbP p{};
  p.bstate = (int32_t*)a.beam_state, p.sstate = (const int32_t*)a.state, p.slots = a.slots, p.flags = a.flags;
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.enc_lens = a.enc_lens, p.first_frame = a.first_frame, p.tab = a.lae_table;
  p.labels = a.labels, p.frames = a.frames, p.n_new_labels = a.n_new_labels, p.commit_len = a.commit_len, p.n_live = a.n_live;
  p.status = a.status, p.tail_labels = a.tail_labels, p.tail_n = a.tail_n;
  p.end_labels = a.end_labels, p.end_n_labels = a.end_n_labels, p.end_score = (long long*)a.end_score;
  p.end_lm_score = (long long*)a.end_lm_score, p.n_hyps = a.n_hyps;
  p.lm = (const int*)a.lm, p.lm_bytes = (long long)a.lm_bytes, p.alpha_q = a.alpha_q, p.beta_q = a.beta_q, p.space = a.space;
  p.slot_words = SBB_HDR + (long long)SBB_ENT * a.beam_width + 2ll * a.F * a.beam_width;
  p.S = a.S, p.Tw = a.Tw, p.N = a.N, p.W = a.beam_width, p.F = a.F, p.Lg = a.Lg, p.K = a.K, p.n_best = a.n_best, p.blank = a.blank;
  p.P = a.P, p.Ptail = a.Ptail, p.Pend = a.Pend, p.Rr = a.Rr, p.spf = a.samples_per_frame;
  p.boost_set = q.boost_set, p.end_boost_score = (long long*)q.end_boost_score, p.n_sets = q.n_sets;
  for (int g = 0; g < SBB_SETS; ++g) {              // unused triples repeat set 0, so that every argument is a valid set
    const int k = g < q.n_sets ? g : 0;
    p.set[g] = (const int*)q.sets[k], p.set_bytes[g] = (long long)q.set_bytes[k], p.set_whole[g] = q.whole_words[k];
  }
  static_assert(sizeof(SbbLds<true>) <= 160 * 1024, "k_stream_beam_boost: the LDS of one gfx950 CU");
  if (a.lm) hipLaunchKernelGGL(k_stream_beam_boost<true>, dim3((unsigned)a.B), dim3(SBB_NT), 0, s, p);
  else hipLaunchKernelGGL(k_stream_beam_boost<false>, dim3((unsigned)a.B), dim3(SBB_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
