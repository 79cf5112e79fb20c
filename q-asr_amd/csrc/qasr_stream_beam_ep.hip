// Streaming beam endpointing (k_stream_beam_ep<LM, BOOST>): the streaming prefix beam search of k_stream_beam / k_stream_beam_boost
// for sessions that k_stream_endpoint cuts into utterances.  The host statement is qasr/stream_beam.py (STREAM_BEAM_EP_RULES
// over STREAM_BEAM_RULES / STREAM_BOOST_RULES), and this file follows it byte for byte, the state block and the ring included.
// The one beam kernel that keeps its own copy (sbe_ names) of the helpers, the selection and the body: on qasr_beam_dev.h
// alone, and on the body of qasr_stream_beam_dev.h, its boosted instantiations measured past the 3 % margin.
//
// One work-group of 256 threads per row, launched AFTER k_stream_emit and k_stream_endpoint of the same rows: lo is the beam
// block's own frames_done (0 on BEGIN), hi the stream block's frames_done as emit left it, and the step's records are read
// only.  Load, frame step, commit round and store are k_stream_beam's (BOOST: k_stream_beam_boost's, the slot block then
// 16 + 24 W words instead of 16 + 20 W).  What differs:
//   * the walk covers ALL of [lo, hi) even while the beam is dead: the frame step and the round are skipped, the cuts are not;
//   * after the round of frame t every unread record with end == t + 1 is a CUT (behind the loop: those with end == hi on a
//     row without frames): the END pass of the rules on the outputs of that cut (unfinished word, boost END pass, ONE
//     re-ordering), the first n_best entries written as suffixes behind commit_len, the best one also appended to the step's
//     delta (cut_delta_end: the delta's length after the cut), then the beam is the single fresh entry again (commit_len 0,
//     LM context at the model's start, boost state at the start of the slot's set, which survives) - alive again unless the
//     model blob is invalid;
//   * header word 5 counts the cuts done; a step whose first record carries another index is out of sync (status 3);
//   * nodes stay t * W + r in ring row t % F and the round phase stays global, so any slicing gives the same bytes.
// Bounds.  Every loop is bounded by W, N, F = Lg + K, E, the step's frames, 256 or the set's probe bound.  Candidates are read
// at rows t - first with first <= lo <= t < hi <= first + enc_len <= first + Tw (statuses 1 and 3 otherwise).  Ring indices
// are (f % F) * W + r with r < W: inside the ring for any node value >= 0.  Cut outputs are indexed by k < n_records <= E
// (status 3 otherwise).  A set is used only if its header describes exactly the bytes the host passed; every automaton state
// is clamped to 0 .. n_nodes - 1 before it indexes (pot, bank)[].  Global memory sees plain vector stores only, by the one
// work-group that owns the slot; LDS atomics only.
#include <climits>

#include "qasr_internal.h"

namespace qasr {

#define SBE_NEG (-(1ll << 62))
#define SBE_DMAX (16ll << 16)
#define SBE_HMUL 0x9E3779B97F4A7C15ull
#define SBE_NT 256
#define SBE_NWAVE (SBE_NT / 64)
#define SBE_W QASR_BEAM_MAX_WIDTH
#define SBE_N QASR_BEAM_MAX_CANDIDATES
#define SBE_TAB QASR_BEAM_TABLE_ENTRIES
#define SBE_K QASR_STREAM_BEAM_ROUND
#define SBE_HDR 16                // header words of a slot's block
#define SBE_REC 10                // words of one endpoint record (index, first, end, ...)
#define SBE_SETS QASR_STREAM_BEAM_MAX_SETS
#define SBE_BOOST_MAGIC 0x31534251
#define SBE_BIAS (1ll << 30)
#define SBE_LM_MAGIC 0x314D4C51
#define SBE_LM_OOV (-1000 * 65536)
#define SBE_LM_RAWLIM 2147483647ll
#define SBE_LM_NOTERM INT_MIN
// the stream block of qasr_stream.hip (read-only here)
#define SBE_ST_WORDS 80
#define SBE_ST_DONE 2

struct SbeP {
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
  const int32_t* records;     // [B][E][10], k_stream_endpoint's of the same step
  const int32_t* n_records;   // [B]
  const int32_t* ep_status;   // [B]
  int32_t* n_cuts;            // [B]
  int32_t* cut_n_hyps;        // [B][E]
  int32_t* cut_delta_end;     // [B][E]
  int32_t* cut_labels;        // [B][E][n_best][Pend]
  int32_t* cut_n_labels;      // [B][E][n_best]
  long long* cut_score;
  long long* cut_lm_score;    // with a model
  long long* cut_boost_score; // boosted
  const int* lm;
  long long lm_bytes, alpha_q, beta_q;
  long long slot_words;
  int space;
  int S, Tw, N, W, F, Lg, K, n_best, blank, P, Ptail, Pend, E;
  const int32_t* boost_set;   // [B]
  const int* set[SBE_SETS];
  long long set_bytes[SBE_SETS];
  int set_whole[SBE_SETS];
  int n_sets;
};

struct SbeState {            // one side of the double buffer
  long long pb[SBE_W], pnb[SBE_W], sc[SBE_W];
  unsigned long long hash[SBE_W], phash[SBE_W];
  long long own[SBE_W], lmt[SBE_W];
  unsigned long long wh[SBE_W];
  int len[SBE_W], last[SBE_W], node[SBE_W], ctx[SBE_W];
  long long bt[SBE_W];        // boost_tot
  int bst[SBE_W];
};

template <bool LM, bool BOOST>
struct SbeLds {
  uint16_t tab[SBE_TAB];
  SbeState st[2];
  long long k_pb[SBE_W], k_pnb[SBE_W], k_sc[SBE_W];
  unsigned long long sel_r[SBE_W];
  int sel_idx[SBE_W];
  unsigned long long child[SBE_W];
  int cid[SBE_N], cq[SBE_N];
  unsigned hist[256];
  long long red_max[SBE_NWAVE], red_min[SBE_NWAVE];
  int red_cnt[SBE_NWAVE], red_a[SBE_NWAVE];
  int bin, kk, n_at, n_sel;
  int old[SBE_W * SBE_K];       // a round: entry e's labels created at or before h, newest first
  int old_fr[SBE_K];           // entry 0's creation frames
  int old_m[SBE_W];
  int raw[LM ? SBE_W * SBE_N : 1];
  unsigned bterm[BOOST ? SBE_W * SBE_N : 1];
};

struct SbeBoostView {
  const int4* table;        // [mask + 1] node, label, next, 0
  const int2* nodes;        // [n_nodes] pot_q, bank_q
  const int* root_next;     // [n_labels]
  int probe, n_labels, n_nodes;
  unsigned mask;
};

struct SbeLmView {
  const int4* trans;
  const int4* words;
  const int2* nodes;
  const int* l2w;
  int order, tprobe, wprobe, n_labels;
  unsigned tmask, wmask;
};

__device__ __forceinline__ long long sbe_lae(long long a, long long b, const uint16_t* tab) {
  const long long m = a > b ? a : b, n = a > b ? b : a;
  if (n == SBE_NEG) return m;
  const long long d = m - n;
  if (d >= SBE_DMAX) return m;
  return m + (long long)tab[d >> 6];
}

__device__ __forceinline__ int sbe_lm_walk(const SbeLmView& m, int ctx, int w, int& next) {
  next = 0;
  if (w < 0) return SBE_LM_OOV;
  long long acc = 0;
  int node = ctx;
  for (int it = 0; it < m.order; ++it) {
    unsigned long long x = (((unsigned long long)(unsigned)node << 32) | (unsigned long long)(unsigned)w) * SBE_HMUL;
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
  acc = acc > SBE_LM_RAWLIM ? SBE_LM_RAWLIM : acc;
  acc = acc < -SBE_LM_RAWLIM ? -SBE_LM_RAWLIM : acc;
  return (int)acc;
}

__device__ __forceinline__ int sbe_lm_word(const SbeLmView& m, unsigned long long h) {
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
__device__ __forceinline__ int sbe_next(const SbeBoostView& v, int s, int c) {
  if (c < 0 || c >= v.n_labels) return 0;
  int rn = v.root_next[c];
  rn = (unsigned)rn < (unsigned)v.n_nodes ? rn : 0;
  if (s == 0) return rn;
  unsigned long long x = (((unsigned long long)(unsigned)s << 32) | (unsigned long long)(unsigned)c) * SBE_HMUL;
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

template <bool LM, bool BOOST>
__global__ void __launch_bounds__(SBE_NT) k_stream_beam_ep(SbeP p) {
  __shared__ SbeLds<LM, BOOST> L;
  constexpr int ENT = BOOST ? 24 : 20;            // words per entry of a slot's block: 8 (9) 64-bit arrays, 4 (6) 32-bit arrays
  constexpr int A32 = BOOST ? 18 : 16;            // the 32-bit arrays begin behind the 64-bit ones
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, N = p.N, W = p.W, N1 = N + 1, blank = p.blank, F = p.F, P = p.P;
  const size_t row = (size_t)b * P;
  const int slot = p.slots[b];
  const bool slot_ok = slot >= 0 && slot < p.S;
  const int32_t* const sblk = p.sstate + (long long)(slot_ok ? slot : 0) * SBE_ST_WORDS;
  int32_t* const bblk = p.bstate + (long long)(slot_ok ? slot : 0) * p.slot_words;
  int2* const ring = reinterpret_cast<int2*>(bblk + SBE_HDR + ENT * W);   // [F][W]
  const int fl = p.flags[b];
  const bool begin = (fl & QASR_STREAM_BEGIN) != 0, end = (fl & QASR_STREAM_END) != 0;
  (void)end;                                          // END shows in the records only: its cut is the END record's
  const int first = p.first_frame[b];
  const int e_len = min(max(p.enc_lens[b], 0), p.Tw);
  const int nb0 = bblk[0], commit0 = bblk[1], done0 = bblk[2], started = bblk[3];
  const int lo = begin ? 0 : done0;                   // this block's frames_done
  const int hi = sblk[SBE_ST_DONE];                   // the stream block's, as emit left it
  const int E = p.E, nrec = p.n_records[b];
  const int cuts0 = begin ? 0 : bblk[5];              // cuts done so far
  const int32_t* const rec = p.records + (size_t)b * E * SBE_REC;
  int status = 0;
  if (!slot_ok) status = 2;
  else if (lo < first || first < 0) status = 1;
  else {
    bool bad = lo > hi || (lo < hi && (long long)hi > (long long)first + e_len) || nrec < 0 || nrec > E || p.ep_status[b] != 0;
    if (!bad && nrec > 0) {
      bad = rec[0] != cuts0;
      int prev = lo;
      for (int k = 0; k < nrec; ++k) {                // ends rise (they may repeat) inside (lo, hi]; end == lo only without frames
        const int en = rec[k * SBE_REC + 2];
        bad = bad || en < prev || en > hi || (en == lo && lo < hi);
        prev = en;
      }
    }
    if (bad) status = 3;
    else if ((long long)hi * W > (long long)INT_MAX) status = 4;
    else if (BOOST && begin && (p.boost_set[b] < -1 || p.boost_set[b] >= p.n_sets)) status = 5;
  }
  const int nbest = p.n_best;
  // the rows of cut k from hypothesis `from` on: hypotheses that do not exist
  auto cut_rows_empty = [&](int k, int from) {
    const size_t at = ((size_t)b * E + k) * nbest;
    int32_t* const cl = p.cut_labels + at * p.Pend;
    for (int i = from * p.Pend + tid; i < nbest * p.Pend; i += SBE_NT) cl[i] = blank;
    for (int h = from + tid; h < nbest; h += SBE_NT) {
      p.cut_n_labels[at + h] = 0;
      p.cut_score[at + h] = SBE_NEG;
      if (LM) p.cut_lm_score[at + h] = 0;
      if (BOOST) p.cut_boost_score[at + h] = 0;
    }
  };
  // the cuts from k on: cuts that did not happen
  auto cuts_empty = [&](int from) {
    for (int k = from; k < E; ++k) cut_rows_empty(k, 0);
    for (int k = from + tid; k < E; k += SBE_NT) p.cut_n_hyps[(size_t)b * E + k] = 0, p.cut_delta_end[(size_t)b * E + k] = 0;
  };
  if (status != 0) {                                  // an empty step, the state untouched (uniform: every thread read the same)
    for (int i = tid; i < P; i += SBE_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    for (int i = tid; i < p.Ptail; i += SBE_NT) p.tail_labels[(size_t)b * p.Ptail + i] = blank;
    cuts_empty(0);
    if (tid == 0) {
      p.n_new_labels[b] = 0, p.commit_len[b] = 0, p.n_live[b] = 0, p.status[b] = status, p.tail_n[b] = 0, p.n_cuts[b] = 0;
    }
    return;
  }
  // the model (validated on the host by qasr_lm_check), as k_beam_lm reads it
  SbeLmView m{};
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
    model_ok = hdr[0] == SBE_LM_MAGIC && (long long)hdr[12] == p.lm_bytes && word_mode == (space >= 0) &&
               hdr[5] >= 0 && hdr[5] < hdr[4] && m.order >= 1 && m.order <= 6;
    lm_start = model_ok ? hdr[5] : 0;
  }
  auto lm_term = [&](int raw) -> long long {
    return raw == SBE_LM_NOTERM ? 0ll : ((((long long)raw * alpha_q + 32768ll) >> 16) + beta_q);
  };
  // the slot's phrase set: header word 4 (a BEGIN row: the input), 0 or a word out of range: no boosting
  int gset = !BOOST ? 0 : begin ? p.boost_set[b] + 1 : bblk[4];
  gset = gset >= 0 && gset <= p.n_sets ? gset : 0;
  SbeBoostView bv{};
  bool whole = false;
  int b_start = 0;
  if (BOOST && gset > 0) {
    const int* bh = p.set[0];
    long long bbytes = p.set_bytes[0];
    int bwhole = p.set_whole[0];
#pragma unroll
    for (int g = 1; g < SBE_SETS; ++g)
      if (g == gset - 1) bh = p.set[g], bbytes = p.set_bytes[g], bwhole = p.set_whole[g];
    const int b_nodes = bh[3], b_cap = bh[7];
    b_start = bh[5];
    bv.n_labels = bh[4], bv.probe = bh[8], bv.mask = (unsigned)b_cap - 1u, bv.n_nodes = b_nodes;
    bv.table = reinterpret_cast<const int4*>(bh + 32);
    bv.nodes = reinterpret_cast<const int2*>(bv.table + (size_t)(b_cap > 0 ? b_cap : 0));
    bv.root_next = reinterpret_cast<const int*>(bv.nodes + (size_t)(b_nodes > 0 ? b_nodes : 0));
    whole = bh[6] != 0;
    // a header that does not fit the bytes given ends the search empty, as in k_beam_boost
    model_ok = model_ok && bh[0] == SBE_BOOST_MAGIC && bh[1] == 1 && (long long)bh[2] == bbytes && b_nodes >= 1 &&
               bv.n_labels >= 1 && b_cap >= 1 && (b_cap & (b_cap - 1)) == 0 && bv.probe >= 1 && bv.probe <= b_cap &&
               b_start >= 0 && b_start < b_nodes &&
               128ll + 16ll * b_cap + 8ll * b_nodes + 4ll * bv.n_labels == bbytes && whole == (bwhole != 0) &&
               (!whole || (space >= 0 && space < bv.n_labels));
    if (!model_ok) gset = 0, b_start = 0;
  }
  const bool bo = BOOST && gset > 0;
  auto st_clamp = [&](int s) -> int { return bo && (unsigned)s < (unsigned)bv.n_nodes ? s : 0; };
  for (int i = tid; i < SBE_TAB; i += SBE_NT) L.tab[i] = p.tab[i];
  // ---- the slot's beam into LDS
  const bool fresh = begin || !started;
  int nb = fresh ? 1 : min(max(nb0, 0), W);
  int commit = fresh ? 0 : max(commit0, 0);
  if (!model_ok) nb = 0;
  {
    SbeState& S = L.st[0];
    const long long* const a64 = reinterpret_cast<const long long*>(bblk + SBE_HDR);
    const int32_t* const a32 = bblk + SBE_HDR + A32 * W;
    if (fresh) {
      if (tid == 0) {
        S.pb[0] = 0, S.pnb[0] = SBE_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.own[0] = 0, S.lmt[0] = 0, S.wh[0] = 0;
        S.len[0] = 0, S.last[0] = -1, S.node[0] = -1, S.ctx[0] = lm_start;
        S.bt[0] = 0, S.bst[0] = b_start;
      }
    } else if (tid < nb) {
      S.pb[tid] = a64[tid], S.pnb[tid] = a64[W + tid], S.sc[tid] = a64[2 * W + tid];
      S.hash[tid] = (unsigned long long)a64[3 * W + tid], S.phash[tid] = (unsigned long long)a64[4 * W + tid];
      S.own[tid] = a64[5 * W + tid], S.lmt[tid] = a64[6 * W + tid], S.wh[tid] = (unsigned long long)a64[7 * W + tid];
      S.len[tid] = a32[tid], S.last[tid] = a32[W + tid], S.node[tid] = a32[2 * W + tid], S.ctx[tid] = a32[3 * W + tid];
      if (BOOST) S.bt[tid] = a64[8 * W + tid], S.bst[tid] = st_clamp(a32[4 * W + tid]);
      else S.bt[tid] = 0, S.bst[tid] = 0;
    }
  }
  const int32_t* const gid = p.cand_id + ((size_t)b * p.Tw) * N;             // row t - first: lo >= first, hi <= first + Tw
  const int32_t* const gq = p.cand_q + ((size_t)b * p.Tw) * N;
  int pf_id = -1, pf_q = 0;
  if (tid < N && hi > lo) pf_id = gid[(size_t)(lo - first) * N + tid], pf_q = gq[(size_t)(lo - first) * N + tid];
  int cur = 0, n_new = 0, rk = 0;
  __syncthreads();                                    // the block has been read; the beam and the table are in LDS
  // ---- a cut: the END pass on the outputs of cut k, the best entry into the delta, then the fresh beam
  auto cut = [&](int k) {
    int side = cur;
    if (((LM && word_mode) || bo) && nb > 0) {        // ONE re-ordering (score descending, ties by the previous rank)
      const SbeState& S = L.st[cur];
      SbeState& D = L.st[cur ^ 1];
      long long sc = SBE_NEG, lmt = 0, bt = 0;
      if (tid < nb) {
        sc = S.sc[tid], lmt = S.lmt[tid], bt = S.bt[tid];
        const int last = S.last[tid];
        if (LM && word_mode && last >= 0 && last != space) {
          int nx;
          const long long tm = lm_term(sbe_lm_walk(m, S.ctx[tid], sbe_lm_word(m, S.wh[tid]), nx));
          sc += tm, lmt += tm;
        }
        if (bo) {
          long long pot = (long long)bv.nodes[S.bst[tid]].x;
          if (whole) {
            const int2 nd = bv.nodes[sbe_next(bv, S.bst[tid], space)];
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
      side = cur ^ 1;
    }
    {
      const SbeState& S = L.st[side];
      const int nh = min(nb, nbest);
      const int u0 = nh > 0 ? min(max(S.len[0] - commit, 0), F) : 0;
      const size_t at0 = ((size_t)b * E + k) * nbest;
      int32_t* const cl = p.cut_labels + at0 * p.Pend;
      for (int i = tid; i < nh * p.Pend; i += SBE_NT) cl[i] = blank;
      cut_rows_empty(k, nh);
      __syncthreads();                                // the fills above are behind every walk's stores
      if (tid < nh) {
        const int hh = tid;
        const int u = min(max(S.len[hh] - commit, 0), F);
        int nd = S.node[hh];
        for (int j = 0; j < u && nd >= 0; ++j) {
          const int f = nd / W, rr = nd - f * W;
          const int2 e = ring[(size_t)(f % F) * W + rr];
          const int at = u - 1 - j;
          if (at < p.Pend) cl[(size_t)hh * p.Pend + at] = e.y;
          if (hh == 0 && n_new + at < P) p.labels[row + n_new + at] = e.y, p.frames[row + n_new + at] = f;
          nd = e.x;
        }
        p.cut_n_labels[at0 + hh] = u;
        p.cut_score[at0 + hh] = S.sc[hh];
        if (LM) p.cut_lm_score[at0 + hh] = S.lmt[hh];
        if (BOOST) p.cut_boost_score[at0 + hh] = S.bt[hh];
      }
      n_new += u0;
      if (tid == 0) p.cut_n_hyps[(size_t)b * E + k] = nh, p.cut_delta_end[(size_t)b * E + k] = min(n_new, P);
    }
    __syncthreads();                                  // every walk has read the beam; now the single fresh entry
    if (tid == 0) {
      SbeState& S = L.st[cur];
      S.pb[0] = 0, S.pnb[0] = SBE_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.own[0] = 0, S.lmt[0] = 0, S.wh[0] = 0;
      S.len[0] = 0, S.last[0] = -1, S.node[0] = -1, S.ctx[0] = lm_start;
      S.bt[0] = 0, S.bst[0] = b_start;
    }
    nb = model_ok ? 1 : 0, commit = 0;                // a beam that died lives again; one without a valid model does not
    __syncthreads();
  };
  for (int t = lo; t < hi; ++t) {
    const int my_id = pf_id, my_q = pf_q;             // the walk reaches every frame, so the prefetch runs with a dead beam too
    if (tid < N && t + 1 < hi) pf_id = gid[(size_t)(t + 1 - first) * N + tid], pf_q = gq[(size_t)(t + 1 - first) * N + tid];
    if (nb > 0) {
      const SbeState& S = L.st[cur];
      SbeState& D = L.st[cur ^ 1];
      if (tid < N) L.cid[tid] = my_id, L.cq[tid] = my_q;
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
        const long long pbn = nbk >= 0 ? S.sc[j] + (long long)L.cq[nbk] : SBE_NEG;
        long long a = SBE_NEG, e = SBE_NEG;
        if (nl >= 0) {
          const long long ql = (long long)L.cq[nl];
          if (S.pnb[j] != SBE_NEG) a = ql + S.pnb[j];
          if (ps >= 0) {
            const long long base = S.last[ps] == c ? S.pb[ps] : S.sc[ps];
            if (base != SBE_NEG) e = ql + base + S.own[j];      // the model's term and the boost's; 0 without both
            atomicOr(&L.child[ps], 1ull << nl);
          }
        }
        const long long pnbn = sbe_lae(a, e, L.tab);
        L.k_pb[j] = pbn, L.k_pnb[j] = pnbn, L.k_sc[j] = sbe_lae(pbn, pnbn, L.tab);
      }
      __syncthreads();
      const int lg = nb > 1 ? 32 - __clz(nb - 1) : 0;
      const int tpr_lg = 8 - lg, tpr = 1 << tpr_lg;
      const int my_i = tid >> tpr_lg, my_sub = tid & (tpr - 1);
      const bool active = my_i < nb;
      const int r_last = active ? S.last[my_i] : -1;
      const long long r_pb = active ? S.pb[my_i] : SBE_NEG, r_sc = active ? S.sc[my_i] : SBE_NEG;
      const long long r_ksc = active ? L.k_sc[my_i] : SBE_NEG;
      const unsigned long long r_child = active ? L.child[my_i] : 0ull;
      const int k_end = active ? N1 : 0;
      int* const my_raw = L.raw + (LM ? my_i * N : 0);            // my_i < 128: inside raw[SBE_W * SBE_N] since N <= SBE_N
      unsigned* const my_bterm = L.bterm + (BOOST ? my_i * N : 0);              // (likewise)
      if (bo) {                                                   // this frame's boost terms, once (k_beam_boost)
        const int r_bst = active ? S.bst[my_i] : 0;
        const long long r_bpot = active ? (long long)bv.nodes[r_bst].x : 0ll;
        for (int k = my_sub; k < k_end; k += tpr) {
          if (k == 0) continue;
          const int n = k - 1, id = L.cid[n];
          long long bt = 0;
          if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
            const int2 nd = bv.nodes[sbe_next(bv, r_bst, id)];
            bt = (long long)nd.x - r_bpot + (long long)nd.y;
          }
          my_bterm[n] = (unsigned)(bt + SBE_BIAS);
        }
      }
      if (LM) {                                                   // this frame's terms, once (k_beam_lm)
        const int r_ctx = active ? S.ctx[my_i] : 0;
        const unsigned long long r_wh = active ? S.wh[my_i] : 0ull;
        const bool inword = r_last >= 0 && r_last != space;
        for (int k = my_sub; k < k_end; k += tpr) {
          if (k == 0) continue;
          const int n = k - 1, id = L.cid[n];
          int rw = SBE_LM_NOTERM, nx;
          if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
            if (!word_mode) rw = sbe_lm_walk(m, r_ctx, id < m.n_labels ? m.l2w[id] : -1, nx);
            else if (id == space && inword) rw = sbe_lm_walk(m, r_ctx, sbe_lm_word(m, r_wh), nx);
          }
          my_raw[n] = rw;
        }
      }
      auto cand = [&](int k) -> long long {
        if (k == 0) return r_ksc;
        const int n = k - 1, id = L.cid[n];
        if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return SBE_NEG;
        const long long base = id == r_last ? r_pb : r_sc;
        if (base == SBE_NEG) return SBE_NEG;
        return base + (long long)L.cq[n] + (LM ? lm_term(my_raw[n]) : 0ll) + (bo ? (long long)my_bterm[n] - SBE_BIAS : 0ll);
      };
      long long mx = LLONG_MIN, mn = LLONG_MAX;
      int cnt = 0;
      for (int k = my_sub; k < k_end; k += tpr) {
        const long long v = cand(k);
        if (v != SBE_NEG) { ++cnt; mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
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
      for (int w = 1; w < SBE_NWAVE; ++w) {
        mx = L.red_max[w] > mx ? L.red_max[w] : mx, mn = L.red_min[w] < mn ? L.red_min[w] : mn;
        cnt += L.red_cnt[w];
      }
      if (cnt == 0) {                                // uniform: the beam died; it stays dead until the next cut
        nb = 0;
      } else {
      auto radix_select = [&](auto keyfn, int nbits, int& kk, int& n_at) -> unsigned long long {
        const int passes = (nbits + 7) >> 3;          // <= 8
        unsigned long long prefix = 0;
        for (int pass = passes - 1; pass >= 0; --pass) {
          const int shift = pass * 8;
          __syncthreads();
          L.hist[tid] = 0;                            // SBE_NT == 256 bins
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
          return v != SBE_NEG;
        }, range ? 64 - __clzll((long long)range) : 0, need, n_at);
        if (n_at > need) {
          const int M = nb * N1;
          ith = (int)radix_select([&](int k, unsigned long long& key) {
            const long long v = cand(k);
            key = (unsigned long long)(my_i * N1 + k);
            return v != SBE_NEG && (unsigned long long)(mx - v) == rth;
          }, 32 - __clz(M), need, n_at);
        }
      }
      for (int k = my_sub; k < k_end; k += tpr) {
        const long long v = cand(k);
        if (v != SBE_NEG) {
          const unsigned long long rr = (unsigned long long)(mx - v);
          const int idx = my_i * N1 + k;
          if (rr < rth || (rr == rth && idx <= ith)) {
            const int at = atomicAdd(&L.n_sel, 1);
            if (at < SBE_W) L.sel_r[at] = rr, L.sel_idx[at] = idx;
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
          unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * SBE_HMUL;
          x ^= x >> 32;
          D.pb[rank] = SBE_NEG, D.pnb[rank] = v, D.sc[rank] = v;
          D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
          D.node[rank] = t * W + rank;                // <= hi * W - 1 <= INT_MAX - 1 (status 4 otherwise)
          ring[(size_t)(t % F) * W + rank] = make_int2(S.node[i], c);
          if (LM) {
            const int raw = L.raw[i * N + k - 1];
            const long long tm = lm_term(raw);
            int ctx = S.ctx[i];
            unsigned long long wh = 0;
            if (word_mode && c != space) {
              wh = (S.wh[i] ^ ((unsigned long long)(long long)c + 1ull)) * SBE_HMUL;
              wh ^= wh >> 32;
            } else if (raw != SBE_LM_NOTERM) {
              const int w = word_mode ? sbe_lm_word(m, S.wh[i]) : (c < m.n_labels ? m.l2w[c] : -1);
              sbe_lm_walk(m, S.ctx[i], w, ctx);
            }
            D.own[rank] = tm, D.lmt[rank] = S.lmt[i] + tm, D.wh[rank] = wh, D.ctx[rank] = ctx;
          } else {
            D.own[rank] = 0, D.lmt[rank] = 0, D.wh[rank] = 0, D.ctx[rank] = 0;
          }
          if (bo) {                                   // written before the barriers of the selection
            const long long btm = (long long)L.bterm[i * N + k - 1] - SBE_BIAS;
            D.own[rank] += btm, D.bt[rank] = S.bt[i] + btm;
            D.bst[rank] = sbe_next(bv, S.bst[i], c);   // the one look-up again, for the next state
          } else {
            D.bt[rank] = 0, D.bst[rank] = 0;
          }
        }
      }
      __syncthreads();                                // the next beam and this frame's ring row are visible to the work-group
      nb = ns, cur ^= 1;
      }
    }
    // ---- the commit round
    if ((t + 1) % p.K == 0 && t >= p.Lg && nb > 0) {
      const SbeState& S = L.st[cur];
      SbeState& D = L.st[cur ^ 1];
      const int h = t - p.Lg;
      if (tid < nb) {
        int nd = S.node[tid], mo = 0;
        const int u = min(max(S.len[tid] - commit, 0), F);      // uncommitted labels: at most F (the plan)
        for (int k = 0; k < u && nd >= 0; ++k) {
          const int f = nd / W, rr = nd - f * W;
          const int2 e = ring[(size_t)(f % F) * W + rr];
          if (f <= h) {
            if (mo < SBE_K) {
              L.old[tid * SBE_K + mo] = e.y;
              if (tid == 0) L.old_fr[mo] = f;
            }
            ++mo;
          }
          nd = e.x;
        }
        L.old_m[tid] = mo;
      }
      __syncthreads();
      const int m0 = min(L.old_m[0], SBE_K);           // at most K by the plan
      bool keep = false;
      if (tid < nb) {
        keep = L.old_m[tid] == m0;
        for (int k = 0; k < m0; ++k) keep = keep && L.old[tid * SBE_K + k] == L.old[k];
        keep = keep || tid == 0;
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) L.red_a[wave] = __popcll(bal);
      __syncthreads();
      int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < SBE_NWAVE; ++w) {
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
    // ---- the cuts behind frame t (rk, nrec and the ends are uniform)
    while (rk < nrec && rec[rk * SBE_REC + 2] == t + 1) cut(rk++);
  }
  while (rk < nrec) cut(rk++);                        // a row without frames: its records end at hi == lo
  __syncthreads();
  // ---- the beam back into the slot's block
  {
    const SbeState& S = L.st[cur];
    long long* const a64 = reinterpret_cast<long long*>(bblk + SBE_HDR);
    int32_t* const a32 = bblk + SBE_HDR + A32 * W;
    if (tid < W) {
      const bool lv = tid < nb;
      a64[tid] = lv ? S.pb[tid] : 0, a64[W + tid] = lv ? S.pnb[tid] : 0, a64[2 * W + tid] = lv ? S.sc[tid] : 0;
      a64[3 * W + tid] = lv ? (long long)S.hash[tid] : 0, a64[4 * W + tid] = lv ? (long long)S.phash[tid] : 0;
      a64[5 * W + tid] = lv ? S.own[tid] : 0, a64[6 * W + tid] = lv ? S.lmt[tid] : 0;
      a64[7 * W + tid] = lv ? (long long)S.wh[tid] : 0;
      a32[tid] = lv ? S.len[tid] : 0, a32[W + tid] = lv ? S.last[tid] : 0, a32[2 * W + tid] = lv ? S.node[tid] : 0;
      a32[3 * W + tid] = lv ? S.ctx[tid] : 0;
      if (BOOST) a64[8 * W + tid] = lv ? S.bt[tid] : 0, a32[4 * W + tid] = lv ? S.bst[tid] : 0, a32[5 * W + tid] = 0;
    }
    if (tid < SBE_HDR)
      bblk[tid] = tid == 0 ? nb : tid == 1 ? commit : tid == 2 ? hi : tid == 3 ? 1 : tid == 4 ? gset : tid == 5 ? cuts0 + nrec : 0;
  }
  // ---- the provisional tail: the best entry's uncommitted labels, oldest first (behind a cut: the fresh beam's, none)
  {
    int32_t* const tl = p.tail_labels + (size_t)b * p.Ptail;
    const SbeState& S = L.st[cur];
    const int u = nb > 0 ? min(max(S.len[0] - commit, 0), F) : 0;
    if (tid == 0) {
      int nd = nb > 0 ? S.node[0] : -1;
      for (int k = 0; k < u && nd >= 0; ++k) {
        const int f = nd / W, rr = nd - f * W;
        const int2 e = ring[(size_t)(f % F) * W + rr];
        const int at = u - 1 - k;
        if (at < p.Ptail) tl[at] = e.y;
        nd = e.x;
      }
      p.tail_n[b] = u;
    }
    for (int i = min(u, p.Ptail) + tid; i < p.Ptail; i += SBE_NT) tl[i] = blank;
    cuts_empty(nrec);
    for (int i = min(n_new, P) + tid; i < P; i += SBE_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    if (tid == 0) {
      p.n_new_labels[b] = min(n_new, P), p.commit_len[b] = commit, p.n_live[b] = nb, p.status[b] = 0, p.n_cuts[b] = nrec;
    }
  }
}

int launch_stream_beam_ep(hipStream_t s, const qasr_stream_beam_ep_args& x) {
  const qasr_stream_beam_boost_args& q = x.boost;
  const qasr_stream_beam_args& a = q.beam;
  const bool boosted = q.n_sets > 0;
  SbeP p{};
  p.bstate = (int32_t*)a.beam_state, p.sstate = (const int32_t*)a.state, p.slots = a.slots, p.flags = a.flags;
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.enc_lens = a.enc_lens, p.first_frame = a.first_frame, p.tab = a.lae_table;
  p.labels = a.labels, p.frames = a.frames, p.n_new_labels = a.n_new_labels, p.commit_len = a.commit_len, p.n_live = a.n_live;
  p.status = a.status, p.tail_labels = a.tail_labels, p.tail_n = a.tail_n;
  p.records = x.records, p.n_records = x.n_records, p.ep_status = x.ep_status, p.E = x.E;
  p.n_cuts = x.n_cuts, p.cut_n_hyps = x.cut_n_hyps, p.cut_delta_end = x.cut_delta_end, p.cut_labels = x.cut_labels;
  p.cut_n_labels = x.cut_n_labels, p.cut_score = (long long*)x.cut_score, p.cut_lm_score = (long long*)x.cut_lm_score;
  p.cut_boost_score = (long long*)x.cut_boost_score;
  p.lm = (const int*)a.lm, p.lm_bytes = (long long)a.lm_bytes, p.alpha_q = a.alpha_q, p.beta_q = a.beta_q, p.space = a.space;
  p.slot_words = SBE_HDR + (boosted ? 24ll : 20ll) * a.beam_width + 2ll * a.F * a.beam_width;
  p.S = a.S, p.Tw = a.Tw, p.N = a.N, p.W = a.beam_width, p.F = a.F, p.Lg = a.Lg, p.K = a.K, p.n_best = a.n_best, p.blank = a.blank;
  p.P = a.P, p.Ptail = a.Ptail, p.Pend = a.Pend;
  p.boost_set = q.boost_set, p.n_sets = boosted ? q.n_sets : 0;
  for (int g = 0; g < SBE_SETS; ++g) {              // unused triples repeat set 0, so that every argument is a valid set
    const int k = g < q.n_sets ? g : 0;
    p.set[g] = boosted ? (const int*)q.sets[k] : nullptr, p.set_bytes[g] = boosted ? (long long)q.set_bytes[k] : 0;
    p.set_whole[g] = boosted ? q.whole_words[k] : 0;
  }
  static_assert(sizeof(SbeLds<true, true>) <= 160 * 1024, "k_stream_beam_ep: the LDS of one gfx950 CU");
  const dim3 grid((unsigned)a.B), block(SBE_NT);
  if (a.lm && boosted) hipLaunchKernelGGL((k_stream_beam_ep<true, true>), grid, block, 0, s, p);
  else if (a.lm) hipLaunchKernelGGL((k_stream_beam_ep<true, false>), grid, block, 0, s, p);
  else if (boosted) hipLaunchKernelGGL((k_stream_beam_ep<false, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_stream_beam_ep<false, false>), grid, block, 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
