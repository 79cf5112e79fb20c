// The body of the streaming beam kernels, stated once for k_stream_beam<LM> (qasr_stream_beam.hip) and k_stream_beam_boost<LM>
// (qasr_stream_beam_boost.hip): the slot's block and its LDS image, the parameters, and StreamBeamRun<LM, BOOST> - the load
// of a slot's beam, the fresh entry, the frame step, the commit round, the store back, the provisional tail and the END pass.
// The host statement is qasr/stream_beam.py, whose _frame every rule set calls in the same way; the kernels follow it byte
// for byte, the state block and the ring included.  k_stream_beam_ep (qasr_stream_beam_ep.hip) keeps a copy of its own,
// because its boosted instantiations measured slower on this body and on the helpers alone.
//
// One work-group of 256 threads per row.  The beam (pb, pnb, score, prefix hash, parent hash, own, lm_tot, word hash, length,
// last label, node, context; boosted: boost_tot and the automaton state bst) is loaded from the slot's block into LDS (8- and
// 4-byte vector loads, thread i entry i) and stored back by this work-group, the only one that owns the slot in the launch
// (the rows' slots are distinct).  A slot's block is 16 header words (nb, commit_len, frames_done, started, set + 1, cuts
// done, zeros), then W entries each as eight 64-bit and four 32-bit arrays (boosted: nine and six, the sixth a pad of zeros
// that keeps every slot's 64-bit arrays 8-byte aligned for odd W), then the ring [F][W] of (parent node, label).  Frames are
// global: frame t reads row t - first_frame of the window's candidates, and the prefix that lands in rank r is node t * W + r
// in ring row t % F.  After every frame t with (t + 1) % K == 0 and t >= Lg a commit round: thread e walks entry e's chain
// through the ring down to commit_len and keeps the labels created at or before h = t - Lg (at most K: L.old[e][]), entry 0's
// are the newly committed text; entries whose old labels differ from entry 0's are dropped, survivors are compacted in order
// (wave ballots) into the other side of the double buffer, bst and boost_tot with them.  The frame's model and boost terms
// are evaluated ONCE, before the selection, by the thread that scores candidate (entry, n), and left in L.raw / L.bterm (the
// boost term biased by 2^30); a winner repeats its one walk / look-up for its next context / state.  The END pass scores the
// unfinished word (word mode), takes the virtual space (whole words), subtracts the unfinished pot and re-orders ONCE, on the
// outputs only.
// Bounds.  Every loop is bounded by W, N, F = Lg + K, the step's frames (<= Tw), 256 or the bounds of qasr_beam_dev.h.
// Candidates are read at rows t - first with first <= lo <= t < hi <= first + Tw (the callers' statuses otherwise).  Ring
// indices are (f % F) * W + r with r < W: inside the ring for ANY node value >= 0, so a corrupt block can give wrong text but
// no access outside the slot.  (The E path adds `own` as the block holds it, as the twin does; k_stream_beam<false> used to
// read it as 0.  Every block a kernel stored holds 0 there without a model and a set; a foreign one changes scores only.)
// EVERY automaton state - loaded from the block, read from the table or from the root row - is
// clamped to 0 .. n_nodes - 1 before it indexes (pot, bank)[]; a set word outside 0 .. n_sets reads as 0.  Global memory sees
// plain vector stores only, by the one work-group that owns the slot; LDS atomics only.
#pragma once
#include "qasr_beam_dev.h"

namespace qasr {

#define STB_K QASR_STREAM_BEAM_ROUND
#define STB_HDR 16                // header words of a slot's block
#define STB_SETS QASR_STREAM_BEAM_MAX_SETS
// the stream block of qasr_stream.hip (read-only here)
#define STB_ST_WORDS 80
#define STB_ST_RECV 0
#define STB_ST_DONE 2

struct StreamBeamP {          // the parameters of k_stream_beam; k_stream_beam_boost adds its sets
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
  const int* lm;
  long long lm_bytes, alpha_q, beta_q;
  long long slot_words;
  int space;
  int S, Tw, N, W, F, Lg, K, n_best, blank, P, Ptail, Pend;
  int32_t* end_labels;        // [B][n_best][Pend]
  int32_t* end_n_labels;      // [B][n_best]
  long long* end_score;
  long long* end_lm_score;    // with a model
  long long* end_boost_score; // boosted
  int32_t* n_hyps;
  int Rr, spf;
};

struct StreamBeamSets {       // the phrase sets of a boosted launch: (pointer, bytes, whole_words) triples the host call validated
  const int32_t* boost_set;   // [B]
  const int* set[STB_SETS];
  long long set_bytes[STB_SETS];
  int set_whole[STB_SETS];
  int n_sets;
};

struct StreamBeamRows {       // where the n-best rows of one END pass go: a row's END outputs, or one cut's
  int32_t* labels;            // [n_best][Pend]
  int32_t* n_labels;          // [n_best]
  long long* score;
  long long* lm_score;        // with a model
  long long* boost_score;     // boosted
};

inline size_t stream_beam_slot_words(int W, int F, bool boosted) {
  return (size_t)STB_HDR + (boosted ? 24 : 20) * (size_t)W + 2 * (size_t)F * (size_t)W;
}

inline size_t stream_beam_block_bytes(int S, int W, int F, bool boosted) {
  if (S < 1 || W < 1 || W > QASR_BEAM_MAX_WIDTH || F < 1 || F > QASR_STREAM_BEAM_MAX_RING) return 0;
  return (size_t)S * 4 * stream_beam_slot_words(W, F, boosted);
}

inline void stream_beam_fill(StreamBeamP& p, const qasr_stream_beam_args& a, bool boosted) {
  p.bstate = (int32_t*)a.beam_state, p.sstate = (const int32_t*)a.state, p.slots = a.slots, p.flags = a.flags;
  p.cand_id = a.cand_id, p.cand_q = a.cand_q, p.enc_lens = a.enc_lens, p.first_frame = a.first_frame, p.tab = a.lae_table;
  p.labels = a.labels, p.frames = a.frames, p.n_new_labels = a.n_new_labels, p.commit_len = a.commit_len, p.n_live = a.n_live;
  p.status = a.status, p.tail_labels = a.tail_labels, p.tail_n = a.tail_n;
  p.lm = (const int*)a.lm, p.lm_bytes = (long long)a.lm_bytes, p.alpha_q = a.alpha_q, p.beta_q = a.beta_q, p.space = a.space;
  p.slot_words = (long long)stream_beam_slot_words(a.beam_width, a.F, boosted);
  p.S = a.S, p.Tw = a.Tw, p.N = a.N, p.W = a.beam_width, p.F = a.F, p.Lg = a.Lg, p.K = a.K, p.n_best = a.n_best, p.blank = a.blank;
  p.P = a.P, p.Ptail = a.Ptail, p.Pend = a.Pend;
  p.end_labels = a.end_labels, p.end_n_labels = a.end_n_labels, p.end_score = (long long*)a.end_score;
  p.end_lm_score = (long long*)a.end_lm_score, p.n_hyps = a.n_hyps;
  p.Rr = a.Rr, p.spf = a.samples_per_frame;
}

inline void stream_beam_fill_sets(StreamBeamSets& g, const qasr_stream_beam_boost_args& q) {
  g.boost_set = q.boost_set, g.n_sets = q.n_sets;
  for (int i = 0; i < STB_SETS; ++i) {              // unused triples repeat set 0, so that every argument is a valid set
    const int k = i < q.n_sets ? i : 0;
    g.set[i] = (const int*)q.sets[k], g.set_bytes[i] = (long long)q.set_bytes[k], g.set_whole[i] = q.whole_words[k];
  }
}

// ---- the LDS image.  What only a boosted kernel keeps is an empty base without BOOST, so that it costs no LDS there.
template <bool BOOST>
struct StreamBeamBoostCols {
  long long bt[BEAM_W];       // boost_tot
  int bst[BEAM_W];
};
template <>
struct StreamBeamBoostCols<false> {};

template <bool BOOST>
struct StreamBeamState : StreamBeamBoostCols<BOOST> {      // one side of the double buffer
  long long pb[BEAM_W], pnb[BEAM_W], sc[BEAM_W];
  unsigned long long hash[BEAM_W], phash[BEAM_W];
  long long own[BEAM_W], lmt[BEAM_W];
  unsigned long long wh[BEAM_W];
  int len[BEAM_W], last[BEAM_W], node[BEAM_W], ctx[BEAM_W];
};

template <bool BOOST>
struct StreamBeamBoostTerms {
  unsigned bterm[BEAM_W * BEAM_N];
};
template <>
struct StreamBeamBoostTerms<false> {};

template <bool LM, bool BOOST>
struct StreamBeamLds : StreamBeamBoostTerms<BOOST> {
  uint16_t tab[BEAM_TAB];
  StreamBeamState<BOOST> st[2];
  long long k_pb[BEAM_W], k_pnb[BEAM_W], k_sc[BEAM_W];
  unsigned long long sel_r[BEAM_W];
  int sel_idx[BEAM_W];
  unsigned long long child[BEAM_W];
  int cid[BEAM_N], cq[BEAM_N];
  unsigned hist[256];
  long long red_max[BEAM_NWAVE], red_min[BEAM_NWAVE];
  int red_cnt[BEAM_NWAVE], red_a[BEAM_NWAVE];
  int bin, kk, n_at, n_sel;
  int old[BEAM_W * STB_K];      // a round: entry e's labels created at or before h, newest first
  int old_fr[STB_K];            // entry 0's creation frames
  int old_m[BEAM_W];
  int raw[LM ? BEAM_W * BEAM_N : 1];
};
static_assert(sizeof(StreamBeamLds<true, true>) <= 160 * 1024, "the streaming beam kernels: the LDS of one gfx950 CU");

// n-best rows from hypothesis `from` on: hypotheses that do not exist
template <bool LM, bool BOOST>
__device__ __forceinline__ void stream_beam_rows_empty(const StreamBeamRows& o, int from, int nbest, int Pend, int blank) {
  const int tid = threadIdx.x;
  for (int i = from * Pend + tid; i < nbest * Pend; i += BEAM_NT) o.labels[i] = blank;
  for (int h = from + tid; h < nbest; h += BEAM_NT) {
    o.n_labels[h] = 0;
    o.score[h] = BEAM_NEG;
    if (LM) o.lm_score[h] = 0;
    if (BOOST) o.boost_score[h] = 0;
  }
}

template <bool LM, bool BOOST>
struct StreamBeamRun {
  typedef StreamBeamState<BOOST> State;
  static constexpr int ENT = BOOST ? 24 : 20;      // words per entry of a slot's block: 8 (9) 64-bit arrays, 4 (6) 32-bit arrays
  static constexpr int A32 = BOOST ? 18 : 16;      // the 32-bit arrays begin behind the 64-bit ones
  const StreamBeamP& p;
  StreamBeamLds<LM, BOOST>& L;
  const int tid, lane, wave, b, N, W, N1, blank, F, P;
  const size_t row;
  int slot;
  bool slot_ok, begin, end;
  const int32_t* sblk;        // the stream block of the row's slot (slot 0 for a slot out of range: status 2)
  int32_t* bblk;              // the beam block
  int2* ring;                 // [F][W]
  int first, e_len;
  LmView m;
  BoostView bv;
  bool model_ok, bo;
  int gset;                   // the slot's phrase set + 1 (header word 4), 0: no boosting
  int nb, commit, cur, n_new, hi;
  const int32_t* gid;         // the row's candidates; row t - first: lo >= first, hi <= first + Tw
  const int32_t* gq;
  int pf_id, pf_q;            // frame t's candidate of this thread, loaded one frame ahead

  // ---- the row's slot and flags; every thread reads the same
  __device__ __forceinline__ StreamBeamRun(const StreamBeamP& p_, StreamBeamLds<LM, BOOST>& L_)
      : p(p_), L(L_), tid(threadIdx.x), lane(threadIdx.x & 63), wave(threadIdx.x >> 6), b(blockIdx.x), N(p_.N), W(p_.W),
        N1(p_.N + 1), blank(p_.blank), F(p_.F), P(p_.P), row((size_t)blockIdx.x * p_.P) {
    slot = p.slots[b];
    slot_ok = slot >= 0 && slot < p.S;
    sblk = p.sstate + (long long)(slot_ok ? slot : 0) * STB_ST_WORDS;
    bblk = p.bstate + (long long)(slot_ok ? slot : 0) * p.slot_words;
    ring = reinterpret_cast<int2*>(bblk + STB_HDR + ENT * W);
    const int fl = p.flags[b];
    begin = (fl & QASR_STREAM_BEGIN) != 0, end = (fl & QASR_STREAM_END) != 0;
    first = p.first_frame[b];
    e_len = min(max(p.enc_lens[b], 0), p.Tw);
    m = LmView{}, bv = BoostView{};
    model_ok = true, bo = false;
    gset = 0, nb = 0, commit = 0, cur = 0, n_new = 0, hi = 0;
    gid = p.cand_id + ((size_t)b * p.Tw) * N, gq = p.cand_q + ((size_t)b * p.Tw) * N;
    pf_id = -1, pf_q = 0;
  }

  // the status of a step over [lo, hi); the block's own frames_done must be where the stream's is (status 3)
  __device__ __forceinline__ int status_of(int lo, int hi_, const StreamBeamSets* g) const {
    if (!slot_ok) return 2;
    if (lo < first || first < 0) return 1;
    if ((begin ? 0 : bblk[2]) != lo) return 3;
    if ((long long)hi_ * W > (long long)INT_MAX) return 4;
    if (BOOST && begin && (g->boost_set[b] < -1 || g->boost_set[b] >= g->n_sets)) return 5;
    return 0;
  }

  // an empty step, the state untouched (the caller adds its own outputs)
  __device__ __forceinline__ void empty_step(int status) const {
    for (int i = tid; i < P; i += BEAM_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    for (int i = tid; i < p.Ptail; i += BEAM_NT) p.tail_labels[(size_t)b * p.Ptail + i] = blank;
    if (tid == 0) p.n_new_labels[b] = 0, p.commit_len[b] = 0, p.n_live[b] = 0, p.status[b] = status, p.tail_n[b] = 0;
  }

  __device__ __forceinline__ void fresh(State& S) const {      // the single empty entry (one thread)
    S.pb[0] = 0, S.pnb[0] = BEAM_NEG, S.sc[0] = 0, S.hash[0] = 0, S.phash[0] = 0, S.own[0] = 0, S.lmt[0] = 0, S.wh[0] = 0;
    S.len[0] = 0, S.last[0] = -1, S.node[0] = -1, S.ctx[0] = m.start;
    if constexpr (BOOST) S.bt[0] = 0, S.bst[0] = bo ? bv.start : 0;
  }

  // ---- the model, the slot's phrase set and the slot's beam into LDS, frame lo's candidates on their way; ends with a barrier
  __device__ __forceinline__ void load(int lo, int hi_, const StreamBeamSets* g) {
    hi = hi_;
    const int nb0 = bblk[0], commit0 = bblk[1], started = bblk[3];
    if (LM) model_ok = lm_view(m, p.lm, p.lm_bytes, p.alpha_q, p.beta_q, p.space);
    if constexpr (BOOST) {
      // header word 4 (a BEGIN row: the input), 0 or a word out of range: no boosting
      gset = begin ? g->boost_set[b] + 1 : bblk[4];
      gset = gset >= 0 && gset <= g->n_sets ? gset : 0;
      if (gset > 0) {
        const int* bh = g->set[0];                 // picked by a chain of compares on constant indices
        long long bbytes = g->set_bytes[0];
        int bwhole = g->set_whole[0];
#pragma unroll
        for (int i = 1; i < STB_SETS; ++i)
          if (i == gset - 1) bh = g->set[i], bbytes = g->set_bytes[i], bwhole = g->set_whole[i];
        model_ok = boost_view(bv, bh, bbytes, bwhole, p.space) && model_ok;
        if (!model_ok) gset = 0;
      }
      bo = gset > 0;
    }
    for (int i = tid; i < BEAM_TAB; i += BEAM_NT) L.tab[i] = p.tab[i];
    const bool is_fresh = begin || !started;
    nb = is_fresh ? 1 : min(max(nb0, 0), W);
    commit = is_fresh ? 0 : max(commit0, 0);
    if (!model_ok) nb = 0;
    State& S = L.st[0];
    const long long* const a64 = reinterpret_cast<const long long*>(bblk + STB_HDR);
    const int32_t* const a32 = bblk + STB_HDR + A32 * W;
    if (is_fresh) {
      if (tid == 0) fresh(S);
    } else if (tid < nb) {
      S.pb[tid] = a64[tid], S.pnb[tid] = a64[W + tid], S.sc[tid] = a64[2 * W + tid];
      S.hash[tid] = (unsigned long long)a64[3 * W + tid], S.phash[tid] = (unsigned long long)a64[4 * W + tid];
      S.own[tid] = a64[5 * W + tid], S.lmt[tid] = a64[6 * W + tid], S.wh[tid] = (unsigned long long)a64[7 * W + tid];
      S.len[tid] = a32[tid], S.last[tid] = a32[W + tid], S.node[tid] = a32[2 * W + tid], S.ctx[tid] = a32[3 * W + tid];
      if constexpr (BOOST) {
        const int s = a32[4 * W + tid];
        S.bt[tid] = a64[8 * W + tid], S.bst[tid] = bo && (unsigned)s < (unsigned)bv.n_nodes ? s : 0;
      }
    }
    if (tid < N && hi > lo) pf_id = gid[(size_t)(lo - first) * N + tid], pf_q = gq[(size_t)(lo - first) * N + tid];
    __syncthreads();                                  // the block has been read; the beam and the table are in LDS
  }

  // ---- frame t of a live beam: the next beam into the other side; a beam that dies leaves nb == 0
  __device__ __forceinline__ void frame(int t) {
    const int my_id = pf_id, my_q = pf_q;
    if (tid < N && t + 1 < hi) pf_id = gid[(size_t)(t + 1 - first) * N + tid], pf_q = gq[(size_t)(t + 1 - first) * N + tid];
    const State& S = L.st[cur];
    State& D = L.st[cur ^ 1];
    const int space = p.space;
    if (tid < N) L.cid[tid] = my_id, L.cq[tid] = my_q;
    if (tid < nb) L.child[tid] = 0;
    if (tid == 0) L.n_sel = 0;
    __syncthreads();
    // ---- the entries themselves (the E path adds the entry's own term, the model's and the boost's: 0 without both)
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
          if (base != BEAM_NEG) e = ql + base + S.own[j];
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
    int* const my_raw = L.raw + (LM ? my_i * N : 0);            // my_i < 128: inside raw[BEAM_W * BEAM_N] since N <= BEAM_N
    unsigned* my_bterm = nullptr;
    if constexpr (BOOST) {                                      // this frame's boost terms, once
      my_bterm = L.bterm + my_i * N;                            // (likewise)
      if (bo) {
        const int r_bst = active ? S.bst[my_i] : 0;
        const long long r_bpot = active ? (long long)bv.nodes[r_bst].x : 0ll;
        for (int k = my_sub; k < k_end; k += tpr) {
          if (k == 0) continue;
          const int n = k - 1, id = L.cid[n];
          long long bt = 0;
          if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
            const int2 nd = bv.nodes[boost_next<true>(bv, r_bst, id)];
            bt = (long long)nd.x - r_bpot + (long long)nd.y;
          }
          my_bterm[n] = (unsigned)(bt + BOOST_BIAS);
        }
      }
    }
    if (LM) {                                                   // this frame's model terms, once
      const int r_ctx = active ? S.ctx[my_i] : 0;
      const unsigned long long r_wh = active ? S.wh[my_i] : 0ull;
      const bool inword = r_last >= 0 && r_last != space;
      for (int k = my_sub; k < k_end; k += tpr) {
        if (k == 0) continue;
        const int n = k - 1, id = L.cid[n];
        int rw = BEAM_LM_NOTERM, nx;
        if (id >= 0 && id != blank && !((r_child >> n) & 1ull)) {
          if (!m.word_mode) rw = lm_walk(m, r_ctx, id < m.n_labels ? m.l2w[id] : -1, nx);
          else if (id == space && inword) rw = lm_walk(m, r_ctx, lm_word(m, r_wh), nx);
        }
        my_raw[n] = rw;
      }
    }
    auto cand = [&](int k) -> long long {
      if (k == 0) return r_ksc;
      const int n = k - 1, id = L.cid[n];
      if (id < 0 || id == blank || ((r_child >> n) & 1ull)) return BEAM_NEG;
      const long long base = id == r_last ? r_pb : r_sc;
      if (base == BEAM_NEG) return BEAM_NEG;
      long long v = base + (long long)L.cq[n] + (LM ? lm_term(m, my_raw[n]) : 0ll);
      if constexpr (BOOST) v += bo ? (long long)my_bterm[n] - BOOST_BIAS : 0ll;
      return v;
    };
    long long mx;
    if (!beam_select(L, cand, my_i, my_sub, tpr, k_end, nb, N1, W, mx)) {
      nb = 0;
      return;
    }
    const int ns = min(L.n_sel, W);
    // ---- order the winners (score descending = r ascending, then candidate index) and write the next beam
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
        if constexpr (BOOST) D.bt[rank] = S.bt[i], D.bst[rank] = S.bst[i];
      } else {
        const int c = L.cid[k - 1];
        const long long v = mx - (long long)rr;
        unsigned long long x = (S.hash[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
        x ^= x >> 32;
        D.pb[rank] = BEAM_NEG, D.pnb[rank] = v, D.sc[rank] = v;
        D.hash[rank] = x, D.phash[rank] = S.hash[i], D.len[rank] = S.len[i] + 1, D.last[rank] = c;
        D.node[rank] = t * W + rank;                // <= hi * W - 1 <= INT_MAX - 1 (status 4 otherwise)
        ring[(size_t)(t % F) * W + rank] = make_int2(S.node[i], c);
        if (LM) {
          const int raw = L.raw[i * N + k - 1];     // written before the barriers of the selection
          const long long tm = lm_term(m, raw);
          int ctx = S.ctx[i];
          unsigned long long wh = 0;
          if (m.word_mode && c != space) {
            wh = (S.wh[i] ^ ((unsigned long long)(long long)c + 1ull)) * BEAM_HMUL;
            wh ^= wh >> 32;
          } else if (raw != BEAM_LM_NOTERM) {       // the token was scored: the one walk again, for its context
            const int w = m.word_mode ? lm_word(m, S.wh[i]) : (c < m.n_labels ? m.l2w[c] : -1);
            lm_walk(m, S.ctx[i], w, ctx);
          }
          D.own[rank] = tm, D.lmt[rank] = S.lmt[i] + tm, D.wh[rank] = wh, D.ctx[rank] = ctx;
        } else {
          D.own[rank] = 0, D.lmt[rank] = 0, D.wh[rank] = 0, D.ctx[rank] = 0;
        }
        if constexpr (BOOST) {
          if (bo) {
            const long long btm = (long long)L.bterm[i * N + k - 1] - BOOST_BIAS;
            D.own[rank] += btm, D.bt[rank] = S.bt[i] + btm;
            D.bst[rank] = boost_next<true>(bv, S.bst[i], c);      // the one look-up again, for the next state
          } else {
            D.bt[rank] = 0, D.bst[rank] = 0;
          }
        }
      }
    }
    __syncthreads();                                // the next beam and this frame's ring row are visible to the work-group
    nb = ns, cur ^= 1;
  }

  // ---- the commit round behind frame t
  __device__ __forceinline__ void commit_round(int t) {
    if ((t + 1) % p.K != 0 || t < p.Lg || nb <= 0) return;
    const State& S = L.st[cur];
    State& D = L.st[cur ^ 1];
    const int h = t - p.Lg;
    if (tid < nb) {
      int nd = S.node[tid], mo = 0;
      const int u = min(max(S.len[tid] - commit, 0), F);      // uncommitted labels: at most F (the plan)
      for (int k = 0; k < u && nd >= 0; ++k) {
        const int f = nd / W, rr = nd - f * W;
        const int2 e = ring[(size_t)(f % F) * W + rr];
        if (f <= h) {
          if (mo < STB_K) {
            L.old[tid * STB_K + mo] = e.y;
            if (tid == 0) L.old_fr[mo] = f;
          }
          ++mo;
        }
        nd = e.x;
      }
      L.old_m[tid] = mo;
    }
    __syncthreads();
    const int m0 = min(L.old_m[0], STB_K);           // at most K by the plan
    bool keep = false;
    if (tid < nb) {
      keep = L.old_m[tid] == m0;
      for (int k = 0; k < m0; ++k) keep = keep && L.old[tid * STB_K + k] == L.old[k];
      keep = keep || tid == 0;
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) L.red_a[wave] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < BEAM_NWAVE; ++w) {
      pos += w < wave ? L.red_a[w] : 0;
      total += L.red_a[w];
    }
    if (keep) {
      D.pb[pos] = S.pb[tid], D.pnb[pos] = S.pnb[tid], D.sc[pos] = S.sc[tid], D.hash[pos] = S.hash[tid];
      D.phash[pos] = S.phash[tid], D.own[pos] = S.own[tid], D.lmt[pos] = S.lmt[tid], D.wh[pos] = S.wh[tid];
      D.len[pos] = S.len[tid], D.last[pos] = S.last[tid], D.node[pos] = S.node[tid], D.ctx[pos] = S.ctx[tid];
      if constexpr (BOOST) D.bt[pos] = S.bt[tid], D.bst[pos] = S.bst[tid];
    }
    if (tid < m0) {                                 // the delta, oldest first
      const int at = n_new + (m0 - 1 - tid);
      if (at < P) p.labels[row + at] = L.old[tid], p.frames[row + at] = L.old_fr[tid];
    }
    __syncthreads();
    nb = total, cur ^= 1, commit += m0, n_new += m0;
  }

  // ---- the beam back into the slot's block
  __device__ __forceinline__ void store() const {
    const State& S = L.st[cur];
    long long* const a64 = reinterpret_cast<long long*>(bblk + STB_HDR);
    int32_t* const a32 = bblk + STB_HDR + A32 * W;
    if (tid < W) {
      const bool lv = tid < nb;
      a64[tid] = lv ? S.pb[tid] : 0, a64[W + tid] = lv ? S.pnb[tid] : 0, a64[2 * W + tid] = lv ? S.sc[tid] : 0;
      a64[3 * W + tid] = lv ? (long long)S.hash[tid] : 0, a64[4 * W + tid] = lv ? (long long)S.phash[tid] : 0;
      a64[5 * W + tid] = lv ? S.own[tid] : 0, a64[6 * W + tid] = lv ? S.lmt[tid] : 0;
      a64[7 * W + tid] = lv ? (long long)S.wh[tid] : 0;
      a32[tid] = lv ? S.len[tid] : 0, a32[W + tid] = lv ? S.last[tid] : 0, a32[2 * W + tid] = lv ? S.node[tid] : 0;
      a32[3 * W + tid] = lv ? S.ctx[tid] : 0;
      if constexpr (BOOST) a64[8 * W + tid] = lv ? S.bt[tid] : 0, a32[4 * W + tid] = lv ? S.bst[tid] : 0, a32[5 * W + tid] = 0;
    }
    if (tid < STB_HDR)
      bblk[tid] = tid == 0 ? nb : tid == 1 ? commit : tid == 2 ? hi : tid == 3 ? 1 : tid == 4 ? gset : 0;
  }

  // ---- the outputs of a step that ends without END: the provisional tail (the best entry's uncommitted labels, oldest
  // first), the rest of the delta, the row's counts
  __device__ __forceinline__ void tail() const {
    int32_t* const tl = p.tail_labels + (size_t)b * p.Ptail;
    const State& S = L.st[cur];
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
    for (int i = min(u, p.Ptail) + tid; i < p.Ptail; i += BEAM_NT) tl[i] = blank;
    for (int i = min(n_new, P) + tid; i < P; i += BEAM_NT) p.labels[row + i] = blank, p.frames[row + i] = 0;
    if (tid == 0) p.n_new_labels[b] = min(n_new, P), p.commit_len[b] = commit, p.n_live[b] = nb, p.status[b] = 0;
  }

  // ---- the END pass on the outputs in o: word mode scores the unfinished word of every entry, a boosted slot takes the
  // virtual space (whole words) and loses its unfinished pot; then ONE re-ordering (score descending, ties by the previous
  // rank) into the other side, which the beam itself does not follow.  The first n_best entries are written as suffixes
  // behind commit_len, the best one also appended to the delta at n_new.  Returns the hypotheses written, in u0 the labels
  // the best one appended.
  __device__ __forceinline__ int end_pass(const StreamBeamRows& o, int& u0) {
    const int space = p.space;
    int side = cur;
    if (((LM && m.word_mode) || bo) && nb > 0) {
      const State& S = L.st[cur];
      State& D = L.st[cur ^ 1];
      long long sc = BEAM_NEG, lmt = 0, bt = 0;
      if (tid < nb) {
        sc = S.sc[tid], lmt = S.lmt[tid];
        const int last = S.last[tid];
        if (LM && m.word_mode && last >= 0 && last != space) {
          int nx;
          const long long tm = lm_term(m, lm_walk(m, S.ctx[tid], lm_word(m, S.wh[tid]), nx));
          sc += tm, lmt += tm;
        }
        if constexpr (BOOST) {
          bt = S.bt[tid];
          if (bo) {
            long long pot = (long long)bv.nodes[S.bst[tid]].x;
            if (bv.whole) {
              const int2 nd = bv.nodes[boost_next<true>(bv, S.bst[tid], space)];
              const long long tm = (long long)nd.x - pot + (long long)nd.y;
              sc += tm, bt += tm, pot = (long long)nd.x;
            }
            sc -= pot, bt -= pot;
          }
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
        D.sc[rank] = sc, D.lmt[rank] = lmt, D.len[rank] = S.len[tid], D.node[rank] = S.node[tid];
        if constexpr (BOOST) D.bt[rank] = bt;
      }
      __syncthreads();
      side = cur ^ 1;
    }
    const State& S = L.st[side];
    const int nh = min(nb, p.n_best);
    u0 = nh > 0 ? min(max(S.len[0] - commit, 0), F) : 0;
    for (int i = tid; i < nh * p.Pend; i += BEAM_NT) o.labels[i] = blank;
    stream_beam_rows_empty<LM, BOOST>(o, nh, p.n_best, p.Pend, blank);
    __syncthreads();                                  // the fills above are behind every walk's stores
    if (tid < nh) {
      const int hh = tid;
      const int u = min(max(S.len[hh] - commit, 0), F);
      int nd = S.node[hh];
      for (int j = 0; j < u && nd >= 0; ++j) {
        const int f = nd / W, rr = nd - f * W;
        const int2 e = ring[(size_t)(f % F) * W + rr];
        const int at = u - 1 - j;
        if (at < p.Pend) o.labels[(size_t)hh * p.Pend + at] = e.y;
        if (hh == 0 && n_new + at < P) p.labels[row + n_new + at] = e.y, p.frames[row + n_new + at] = f;
        nd = e.x;
      }
      o.n_labels[hh] = u;
      o.score[hh] = S.sc[hh];
      if (LM) o.lm_score[hh] = S.lmt[hh];
      if constexpr (BOOST) o.boost_score[hh] = S.bt[hh];
    }
    return nh;
  }
};

// ---- the body of k_stream_beam<LM> (BOOST false, g null) and k_stream_beam_boost<LM> (BOOST true), launched BEFORE
// k_stream_emit, which advances frames_done: lo is the stream block's frames_done, hi what the samples received make final
// (END: all of the window).  A beam that dies ends the walk.
template <bool LM, bool BOOST>
__device__ __forceinline__ void stream_beam_body(const StreamBeamP& p, const StreamBeamSets* g, StreamBeamLds<LM, BOOST>& L) {
  StreamBeamRun<LM, BOOST> R(p, L);
  const int tid = R.tid, b = R.b, nbest = p.n_best;
  long long r = *(const long long*)(R.sblk + STB_ST_RECV);
  r = r < 0 ? 0 : r;
  const int lo = R.sblk[STB_ST_DONE];
  const long long top = (long long)R.first + R.e_len;
  const long long lim = r >= p.Rr ? (r - p.Rr) / p.spf : -1;
  const long long hi64 = R.end ? max((long long)lo, top) : max((long long)lo, min(top, lim));
  const int hi = (int)min(hi64, (long long)INT_MAX);
  const int status = R.status_of(lo, hi, g);
  const size_t at0 = (size_t)b * nbest;
  const StreamBeamRows o{p.end_labels + at0 * p.Pend, p.end_n_labels + at0, p.end_score + at0, LM ? p.end_lm_score + at0 : nullptr,
                         BOOST ? p.end_boost_score + at0 : nullptr};
  if (status != 0) {                                  // uniform: every thread read the same
    R.empty_step(status);
    stream_beam_rows_empty<LM, BOOST>(o, 0, nbest, p.Pend, R.blank);
    if (tid == 0) p.n_hyps[b] = 0;
    return;
  }
  R.load(lo, hi, g);
  for (int t = lo; t < hi && R.nb > 0; ++t) {
    R.frame(t);
    R.commit_round(t);
  }
  __syncthreads();
  R.store();                                          // before END re-orders the outputs
  if (!R.end) {
    R.tail();
    stream_beam_rows_empty<LM, BOOST>(o, 0, nbest, p.Pend, R.blank);
    if (tid == 0) p.n_hyps[b] = 0;
    return;
  }
  int u0;
  const int nh = R.end_pass(o, u0);
  for (int i = tid; i < p.Ptail; i += BEAM_NT) p.tail_labels[(size_t)b * p.Ptail + i] = R.blank;
  for (int i = min(R.n_new + u0, R.P) + tid; i < R.P; i += BEAM_NT) p.labels[R.row + i] = R.blank, p.frames[R.row + i] = 0;
  if (tid == 0) {
    p.n_new_labels[b] = min(R.n_new + u0, R.P), p.commit_len[b] = R.commit + u0, p.n_live[b] = R.nb, p.status[b] = 0;
    p.tail_n[b] = 0, p.n_hyps[b] = nh;
  }
}

}  // namespace qasr
