// What the beam kernels share, stated once for k_beam / k_beam_lm (qasr_beam.hip), k_beam_boost (qasr_beam_boost.hip) and the
// streaming family (qasr_stream_beam_dev.h): the constants, the log-add-exp look-up, the views of the packed n-gram model and
// of a packed phrase set with their header checks, the model walks, the automaton's transition, and the selection of a frame's
// best W candidates.  The host statements are qasr/beam.py (RULES, LM_RULES) and qasr/boost.py (BOOST_RULES).  The fixed-point
// arithmetic (NEG, fx_lae, fx_key, fx_quantize) is qasr_fixed_dev.h's, shared with the lattice kernels.
// Bounds.  A model walk is bounded by the order (<= 6) and the header's probe bounds, its table indices are masked; a set is
// used only if its header describes exactly the bytes the host passed (128 + 16 cap + 8 nodes + 4 labels == bytes, cap a power
// of two), its table indices are masked by cap - 1, root-row indices are checked against n_labels, and every state that
// boost_next<true> returns is clamped to 0 .. n_nodes - 1 before it indexes (pot, bank)[].  The selection touches LDS only (atomics
// on the histogram and the winner count); every loop in it is bounded by N + 1, 256 bins or 8 passes.
#pragma once
#include <climits>

#include "qasr_fixed_dev.h"

namespace qasr {

#define BEAM_NEG FX_NEG
#define BEAM_HMUL 0x9E3779B97F4A7C15ull
#define BEAM_NT 256
#define BEAM_NWAVE (BEAM_NT / 64)
#define BEAM_W QASR_BEAM_MAX_WIDTH
#define BEAM_N QASR_BEAM_MAX_CANDIDATES
#define BEAM_TAB FX_TAB
#define BEAM_LM_MAGIC 0x314D4C51
#define BEAM_LM_OOV (-1000 * 65536)
#define BEAM_LM_RAWLIM 2147483647ll
#define BEAM_LM_NOTERM INT_MIN
#define BOOST_MAGIC 0x31534251
#define BOOST_BIAS (1ll << 30)

struct BeamP {              // the offline kernels' parameters (k_beam; k_beam_lm and k_beam_boost extend them)
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

struct BeamState {          // one side of the offline kernels' double buffer
  long long pb[BEAM_W], pnb[BEAM_W], sc[BEAM_W];
  unsigned long long hash[BEAM_W], phash[BEAM_W];
  int len[BEAM_W], last[BEAM_W], node[BEAM_W];
};

// ---------------------------------------------------------------------------------------------------- the n-gram model
struct LmView {
  const int4* trans;        // [tmask + 1] node, word, prob_q, next
  const int4* words;        // [wmask + 1] hash lo, hash hi, word id, 0
  const int2* nodes;        // [n_nodes] backoff_q, suffix
  const int* l2w;           // [n_labels]
  int order, tprobe, wprobe, n_labels;
  unsigned tmask, wmask;
  long long alpha_q, beta_q;
  int start;                // the context of an empty prefix (0 for a header that fails the check)
  bool word_mode;
};

// the view of a packed model (validated on the host by qasr_lm_check); false: the header does not fit the bytes given, and
// the search ends empty
__device__ __forceinline__ bool lm_view(LmView& m, const int* hdr, long long lm_bytes, long long alpha_q, long long beta_q,
                                        int space) {
  m.order = hdr[2], m.tprobe = hdr[7], m.wprobe = hdr[10], m.n_labels = hdr[8];
  m.tmask = (unsigned)hdr[6] - 1u, m.wmask = (unsigned)hdr[9] - 1u;
  m.trans = reinterpret_cast<const int4*>(hdr + 32);
  m.words = m.trans + (size_t)hdr[6];
  m.nodes = reinterpret_cast<const int2*>(m.words + (size_t)hdr[9]);
  m.l2w = reinterpret_cast<const int*>(m.nodes + (size_t)hdr[4]);
  m.word_mode = hdr[3] != 0;
  m.alpha_q = alpha_q, m.beta_q = beta_q;
  const bool ok = hdr[0] == BEAM_LM_MAGIC && (long long)hdr[12] == lm_bytes && m.word_mode == (space >= 0) &&
                  hdr[5] >= 0 && hdr[5] < hdr[4] && m.order >= 1 && m.order <= 6;
  m.start = ok ? hdr[5] : 0;
  return ok;
}

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

// the term a raw model score adds to a candidate
__device__ __forceinline__ long long lm_term(const LmView& m, int raw) {
  return raw == BEAM_LM_NOTERM ? 0ll : ((((long long)raw * m.alpha_q + 32768ll) >> 16) + m.beta_q);
}

// ------------------------------------------------------------------------------------------------------ the phrase set
struct BoostView {
  const int4* table;        // [mask + 1] node, label, next, 0
  const int2* nodes;        // [n_nodes] pot_q, bank_q
  const int* root_next;     // [n_labels]
  int probe, n_labels, n_nodes;
  unsigned mask;
  int start;                // the state of an empty prefix
  bool whole;               // whole words: END takes a virtual space
};

// the view of a packed set (validated on the host by qasr_boost_check); false: the header does not describe exactly the
// bytes and the whole-words flag the host passed, and the search ends empty
__device__ __forceinline__ bool boost_view(BoostView& v, const int* bh, long long bytes, int whole_words, int space) {
  const int b_nodes = bh[3], b_cap = bh[7];
  v.start = bh[5];
  v.n_labels = bh[4], v.probe = bh[8], v.mask = (unsigned)b_cap - 1u, v.n_nodes = b_nodes;
  v.table = reinterpret_cast<const int4*>(bh + 32);
  v.nodes = reinterpret_cast<const int2*>(v.table + (size_t)(b_cap > 0 ? b_cap : 0));
  v.root_next = reinterpret_cast<const int*>(v.nodes + (size_t)(b_nodes > 0 ? b_nodes : 0));
  v.whole = bh[6] != 0;
  return bh[0] == BOOST_MAGIC && bh[1] == 1 && (long long)bh[2] == bytes && b_nodes >= 1 && v.n_labels >= 1 && b_cap >= 1 &&
         (b_cap & (b_cap - 1)) == 0 && v.probe >= 1 && v.probe <= b_cap && v.start >= 0 && v.start < b_nodes &&
         128ll + 16ll * b_cap + 8ll * b_nodes + 4ll * v.n_labels == bytes && v.whole == (whole_words != 0) &&
         (!v.whole || (space >= 0 && space < v.n_labels));
}

// delta(s, c): one bounded probe sequence, a miss is the root's row; the root itself reads its row only.  CLAMP: the result
// is clamped into the nodes, for the streaming kernels, whose states also come back from a block in memory.  k_beam_boost
// starts every search at the checked header's state and takes the look-up without it: the select on the hit path costs it
// a dependent load per probe (3 to 8 % of a launch with 1 000 and 10 000 phrases: taken_back in profiles/beam_dev_ab.json).
template <bool CLAMP>
__device__ __forceinline__ int boost_next(const BoostView& v, int s, int c) {
  if (c < 0 || c >= v.n_labels) return 0;
  int rn = v.root_next[c];
  if constexpr (CLAMP) rn = (unsigned)rn < (unsigned)v.n_nodes ? rn : 0;
  if (s == 0) return rn;
  unsigned long long x = (((unsigned long long)(unsigned)s << 32) | (unsigned long long)(unsigned)c) * BEAM_HMUL;
  x ^= x >> 32;
  unsigned k = (unsigned)x & v.mask;
  for (int pr = 0; pr < v.probe; ++pr) {
    const int4 e = v.table[k];
    if (e.x == s && e.y == c) return !CLAMP || (unsigned)e.z < (unsigned)v.n_nodes ? e.z : 0;
    if (e.x < 0) break;
    k = (k + 1) & v.mask;
  }
  return rn;
}

// ------------------------------------------------------------------------------------------------------- the selection
// The candidates of a frame: idx = i * (N + 1) + k, k == 0 the entry in slot i itself, else its extension by candidate k - 1.
// A row of candidates (one slot) belongs to 256 / rows threads, rows = nb rounded up to a power of two: thread (my_i, my_sub)
// scores k = my_sub, my_sub + tpr, ... < k_end with cand(k), which keeps the slot's state in registers (BEAM_NEG: no such
// candidate).  L is the kernel's LDS struct (hist, red_max, red_min, red_cnt, red_a, bin, kk, n_at, n_sel, sel_r, sel_idx).

// MSB-first radix select over this thread's candidates: the kk-th smallest key among those `keyfn` admits; returns the key,
// leaves in kk how many candidates of exactly that key belong to the kk, in n_at how many have that key
template <typename Lds, typename Key>
__device__ __forceinline__ unsigned long long beam_radix_select(Lds& L, Key keyfn, int nbits, int my_sub, int tpr, int k_end,
                                                                int& kk, int& n_at) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int passes = (nbits + 7) >> 3;          // <= 8
  unsigned long long prefix = 0;
  for (int pass = passes - 1; pass >= 0; --pass) {
    const int shift = pass * 8;
    __syncthreads();                            // the previous pass's bin / kk and histogram have been read
    L.hist[tid] = 0;                            // BEAM_NT == 256 bins
    __syncthreads();
    for (int k = my_sub; k < k_end; k += tpr) {
      unsigned long long key;
      if (keyfn(k, key) && (shift + 8 >= 64 || (key >> (shift + 8)) == prefix))
        atomicAdd(&L.hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const int mine = (int)L.hist[tid];
    int inc = mine;                             // inclusive prefix sum over the 256 bins, smallest key first
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
}

// The best W of the frame's candidates, found by a radix select on r = max score - score (as many 8-bit passes as the
// frame's score range needs; a tie at the cut is settled by a second select on the candidate index, the tie rule).  Returns
// false if no candidate lives (uniform: every thread read the same totals); else leaves the winners' (r, idx) in L.sel_r /
// L.sel_idx in any order, their count in L.n_sel (the caller zeroed it before its last barrier), the frame's best score in
// mx, and ends with a barrier.  The caller ranks them and writes the next beam.
template <typename Lds, typename Cand>
__device__ __forceinline__ bool beam_select(Lds& L, Cand cand, int my_i, int my_sub, int tpr, int k_end, int nb, int N1, int W,
                                            long long& mx) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long mn = LLONG_MAX;
  int cnt = 0;
  mx = LLONG_MIN;
  for (int k = my_sub; k < k_end; k += tpr) {
    const long long v = cand(k);
    if (v != BEAM_NEG) { ++cnt; mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
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
  if (cnt == 0) return false;
  // ---- the W-th smallest r = mx - score: its value rth; of the candidates with exactly rth, those up to index ith win
  unsigned long long rth = ~0ull;
  int ith = INT_MAX;
  if (cnt > W) {
    const long long top = mx;
    const unsigned long long range = (unsigned long long)(mx - mn);
    int need = W, n_at = cnt;                     // (a range of 0: every candidate has r == 0)
    rth = beam_radix_select(L, [&](int k, unsigned long long& key) {
      const long long v = cand(k);
      key = (unsigned long long)(top - v);
      return v != BEAM_NEG;
    }, range ? 64 - __clzll((long long)range) : 0, my_sub, tpr, k_end, need, n_at);
    if (n_at > need) {                            // a tie at the cut: the lower candidate indices win
      const int M = nb * N1;
      ith = (int)beam_radix_select(L, [&](int k, unsigned long long& key) {
        const long long v = cand(k);
        key = (unsigned long long)(my_i * N1 + k);
        return v != BEAM_NEG && (unsigned long long)(top - v) == rth;
      }, 32 - __clz(M), my_sub, tpr, k_end, need, n_at);
    }
  }
  // ---- collect the winners (in any order: the caller sorts them)
  for (int k = my_sub; k < k_end; k += tpr) {
    const long long v = cand(k);
    if (v != BEAM_NEG) {
      const unsigned long long r = (unsigned long long)(mx - v);
      const int idx = my_i * N1 + k;
      if (r < rth || (r == rth && idx <= ith)) {
        const int at = atomicAdd(&L.n_sel, 1);
        if (at < BEAM_W) L.sel_r[at] = r, L.sel_idx[at] = idx;
      }
    }
  }
  __syncthreads();
  return true;
}

}  // namespace qasr
