// Word and character error counts (k_edit_cut, k_edit, k_edit_totals); the host statement is EDIT_RULES and edit_host of
// qasr/edit.py, and this file follows it byte for byte.  D[i][j] over the first i hypothesis units and the first j reference
// units, unit costs, ties diagonal > deletion (i, j - 1) > insertion (i - 1, j); a cell carries (cost, S, D) of the path picked.
//
// k_edit_cut<MODE>: one WAVE per row (the B * K hypothesis rows, then the B reference rows), four to a work-group.  It checks
// the length and every id inside it - rows are device data - and leaves (units, state) per row in the workspace.  In word mode
// it also cuts the row: per 64-id chunk a __ballot of "not whitespace", word starts = mask & ~(mask << 1 | carry), a word's
// index = words before the chunk + popc of the starts below the lane; the lane behind a word's last id stores its end.  Then
// lane w hashes word w (FNV-1a over the ids, 64 bits) and stores (start, len, hash).  is_space is read at a checked id only.
// k_edit<MODE, NC>: one WAVE per problem p = b * K + k, four to a work-group, no LDS, no barrier.  Lane l owns the NC contiguous
// reference columns l * NC .. l * NC + NC - 1 of a strip of 64 * NC columns: their units and their (cost, S, D) of the row above
// stay in registers.  The hypothesis streams through skewed: at step s lane l works on hypothesis unit s - l.  A step's
// cross-lane traffic is one __shfl_up of lane l - 1's last column (its value one step ago is this step's diagonal) and one of
// the hypothesis unit.  Lane 0 takes both from a block of 64 rows that all lanes loaded 64 steps ahead (one coalesced read, then
// a read of lane s & 63): the hypothesis units, and behind the first strip the previous strip's last column, which lane 63 left
// in the workspace (3 int32 per hypothesis unit).  The column is rewritten in place: row r is read at step <= r and written at
// step r + 63 of the same wave; a __threadfence between strips makes the stores visible to the next strip's loads.
// k_edit_totals: one work-group; thread t sums the rows b = t, t + 256, ..., an LDS tree adds the 256 partial sums, thread w
// adds word w to totals[w].  No atomics anywhere; every store is a plain vector store; nothing is read on the host.
// Every loop is bounded by a row width, a unit count taken from a checked length, or a constant.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qasr_internal.h"

namespace qasr {

#define EDIT_NT 256
#define EDIT_WAVE 64
#define EDIT_WAVES (EDIT_NT / EDIT_WAVE)
#define EDIT_NC_MAX 16

// a row holds at most this many units: every id in char mode, every other id in word mode
static inline long long edit_units(int width, int mode) { return mode == QASR_EDIT_WORD ? ((long long)width + 1) / 2 : width; }
static inline size_t edit_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace: info int32 [2 P][2] | word mode: hypothesis words int4 [P][HU], reference words int4 [P][RU] | when a reference
// can span more than one strip (RU > 64 * 16): the strip column int32 [P][3 * (HU + 1)]
struct EditLayout {
  size_t info, hrec, rrec, carry, bytes;
  long long HU, RU;
};
static EditLayout edit_layout(long long P, int max_hyp, int max_ref, int mode) {
  EditLayout L{};
  L.HU = edit_units(max_hyp, mode), L.RU = edit_units(max_ref, mode);
  size_t at = 0;
  L.info = at, at += edit_up16((size_t)P * 2 * 2 * sizeof(int32_t));
  L.hrec = at;
  if (mode == QASR_EDIT_WORD) at += (size_t)P * L.HU * 16;
  L.rrec = at;
  if (mode == QASR_EDIT_WORD) at += (size_t)P * L.RU * 16;
  L.carry = at;
  if (L.RU > EDIT_WAVE * EDIT_NC_MAX) at += edit_up16((size_t)P * 3 * (L.HU + 1) * sizeof(int32_t));
  L.bytes = at;
  return L;
}
size_t edit_workspace_bytes(long long P, int max_hyp, int max_ref, int mode) { return edit_layout(P, max_hyp, max_ref, mode).bytes; }

struct EditP {
  const int32_t* hyp;
  const int32_t* hyp_lens;      // optional [P]
  const int32_t* ref;
  const int32_t* ref_lens;      // optional [B]
  const int32_t* n_hyps;        // optional [B]
  const uint8_t* is_space;      // [C], word mode
  int32_t* rows;                // [P][8]
  long long* totals;            // [16]
  int2* info;                   // [P + B]: (units, state: 1 valid, 0 invalid, 2 absent)
  int4* hrec;                   // [P][HU] (start, len, hash lo, hash hi)
  int4* rrec;                   // [B][RU]
  int32_t* carry;               // [P][3 * (HU + 1)]
  long long hyp_pitch, ref_pitch, HU, RU;
  int P, B, K, C, max_hyp, max_ref;
};

template <int MODE>
__global__ void __launch_bounds__(EDIT_NT) k_edit_cut(EditP p) {
  const int lane = threadIdx.x & (EDIT_WAVE - 1);
  const long long rl = (long long)blockIdx.x * EDIT_WAVES + (threadIdx.x / EDIT_WAVE);
  if (rl >= (long long)p.P + p.B) return;                           // wave-uniform; no barrier follows
  const int r = (int)rl;
  const bool is_ref = r >= p.P;
  const int q = is_ref ? r - p.P : r;                               // the row in its matrix
  if (!is_ref && p.n_hyps) {
    const int b = q / p.K, k = q - b * p.K;
    if (k >= p.n_hyps[b]) {                                         // an absent n-best row: nothing of it is read
      if (lane == 0) p.info[r] = make_int2(0, 2);
      return;
    }
  }
  const int32_t* const row = is_ref ? p.ref + (long long)q * p.ref_pitch : p.hyp + (long long)q * p.hyp_pitch;
  const int32_t* const lens = is_ref ? p.ref_lens : p.hyp_lens;
  const int W = is_ref ? p.max_ref : p.max_hyp;
  const int n = lens ? lens[q] : W;
  if (n < 0 || n > W) {
    if (lane == 0) p.info[r] = make_int2(0, 0);
    return;
  }
  const int C = p.C;
  if (MODE == QASR_EDIT_CHAR) {
    bool bad = false;
    for (int i = lane; i < n; i += EDIT_WAVE) {
      const int c = row[i];
      if (c < 0 || c >= C) bad = true;
    }
    const bool valid = __ballot(bad) == 0;
    if (lane == 0) p.info[r] = make_int2(valid ? n : 0, valid ? 1 : 0);
    return;
  }
  int4* const rec = is_ref ? p.rrec + (long long)q * p.RU : p.hrec + (long long)q * p.HU;   // <= (n + 1) / 2 <= RU (HU) words
  const unsigned long long below = (1ull << lane) - 1;
  unsigned long long carry = 0;                                     // bit 0: the id before the chunk is part of a word
  int count = 0;
  bool bad = false;
  for (int base = 0; base <= n; base += EDIT_WAVE) {                // position n, the end of the row, closes the last word
    const int pos = base + lane;
    bool word = false;
    if (pos < n) {
      const int c = row[pos];
      if (c < 0 || c >= C) bad = true;
      else word = p.is_space[c] == 0;
    }
    const unsigned long long m = __ballot(word), prev = (m << 1) | carry;
    const unsigned long long starts = m & ~prev, ends = ~m & prev;
    const int at = count + __popcll(starts & below);                // words that start below this position
    if ((starts >> lane) & 1) rec[at].x = pos;
    if ((ends >> lane) & 1) rec[at - 1].y = pos;                    // at >= 1: the word that ends here started below
    count += __popcll(starts), carry = m >> 63;
  }
  if (__ballot(bad) != 0) {
    if (lane == 0) p.info[r] = make_int2(0, 0);
    return;
  }
  __threadfence();                                                  // the starts and ends, written by other lanes of this wave
  for (int w = lane; w < count; w += EDIT_WAVE) {
    const int s = rec[w].x, e = rec[w].y;                           // 0 <= s < e <= n
    unsigned long long h = 14695981039346656037ull;
    for (int i = s; i < e; ++i) h = (h ^ (unsigned)row[i]) * 1099511628211ull;
    rec[w] = make_int4(s, e - s, (int)(unsigned)h, (int)(unsigned)(h >> 32));
  }
  if (lane == 0) p.info[r] = make_int2(count, 1);
}

struct EditCell {
  int c, s, d;                                                      // cost, substitutions, deletions of the path picked
};
__device__ __forceinline__ EditCell edit_shfl_up(const EditCell& a) {
  return EditCell{__shfl_up(a.c, 1), __shfl_up(a.s, 1), __shfl_up(a.d, 1)};
}
__device__ __forceinline__ EditCell edit_shfl(const EditCell& a, int src) {
  return EditCell{__shfl(a.c, src), __shfl(a.s, src), __shfl(a.d, src)};
}
__device__ __forceinline__ int4 edit_shfl_up(const int4& a) {
  return make_int4(__shfl_up(a.x, 1), __shfl_up(a.y, 1), __shfl_up(a.z, 1), __shfl_up(a.w, 1));
}
__device__ __forceinline__ int4 edit_shfl(const int4& a, int src) {
  return make_int4(__shfl(a.x, src), __shfl(a.y, src), __shfl(a.z, src), __shfl(a.w, src));
}
__device__ __forceinline__ int edit_shfl_up(int a) { return __shfl_up(a, 1); }
__device__ __forceinline__ int edit_shfl(int a, int src) { return __shfl(a, src); }

template <int MODE, int NC>
__global__ void __launch_bounds__(EDIT_NT) k_edit(EditP p) {
  using Unit = typename std::conditional<MODE == QASR_EDIT_WORD, int4, int>::type;   // a word's record, or an id
  const int lane = threadIdx.x & (EDIT_WAVE - 1);
  const long long pl = (long long)blockIdx.x * EDIT_WAVES + (threadIdx.x / EDIT_WAVE);
  if (pl >= p.P) return;                                            // wave-uniform; no barrier follows
  const int pr = (int)pl, b = pr / p.K;
  int4* const out = (int4*)(p.rows + (size_t)pr * QASR_EDIT_ROW_WORDS);
  const int2 hi = p.info[pr], ri = p.info[p.P + b];
  const int ok = hi.y == 2 ? 2 : (hi.y == 1 && ri.y == 1 ? 1 : 0);
  const int n = hi.x, m = ri.x;                                     // units: n <= HU, m <= RU (k_edit_cut counted them)
  if (ok != 1 || n == 0 || m == 0) {                                // nothing to walk: n insertions or m deletions
    if (lane == 0) {
      out[0] = ok == 1 ? make_int4(n + m, 0, m, n) : make_int4(0, 0, 0, 0);
      out[1] = ok == 1 ? make_int4(m, n, 1, 0) : make_int4(0, 0, ok, 0);
    }
    return;
  }
  const int32_t* const hrow = p.hyp + (long long)pr * p.hyp_pitch;
  const int32_t* const rrow = p.ref + (long long)b * p.ref_pitch;
  const int4* const hrec = p.hrec + (long long)pr * p.HU;
  const int4* const rrec = p.rrec + (long long)b * p.RU;
  int32_t* const col = p.carry + (long long)pr * 3 * (p.HU + 1);    // touched only when m > 64 * NC, which needs NC = 16
  auto hyp_unit = [&](int i) -> Unit {                              // unit i of the hypothesis; behind n: never compared
    if constexpr (MODE == QASR_EDIT_WORD) return i < n ? hrec[i] : make_int4(0, -2, 0, 0);
    else return i < n ? hrow[i] : -2;
  };
  auto ref_unit = [&](int j) -> Unit {                              // unit j of the reference; behind m: equal to nothing
    if constexpr (MODE == QASR_EDIT_WORD) return j < m ? rrec[j] : make_int4(0, -1, 0, 0);
    else return j < m ? rrow[j] : -1;
  };
  auto differ = [&](const Unit& h, const Unit& r) -> int {
    if constexpr (MODE == QASR_EDIT_WORD) {
      if (h.y != r.y || h.z != r.z || h.w != r.w) return 1;         // length and hash first
      for (int t = 0; t < h.y; ++t)                                 // then the ids: both words lie inside their checked rows
        if (hrow[h.x + t] != rrow[r.x + t]) return 1;
      return 0;
    } else {
      return h != r;
    }
  };

  EditCell cur[NC];
  int res_c = 0, res_s = 0, res_d = 0;
  for (int base = 0; base < m; base += EDIT_WAVE * NC) {
    const bool first = base == 0, last = base + EDIT_WAVE * NC >= m;
    const int cols = min(m - base, EDIT_WAVE * NC), lanes = (cols + NC - 1) / NC;
    const int j0 = base + lane * NC;                                // this lane's first column (0-based; D's column j0 + 1)
    Unit ru[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      ru[k] = ref_unit(j0 + k);
      cur[k] = EditCell{j0 + k + 1, 0, j0 + k + 1};                 // row 0: deletions only
    }
    EditCell diag{j0, 0, j0};                                       // D[0][j0]: the diagonal of this lane's first row
    Unit hu = hyp_unit(0), hblk = hu, hnxt = hyp_unit(lane);        // hblk / hnxt: units s0 + lane of this and the next 64 steps
    EditCell cblk{0, 0, 0}, cnxt{0, 0, 0};                          // the same of the previous strip's last column
    if (!first && lane < n) cnxt = EditCell{col[3 * lane], col[3 * lane + 1], col[3 * lane + 2]};
    const int steps = n + lanes - 1;
    for (int s = 0; s < steps; ++s) {
      if ((s & (EDIT_WAVE - 1)) == 0) {
        const int r = s + EDIT_WAVE + lane;                         // the rows of the 64 steps after these
        hblk = hnxt, hnxt = hyp_unit(r);
        cblk = cnxt;
        if (!first && r < n) cnxt = EditCell{col[3 * r], col[3 * r + 1], col[3 * r + 2]};   // row r is rewritten at step r + 63
      }
      const int src = s & (EDIT_WAVE - 1);
      const Unit hup = edit_shfl_up(hu), h0 = edit_shfl(hblk, src);
      EditCell left = edit_shfl_up(cur[NC - 1]);                    // lane l - 1's last column, of the row this lane enters
      const EditCell c0 = edit_shfl(cblk, src);
      hu = lane == 0 ? h0 : hup;
      if (lane == 0) left = first ? EditCell{s + 1, 0, 0} : c0;     // column 0 of D: insertions only
      const int i = s - lane;                                       // this lane's hypothesis unit
      if (i >= 0 && i < n) {
        EditCell o = diag, l = left;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const EditCell u = cur[k];
          const int neq = differ(hu, ru[k]);
          EditCell v{o.c + neq, o.s + neq, o.d};                    // the diagonal: a hit or a substitution
          if (l.c + 1 < v.c) v = EditCell{l.c + 1, l.s, l.d + 1};   // the deletion, only when strictly cheaper
          if (u.c + 1 < v.c) v = EditCell{u.c + 1, u.s, u.d};       // the insertion, likewise
          cur[k] = v, o = u, l = v;
        }
        diag = left;
        if (!last && lane == EDIT_WAVE - 1)                         // a full strip: its last column, for the next strip
          col[3 * i] = cur[NC - 1].c, col[3 * i + 1] = cur[NC - 1].s, col[3 * i + 2] = cur[NC - 1].d;   // i < n <= HU
      }
    }
    if (last) {
      const int fl = (m - 1 - base) / NC, fk = (m - 1 - base) - fl * NC;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k == fk) res_c = cur[k].c, res_s = cur[k].s, res_d = cur[k].d;
      if (lane == fl) {
        out[0] = make_int4(res_c, res_s, res_d, res_c - res_s - res_d);
        out[1] = make_int4(m, n, 1, 0);
      }
    } else {
      __threadfence();                                              // the column, stored by lane 63, is read by all lanes next
    }
  }
}

#define EDIT_SUMS 9
__global__ void __launch_bounds__(EDIT_NT) k_edit_totals(EditP p) {
  __shared__ long long red[EDIT_SUMS][EDIT_NT];
  const int tid = threadIdx.x;
  long long acc[EDIT_SUMS];
#pragma unroll
  for (int w = 0; w < EDIT_SUMS; ++w) acc[w] = 0;
  for (int b = tid; b < p.B; b += EDIT_NT) {
    const int4* const row = (const int4*)(p.rows + (size_t)b * p.K * QASR_EDIT_ROW_WORDS);
    long long best = -1, invalid = 0;
    for (int k = 0; k < p.K; ++k) {
      const int4 x = row[2 * k], y = row[2 * k + 1];                // errors S D I | ref_units hyp_units ok 0
      if (y.z == 1) {
        if (best < 0 || x.x < best) best = x.x;
        if (k == 0) acc[0] += x.x, acc[1] += y.x, acc[2] += x.y, acc[3] += x.z, acc[4] += x.w, acc[5] += y.y, acc[6] += 1;
      }
      invalid += y.z == 0;
    }
    if (best >= 0) acc[7] += best;
    acc[8] += invalid;
  }
#pragma unroll
  for (int w = 0; w < EDIT_SUMS; ++w) red[w][tid] = acc[w];
  __syncthreads();
  for (int half = EDIT_NT / 2; half >= 1; half >>= 1) {
    if (tid < half)
#pragma unroll
      for (int w = 0; w < EDIT_SUMS; ++w) red[w][tid] += red[w][tid + half];
    __syncthreads();
  }
  if (tid < QASR_EDIT_TOTAL_WORDS) p.totals[tid] += tid < EDIT_SUMS ? red[tid < EDIT_SUMS ? tid : 0][0] : 0;
}

template <int MODE>
static void edit_launch_dp(hipStream_t s, const EditP& p, dim3 grid) {
  const dim3 block(EDIT_NT);
  if (p.RU <= 1 * EDIT_WAVE) hipLaunchKernelGGL((k_edit<MODE, 1>), grid, block, 0, s, p);
  else if (p.RU <= 4 * EDIT_WAVE) hipLaunchKernelGGL((k_edit<MODE, 4>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_edit<MODE, EDIT_NC_MAX>), grid, block, 0, s, p);
}

int launch_edit(hipStream_t s, const qasr_edit_args& a) {
  const long long P = (long long)a.B * a.K;
  const EditLayout L = edit_layout(P, a.max_hyp, a.max_ref, a.mode);
  char* const ws = (char*)a.workspace;
  EditP p{};
  p.hyp = a.hyp, p.hyp_lens = a.hyp_lens, p.ref = a.ref, p.ref_lens = a.ref_lens, p.n_hyps = a.n_hyps, p.is_space = a.is_space;
  p.rows = a.rows, p.totals = (long long*)a.totals;
  p.info = (int2*)(ws + L.info), p.hrec = (int4*)(ws + L.hrec), p.rrec = (int4*)(ws + L.rrec), p.carry = (int32_t*)(ws + L.carry);
  p.hyp_pitch = a.hyp_pitch, p.ref_pitch = a.ref_pitch, p.HU = L.HU, p.RU = L.RU;
  p.P = (int)P, p.B = a.B, p.K = a.K, p.C = a.C, p.max_hyp = a.max_hyp, p.max_ref = a.max_ref;
  const dim3 block(EDIT_NT), rows_grid((unsigned)((P + a.B + EDIT_WAVES - 1) / EDIT_WAVES)), grid((unsigned)((P + EDIT_WAVES - 1) / EDIT_WAVES));
  if (a.mode == QASR_EDIT_WORD) {
    hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_WORD>, rows_grid, block, 0, s, p);
    edit_launch_dp<QASR_EDIT_WORD>(s, p, grid);
  } else {
    hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_CHAR>, rows_grid, block, 0, s, p);
    edit_launch_dp<QASR_EDIT_CHAR>(s, p, grid);
  }
  hipLaunchKernelGGL(k_edit_totals, dim3(1), block, 0, s, p);
  return QASR_OK;
}

// ---- the edit path (k_edit_trace); the host statement is TRACE_RULES and trace_host of qasr/edit.py ---------------------------
// k_edit_trace<MODE, NC>: k_edit's frame step, stated a second time, with the choice of every cell - 0 hit, 1 substitution,
// 2 deletion, 3 insertion: the op the path takes INTO the cell - kept in a back-pointer plane, then the walk from (n, m) back to
// (0, 0) by the same wave.  One WAVE per problem, four to a work-group, no LDS, no barrier.
// The plane is step-major: [strip][step][lane], one word per lane and step that holds the lane's NC choices at 2 bits each
// (NC = 16: a uint32; NC = 4 and 1: a uint8), so a step is one coalesced store.  The cell of hypothesis unit i and reference
// column c (both 0-based) lies at strip = c / (64 NC), lane = c % (64 NC) / NC, bits 2 (c % NC), step = i + lane.
// A strip has HU + 63 steps: step = i + lane <= (n - 1) + 63 with n <= HU.
// The walk is serial, at most n + m ops.  Its length is known before it starts: n_ops = ref_units + I, so the ops go straight
// to their forward place ops[n_ops - 1 - t] (t counts from the last cell), 64 at a time from a register per lane: no reversed
// copy.  The plane is read through a window in registers: lane q holds the words of step s0 - q of the lanes L and L - 1, a
// choice is one __shfl of it; a step back lowers the step by 0 .. 2 and the lane by 0 .. 1, so a path near the diagonal loads a
// window every 17 .. 32 ops at NC = 16, every 5 .. 8 at NC = 4 and every 2 at NC = 1.  The loop is bounded by n + m <= HU + RU <= ops_pitch; i and j never fall below 0 whatever the
// plane holds, and every index into the plane is formed from them: step = i + lane < HU + 63.
struct EditTraceP {
  EditP e;
  uint8_t* ops;                 // [P][ops_pitch]
  int32_t* n_ops;               // [P]
  char* plane;                  // [P][plane_pitch] bytes
  long long ops_pitch, plane_pitch, S;   // S = HU + 63 steps per strip
};

static inline int edit_nc(long long RU) { return RU <= 1 * EDIT_WAVE ? 1 : (RU <= 4 * EDIT_WAVE ? 4 : EDIT_NC_MAX); }
static inline size_t edit_plane_pitch(long long HU, long long RU) {
  const long long nc = edit_nc(RU), strips = (RU + EDIT_WAVE * nc - 1) / (EDIT_WAVE * nc);
  return edit_up16((size_t)strips * (size_t)(HU + EDIT_WAVE - 1) * EDIT_WAVE * (nc == EDIT_NC_MAX ? 4 : 1));
}
// workspace: qasr_edit_distance's | the planes [P][plane_pitch]
size_t edit_trace_workspace_bytes(long long P, int max_hyp, int max_ref, int mode) {
  const EditLayout L = edit_layout(P, max_hyp, max_ref, mode);
  return edit_up16(L.bytes) + (size_t)P * edit_plane_pitch(L.HU, L.RU);
}

template <int MODE, int NC>
__global__ void __launch_bounds__(EDIT_NT) k_edit_trace(EditTraceP tp) {
  using Unit = typename std::conditional<MODE == QASR_EDIT_WORD, int4, int>::type;   // a word's record, or an id
  using Word = typename std::conditional<NC == EDIT_NC_MAX, uint32_t, uint8_t>::type;   // a lane's choices of one step
  static_assert(2 * NC <= 8 * sizeof(Word), "a lane's choices fit its word");
  const EditP& p = tp.e;
  const int lane = threadIdx.x & (EDIT_WAVE - 1);
  const long long pl = (long long)blockIdx.x * EDIT_WAVES + (threadIdx.x / EDIT_WAVE);
  if (pl >= p.P) return;                                            // wave-uniform; no barrier follows
  const int pr = (int)pl, b = pr / p.K;
  int4* const out = (int4*)(p.rows + (size_t)pr * QASR_EDIT_ROW_WORDS);
  uint8_t* const ops = tp.ops + (long long)pr * tp.ops_pitch;
  const int2 hi = p.info[pr], ri = p.info[p.P + b];
  const int ok = hi.y == 2 ? 2 : (hi.y == 1 && ri.y == 1 ? 1 : 0);
  const int n = hi.x, m = ri.x;                                     // units: n <= HU, m <= RU (k_edit_cut counted them)
  if (ok != 1 || n == 0 || m == 0) {                                // nothing to walk: n insertions or m deletions
    if (lane == 0) {
      out[0] = ok == 1 ? make_int4(n + m, 0, m, n) : make_int4(0, 0, 0, 0);
      out[1] = ok == 1 ? make_int4(m, n, 1, 0) : make_int4(0, 0, ok, 0);
      tp.n_ops[pr] = ok == 1 ? n + m : 0;
    }
    if (ok == 1)
      for (int t = lane; t < n + m; t += EDIT_WAVE) ops[t] = n == 0 ? 2 : 3;   // n + m <= HU + RU <= ops_pitch
    return;
  }
  const int32_t* const hrow = p.hyp + (long long)pr * p.hyp_pitch;
  const int32_t* const rrow = p.ref + (long long)b * p.ref_pitch;
  const int4* const hrec = p.hrec + (long long)pr * p.HU;
  const int4* const rrec = p.rrec + (long long)b * p.RU;
  int32_t* const col = p.carry + (long long)pr * 3 * (p.HU + 1);    // touched only when m > 64 * NC, which needs NC = 16
  Word* const plane = (Word*)(tp.plane + (long long)pr * tp.plane_pitch);
  const long long S = tp.S;
  auto hyp_unit = [&](int i) -> Unit {                              // unit i of the hypothesis; behind n: never compared
    if constexpr (MODE == QASR_EDIT_WORD) return i < n ? hrec[i] : make_int4(0, -2, 0, 0);
    else return i < n ? hrow[i] : -2;
  };
  auto ref_unit = [&](int j) -> Unit {                              // unit j of the reference; behind m: equal to nothing
    if constexpr (MODE == QASR_EDIT_WORD) return j < m ? rrec[j] : make_int4(0, -1, 0, 0);
    else return j < m ? rrow[j] : -1;
  };
  auto differ = [&](const Unit& h, const Unit& r) -> int {
    if constexpr (MODE == QASR_EDIT_WORD) {
      if (h.y != r.y || h.z != r.z || h.w != r.w) return 1;         // length and hash first
      for (int t = 0; t < h.y; ++t)                                 // then the ids: both words lie inside their checked rows
        if (hrow[h.x + t] != rrow[r.x + t]) return 1;
      return 0;
    } else {
      return h != r;
    }
  };

  // ---- forward: k_edit's strips and skewed steps; every step stores its choices
  EditCell cur[NC];
  int res_c = 0, res_s = 0, res_d = 0, res_lane = 0;
  int strip = 0;
  for (int base = 0; base < m; base += EDIT_WAVE * NC, ++strip) {
    const bool first = base == 0, last = base + EDIT_WAVE * NC >= m;
    const int cols = min(m - base, EDIT_WAVE * NC), lanes = (cols + NC - 1) / NC;
    const int j0 = base + lane * NC;                                // this lane's first column (0-based; D's column j0 + 1)
    Word* const sp = plane + (long long)strip * S * EDIT_WAVE;      // the strip's steps
    Unit ru[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      ru[k] = ref_unit(j0 + k);
      cur[k] = EditCell{j0 + k + 1, 0, j0 + k + 1};                 // row 0: deletions only
    }
    EditCell diag{j0, 0, j0};                                       // D[0][j0]: the diagonal of this lane's first row
    Unit hu = hyp_unit(0), hblk = hu, hnxt = hyp_unit(lane);        // hblk / hnxt: units s0 + lane of this and the next 64 steps
    EditCell cblk{0, 0, 0}, cnxt{0, 0, 0};                          // the same of the previous strip's last column
    if (!first && lane < n) cnxt = EditCell{col[3 * lane], col[3 * lane + 1], col[3 * lane + 2]};
    const int steps = n + lanes - 1;                                // <= HU + 63 = S
    for (int s = 0; s < steps; ++s) {
      if ((s & (EDIT_WAVE - 1)) == 0) {
        const int r = s + EDIT_WAVE + lane;                         // the rows of the 64 steps after these
        hblk = hnxt, hnxt = hyp_unit(r);
        cblk = cnxt;
        if (!first && r < n) cnxt = EditCell{col[3 * r], col[3 * r + 1], col[3 * r + 2]};   // row r is rewritten at step r + 63
      }
      const int src = s & (EDIT_WAVE - 1);
      const Unit hup = edit_shfl_up(hu), h0 = edit_shfl(hblk, src);
      EditCell left = edit_shfl_up(cur[NC - 1]);                    // lane l - 1's last column, of the row this lane enters
      const EditCell c0 = edit_shfl(cblk, src);
      hu = lane == 0 ? h0 : hup;
      if (lane == 0) left = first ? EditCell{s + 1, 0, 0} : c0;     // column 0 of D: insertions only
      const int i = s - lane;                                       // this lane's hypothesis unit
      if (i >= 0 && i < n) {
        EditCell o = diag, l = left;
        uint32_t picks = 0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const EditCell u = cur[k];
          const int neq = differ(hu, ru[k]);
          EditCell v{o.c + neq, o.s + neq, o.d};                    // the diagonal: a hit or a substitution
          uint32_t pick = (uint32_t)neq;
          if (l.c + 1 < v.c) v = EditCell{l.c + 1, l.s, l.d + 1}, pick = 2;   // the deletion, only when strictly cheaper
          if (u.c + 1 < v.c) v = EditCell{u.c + 1, u.s, u.d}, pick = 3;       // the insertion, likewise
          picks |= pick << (2 * k);
          cur[k] = v, o = u, l = v;
        }
        diag = left;
        sp[(long long)s * EDIT_WAVE + lane] = (Word)picks;          // s < S, lane < 64: inside the strip
        if (!last && lane == EDIT_WAVE - 1)                         // a full strip: its last column, for the next strip
          col[3 * i] = cur[NC - 1].c, col[3 * i + 1] = cur[NC - 1].s, col[3 * i + 2] = cur[NC - 1].d;   // i < n <= HU
      }
    }
    if (last) {
      const int fl = (m - 1 - base) / NC, fk = (m - 1 - base) - fl * NC;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k == fk) res_c = cur[k].c, res_s = cur[k].s, res_d = cur[k].d;
      res_lane = fl;
      if (lane == fl) {
        out[0] = make_int4(res_c, res_s, res_d, res_c - res_s - res_d);
        out[1] = make_int4(m, n, 1, 0);
      }
    }
    __threadfence();                                                // the column and the plane, stored by other lanes of this wave
  }

  // ---- the walk: from (n, m) back; i hypothesis units and j reference units are left
  res_c = __shfl(res_c, res_lane), res_s = __shfl(res_s, res_lane), res_d = __shfl(res_d, res_lane);
  const int total = min(max(m + (res_c - res_s - res_d), 0), n + m);   // n_ops = ref_units + I; the bound holds by TRACE_RULES
  int i = n, j = m;
  int wstrip = -1, wl = 0, ws0 = 0;                                 // the window: strip, lane L, first step s0
  uint32_t wa = 0, wb = 0;                                          // step s0 - lane of lane L and of lane L - 1
  uint32_t mine = 0;                                                // this lane's op of the 64 in flight
  for (int t = 0; t < total; ++t) {
    uint32_t op;
    if (i == 0) op = 2;
    else if (j == 0) op = 3;
    else {
      const int c = j - 1, st = c / (EDIT_WAVE * NC), rem = c - st * (EDIT_WAVE * NC), l = rem / NC, k = rem - l * NC;
      const int step = i - 1 + l;                                   // 0 <= step <= n - 1 + 63 < S
      if (st != wstrip || l > wl || l < wl - 1 || step > ws0 || step <= ws0 - EDIT_WAVE) {
        wstrip = st, wl = l, ws0 = step;
        const Word* const sp = plane + (long long)st * S * EDIT_WAVE;
        const int q = step - lane;
        wa = q >= 0 ? (uint32_t)sp[(long long)q * EDIT_WAVE + l] : 0u;
        wb = q >= 0 && l >= 1 ? (uint32_t)sp[(long long)q * EDIT_WAVE + l - 1] : 0u;
      }
      const uint32_t w = (uint32_t)__shfl((int)(l == wl ? wa : wb), ws0 - step);
      op = (w >> (2 * k)) & 3u;
    }
    i -= op != 2, j -= op != 3;                                     // op 2 is taken at j >= 1 only, op 3 at i >= 1 only
    if (lane == (t & (EDIT_WAVE - 1))) mine = op;
    if ((t & (EDIT_WAVE - 1)) == EDIT_WAVE - 1 || t == total - 1) {
      const int t0 = t & ~(EDIT_WAVE - 1);
      if (t0 + lane <= t) ops[total - 1 - (t0 + lane)] = (uint8_t)mine;   // 0 <= total - 1 - t' < total <= ops_pitch
    }
  }
  if (lane == 0) tp.n_ops[pr] = total;
}

template <int MODE>
static void edit_launch_trace(hipStream_t s, const EditTraceP& tp, dim3 grid) {
  const dim3 block(EDIT_NT);
  switch (edit_nc(tp.e.RU)) {
    case 1: hipLaunchKernelGGL((k_edit_trace<MODE, 1>), grid, block, 0, s, tp); break;
    case 4: hipLaunchKernelGGL((k_edit_trace<MODE, 4>), grid, block, 0, s, tp); break;
    default: hipLaunchKernelGGL((k_edit_trace<MODE, EDIT_NC_MAX>), grid, block, 0, s, tp);
  }
}

int launch_edit_trace(hipStream_t s, const qasr_edit_trace_args& a) {
  const long long P = (long long)a.B * a.K;
  const EditLayout L = edit_layout(P, a.max_hyp, a.max_ref, a.mode);
  char* const ws = (char*)a.workspace;
  EditTraceP tp{};
  EditP& p = tp.e;
  p.hyp = a.hyp, p.hyp_lens = a.hyp_lens, p.ref = a.ref, p.ref_lens = a.ref_lens, p.n_hyps = a.n_hyps, p.is_space = a.is_space;
  p.rows = a.rows, p.totals = nullptr;
  p.info = (int2*)(ws + L.info), p.hrec = (int4*)(ws + L.hrec), p.rrec = (int4*)(ws + L.rrec), p.carry = (int32_t*)(ws + L.carry);
  p.hyp_pitch = a.hyp_pitch, p.ref_pitch = a.ref_pitch, p.HU = L.HU, p.RU = L.RU;
  p.P = (int)P, p.B = a.B, p.K = a.K, p.C = a.C, p.max_hyp = a.max_hyp, p.max_ref = a.max_ref;
  tp.ops = a.ops, tp.n_ops = a.n_ops, tp.plane = ws + edit_up16(L.bytes);
  tp.ops_pitch = a.ops_pitch, tp.plane_pitch = (long long)edit_plane_pitch(L.HU, L.RU), tp.S = L.HU + EDIT_WAVE - 1;
  const dim3 block(EDIT_NT), rows_grid((unsigned)((P + a.B + EDIT_WAVES - 1) / EDIT_WAVES)), grid((unsigned)((P + EDIT_WAVES - 1) / EDIT_WAVES));
  if (a.mode == QASR_EDIT_WORD) {
    hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_WORD>, rows_grid, block, 0, s, p);
    edit_launch_trace<QASR_EDIT_WORD>(s, tp, grid);
  } else {
    hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_CHAR>, rows_grid, block, 0, s, p);
    edit_launch_trace<QASR_EDIT_CHAR>(s, tp, grid);
  }
  return QASR_OK;
}

// k_edit_cut over P hypothesis rows alone (no reference rows: the guard P + B holds with B = 0), for qasr_mbr.hip
void launch_edit_cut_rows(hipStream_t s, int mode, const int32_t* rows, const int32_t* lens, const int32_t* n_hyps,
                          const uint8_t* is_space, int2* info, int4* rec, long long pitch, long long HU, int P, int K, int C,
                          int width) {
  EditP p{};
  p.hyp = rows, p.hyp_lens = lens, p.n_hyps = n_hyps, p.is_space = is_space, p.info = info, p.hrec = rec;
  p.hyp_pitch = pitch, p.HU = HU, p.P = P, p.B = 0, p.K = K, p.C = C, p.max_hyp = width;
  const dim3 block(EDIT_NT), grid((unsigned)(((long long)P + EDIT_WAVES - 1) / EDIT_WAVES));
  if (mode == QASR_EDIT_WORD) hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_WORD>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_edit_cut<QASR_EDIT_CHAR>, grid, block, 0, s, p);
}

}  // namespace qasr
