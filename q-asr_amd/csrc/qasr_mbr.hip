// Minimum Bayes risk re-ranking of n-best rows (k_edit_cut of qasr_edit.hip, k_mbr_pair, k_mbr_pick); the host statement is
// MBR_RULES and mbr_host of qasr/mbr.py, and this file follows it byte for byte.
//
// k_edit_cut<MODE>, as it is, over the B * K rows (no reference rows): it checks the length and every id of a row and leaves
// (units, state) per row in the workspace, in word mode also the words as (start, len, hash).
// k_mbr_pair<MODE, NC>: one WAVE per unordered pair (b, i < j), four to a work-group, no LDS, no barrier.  It is k_edit's
// skewed schedule with a cost-only cell: lane l owns the NC contiguous columns l * NC .. l * NC + NC - 1 of a strip of 64 * NC
// columns - their units and their cost of the row above stay in registers -, the other row streams through the lanes: at step
// s lane l works on streamed unit s - l.  A step's cross-lane traffic is one __shfl_up of lane l - 1's last column (its value
// one step ago is this step's diagonal) and one of the streamed unit; lane 0 takes both from a block of 64 rows that all lanes
// loaded 64 steps ahead.  The distance is symmetric, so the columns come from the row with FEWER units: fewer strips.  Rows of
// more than 64 * 16 units go in strips through a workspace column of one int32 per streamed unit, rewritten in place: row r is
// read at step <= r and written at step r + 63 of the same wave; a __threadfence between strips makes the stores visible.
// The wave writes dist[b][i][j] and dist[b][j][i]; a pair with a row that is not present writes -1 and returns before any id.
// k_mbr_pick: one work-group per utterance: weights and wsum, the K risks (K * K products, two partial sums per row added in
// LDS in a fixed order), the order by counting - each present row counts the rows that precede it under (risk ascending, score
// descending, k ascending) -, the diagonal of dist and the fills of the rows that are not present.
// No atomics anywhere; every store is a plain vector store; nothing is read on the host; every output element is written
// exactly once per call.  Every loop is bounded by K, a unit count that k_edit_cut took from a checked length, or a constant.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "qasr_internal.h"

namespace qasr {

#define MBR_NT 256
#define MBR_WAVE 64
#define MBR_WAVES (MBR_NT / MBR_WAVE)
#define MBR_NC_MAX 16
#define MBR_SCORE_FLOOR (-(1ll << 61))

static inline long long mbr_units(int width, int mode) { return mode == QASR_EDIT_WORD ? ((long long)width + 1) / 2 : width; }
static inline size_t mbr_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace: info int2 [B K] | word mode: words int4 [B K][U] | rows that can span more than one strip (U > 64 * 16): the
// strip column int32 [pairs][U] | without a caller's dist: the matrix int32 [B][K][K]
struct MbrLayout {
  size_t info, rec, carry, dist, bytes;
  long long U, pairs;
};
static MbrLayout mbr_layout(int B, int K, int max_ids, int mode) {
  MbrLayout L{};
  const size_t P = (size_t)B * K;
  L.U = mbr_units(max_ids, mode), L.pairs = (long long)B * K * (K - 1) / 2;
  size_t at = 0;
  L.info = at, at += mbr_up16(P * sizeof(int2));
  L.rec = at;
  if (mode == QASR_EDIT_WORD) at += P * (size_t)L.U * 16;
  L.carry = at;
  if (L.U > MBR_WAVE * MBR_NC_MAX) at += mbr_up16((size_t)L.pairs * (size_t)L.U * sizeof(int32_t));
  L.dist = at, at += mbr_up16(P * K * sizeof(int32_t));
  L.bytes = at;
  return L;
}
size_t mbr_workspace_bytes(int B, int K, int max_ids, int mode) { return mbr_layout(B, K, max_ids, mode).bytes; }

struct MbrP {
  const int32_t* labels;        // [B K][pitch]
  const long long* score;       // [B K]
  const uint8_t* is_space;
  const uint32_t* wtab;         // [16384]
  const int2* info;             // [B K]: (units, state: 1 valid, 0 invalid, 2 absent), k_edit_cut's
  const int4* rec;              // [B K][U] (start, len, hash lo, hash hi), k_edit_cut's
  int32_t* carry;               // [pairs][U]
  int32_t* dist;                // [B][K][K]
  int32_t* weight;              // [B][K]
  long long* wsum;              // [B]
  long long* risk;              // [B][K]
  int32_t* order;               // [B][K]
  int32_t* ok;                  // [B][K]
  long long pitch, U, pairs;    // pairs = B * PP
  int B, K, PP, scale_q;        // PP = K (K - 1) / 2 pairs per utterance
};

__device__ __forceinline__ int4 mbr_shfl_up(const int4& a) {
  return make_int4(__shfl_up(a.x, 1), __shfl_up(a.y, 1), __shfl_up(a.z, 1), __shfl_up(a.w, 1));
}
__device__ __forceinline__ int4 mbr_shfl(const int4& a, int src) {
  return make_int4(__shfl(a.x, src), __shfl(a.y, src), __shfl(a.z, src), __shfl(a.w, src));
}
__device__ __forceinline__ int mbr_shfl_up(int a) { return __shfl_up(a, 1); }
__device__ __forceinline__ int mbr_shfl(int a, int src) { return __shfl(a, src); }

template <int MODE, int NC>
__global__ void __launch_bounds__(MBR_NT) k_mbr_pair(MbrP p) {
  using Unit = typename std::conditional<MODE == QASR_EDIT_WORD, int4, int>::type;   // a word's record, or an id
  const int lane = threadIdx.x & (MBR_WAVE - 1);
  const long long gl = (long long)blockIdx.x * MBR_WAVES + (threadIdx.x / MBR_WAVE);
  if (gl >= p.pairs) return;                                        // wave-uniform; no barrier follows
  const int K = p.K;
  const int b = (int)(gl / p.PP);
  int rem = (int)(gl - (long long)b * p.PP), pi = 0;                // the pair's number inside b -> (pi < pj), at most K steps
  while (rem >= K - 1 - pi) rem -= K - 1 - pi, ++pi;
  const int pj = pi + 1 + rem;                                      // pi < pj < K
  const long long ra = (long long)b * K + pi, rb = (long long)b * K + pj;
  int32_t* const dm = p.dist + (long long)b * K * K;
  const int2 ia = p.info[ra], ib = p.info[rb];
  const bool present = ia.y == 1 && ib.y == 1 && p.score[ra] > MBR_SCORE_FLOOR && p.score[rb] > MBR_SCORE_FLOOR;
  if (!present) {                                                   // nothing of either row is read
    if (lane == 0) dm[pi * K + pj] = -1, dm[pj * K + pi] = -1;
    return;
  }
  const bool swap = ib.x < ia.x;                                    // the columns: the row with fewer units
  const long long rc = swap ? rb : ra, rs = swap ? ra : rb;
  const int m = swap ? ib.x : ia.x, n = swap ? ia.x : ib.x;         // m <= n <= U (k_edit_cut counted them)
  if (m == 0) {                                                     // nothing to walk: n insertions
    if (lane == 0) dm[pi * K + pj] = n, dm[pj * K + pi] = n;
    return;
  }
  const int32_t* const srow = p.labels + rs * p.pitch;              // the streamed row
  const int32_t* const crow = p.labels + rc * p.pitch;              // the row of the columns
  const int4* const srec = p.rec + rs * p.U;
  const int4* const crec = p.rec + rc * p.U;
  int32_t* const col = p.carry + gl * p.U;                          // touched only when m > 64 * NC, which needs NC = 16
  auto s_unit = [&](int i) -> Unit {                                // unit i of the streamed row; behind n: never compared
    if constexpr (MODE == QASR_EDIT_WORD) return i < n ? srec[i] : make_int4(0, -2, 0, 0);
    else return i < n ? srow[i] : -2;
  };
  auto c_unit = [&](int j) -> Unit {                                // unit j of the columns' row; behind m: equal to nothing
    if constexpr (MODE == QASR_EDIT_WORD) return j < m ? crec[j] : make_int4(0, -1, 0, 0);
    else return j < m ? crow[j] : -1;
  };
  auto differ = [&](const Unit& h, const Unit& r) -> int {
    if constexpr (MODE == QASR_EDIT_WORD) {
      if (h.y != r.y || h.z != r.z || h.w != r.w) return 1;         // length and hash first
      for (int t = 0; t < h.y; ++t)                                 // then the ids: both words lie inside their checked rows
        if (srow[h.x + t] != crow[r.x + t]) return 1;
      return 0;
    } else {
      return h != r;
    }
  };

  int cur[NC];
  for (int base = 0; base < m; base += MBR_WAVE * NC) {
    const bool first = base == 0, last = base + MBR_WAVE * NC >= m;
    const int cols = min(m - base, MBR_WAVE * NC), lanes = (cols + NC - 1) / NC;
    const int j0 = base + lane * NC;                                // this lane's first column (0-based; D's column j0 + 1)
    Unit cu[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      cu[k] = c_unit(j0 + k);
      cur[k] = j0 + k + 1;                                          // row 0 of D
    }
    int diag = j0;                                                  // D[0][j0]: the diagonal of this lane's first row
    Unit su = s_unit(0), sblk = su, snxt = s_unit(lane);            // sblk / snxt: units s0 + lane of this and the next 64 steps
    int cblk = 0, cnxt = 0;                                         // the same of the previous strip's last column
    if (!first && lane < n) cnxt = col[lane];
    const int steps = n + lanes - 1;
    for (int s = 0; s < steps; ++s) {
      if ((s & (MBR_WAVE - 1)) == 0) {
        const int r = s + MBR_WAVE + lane;                          // the rows of the 64 steps after these
        sblk = snxt, snxt = s_unit(r);
        cblk = cnxt;
        if (!first && r < n) cnxt = col[r];                         // row r is rewritten at step r + 63
      }
      const int src = s & (MBR_WAVE - 1);
      const Unit sup = mbr_shfl_up(su), s0 = mbr_shfl(sblk, src);
      int left = __shfl_up(cur[NC - 1], 1);                         // lane l - 1's last column, of the row this lane enters
      const int c0 = __shfl(cblk, src);
      su = lane == 0 ? s0 : sup;
      if (lane == 0) left = first ? s + 1 : c0;                     // column 0 of D
      const int i = s - lane;                                       // this lane's streamed unit
      if (i >= 0 && i < n) {
        int o = diag, l = left;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const int u = cur[k];
          const int v = min(min(o + differ(su, cu[k]), l + 1), u + 1);
          cur[k] = v, o = u, l = v;
        }
        diag = left;
        if (!last && lane == MBR_WAVE - 1) col[i] = cur[NC - 1];    // a full strip: its last column; i < n <= U
      }
    }
    if (last) {
      const int fl = (m - 1 - base) / NC, fk = (m - 1 - base) - fl * NC;
      int res = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k == fk) res = cur[k];
      if (lane == fl) dm[pi * K + pj] = res, dm[pj * K + pi] = res;
    } else {
      __threadfence();                                              // the column, stored by lane 63, is read by all lanes next
    }
  }
}

#define MBR_MAX_K 128
static_assert(MBR_MAX_K == QASR_BEAM_MAX_WIDTH && 2 * MBR_MAX_K == MBR_NT, "two threads per row");

__global__ void __launch_bounds__(MBR_NT) k_mbr_pick(MbrP p) {
  __shared__ long long s_score[MBR_MAX_K], s_risk[MBR_MAX_K], s_part[MBR_NT];
  __shared__ int s_w[MBR_MAX_K], s_ok[MBR_MAX_K];
  const int tid = threadIdx.x, b = blockIdx.x, K = p.K;
  const long long r0 = (long long)b * K;
  int32_t* const dm = p.dist + r0 * K;
  if (tid < K) {
    const int state = p.info[r0 + tid].y;
    const long long sc = p.score[r0 + tid];
    s_score[tid] = sc;
    s_ok[tid] = state == 2 ? 2 : (state == 1 && sc > MBR_SCORE_FLOOR ? 1 : 0);
  }
  __syncthreads();
  if (tid < K) {                                                    // the weight: smax over the present rows, then the table
    bool any = false;
    long long smax = 0;
    for (int k = 0; k < K; ++k)
      if (s_ok[k] == 1 && (!any || s_score[k] > smax)) smax = s_score[k], any = true;
    int w = 0;
    if (s_ok[tid] == 1) {
      unsigned long long d = (unsigned long long)smax - (unsigned long long)s_score[tid];   // >= 0: exact without a sign
      if (d > (1ull << 40)) d = 1ull << 40;
      const unsigned long long x = (d * (unsigned long long)p.scale_q + (1ull << 15)) >> 16;   // < 2^60
      w = x >= (16ull << 16) ? 0 : (int)p.wtab[x >> 6];             // x >> 6 < 16384
    }
    s_w[tid] = w;
  }
  __syncthreads();
  {                                                                 // row i = tid / 2 sums its columns half * 64 .. + 63
    const int i = tid >> 1, j0 = (tid & 1) * (MBR_MAX_K / 2);
    long long acc = 0;
    if (i < K && s_ok[i] == 1)
      for (int j = j0; j < min(j0 + MBR_MAX_K / 2, K); ++j)
        if (j != i && s_ok[j] == 1) acc += (long long)s_w[j] * dm[i * K + j];
    s_part[tid] = acc;
  }
  __syncthreads();
  if (tid < K) s_risk[tid] = s_ok[tid] == 1 ? s_part[2 * tid] + s_part[2 * tid + 1] : -1;
  __syncthreads();
  if (tid < K) {
    int n_present = 0, before = 0;
    long long wsum = 0;
    const long long rk = s_risk[tid], sk = s_score[tid];
    for (int j = 0; j < K; ++j) {
      if (s_ok[j] != 1) continue;
      ++n_present, wsum += s_w[j];
      const long long rj = s_risk[j], sj = s_score[j];
      before += rj < rk || (rj == rk && (sj > sk || (sj == sk && j < tid)));
    }
    const bool present = s_ok[tid] == 1;
    if (present) p.order[r0 + before] = tid;                        // the ranks of the present rows are 0 .. n_present - 1
    if (tid >= n_present) p.order[r0 + tid] = -1;
    p.weight[r0 + tid] = s_w[tid], p.risk[r0 + tid] = rk, p.ok[r0 + tid] = s_ok[tid];
    dm[tid * K + tid] = present ? 0 : -1;
    if (tid == 0) p.wsum[b] = wsum;
  }
}

template <int MODE>
static void mbr_launch_pair(hipStream_t s, const MbrP& p, dim3 grid) {
  const dim3 block(MBR_NT);
  if (p.U <= 1 * MBR_WAVE) hipLaunchKernelGGL((k_mbr_pair<MODE, 1>), grid, block, 0, s, p);
  else if (p.U <= 4 * MBR_WAVE) hipLaunchKernelGGL((k_mbr_pair<MODE, 4>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((k_mbr_pair<MODE, MBR_NC_MAX>), grid, block, 0, s, p);
}

int launch_mbr(hipStream_t s, const qasr_mbr_args& a) {
  const MbrLayout L = mbr_layout(a.B, a.K, a.max_ids, a.mode);
  char* const ws = (char*)a.workspace;
  int2* const info = (int2*)(ws + L.info);
  int4* const rec = (int4*)(ws + L.rec);
  launch_edit_cut_rows(s, a.mode, a.labels, a.n_labels, a.n_hyps, a.is_space, info, rec, a.label_pitch, L.U, a.B * a.K, a.K, a.C,
                       a.max_ids);
  MbrP p{};
  p.labels = a.labels, p.score = (const long long*)a.score, p.is_space = a.is_space, p.wtab = a.wtab, p.info = info, p.rec = rec;
  p.carry = (int32_t*)(ws + L.carry), p.dist = a.dist ? a.dist : (int32_t*)(ws + L.dist);
  p.weight = a.weight, p.wsum = (long long*)a.wsum, p.risk = (long long*)a.risk, p.order = a.order, p.ok = a.ok;
  p.pitch = a.label_pitch, p.U = L.U, p.pairs = L.pairs;
  p.B = a.B, p.K = a.K, p.PP = a.K * (a.K - 1) / 2, p.scale_q = a.scale_q;
  if (L.pairs > 0) {
    const dim3 grid((unsigned)((L.pairs + MBR_WAVES - 1) / MBR_WAVES));
    if (a.mode == QASR_EDIT_WORD) mbr_launch_pair<QASR_EDIT_WORD>(s, p, grid);
    else mbr_launch_pair<QASR_EDIT_CHAR>(s, p, grid);
  }
  hipLaunchKernelGGL(k_mbr_pick, dim3((unsigned)a.B), dim3(MBR_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
