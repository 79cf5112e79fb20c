// Streaming at any sample rate (k_stream_rs_append, k_stream_rs_fir); the host statement is qasr/stream_rs.py
// (RS_STREAM_RULES), and this file follows it byte for byte, both states included.  The arithmetic of an output is that of
// k_resample: qasr_resample_dev.h states it once for both files.
//
// Resampler state: S blocks of RS_ST_WORDS 32-bit words (in_received i64, the slot's sample format + 1, zeros), then S
// histories of hcap 8-byte entries; input frame k lives at entry k % hcap as its channel sum (int64 for int16 input, float64
// for float32 input).  The stream state (blocks of 80 words and sample rings) is that of qasr_stream.hip, unchanged.
//
// The outputs of one row are worth several work-groups, while `received` has one owner; so the work is cut in two launches
// and no work-group reads a word that another work-group of the same launch writes:
// k_stream_rs_append: one work-group of 256 threads per row (the rows' slots are distinct).  It clamps the append, stores the
//   channel sums into the history, advances in_received, decides how many outputs k the row produces, writes the row's job
//   record (first output, k, format, in_received, slot) into the workspace, advances the stream block's `received` by k (the
//   outputs themselves are written by the next launch: stream order puts them before anything that reads the ring) and
//   writes n_taken / n_out / status.
// k_stream_rs_fir<STAGED>: one work-group per (row, tile of 256 outputs); thread tid owns output first + 256 tile + tid.  It
//   reads the job record, the history and the table only.  STAGED: the tile's stretch of history, frames q(first) - W + 1 ..
//   q(last) + W (zeros outside [0, in_received)), is read once into LDS, then the tap loop of k_resample runs on it; the host
//   picks the direct instantiation, which reads the history per tap, by k_resample's own inequality.  The result goes to the
//   sample ring at ring[i % cap].  A tile behind k returns at once.
// Global memory sees plain vector stores; no atomics; nothing is read back on the host.
#include "qasr_internal.h"
#include "qasr_resample_dev.h"

namespace qasr {

#define SR_NT 256
#define SR_TILE 256
#define SR_STAGE 4096
#define SR_ST_WORDS 80          // the stream block of qasr_stream.hip: received i64 in words 0-1
#define RS_ST_WORDS 16
#define RS_ST_FMT 2
#define SR_JOB_WORDS 8
#define SR_MAX_HCAP (1 << 26)

struct RsPushP {
  int32_t* state;               // stream blocks + rings
  int32_t* rs_state;            // resampler blocks + histories
  int32_t* work;                // [B][SR_JOB_WORDS]
  const int32_t* blob;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* n_in;
  const int32_t* out_limit;
  const void* chunk;
  int32_t* n_taken;
  int32_t* n_out;
  int32_t* status;
  long long pitch;
  int S, C, cap, hcap, Ain, L, M, W, Wf, ch, fmt;       // W: the header's; Wf: the filter's reach (0 for equal rates)
};

__device__ __forceinline__ long long sr_nonneg(long long v) { return v < 0 ? 0 : v; }

template <typename T>
__device__ __forceinline__ void sr_store_frames(const RsPushP& p, int b, long long* hist, long long in0, int n, int tid) {
  const T* const row = (const T*)p.chunk + (long long)b * p.pitch * p.ch;
  for (int f = tid; f < n; f += SR_NT) {
    long long* const e = hist + (in0 + f) % p.hcap;
    if constexpr (sizeof(T) == 2) *e = (long long)rs_frame(row, (long long)f, p.ch);
    else *(double*)e = rs_frame(row, (long long)f, p.ch);
  }
}

__global__ void __launch_bounds__(SR_NT) k_stream_rs_append(RsPushP p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t* const job = p.work + (long long)b * SR_JOB_WORDS;
  const int slot = p.slots[b];
  ResampleP hp{};
  hp.blob = p.blob, hp.L = p.L, hp.M = p.M, hp.W = p.W;
  const bool slot_ok = slot >= 0 && slot < p.S, hdr_ok = rs_header_ok(hp);
  if (!slot_ok || !hdr_ok) {
    if (tid < SR_JOB_WORDS) job[tid] = tid == 6 ? -1 : 0;
    if (tid == 0) {
      p.n_taken[b] = 0;
      p.n_out[b] = 0;
      p.status[b] = slot_ok ? 4 : 2;
    }
    return;
  }
  int32_t* const blk = p.state + (long long)slot * SR_ST_WORDS;
  int32_t* const rsb = p.rs_state + (long long)slot * RS_ST_WORDS;
  long long* const hist = (long long*)(p.rs_state + (long long)p.S * RS_ST_WORDS) + (long long)slot * p.hcap;
  const int flags = p.flags[b];
  const bool begin = (flags & QASR_STREAM_BEGIN) != 0;
  const long long r0 = begin ? 0 : sr_nonneg(*(const long long*)blk);
  const long long in0 = begin ? 0 : sr_nonneg(*(const long long*)rsb);
  const int fmt0 = begin ? 0 : rsb[RS_ST_FMT];
  __syncthreads();                                  // every thread has read the counters before anyone writes the blocks
  if (begin) {
    if (tid >= 2 && tid < SR_ST_WORDS) blk[tid] = 0;
    if (tid >= 3 && tid < RS_ST_WORDS) rsb[tid] = 0;
  }
  const long long L = p.L, M = p.M;
  const bool fmt_ok = fmt0 == 0 || fmt0 == p.fmt + 1;
  const int fmt = fmt0 ? fmt0 - 1 : p.fmt;
  const int want = fmt_ok ? (int)max(0ll, min((long long)p.n_in[b], min(p.pitch, (long long)p.Ain))) : 0;
  // frames from `keep` on are still read by an output >= r0 (equal rates: output r0 is frame r0)
  const long long keep = p.Wf ? max(0ll, (r0 * M) / L - p.Wf + 1) : r0;
  const int n = (int)min((long long)want, max(0ll, keep + p.hcap - in0));
  if (fmt == QASR_PCM_S16) sr_store_frames<int16_t>(p, b, hist, in0, n, tid);
  else sr_store_frames<float>(p, b, hist, in0, n, tid);
  const long long in1 = in0 + n;
  long long target;
  if (flags & QASR_STREAM_FLUSH) target = (in1 * L + M - 1) / M;
  else target = in1 > p.Wf ? ((in1 - p.Wf) * L + M - 1) / M : 0;
  const int k = (int)max(0ll, min(target - r0, (long long)min(p.out_limit[b], p.C)));
  if (tid == 0) {
    *(long long*)job = r0;
    job[2] = k, job[3] = fmt;
    *(long long*)(job + 4) = in1;
    job[6] = slot, job[7] = 0;
    *(long long*)blk = r0 + k;
    *(long long*)rsb = in1;
    rsb[RS_ST_FMT] = fmt + 1;
    p.n_taken[b] = n;
    p.n_out[b] = k;
    p.status[b] = !fmt_ok ? 3 : (n < want ? 1 : 0);
  }
}

template <typename T>
__device__ __forceinline__ typename RsAcc<T>::stage_t sr_entry(const long long* hist, long long k, int hcap) {
  const long long* const e = hist + k % hcap;
  if constexpr (sizeof(T) == 2) return (int32_t)*e;
  else return *(const double*)e;
}

// equal rates: the bypass of RULES from a channel sum
__device__ __forceinline__ float sr_equal(int32_t sum, int ch) {
  const float s = (float)sum * 3.0517578125e-05f;       // 2^-15: exact
  return ch > 1 ? s / (float)ch : s;
}
__device__ __forceinline__ float sr_equal(double sum, int ch) { return ch > 1 ? (float)(sum / (double)ch) : (float)sum; }

template <typename T, bool STAGED>
__device__ __forceinline__ void sr_fir_tile(const RsPushP& p, const long long* hist, float* ring, long long first, int k, long long n,
                                            void* lds) {
  typedef typename RsAcc<T>::acc_t acc_t;
  typedef typename RsAcc<T>::stage_t stage_t;
  stage_t* const xs = (stage_t*)lds;
  const int tid = threadIdx.x;
  const long long L = p.L, M = p.M;
  const int W = p.Wf, ch = p.ch;
  const long long i0 = first + (long long)blockIdx.x * SR_TILE, i = i0 + tid;
  const long long iend = first + k;                 // one behind the row's last output
  if (W == 0) {                                     // uniform: equal rates, output i is frame i < n
    if (i < iend) ring[(int)(i % p.cap)] = i < n ? sr_equal(sr_entry<T>(hist, i, p.hcap), ch) : 0.f;
    return;
  }
  const long long i1 = min(i0 + SR_TILE - 1, iend - 1);
  const long long k_lo = (i0 * M) / L - W + 1;
  if (STAGED) {
    const int count = (int)((i1 * M) / L + W - k_lo + 1);             // <= SR_STAGE: the host chose this instantiation by it
    for (int s = tid; s < count && s < SR_STAGE; s += SR_NT) {
      const long long kk = k_lo + s;
      xs[s] = (kk >= 0 && kk < n) ? sr_entry<T>(hist, kk, p.hcap) : (stage_t)0;
    }
    __syncthreads();
  }
  if (i >= iend) return;
  const long long pp = i * M, q = pp / L;
  const int r = (int)(i % L);
  const int32_t* tab = p.blob + 32 + r;
  acc_t acc = 0;
  if (STAGED) {
    const stage_t* x = xs + (int)(q + W - k_lo);                      // tap j reads x[-j]: inside [0, count)
#pragma unroll 4
    for (int j = 0; j < 2 * W; ++j) acc = rs_tap(acc, tab[(size_t)j * (size_t)L], x[-j]);
  } else {
    for (int j = 0; j < 2 * W; ++j) {
      const long long kk = q + W - j;
      const stage_t x = (kk >= 0 && kk < n) ? sr_entry<T>(hist, kk, p.hcap) : (stage_t)0;
      acc = rs_tap(acc, tab[(size_t)j * (size_t)L], x);
    }
  }
  ring[(int)(i % p.cap)] = rs_finish(acc, ch);
}

template <bool STAGED>
__global__ void __launch_bounds__(SR_NT) k_stream_rs_fir(RsPushP p) {
  __shared__ double lds[STAGED ? SR_STAGE : 1];
  const int32_t* const job = p.work + (long long)blockIdx.y * SR_JOB_WORDS;
  const int k = job[2];
  if ((long long)blockIdx.x * SR_TILE >= k) return;                   // uniform: nothing (left) to produce for this row
  const int slot = job[6];
  if (slot < 0 || slot >= p.S) return;
  const long long first = *(const long long*)job, n = *(const long long*)(job + 4);
  const long long* const hist = (const long long*)(p.rs_state + (long long)p.S * RS_ST_WORDS) + (long long)slot * p.hcap;
  float* const ring = (float*)(p.state + (long long)p.S * SR_ST_WORDS) + (long long)slot * p.cap;
  if (job[3] == QASR_PCM_S16) sr_fir_tile<int16_t, STAGED>(p, hist, ring, first, k, n, lds);
  else sr_fir_tile<float, STAGED>(p, hist, ring, first, k, n, lds);
}

size_t stream_rs_state_bytes(int S, int hcap) {
  if (S < 1 || hcap < 4 || hcap % 4 || hcap > SR_MAX_HCAP) return 0;
  return (size_t)S * (4 * RS_ST_WORDS + 8 * (size_t)hcap);
}

size_t stream_rs_work_bytes(int B) { return B < 1 ? 0 : (size_t)B * 4 * SR_JOB_WORDS; }

static bool stream_rs_staged(int L, int M, int W) {                   // resample_staged's inequality
  return ((long long)(SR_TILE - 1) * M + L - 1) / L + 1 + 2ll * W <= SR_STAGE;
}

int launch_stream_rs_push(hipStream_t s, const qasr_stream_rs_push_args& a) {
  RsPushP p{};
  p.state = (int32_t*)a.state, p.rs_state = (int32_t*)a.rs_state, p.work = (int32_t*)a.work, p.blob = (const int32_t*)a.blob;
  p.slots = a.slots, p.flags = a.flags, p.n_in = a.n_in, p.out_limit = a.out_limit, p.chunk = a.chunk;
  p.n_taken = a.n_taken, p.n_out = a.n_out, p.status = a.status, p.pitch = a.pitch;
  p.S = a.S, p.C = a.C, p.cap = (a.Wl + a.C + 3) / 4 * 4, p.hcap = a.hcap;
  p.Ain = (int)max(1ll, min((long long)a.C * a.M / a.L, (long long)INT32_MAX));
  p.L = a.L, p.M = a.M, p.W = a.W, p.Wf = (a.L == 1 && a.M == 1) ? 0 : a.W, p.ch = a.channels, p.fmt = a.dtype;
  hipLaunchKernelGGL(k_stream_rs_append, dim3((unsigned)a.B), dim3(SR_NT), 0, s, p);
  const dim3 grid((unsigned)((a.C + SR_TILE - 1) / SR_TILE), (unsigned)a.B), block(SR_NT);
  if (stream_rs_staged(a.L, a.M, p.Wf)) hipLaunchKernelGGL(k_stream_rs_fir<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_stream_rs_fir<false>, grid, block, 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
