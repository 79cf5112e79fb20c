// Streaming recognition, buffered (k_stream_push, k_stream_window, k_stream_emit); the host statement is qasr/stream.py
// (STREAM_RULES), and this file follows it byte for byte, the state block included.
//
// State: S blocks of ST_WORDS 32-bit words, then S rings of cap floats (cap = Wl + C rounded up to a multiple of 4); sample i
// of a stream lives at ring[i % cap].  Every block and ring is written by the one work-group that owns the slot in that
// launch (the rows' slots are distinct), with plain vector stores; no atomics; nothing is read back on the host.
//
// k_stream_push: one work-group of 256 threads per row.  The ring position of the first new sample decides the path: up to
// three scalars bring the position to a multiple of 4; from there a thread moves four samples as one 16-byte store (cap is a
// multiple of 4, so such a quad never wraps) fed by one 16-byte load (float32) or one 8-byte load (int16) when the source
// is aligned there too, scalars otherwise.  `received` is advanced by thread 0 behind a barrier.
//
// k_stream_window: one work-group per (row, tile of SM_TILE = 1024 samples); thread tid owns four consecutive samples, as in
// k_cut.  Reads the counters, writes none.
//
// k_stream_emit: one work-group per row: k_ctc's chunked ballot / segmented-scan collapse over the final range [lo, hi), with
// the carry (labels so far in this step, first frame and running maximum of the open run) seeded from the slot's state and
// stored back at the end.  Chunks are cut from lo, so a chunk's lanes are NOT the frames' t % 64: the 64 partial sums are
// indexed by the global frame, lane l of wave 0 walking t = l (mod 64) from lo upwards.  Wave 1 lists the provisional tail.
#include <climits>

#include "qasr_internal.h"

namespace qasr {

#define SM_NT 256
#define SM_TILE 1024
#define SM_MAX_WAVES 16
#define ST_WORDS 80
#define ST_RECV 0
#define ST_DONE 2
#define ST_OPEN 3
#define ST_FIRST 4
#define ST_MAX 5
#define ST_NLAB 6
#define ST_PART 16

__device__ __forceinline__ int sm_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

__device__ __forceinline__ long long sm_received(const int32_t* blk) {
  const long long r = *(const long long*)(blk + ST_RECV);
  return r < 0 ? 0 : r;
}

struct PushP {
  int32_t* state;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* n_new;
  const void* chunk;
  long long pitch;
  int S, C, cap, is_s16;
};

__device__ __forceinline__ float sm_s16(short v) { return (float)v / 32768.0f; }

__global__ void __launch_bounds__(SM_NT) k_stream_push(PushP p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int slot = p.slots[b];
  if (slot < 0 || slot >= p.S) return;
  int32_t* blk = p.state + (long long)slot * ST_WORDS;
  float* ring = (float*)(p.state + (long long)p.S * ST_WORDS) + (long long)slot * p.cap;
  const bool begin = (p.flags[b] & QASR_STREAM_BEGIN) != 0;
  const long long r0 = begin ? 0 : sm_received(blk);
  const int n = (int)max(0ll, min((long long)p.n_new[b], min(p.pitch, (long long)p.C)));
  __syncthreads();                                  // every thread has read `received` before anyone writes the block
  if (begin && tid >= 2 && tid < ST_WORDS) blk[tid] = 0;
  const int p0 = (int)(r0 % p.cap);
  const int head = min(n, (4 - (p0 & 3)) & 3);
  if (p.is_s16) {
    const short* src = (const short*)p.chunk + (long long)b * p.pitch;
    const bool vec = (((uintptr_t)(src + head)) & 7) == 0 && (((uintptr_t)ring) & 15) == 0;
    const int nq = vec ? (n - head) >> 2 : 0, body = head + 4 * nq;
    for (int q = tid; q < nq; q += SM_NT) {
      const int i = head + 4 * q;
      const short4 v = *(const short4*)(src + i);
      *(float4*)(ring + (int)(((long long)p0 + i) % p.cap)) = make_float4(sm_s16(v.x), sm_s16(v.y), sm_s16(v.z), sm_s16(v.w));
    }
    for (int i = tid; i < head; i += SM_NT) ring[(int)(((long long)p0 + i) % p.cap)] = sm_s16(src[i]);
    for (int i = body + tid; i < n; i += SM_NT) ring[(int)(((long long)p0 + i) % p.cap)] = sm_s16(src[i]);
  } else {
    const float* src = (const float*)p.chunk + (long long)b * p.pitch;
    const bool vec = (((uintptr_t)(src + head)) & 15) == 0 && (((uintptr_t)ring) & 15) == 0;
    const int nq = vec ? (n - head) >> 2 : 0, body = head + 4 * nq;
    for (int q = tid; q < nq; q += SM_NT) {
      const int i = head + 4 * q;
      *(float4*)(ring + (int)(((long long)p0 + i) % p.cap)) = *(const float4*)(src + i);
    }
    for (int i = tid; i < head; i += SM_NT) ring[(int)(((long long)p0 + i) % p.cap)] = src[i];
    for (int i = body + tid; i < n; i += SM_NT) ring[(int)(((long long)p0 + i) % p.cap)] = src[i];
  }
  __syncthreads();
  if (tid == 0) *(long long*)(blk + ST_RECV) = r0 + n;
}

struct WindowP {
  const int32_t* state;
  const int32_t* slots;
  float* windows;
  int32_t* window_lens;
  int32_t* first_frame;
  int S, Wl, cap, spf;
};

__global__ void __launch_bounds__(SM_NT) k_stream_window(WindowP p) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int slot = p.slots[b];
  long long start = 0, n = 0;
  const float* ring = (const float*)(p.state + (long long)p.S * ST_WORDS);
  if (slot >= 0 && slot < p.S) {
    const long long r = sm_received(p.state + (long long)slot * ST_WORDS);
    if (r > p.Wl) start = (r - p.Wl + p.spf - 1) / p.spf * p.spf;
    n = min(r - start, (long long)p.Wl);
    ring += (long long)slot * p.cap;
  }
  if (blockIdx.x == 0 && tid == 0) {
    p.window_lens[b] = (int32_t)n;
    p.first_frame[b] = (int32_t)(start / p.spf);
  }
  const long long i = (long long)blockIdx.x * SM_TILE + 4ll * tid;
  if (i >= p.Wl) return;
  float* dst = p.windows + (long long)b * p.Wl + i;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) {
    const int q = (int)((start + i) % p.cap);
    if (i + 4 <= n && (q & 3) == 0 && (((uintptr_t)(ring + q)) & 15) == 0) {   // cap is a multiple of 4: the quad does not wrap
      v = *(const float4*)(ring + q);
    } else {
      v.x = ring[q];
      if (i + 1 < n) v.y = ring[(int)((q + 1ll) % p.cap)];
      if (i + 2 < n) v.z = ring[(int)((q + 2ll) % p.cap)];
      if (i + 3 < n) v.w = ring[(int)((q + 3ll) % p.cap)];
    }
  }
  if (i + 4 <= p.Wl && (((uintptr_t)dst) & 15) == 0) {
    *(float4*)dst = v;
  } else {
    dst[0] = v.x;
    if (i + 1 < p.Wl) dst[1] = v.y;
    if (i + 2 < p.Wl) dst[2] = v.z;
    if (i + 3 < p.Wl) dst[3] = v.w;
  }
}

struct EmitP {
  int32_t* state;
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* tokens;      // [B][Tw]
  const float* fs;            // [B][Tw]
  const int32_t* enc_lens;
  const int32_t* first_frame;
  int32_t* labels;            // [B][P]
  int32_t* start;
  int32_t* nframes;
  float* score;
  int32_t* n_new_labels;      // [B]
  int32_t* status;
  int32_t* total_frames;
  float* utt_score;
  int32_t* tail_labels;       // optional [B][Ptail]
  int32_t* tail_n;
  int S, Tw, P, Ptail, Rr, spf, blank;
};

__global__ void __launch_bounds__(SM_NT) k_stream_emit(EmitP p) {
  __shared__ int sm_cnt[2][SM_MAX_WAVES], sm_last[2][SM_MAX_WAVES], sm_max[2][SM_MAX_WAVES];
  __shared__ float sm_part[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int b = blockIdx.x, P = p.P;
  const size_t row = (size_t)b * P;
  const int slot = p.slots[b];
  const bool slot_ok = slot >= 0 && slot < p.S;
  int32_t* blk = p.state + (long long)(slot_ok ? slot : 0) * ST_WORDS;
  const bool end = (p.flags[b] & QASR_STREAM_END) != 0;
  const long long r = sm_received(blk);
  const int first = p.first_frame[b];
  const int e = min(max(p.enc_lens[b], 0), p.Tw);
  const int lo = blk[ST_DONE];
  const int open_tok = blk[ST_OPEN] - 1;            // -1: no run is open
  const int open_first = blk[ST_FIRST], open_max = blk[ST_MAX];
  const int nlab0 = blk[ST_NLAB];
  const long long top = (long long)first + e;
  const long long lim = r >= p.Rr ? (r - p.Rr) / p.spf : -1;
  const long long hi64 = end ? max((long long)lo, top) : max((long long)lo, min(top, lim));
  const int hi = (int)min(hi64, (long long)INT_MAX);
  __syncthreads();                                  // the header is read before thread 0 may rewrite it
  if (!slot_ok || lo < first || first < 0) {       // frames were lost (or there is no such slot): an empty step, state untouched
    for (int i = tid; i < P; i += blockDim.x) {
      p.labels[row + i] = p.blank;
      p.start[row + i] = 0;
      p.nframes[row + i] = 0;
      p.score[row + i] = 0.f;
    }
    if (p.tail_labels)
      for (int i = tid; i < p.Ptail; i += blockDim.x) p.tail_labels[(size_t)b * p.Ptail + i] = p.blank;
    if (tid == 0) {
      p.n_new_labels[b] = 0;
      p.status[b] = slot_ok ? 1 : 2;
      p.total_frames[b] = 0;
      p.utt_score[b] = 0.f;
      if (p.tail_n) p.tail_n[b] = 0;
    }
    return;
  }
  // lo >= first and hi <= first + Tw: local indices t - first lie in 0 .. Tw
  const int n = hi - lo;
  const int32_t* const tok = p.tokens + (size_t)b * p.Tw - first;       // indexed by the global frame
  const float* const fs = p.fs + (size_t)b * p.Tw - first;
  const int carried = open_tok >= 0 ? 1 : 0;
  const int prev0 = carried ? open_tok : p.blank;
  // the carried run closes at lo when frame lo differs from it (on END with nothing final: at hi)
  const bool close0 = carried && (n > 0 ? tok[lo] != open_tok : end);
  if (close0 && tid == 0 && P > 0) {
    p.labels[row] = open_tok;
    p.start[row] = open_first;
    p.nframes[row] = lo - open_first;
    p.score[row] = __int_as_float(sm_key(open_max));
  }
  const int nchunks = (n + 63) >> 6, rounds = (nchunks + nw - 1) / nw;
  int base = carried, cs = open_first, cm = carried ? open_max : INT_MIN;
  for (int rd = 0; rd < rounds; ++rd) {
    const int i0 = (rd * nw + wave) << 6, i = i0 + lane, t = lo + i;
    const bool valid = i < n;
    int me = p.blank, v = INT_MIN;
    bool is_start = false, is_end = false;
    if (valid) {
      me = tok[t];
      if (me != p.blank) {
        is_start = (i == 0 ? prev0 : tok[t - 1]) != me;
        is_end = i + 1 == n ? end : tok[t + 1] != me;
      }
      v = sm_key(__float_as_int(fs[t]));
    }
    const unsigned long long smask = __ballot(is_start);
    const unsigned long long le = smask & ((2ull << lane) - 1ull);
    const int h = le ? 63 - __clzll((long long)le) : -1;
    const int hs = max(h, 0);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d);
      if (lane - d >= hs) v = max(v, o);
    }
    const int buf = rd & 1;
    if (lane == 63) {
      sm_cnt[buf][wave] = __popcll(smask);
      sm_last[buf][wave] = h >= 0 ? lo + i0 + h : -1;
      sm_max[buf][wave] = v;
    }
    __syncthreads();
    int mybase = 0, mycs = 0, mycm = INT_MIN;
    for (int w = 0; w < nw; ++w) {
      if (w == wave) { mybase = base; mycs = cs; mycm = cm; }
      base += sm_cnt[buf][w];
      const int last = sm_last[buf][w], mx = sm_max[buf][w];
      if (last >= 0) { cs = last; cm = mx; } else { cm = max(cm, mx); }
    }
    if (is_end) {
      const int idx = mybase + __popcll(le) - 1;
      if (idx >= 0 && idx < P) {
        const int rs = h >= 0 ? lo + i0 + h : mycs;
        p.labels[row + idx] = me;
        p.start[row + idx] = rs;
        p.nframes[row + idx] = t - rs + 1;
        p.score[row + idx] = __int_as_float(sm_key(h >= 0 ? v : max(v, mycm)));
      }
    }
  }
  // every thread holds the same carry now.  `base` counts the carried run and every start: all of them have closed but the
  // run that reaches hi - 1 (not END) - or the carried run itself when nothing was final
  const int last_tok = n > 0 ? tok[hi - 1] : prev0;
  const bool open_after = !end && last_tok != p.blank;
  const int emitted = base - (open_after ? 1 : 0);
  const int nn = min(emitted, P);
  for (int i = nn + tid; i < P; i += blockDim.x) {
    p.labels[row + i] = p.blank;
    p.start[row + i] = 0;
    p.nframes[row + i] = 0;
    p.score[row + i] = 0.f;
  }
  if (wave == 0) {                                  // part[t % 64] += fs[t], t global and increasing
    float part = __int_as_float(blk[ST_PART + lane]);
    for (long long t = (long long)lo + ((lane - lo) & 63); t < hi; t += 64) part += fs[t];
    blk[ST_PART + lane] = __float_as_int(part);
    sm_part[lane] = part;
  } else if (wave == 1 && p.tail_labels) {          // the provisional tail: labels of [hi, top) behind the open run
    int32_t* tl = p.tail_labels + (size_t)b * p.Ptail;
    int cnt = open_after ? 1 : 0;
    if (open_after && lane == 0 && p.Ptail > 0) tl[0] = last_tok;
    const int tprev = open_after ? last_tok : p.blank;
    for (long long t0 = hi; t0 < top && cnt < p.Ptail; t0 += 64) {
      const long long t = t0 + lane;
      int me = p.blank;
      bool st = false;
      if (t < top) {
        me = tok[t];
        st = me != p.blank && me != (t == hi ? tprev : tok[t - 1]);
      }
      const unsigned long long m = __ballot(st);
      const int idx = cnt + __popcll(m & ((1ull << lane) - 1ull));
      if (st && idx < p.Ptail) tl[idx] = me;
      cnt += __popcll(m);
    }
    cnt = min(cnt, p.Ptail);
    for (int i = cnt + lane; i < p.Ptail; i += 64) tl[i] = p.blank;
    if (lane == 0) p.tail_n[b] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    if (end)
      for (int l = 0; l < 64; ++l) acc += sm_part[l];
    p.utt_score[b] = acc;
    p.n_new_labels[b] = nn;
    p.status[b] = 0;
    p.total_frames[b] = hi;
    blk[ST_DONE] = hi;
    blk[ST_OPEN] = open_after ? last_tok + 1 : 0;
    blk[ST_FIRST] = open_after ? cs : 0;
    blk[ST_MAX] = open_after ? cm : 0;
    blk[ST_NLAB] = nlab0 + emitted;
  }
}

size_t stream_state_bytes(int S, int Wl, int C) {
  if (S < 1 || Wl < 1 || C < 1 || (long long)Wl + C > INT_MAX - 4) return 0;
  const size_t cap = ((size_t)Wl + C + 3) / 4 * 4;
  return (size_t)S * (4 * ST_WORDS + 4 * cap);
}

int launch_stream_push(hipStream_t s, const qasr_stream_push_args& a) {
  PushP p{};
  p.state = (int32_t*)a.state, p.slots = a.slots, p.flags = a.flags, p.n_new = a.n_new, p.chunk = a.chunk, p.pitch = a.pitch;
  p.S = a.S, p.C = a.C, p.cap = (a.Wl + a.C + 3) / 4 * 4, p.is_s16 = a.dtype == QASR_PCM_S16;
  hipLaunchKernelGGL(k_stream_push, dim3((unsigned)a.B), dim3(SM_NT), 0, s, p);
  return QASR_OK;
}

int launch_stream_window(hipStream_t s, const qasr_stream_window_args& a) {
  WindowP p{};
  p.state = (const int32_t*)a.state, p.slots = a.slots, p.windows = a.windows, p.window_lens = a.window_lens;
  p.first_frame = a.first_frame, p.S = a.S, p.Wl = a.Wl, p.cap = (a.Wl + a.C + 3) / 4 * 4, p.spf = a.samples_per_frame;
  const dim3 grid((unsigned)((a.Wl + SM_TILE - 1) / SM_TILE), (unsigned)a.B), block(SM_NT);
  hipLaunchKernelGGL(k_stream_window, grid, block, 0, s, p);
  return QASR_OK;
}

int launch_stream_emit(hipStream_t s, const qasr_stream_emit_args& a) {
  EmitP p{};
  p.state = (int32_t*)a.state, p.slots = a.slots, p.flags = a.flags, p.tokens = a.tokens, p.fs = a.frame_score;
  p.enc_lens = a.enc_lens, p.first_frame = a.first_frame;
  p.labels = a.labels, p.start = a.start, p.nframes = a.nframes, p.score = a.score, p.n_new_labels = a.n_new_labels;
  p.status = a.status, p.total_frames = a.total_frames, p.utt_score = a.utt_score;
  p.tail_labels = a.tail_labels, p.tail_n = a.tail_n;
  p.S = a.S, p.Tw = a.Tw, p.P = a.P, p.Ptail = a.tail_labels ? a.Ptail : 0, p.Rr = a.Rr, p.spf = a.samples_per_frame, p.blank = a.blank;
  hipLaunchKernelGGL(k_stream_emit, dim3((unsigned)a.B), dim3(SM_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
