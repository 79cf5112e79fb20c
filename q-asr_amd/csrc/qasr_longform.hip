// Long recordings as overlapped windows (k_cut, k_stitch); the host statement is qasr/longform.py (SEAM_RULES), and this file
// follows it byte for byte.
//
// k_cut: one work-group of 256 threads per (window, tile of LF_TILE = 1024 samples); thread tid owns four consecutive samples.
// A window's source row starts at a multiple of samples_per_frame floats, so it is 16-byte aligned whenever the audio's base
// and pitch are: such a row moves as one 16-byte load and one 16-byte store per thread; any other row is read sample by
// sample.  The quad that straddles the window's length is assembled from scalars, zeros behind the length.  Work-group 0 of a
// window writes window_lens.
//
// k_stitch: one work-group of 256 threads per window.  Phase 1: the group computes the seam with its left and with its right
// neighbour (each seam is thus computed twice, by both neighbours, from the same inputs: no communication between groups).
// Every lane folds the keys of its candidates g = first + tid, first + tid + 256, ... into one u64 maximum; the maximum over
// the wave is taken by shuffles, over the waves through LDS.  Keys of different frames differ, so the maximum is one frame
// whatever the launch geometry.  Phase 2: the frames [left seam, right seam) of every plane move to the recording's row, 16
// bytes per thread when bytes_per_frame and both bases allow it, 4 bytes otherwise; frames the window does not hold, and -
// by a recording's last window - the tail behind total_frames, are filled.  Global memory sees plain vector stores; no atomics;
// nothing is read back on the host.
#include "qasr_internal.h"

namespace qasr {

#define LF_NT 256
#define LF_TILE 1024
#define LF_DMAX 0x1fffffff

struct CutP {
  const float* audio;
  const int32_t* lens;
  const int32_t* table;
  float* windows;
  int32_t* window_lens;
  long long pitch;
  int Wl, R;
};

__global__ void __launch_bounds__(LF_NT) k_cut(CutP p) {
  const int w = blockIdx.y, tid = threadIdx.x;
  const int32_t* row = p.table + 4 * (long long)w;
  const int rec = row[0];
  const long long start = row[1];
  long long n = 0;
  if (rec >= 0 && rec < p.R && start >= 0) {
    const long long have = min((long long)p.lens[rec], p.pitch) - start;
    n = max(0ll, min(min((long long)row[2], (long long)p.Wl), have));
  }
  if (blockIdx.x == 0 && tid == 0) p.window_lens[w] = (int32_t)n;
  const long long i = (long long)blockIdx.x * LF_TILE + 4ll * tid;
  if (i >= p.Wl) return;
  const float* src = p.audio + (long long)(n > 0 ? rec : 0) * p.pitch + (n > 0 ? start : 0);
  float* dst = p.windows + (long long)w * p.Wl + i;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i + 4 <= n && (((uintptr_t)src) & 15) == 0) {
    v = *(const float4*)(src + i);
  } else if (i < n) {
    v.x = src[i];
    if (i + 1 < n) v.y = src[i + 1];
    if (i + 2 < n) v.z = src[i + 2];
    if (i + 3 < n) v.w = src[i + 3];
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

struct StitchPlane {
  const char* src;
  char* dst;
  long long bpf;
  uint32_t fill;
  int vec;          // 16-byte moves: bytes_per_frame and both bases are multiples of 16
};

struct StitchP {
  const int32_t* table;
  const int32_t* enc_lens;
  const int32_t* tokens;
  const float* frame_score;
  int32_t* total_frames;
  int32_t* seams;
  StitchPlane pl[QASR_LONGFORM_MAX_PLANES];
  int n_planes, Wn, R, Tw, Tmax, guard, hop_frames, blank, middle;
};

__device__ __forceinline__ int lf_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

__device__ __forceinline__ unsigned long long lf_shfl_xor(unsigned long long v, int d) {
  const unsigned lo = __shfl_xor((unsigned)v, d), hi = __shfl_xor((unsigned)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int lf_enc(const StitchP& p, int w) { return min(max(p.enc_lens[w], 0), min(p.Tw, 2 * p.hop_frames)); }

// the seam between windows a and a + 1 of one recording; every thread of the group calls it and gets the same value
__device__ int lf_seam(const StitchP& p, int a, unsigned long long* red) {
  const int tid = threadIdx.x;
  const int loA = p.table[4 * a + 3], lo = p.table[4 * (a + 1) + 3];
  const int encB = lf_enc(p, a + 1);
  const int hi = loA + lf_enc(p, a);
  const int mid = (lo + hi) >> 1;                                     // both are >= 0
  const int first = max(lo, loA) + p.guard, end = min(hi - p.guard, lo + encB);     // (lo >= loA in every plan's table)
  const int32_t* ta = p.tokens + (long long)a * p.Tw - loA;
  const int32_t* tb = p.tokens + (long long)(a + 1) * p.Tw - lo;
  const float* fa = p.frame_score ? p.frame_score + (long long)a * p.Tw - loA : nullptr;
  const float* fb = p.frame_score ? p.frame_score + (long long)(a + 1) * p.Tw - lo : nullptr;
  unsigned long long best = 0;
  for (int g = first + tid; g < end; g += LF_NT) {
    const int d = g < mid ? mid - g : g - mid;
    unsigned long long key = ((unsigned long long)(LF_DMAX - d) << 1) | (g <= mid ? 1ull : 0ull);
    if (!p.middle) {
      const int x = ta[g], y = tb[g];
      const unsigned long long cls = x == y ? (x == p.blank ? 2ull : 1ull) : 0ull;
      int ok = 0;
      if (fa) ok = lf_key(__float_as_int(fa[g] + fb[g]));
      key |= (cls << 62) | ((unsigned long long)((unsigned)ok ^ 0x80000000u) << 30);
    }
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = lf_shfl_xor(best, d);
    best = o > best ? o : best;
  }
  __syncthreads();                                                    // red is reused between the two seams
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  for (int i = 0; i < LF_NT / 64; ++i) best = red[i] > best ? red[i] : best;
  if (best == 0) return max(lo, min(min(hi, lo + encB), max(lo, mid)));
  const int d = LF_DMAX - (int)((best >> 1) & LF_DMAX);
  return (best & 1) ? mid - d : mid + d;
}

__global__ void __launch_bounds__(LF_NT) k_stitch(StitchP p) {
  __shared__ unsigned long long red[LF_NT / 64];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int rec = p.table[4 * w], f0 = p.table[4 * w + 3];
  const bool has_left = w > 0 && p.table[4 * (w - 1)] == rec;
  const bool is_last = w + 1 >= p.Wn || p.table[4 * (w + 1)] != rec;
  const int ls = has_left ? lf_seam(p, w - 1, red) : 0;
  const int own_end = f0 + lf_enc(p, w);
  const int rs = is_last ? min(own_end, p.Tmax) : lf_seam(p, w, red);
  if (tid == 0) {
    p.seams[w] = ls;
    if (is_last && rec >= 0 && rec < p.R) p.total_frames[rec] = rs;
  }
  if (rec < 0 || rec >= p.R) return;
  const long long c0 = min(max(max(ls, f0), 0), p.Tmax);                          // (ls >= f0 >= 0 in every plan's table)
  const long long c1 = max(c0, (long long)min(min(rs, own_end), p.Tmax));      // copied: [c0, c1)
  const long long e1 = is_last ? p.Tmax : max(c1, (long long)min(rs, p.Tmax));  // filled: [c1, e1)
  for (int k = 0; k < p.n_planes; ++k) {
    const StitchPlane pl = p.pl[k];
    const char* src = pl.src + ((long long)w * p.Tw - f0 + c0) * pl.bpf;
    char* dst = pl.dst + ((long long)rec * p.Tmax + c0) * pl.bpf;
    const long long nb = (c1 - c0) * pl.bpf, fb = (e1 - c1) * pl.bpf;
    if (pl.vec) {
      for (long long i = 16ll * tid; i < nb; i += 16ll * LF_NT) *(uint4*)(dst + i) = *(const uint4*)(src + i);
      const uint4 f = make_uint4(pl.fill, pl.fill, pl.fill, pl.fill);
      for (long long i = 16ll * tid; i < fb; i += 16ll * LF_NT) *(uint4*)(dst + nb + i) = f;
    } else {
      for (long long i = 4ll * tid; i < nb; i += 4ll * LF_NT) *(uint32_t*)(dst + i) = *(const uint32_t*)(src + i);
      for (long long i = 4ll * tid; i < fb; i += 4ll * LF_NT) *(uint32_t*)(dst + nb + i) = pl.fill;
    }
  }
}

int launch_longform_cut(hipStream_t s, const qasr_longform_cut_args& a) {
  CutP p{};
  p.audio = a.audio, p.lens = a.lens, p.table = a.table, p.windows = a.windows, p.window_lens = a.window_lens;
  p.pitch = a.pitch, p.Wl = a.Wl, p.R = a.R;
  const dim3 grid((unsigned)((a.Wl + LF_TILE - 1) / LF_TILE), (unsigned)a.Wn), block(LF_NT);
  hipLaunchKernelGGL(k_cut, grid, block, 0, s, p);
  return QASR_OK;
}

int launch_longform_stitch(hipStream_t s, const qasr_longform_stitch_args& a) {
  StitchP p{};
  p.table = a.table, p.enc_lens = a.enc_lens, p.tokens = a.tokens, p.frame_score = a.frame_score;
  p.total_frames = a.total_frames, p.seams = a.seams;
  p.n_planes = a.n_planes, p.Wn = a.Wn, p.R = a.R, p.Tw = a.Tw, p.Tmax = a.Tmax, p.guard = a.guard, p.hop_frames = a.hop_frames;
  p.blank = a.blank, p.middle = a.seam_mode == QASR_SEAM_MIDDLE;
  for (int k = 0; k < a.n_planes; ++k) {
    const qasr_longform_plane& q = a.planes[k];
    p.pl[k].src = (const char*)q.src, p.pl[k].dst = (char*)q.dst, p.pl[k].bpf = q.bytes_per_frame, p.pl[k].fill = q.fill;
    p.pl[k].vec = q.bytes_per_frame % 16 == 0 && (((uintptr_t)q.src | (uintptr_t)q.dst) & 15) == 0;
  }
  hipLaunchKernelGGL(k_stitch, dim3((unsigned)a.Wn), dim3(LF_NT), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
