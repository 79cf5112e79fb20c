// Streaming endpointing (k_stream_endpoint); the host statement is qasr/stream_ep.py (EP_RULES), and this file follows it
// byte for byte, the state block included.
//
// State: S blocks of EP_WORDS 32-bit words, a buffer of its own next to the stream state.  A block is written by the one
// work-group that owns the slot in that launch (the rows' slots are distinct), with plain vector stores; no atomics; nothing is
// read back on the host but the row's records.  The stream block (frames_done, n_labels) and k_stream_emit's delta of the same
// step are read, never written: the launch goes behind k_stream_emit on the same queue and can be captured with it.
//
// k_stream_endpoint: one wave64 work-group per row.  The final range [lo, hi) is taken in chunks of 64 frames cut from lo, lane l
// holding frame c0 + l.  A ballot gives the chunk's speech mask; from the mask bits of its segment at or below it and the
// carried state (utt_first, last speech + 1) every lane derives its own trailing and length and so the rule that would fire
// there IF nothing fired before it in the segment; a second ballot finds the first firing lane f.  The frames [s0, f] are folded
// into the carried state, the record is written, the state resets, and the lanes behind f are evaluated again with s0 = f + 1:
// one pass per record, so at most E + 1 passes per chunk where the plan's bound holds (and never more than 64: s0 grows).
// part[(t - utt_first) % 64] lives in lane (t - utt_first) % 64: inside one segment of a chunk the frames hit distinct indices,
// so one shuffled add per segment keeps every partial sum's additions in increasing t.  The score is the serial sum of the 64
// lanes' values in index order from 0.0f (k_stream_emit's utt_score order), read lane by lane.
#include <climits>

#include "qasr_internal.h"

namespace qasr {

#define EP_WORDS 80
#define EP_DONE 0
#define EP_INDEX 1
#define EP_FIRST 2
#define EP_SP0 3
#define EP_SP1 4
#define EP_NSP 5
#define EP_LDONE 6
#define EP_PART 16
#define EP_REC 10
// the stream block of qasr_stream.hip, read-only here
#define EP_ST_WORDS 80
#define EP_ST_DONE 2
#define EP_ST_NLAB 6

struct EndpointP {
  const int32_t* state;       // the stream state
  int32_t* ep;                // [S][EP_WORDS]
  const int32_t* slots;
  const int32_t* flags;
  const int32_t* tokens;      // [B][Tw]
  const float* fs;            // [B][Tw]
  const int32_t* enc_lens;
  const int32_t* first_frame;
  const int32_t* em_start;    // [B][P]
  const int32_t* em_nframes;  // [B][P]
  const int32_t* em_n;        // [B]
  const int32_t* em_status;   // [B]
  int32_t* records;           // [B][E][EP_REC]
  int32_t* n_records;         // [B]
  int32_t* status;            // [B]
  int S, Tw, P, E, blank, Fsil, Fstart, Fmax, Fhard;
  float min_logp;
};

__device__ __forceinline__ float ep_sum64(float part) {          // part[0] + ... + part[63] in index order from 0.0f
  float acc = 0.f;
#pragma unroll 8
  for (int l = 0; l < 64; ++l) acc += __shfl(part, l);
  return acc;
}

__global__ void __launch_bounds__(64) k_stream_endpoint(EndpointP p) {
  const int lane = threadIdx.x, b = blockIdx.x, E = p.E;
  int32_t* const rec = p.records + (size_t)b * E * EP_REC;
  const int slot = p.slots[b];
  const bool slot_ok = slot >= 0 && slot < p.S;
  const int32_t* sblk = p.state + (long long)(slot_ok ? slot : 0) * EP_ST_WORDS;
  int32_t* blk = p.ep + (long long)(slot_ok ? slot : 0) * EP_WORDS;
  const int fl = p.flags[b];
  const bool begin = (fl & QASR_STREAM_BEGIN) != 0, end = (fl & QASR_STREAM_END) != 0;
  const int hi = sblk[EP_ST_DONE], n_labels = sblk[EP_ST_NLAB];
  const int first = p.first_frame[b];
  const int e = min(max(p.enc_lens[b], 0), p.Tw);
  const int lo = begin ? 0 : blk[EP_DONE];
  int st = 0;
  if (!slot_ok) st = 2;
  else if (p.em_status[b] != 0) st = 1;
  else if (lo > hi || lo < first || (lo < hi && (long long)hi > (long long)first + e)) st = 3;
  if (st) {                                         // an empty row, the state untouched
    for (int i = lane; i < E * EP_REC; i += 64) rec[i] = 0;
    if (lane == 0) {
      p.n_records[b] = 0;
      p.status[b] = st;
    }
    return;
  }
  // first <= lo and hi <= first + e <= first + Tw wherever a frame is read: window indices t - first lie in 0 .. Tw - 1
  const int32_t* const tok = p.tokens + (size_t)b * p.Tw - first;       // indexed by the global frame
  const float* const fs = p.fs + (size_t)b * p.Tw - first;
  const int n_em = min(max(p.em_n[b], 0), p.P);
  const int32_t* const es = p.em_start + (size_t)b * p.P;
  const int32_t* const en = p.em_nframes + (size_t)b * p.P;
  const int n_before = n_labels - n_em;
  int index = 0, utt_first = 0, sp0 = 0, sp1 = 0, nsp = 0, ldone = 0;
  float part = 0.f;                                 // part[lane]
  if (!begin) {
    index = blk[EP_INDEX], utt_first = blk[EP_FIRST], sp0 = blk[EP_SP0], sp1 = blk[EP_SP1], nsp = blk[EP_NSP];
    ldone = blk[EP_LDONE];
    part = __int_as_float(blk[EP_PART + lane]);
  }
  int nrec = 0;
  for (long long c0 = lo; c0 < hi; c0 += 64) {
    const int nv = (int)min(64ll, (long long)hi - c0);        // the chunk's frames
    const int t = (int)(c0 + lane);
    const bool valid = lane < nv;
    int me = p.blank;
    float x = 0.f;
    if (valid) {
      me = tok[t];
      x = fs[t];
    }
    const bool is_blank = me == p.blank;
    const unsigned long long smask = __ballot(valid && !is_blank && x >= p.min_logp);
    const unsigned long long le = (2ull << lane) - 1ull;      // lanes 0 .. lane
    int s0 = 0;
    while (s0 < nv) {
      const unsigned long long from = ~0ull << s0;            // lanes s0 .. 63
      const unsigned long long m = smask & le & from;
      const int last1 = m ? (int)c0 + (63 - __clzll((long long)m)) + 1 : sp1;    // last speech frame + 1 up to this lane
      const int trailing = t + 1 - (last1 ? last1 : utt_first);
      const int length = t + 1 - utt_first;
      int why = 0;
      if (valid && lane >= s0) {
        if (last1 && trailing >= p.Fsil) why = 1;
        else if (!last1 && trailing >= p.Fstart) why = 2;
        else if (length >= p.Fmax && is_blank) why = 3;
        else if (length >= p.Fhard) why = 4;
      }
      const unsigned long long fmask = __ballot(why != 0);
      const int f = fmask ? __ffsll((long long)fmask) - 1 : nv - 1;             // the segment is lanes s0 .. f
      // lane j holds part[j]; frame c0 + l of the segment adds to index (c0 + l - utt_first) % 64
      const int src = (lane - (int)((c0 - utt_first) & 63)) & 63;
      const float add = __shfl(x, src);
      if (src >= s0 && src <= f) part += add;
      const unsigned long long seg = smask & from & ((2ull << f) - 1ull);
      if (seg) {
        if (!sp0) sp0 = (int)c0 + __ffsll((long long)seg);                      // first speech frame + 1
        sp1 = (int)c0 + (63 - __clzll((long long)seg)) + 1;
        nsp += __popcll(seg);
      }
      if (!fmask) break;
      const int tf = (int)c0 + f;
      const int reason = __shfl(why, f);
      const float score = ep_sum64(part);
      int closed = 0;                                         // delta entries whose run a frame at or before tf closed
      for (int j0 = 0; j0 < n_em; j0 += 64) {
        const int j = j0 + lane;
        closed += __popcll(__ballot(j < n_em && (long long)es[j] + en[j] <= tf));
      }
      const int label_end = n_before + closed;
      if (nrec < E && lane < EP_REC) {
        int v = 0;
        switch (lane) {
          case 0: v = index; break;
          case 1: v = utt_first; break;
          case 2: v = tf + 1; break;
          case 3: v = sp0 - 1; break;
          case 4: v = sp1 - 1; break;
          case 5: v = nsp; break;
          case 6: v = reason; break;
          case 7: v = __float_as_int(score); break;
          case 8: v = label_end; break;
          default: break;
        }
        rec[nrec * EP_REC + lane] = v;
      }
      nrec = min(nrec + 1, E);
      index += 1, utt_first = tf + 1, sp0 = 0, sp1 = 0, nsp = 0, ldone = label_end;
      part = 0.f;
      s0 = f + 1;
    }
  }
  if (end) {                                        // the utterance that is open at the stream's end, empty or not
    const float score = ep_sum64(part);
    if (nrec < E && lane < EP_REC) {
      int v = 0;
      switch (lane) {
        case 0: v = index; break;
        case 1: v = utt_first; break;
        case 2: v = hi; break;
        case 3: v = sp0 - 1; break;
        case 4: v = sp1 - 1; break;
        case 5: v = nsp; break;
        case 6: v = 5; break;
        case 7: v = __float_as_int(score); break;
        case 8: v = n_labels; break;
        default: break;
      }
      rec[nrec * EP_REC + lane] = v;
    }
    nrec = min(nrec + 1, E);
    index += 1, utt_first = hi, sp0 = 0, sp1 = 0, nsp = 0, ldone = n_labels;
    part = 0.f;
  }
  for (int i = nrec * EP_REC + lane; i < E * EP_REC; i += 64) rec[i] = 0;
  blk[EP_PART + lane] = __float_as_int(part);
  if (lane < EP_PART) {
    int v = 0;
    switch (lane) {
      case EP_DONE: v = hi; break;
      case EP_INDEX: v = index; break;
      case EP_FIRST: v = utt_first; break;
      case EP_SP0: v = sp0; break;
      case EP_SP1: v = sp1; break;
      case EP_NSP: v = nsp; break;
      case EP_LDONE: v = ldone; break;
      default: break;
    }
    blk[lane] = v;
  }
  if (lane == 0) {
    p.n_records[b] = nrec;
    p.status[b] = 0;
  }
}

size_t stream_ep_state_bytes(int S) {
  if (S < 1) return 0;
  return (size_t)S * 4 * EP_WORDS;
}

int launch_stream_endpoint(hipStream_t s, const qasr_stream_endpoint_args& a) {
  EndpointP p{};
  p.state = (const int32_t*)a.state, p.ep = (int32_t*)a.ep_state, p.slots = a.slots, p.flags = a.flags, p.tokens = a.tokens;
  p.fs = a.frame_score, p.enc_lens = a.enc_lens, p.first_frame = a.first_frame;
  p.em_start = a.emit_start, p.em_nframes = a.emit_nframes, p.em_n = a.emit_n_new_labels, p.em_status = a.emit_status;
  p.records = a.records, p.n_records = a.n_records, p.status = a.status;
  p.S = a.S, p.Tw = a.Tw, p.P = a.P, p.E = a.E, p.blank = a.blank;
  p.Fsil = a.Fsil, p.Fstart = a.Fstart, p.Fmax = a.Fmax, p.Fhard = a.Fhard, p.min_logp = a.min_logp;
  hipLaunchKernelGGL(k_stream_endpoint, dim3((unsigned)a.B), dim3(64), 0, s, p);
  return QASR_OK;
}

}  // namespace qasr
