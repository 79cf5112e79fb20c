"""Long recordings as overlapped windows: the plan, the seam rule and the host statement of k_cut / k_stitch
(csrc/qasr_longform.hip, include/qasr.h).  NumPy only: no GPU, no native library.

A recording is cut into windows of equal length that overlap, the windows run through the model as a batch, and the
per-frame outputs of neighbouring windows are joined at one frame of their overlap - the seam - chosen per pair.
`cut_host` and `stitch_host` are the CPU path of EncDecCTCModel.decode_long and the yardstick the GPU tests compare the
kernels with, byte for byte.  Normalisation and every other per-utterance statistic of the model is per WINDOW: the
stitched result is not the result of one run over the whole recording."""
from typing import Sequence

import numpy as np

from .ctc import _order_key

MAX_PLANES = 6                          # planes of one stitch, tokens and frame scores included
_DMAX = (1 << 29) - 1                   # the distance field of a key

SEAM_RULES = """Windows A = k and B = k + 1 of one recording overlap on the global frames [lo, hi), lo = first_global_frame(B),
hi = first_global_frame(A) + enc_len(A).  Encoded lengths are first clamped to 0 .. min(Tw, 2 H / samples_per_frame) (Tw:
the row pitch of the window outputs); a model's own lengths never reach the clamp, because Wl >= 2 Ov.

Candidates are the frames g of [lo + guard, hi - guard) that B holds too (g - lo < enc_len(B)).  With mid = (lo + hi) // 2
the seam is the candidate of largest key, compared field by field:
  1. class: 2 if A[g] == B[g] == blank, 1 if A[g] == B[g], else 0;
  2. _order_key(float32(fsA[g] + fsB[g])), the order-preserving integer image of the float32 sum that k_ctc takes maxima
     in (-0 < +0, every bit pattern ordered); 0 without frame scores;
  3. the smaller |g - mid|;
  4. the smaller g.
seam='middle' uses 3 and 4 alone (the middle merge of buffered inference).  Without a candidate the seam is
min(hi, max(lo, mid)) - and, for lengths no model produces, never past B's last frame (lo + enc_len(B)) nor before lo.

The key is one unsigned 64-bit word, (class << 62) | ((order key ^ 0x80000000) << 30) | ((2^29 - 1 - |g - mid|) << 1) |
(g <= mid); a maximum over it does not depend on the order in which candidates are visited.

Frames g < seam come from A, frames g >= seam from B; the seams of a recording ascend, so every global frame has one
owner.  A frame its owner does not hold (behind the owner's encoded length: only with lengths no model produces) is
filled like a tail.  total_frames[r] = first_global_frame(last) + enc_len(last), capped at the row pitch Tmax; behind it a
row holds `blank` in the token plane and zero bytes in every other plane.  seams[k] is the first global frame window k
contributes: 0 for the first window of a recording."""


class WindowPlan:
    """Windows of R recordings of lens_samples[r] samples at `sample_rate`.

    Wl (window) and Ov (overlap) are window_s / overlap_s rounded to multiples of samples_per_frame (featurizer hop x
    encoder stride: 320 for the registered models), H = Wl - Ov.  A recording of S samples has 1 window if S <= Wl, else
    1 + ceil((S - Wl) / H); window k starts at k H and has min(Wl, S - k H) samples, so the last one is longer than Ov.
    Frame j of window k is global frame k H / samples_per_frame + j.

    table     int32 [Wn][4] = (recording, start_sample, n_samples, first_global_frame)
    first     int32 [R] first window of each recording;  count  int32 [R] its windows
    guard     frames kept clear of a window's edges when a seam is chosen
    Tmax      row pitch of the stitched outputs: max over recordings of first_global_frame(last) + frames_of(n_samples(last))
    frames_of: samples -> an upper bound of the encoded frames of a window that long (default: n // samples_per_frame + 1,
    the unpadded front-end; an engine whose front-end pads passes its own)."""

    def __init__(self, lens_samples: Sequence[int], window_s=30.0, overlap_s=4.0, guard_s=1.0, sample_rate=16000,
                 samples_per_frame=320, frames_of=None):
        spf = int(samples_per_frame)
        if spf < 1 or int(sample_rate) < 1:
            raise ValueError(f'WindowPlan: sample_rate {sample_rate} and samples_per_frame {samples_per_frame} must be positive')
        to_frames = lambda s: int(round(float(s) * int(sample_rate) / spf))
        wf, of, gf = to_frames(window_s), to_frames(overlap_s), to_frames(guard_s)
        if of <= 0:
            raise ValueError(f'WindowPlan: overlap_s {overlap_s} rounds to {of} frames, it must be positive')
        if of >= wf:
            raise ValueError(f'WindowPlan: overlap_s {overlap_s} ({of} frames) must be shorter than the window of {wf} frames')
        if wf < 2 * of:
            raise ValueError(f'WindowPlan: window_s {window_s} ({wf} frames) must be at least twice the overlap of {of} frames')
        if gf < 0 or 2 * gf >= of:
            raise ValueError(f'WindowPlan: guard_s {guard_s} ({gf} frames): twice the guard must be shorter than the overlap of '
                             f'{of} frames, and it must not be negative')
        lens = [int(s) for s in np.asarray(lens_samples).reshape(-1)]
        if not lens or min(lens) < 1:
            raise ValueError('WindowPlan: lens_samples needs at least one recording, each of at least one sample')
        self.sample_rate, self.samples_per_frame = int(sample_rate), spf
        self.window_frames, self.overlap_frames, self.guard, self.hop_frames = wf, of, gf, wf - of
        self.Wl, self.Ov, self.H = wf * spf, of * spf, (wf - of) * spf
        self.lens = np.array(lens, dtype=np.int64)
        self.frames_of = frames_of if frames_of is not None else (lambda n: n // spf + 1)
        rows, first, count = [], [], []
        for r, S in enumerate(lens):
            n = 1 if S <= self.Wl else 1 + -(-(S - self.Wl) // self.H)
            first.append(len(rows))
            count.append(n)
            for k in range(n):
                rows.append((r, k * self.H, min(self.Wl, S - k * self.H), k * self.hop_frames))
        if max(max(row) for row in rows) >= 2 ** 31:
            raise ValueError('WindowPlan: a recording is too long for int32 sample offsets')
        self.table = np.array(rows, dtype=np.int32).reshape(-1, 4)
        self.first, self.count = np.array(first, dtype=np.int32), np.array(count, dtype=np.int32)
        self.R, self.Wn = len(lens), len(rows)
        last = self.table[self.first + self.count - 1]
        self.Tmax = int(max(int(f) + int(self.frames_of(int(n))) for _, _, n, f in last))

    def seconds_per_frame(self):
        return self.samples_per_frame / float(self.sample_rate)


def cut_host(audio, lens, plan: WindowPlan):
    """audio float32 [R][>= max lens], lens int [R] -> (windows float32 [Wn][Wl], zeros behind each length; window_lens
    int32 [Wn]).  A window holds what `lens` leaves of it: min(n_samples, lens[r] - start), never below 0."""
    x = np.asarray(audio, dtype=np.float32)
    ln = np.asarray(lens).reshape(-1)
    win = np.zeros((plan.Wn, plan.Wl), dtype=np.float32)
    wl = np.zeros(plan.Wn, dtype=np.int32)
    for w, (r, s, n, _) in enumerate(plan.table.tolist()):
        n = max(0, min(n, min(int(ln[r]), x.shape[1]) - s))
        win[w, :n] = x[r, s:s + n]
        wl[w] = n
    return win, wl


def _clamped_lens(plan, enc_lens, Tw):
    return np.clip(np.asarray(enc_lens).reshape(-1).astype(np.int64), 0, min(int(Tw), 2 * plan.hop_frames))


def seam_host(plan: WindowPlan, a: int, enc, tokens, frame_score, blank, seam='blank') -> int:
    """the seam between windows a and a + 1 (one recording) under SEAM_RULES; enc: the clamped lengths"""
    loA, lo = int(plan.table[a, 3]), int(plan.table[a + 1, 3])
    hi = loA + int(enc[a])
    mid = (lo + hi) // 2
    g = np.arange(lo + plan.guard, min(hi - plan.guard, lo + int(enc[a + 1])), dtype=np.int64)
    if len(g) == 0:
        return max(lo, min(hi, lo + int(enc[a + 1]), max(lo, mid)))
    d = np.abs(g - mid)
    key = ((_DMAX - d).astype(np.uint64) << np.uint64(1)) | (g <= mid).astype(np.uint64)
    if seam == 'blank':
        ta, tb = tokens[a, g - loA], tokens[a + 1, g - lo]
        cls = np.where(ta == tb, np.where(ta == blank, 2, 1), 0).astype(np.uint64)
        if frame_score is not None:
            ok = _order_key((frame_score[a, g - loA] + frame_score[a + 1, g - lo]).astype(np.float32))
        else:
            ok = np.zeros(len(g), dtype=np.int32)
        oku = (ok.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
        key |= (cls << np.uint64(62)) | (oku << np.uint64(30))
    elif seam != 'middle':
        raise ValueError(f"stitch: seam must be 'blank' or 'middle', got {seam!r}")
    return int(g[int(np.argmax(key))])                  # keys are distinct: one maximum


def stitch_host(plan: WindowPlan, enc_lens, tokens, frame_score=None, planes=(), blank=None, seam='blank'):
    """tokens int32 [Wn][Tw]; frame_score float32 [Wn][Tw] or None; planes: arrays [Wn][Tw][...] of bytes_per_frame (a
    multiple of 4) each; enc_lens int [Wn].  Returns (out_planes, total_frames int32 [R], seams int32 [Wn]): out_planes =
    [tokens, frame_score (if given), *planes] stitched per recording, each [R][Tmax][...] in its own dtype."""
    if blank is None:
        raise ValueError('stitch: blank is required (the decoder\'s last class)')
    if seam not in ('blank', 'middle'):
        raise ValueError(f"stitch: seam must be 'blank' or 'middle', got {seam!r}")
    tok = np.ascontiguousarray(tokens, dtype=np.int32)
    if tok.ndim != 2 or tok.shape[0] != plan.Wn:
        raise ValueError(f'stitch: tokens must be [{plan.Wn}][Tw], got {tok.shape}')
    Tw = tok.shape[1]
    fs = None if frame_score is None else np.ascontiguousarray(frame_score, dtype=np.float32)
    if fs is not None and fs.shape != tok.shape:
        raise ValueError('stitch: frame_score must have the shape of tokens')
    src = [tok] + ([fs] if fs is not None else []) + [np.ascontiguousarray(p) for p in planes]
    if len(src) > MAX_PLANES:
        raise ValueError(f'stitch: at most {MAX_PLANES} planes, tokens and frame_score included, got {len(src)}')
    for i, p in enumerate(src):
        if p.ndim < 2 or p.shape[:2] != (plan.Wn, Tw) or (p.dtype.itemsize * int(np.prod(p.shape[2:], dtype=np.int64))) % 4:
            raise ValueError(f'stitch: plane {i} must be [{plan.Wn}][{Tw}][bytes_per_frame, a multiple of 4], got {p.shape} {p.dtype}')
    enc = _clamped_lens(plan, enc_lens, Tw)
    if len(enc) != plan.Wn:
        raise ValueError(f'stitch: {plan.Wn} windows but {len(enc)} encoded lengths')
    Tmax = plan.Tmax
    out = [np.zeros((plan.R, Tmax) + p.shape[2:], dtype=p.dtype) for p in src]
    out[0][...] = blank
    total = np.zeros(plan.R, dtype=np.int32)
    seams = np.zeros(plan.Wn, dtype=np.int32)
    for r in range(plan.R):
        w0, n = int(plan.first[r]), int(plan.count[r])
        for k in range(1, n):
            seams[w0 + k] = seam_host(plan, w0 + k - 1, enc, tok, fs, blank, seam)
        last = w0 + n - 1
        total[r] = min(int(plan.table[last, 3]) + int(enc[last]), Tmax)
        for w in range(w0, w0 + n):
            f0 = int(plan.table[w, 3])
            ls = int(seams[w])
            rs = int(seams[w + 1]) if w < last else int(total[r])
            c1 = min(rs, f0 + int(enc[w]), Tmax)
            if c1 > ls:
                for o, p in zip(out, src):
                    o[r, ls:c1] = p[w, ls - f0:c1 - f0]
    return out, total, seams
