"""Rational polyphase resampling of PCM audio to the model's rate: the arithmetic contract of k_resample
(csrc/qasr_resample.hip), stated in NumPy.  This module is the CPU path (read_wav, the host modules) and the yardstick of
the tests; the kernel equals it byte for byte.

The reference resamples in AudioSegment.__init__ with librosa.core.resample (parts/segment.py:57-59), whose default filters
are resampy's 'kaiser_best' / 'kaiser_fast'.  The two presets here carry the published parameters of those filters (zero
crossings, roll-off, Kaiser beta).  Bit parity with librosa is NOT pinned: neither librosa nor resampy is importable where
this was written, and resampy interpolates linearly in a precomputed, oversampled table where this module evaluates the
windowed sinc exactly at every phase.

RULES
  ratio    g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g.  An utterance of n input frames gives
           out_len(n) = ceil(n L / M) outputs.  Output i sits at p = i M (units of 1 / L input frame, a 64-bit quantity):
           q = p // L, phi = p % L.
  filter   s = rolloff * min(1, L / M), W = ceil(Z / s),
           h(t) = s sinc(s t) I0(beta sqrt(1 - (s t / Z)^2)) / I0(beta) for |s t| < Z, else 0      (float64)
           Output i has the 2 W taps j = 0 .. 2 W - 1: d = j - W, input frame k = q - d, argument t = phi / L + d.
           Frames outside [0, n) of the utterance's own length are zero.
  table    c[phi][j] = rint(h(phi / L + j - W) * 2^30), int32.
  int16    xs[k] = the integer sum of the `ch` channels of frame k; acc = the exact int64 sum of c[phi][j] * xs[k];
           out = float32(float64(acc) / float64(ch * 2^45)): one correctly rounded float64 division, one rounding to float32.
           pack() asserts max_phi sum_j |c| * 32768 * 8 < 2^53, so the sum is exact for up to 8 channels.
  float32  xs[k] = the float64 sum of the channels in ascending channel order; hq = c * 2^-30 (float64, exact);
           acc = 0.0, then for j ascending acc = acc + hq * xs[k]: a float64 product rounded on its own, then a float64 sum
           (no fused multiply-add); out = float32(acc / float64(ch)).
  equal    sr_in == sr_out bypasses the filter: int16 samples are divided by 32768 in float32 and the float32 channel mean is
           taken, exactly as read_wav always did (the sum of <= 8 such values is exact in float32); float32 mono is copied,
           float32 multi-channel is float32(float64 channel sum / ch).
  plans    any integer sr_in >= 1000 with L * 2 W <= 2^20 table entries and W <= 4096; everything else is refused.
  rows     out[b][0 .. out_len) holds the result, the rest of the row is zero, out_lens[b] = out_len.  A sample at or behind
           lens[b] is never read.

PACKED TABLE (pack(); validated by qasr_resample_check before upload): 32 int32 header words - magic 'QRS1', version 1,
total bytes, L, M, W, sr_in, sr_out, quality (0 best, 1 fast), entries (L * 2 W), zeros - then the entries as int32
[j][r], r = i mod L the slot of output i, holding c[(r M) mod L][j]: consecutive outputs read consecutive words.
"""
import math

import numpy as np

MAGIC = 0x31535251                      # 'QRS1'
VERSION = 1
HDR_WORDS = 32
MAX_ENTRIES = 1 << 20
MAX_W = 4096
MIN_RATE = 1000
MAX_CHANNELS = 8
PRESETS = {
    'best': (64, 0.9475937167399596, 14.769656459379492),
    'fast': (16, 0.85, 8.555504641634386),
}
_QUALITY_ID = {'best': 0, 'fast': 1}
_CHUNK = 8192


class ResamplePlan:
    """The ratio, the filter and the fixed-point table of one (sr_in, sr_out, quality)."""

    def __init__(self, sr_in, sr_out=16000, quality='best'):
        if quality not in PRESETS:
            raise ValueError(f'resample: quality must be one of {sorted(PRESETS)}, got {quality!r}')
        if isinstance(sr_in, bool) or int(sr_in) != sr_in or isinstance(sr_out, bool) or int(sr_out) != sr_out:
            raise ValueError(f'resample: sample rates must be integers, got {sr_in!r} -> {sr_out!r}')
        sr_in, sr_out = int(sr_in), int(sr_out)
        if sr_in < MIN_RATE or sr_out < MIN_RATE:
            raise ValueError(f'resample: sample rate {min(sr_in, sr_out)} Hz is below {MIN_RATE} Hz')
        self.sr_in, self.sr_out, self.quality = sr_in, sr_out, quality
        g = math.gcd(sr_in, sr_out)
        self.L, self.M = sr_out // g, sr_in // g
        self.Z, self.rolloff, self.beta = PRESETS[quality]
        self.s = self.rolloff * min(1.0, self.L / self.M)
        self.W = int(math.ceil(self.Z / self.s))
        if self.W > MAX_W:
            raise ValueError(f'resample: {sr_in} Hz -> {sr_out} Hz needs {self.W} taps a side, at most {MAX_W} are supported')
        if self.L * 2 * self.W > MAX_ENTRIES:
            raise ValueError(f'resample: {sr_in} Hz -> {sr_out} Hz needs a table of {self.L * 2 * self.W} entries '
                             f'({self.L} phases x {2 * self.W} taps), at most {MAX_ENTRIES} are supported')
        self._h = self._table = self._blob = None

    @property
    def equal(self):
        return self.L == 1 and self.M == 1

    def out_len(self, n):
        n = int(n)
        return -((-n * self.L) // self.M) if n > 0 else 0

    @property
    def h(self):
        """float64 [L][2 W]: the unrounded filter, h[phi][j] = h(phi / L + j - W)"""
        if self._h is None:
            phi = np.arange(self.L, dtype=np.float64)[:, None]
            d = np.arange(-self.W, self.W, dtype=np.float64)[None, :]
            u = self.s * (phi / self.L + d)
            inside = np.abs(u) < self.Z
            win = np.i0(self.beta * np.sqrt(np.clip(1.0 - (u / self.Z) ** 2, 0.0, None))) / np.i0(self.beta)
            self._h = np.where(inside, self.s * np.sinc(u) * win, 0.0)
        return self._h

    @property
    def table(self):
        """int32 [L][2 W]: c[phi][j] = rint(h * 2^30)"""
        if self._table is None:
            self._table = np.rint(self.h * float(1 << 30)).astype(np.int32)
        return self._table

    def abs_sum(self):
        """max over the phases of sum_j |c|: the accumulator bound is this * 32768 * channels"""
        return int(np.abs(self.table.astype(np.int64)).sum(axis=1).max())

    def pack(self):
        if self._blob is None:
            assert self.abs_sum() * 32768 * MAX_CHANNELS < (1 << 53), 'the int64 accumulator would not convert exactly'
            L, M, W = self.L, self.M, self.W
            hdr = np.zeros(HDR_WORDS, dtype=np.int32)
            slots = (np.arange(L, dtype=np.int64) * M) % L                   # the phase of slot r = i mod L
            body = np.ascontiguousarray(self.table[slots].T)                  # [j][r]
            hdr[:10] = [MAGIC, VERSION, 4 * (HDR_WORDS + body.size), L, M, W, self.sr_in, self.sr_out, _QUALITY_ID[self.quality],
                        body.size]
            self._blob = hdr.tobytes() + body.tobytes()
        return self._blob


def _rows(x, lens, channels):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    if x.dtype not in (np.int16, np.float32):
        raise ValueError(f'resample: int16 or float32 samples, got {x.dtype}')
    if not 1 <= int(channels) <= MAX_CHANNELS:
        raise ValueError(f'resample: channels must be 1 .. {MAX_CHANNELS}, got {channels}')
    ch = int(channels)
    if x.ndim != 2 or x.shape[1] % ch:
        raise ValueError(f'resample: samples must be [B][frames * {ch}], got shape {x.shape}')
    S = x.shape[1] // ch
    lens = np.minimum(np.maximum(np.asarray(lens, dtype=np.int64).reshape(-1), 0), S)
    if lens.shape[0] != x.shape[0]:
        raise ValueError(f'resample: {lens.shape[0]} lengths for {x.shape[0]} rows')
    return x, lens, ch, S


def _channel_sum(row, n, ch, dtype):
    """xs[0 .. n): int64 sums (int16 input) or float64 sums in ascending channel order (float32 input)"""
    fr = row[:n * ch].reshape(n, ch)
    xs = fr[:, 0].astype(dtype)
    for c in range(1, ch):
        xs = xs + fr[:, c].astype(dtype)
    return xs


def _equal_row(row, n, ch):
    if row.dtype == np.int16:
        y = row[:n * ch].astype(np.float32) / np.float32(32768.0)
        return y.reshape(n, ch).mean(axis=1) if ch > 1 else y
    if ch == 1:
        return row[:n].copy()
    return (_channel_sum(row, n, ch, np.float64) / np.float64(ch)).astype(np.float32)


def _filter_row(xs, n, plan, coef, i0, i1):
    """acc[i0 .. i1) of one utterance: sequential in j, vectorised over the outputs (int64 exact, or float64 with a rounded
    product and a rounded sum per tap)"""
    if i1 - i0 > _CHUNK:                                         # bounds the [2 W][outputs] coefficient gather
        return np.concatenate([_filter_row(xs, n, plan, coef, a, min(a + _CHUNK, i1)) for a in range(i0, i1, _CHUNK)])
    L, M, W = plan.L, plan.M, plan.W
    i = np.arange(i0, i1, dtype=np.int64)
    p = i * M
    q, phi = p // L, p % L
    lo = int(q[0]) - W + 1 if i.size else 0                      # frames lo .. hi feed these outputs
    hi = int(q[-1]) + W if i.size else -1
    pad = np.zeros(max(hi - lo + 1, 0), dtype=xs.dtype)
    a, b = max(lo, 0), min(hi + 1, n)
    if b > a:
        pad[a - lo:b - lo] = xs[a:b]
    acc = np.zeros(i.size, dtype=xs.dtype)
    base = q + W - lo
    cphi = np.ascontiguousarray(coef[phi].T)                     # [j][output]
    for j in range(2 * W):
        acc = acc + cphi[j] * pad[base - j]
    return acc


def resample_host(x, lens, plan, channels=1, out_range=None):
    """The twin of k_resample.  x: int16 or float32 [B][S * channels] (interleaved), lens: frames per utterance.  Returns
    (out float32 [B][P], out_lens int32 [B]) with P = plan.out_len(S), rows zero behind their length.  out_range = (i0, i1)
    evaluates the outputs i0 .. i1 only and returns [B][i1 - i0] (entries at or behind a row's length are zero)."""
    x, lens, ch, S = _rows(x, lens, channels)
    B = x.shape[0]
    P = plan.out_len(S)
    i0, i1 = (0, P) if out_range is None else (int(out_range[0]), int(out_range[1]))
    if not 0 <= i0 <= i1 <= P:
        raise ValueError(f'resample: out_range {out_range} outside 0 .. {P}')
    out = np.zeros((B, i1 - i0), dtype=np.float32)
    out_lens = np.array([plan.out_len(n) for n in lens], dtype=np.int32)
    is_int = x.dtype == np.int16
    for b in range(B):
        n, e = int(lens[b]), min(int(out_lens[b]), i1)
        if e <= i0:
            continue
        if plan.equal:
            out[b, :e - i0] = _equal_row(x[b], n, ch)[i0:e]
        elif is_int:
            acc = _filter_row(_channel_sum(x[b], n, ch, np.int64), n, plan, plan.table.astype(np.int64), i0, e)
            out[b, :e - i0] = (acc.astype(np.float64) / np.float64(ch * (1 << 45))).astype(np.float32)
        else:
            hq = plan.table.astype(np.float64) * 2.0 ** -30
            acc = _filter_row(_channel_sum(x[b], n, ch, np.float64), n, plan, hq, i0, e)
            out[b, :e - i0] = (acc / np.float64(ch)).astype(np.float32)
    return out, out_lens


def resample_direct(x, n, plan, channels=1):
    """float64 direct sum with the unrounded filter over one utterance's first n frames (int16 input is scaled by 2^-15):
    the channel mean convolved with h, no fixed point, for the tests"""
    row = np.asarray(x).reshape(-1)
    ch = int(channels)
    xs = _channel_sum(row, int(n), ch, np.float64) / ch
    if row.dtype == np.int16:
        xs = xs / 32768.0
    if plan.equal:
        return xs
    return _filter_row(xs, int(n), plan, plan.h, 0, plan.out_len(n))
