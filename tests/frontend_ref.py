"""Float64 reference of the mel front-end (csrc/qasr_frontend.hip), a float32 restatement of the kernel's rounding, the
case lists the CPU and the GPU tests share, and a NumPy packing of the plan workspace.  NumPy only.

ref64   FilterbankFeatures.forward + normalize_batch with everything behind the windowed float32 frames in float64.
emu32   the same pipeline with the roundings k_mel / k_norm apply - a model on the reference's side, not the code under
        test: it says how far a correct float32 implementation sits from ref64 (the floor) and, with a fault switched on,
        how far a wrong one does.

Error metric (log-mel units, used everywhere):
  normalised output   |y - y_ref| * (std_ref + 1e-5), std_ref the float64 standard deviation of the mel row over its valid
                      frames.  A tolerance on y itself means nothing: a mel row that hardly moves over the valid frames
                      (quiet audio, a chirp that has not reached the band yet) has a tiny std, and dividing by it scales
                      float32 rounding without limit - emu32 is 2e-2 from ref64 on such rows and 2.5e-6 in this metric.
  raw log-mel         |lm - lm_ref|.
  std_ref == 0        (digital silence) the output must also be exactly 0.0: the scaled metric would let 1.0 pass there.
"""
import os
from collections import namedtuple

import numpy as np

from qasr import melbank

NFFT, NBIN, HOP, WIN, WOFF, PAD = 512, 257, 160, 320, 96, 256
GUARD = 2.0 ** -24
CONSTANT = 1e-5
MEL_FBMAX, MEL_MAXM, MEL_MAGIC = 768, 128, 0x4d454c32
F32, F64 = np.float32, np.float64

# emu32 against ref64 over every case below (tests/test_frontend_ref_cpu.py::test_noise_floor measures it):
FLOOR = 2.36e-6          # measured maximum (normalised, e_long_S163679); raw log-mel alone: 1.12e-6
BOUND = 1e-5             # 4 x FLOOR rounded up to one significant digit: faithful (not correctly rounded) logf and division
#                          on the device, another order of the normalisation sums, one ulp of a log-mel near -16.6 (1.9e-6)

S0 = 4005                # 26 frames: one full 16-frame tile of k_mel and a partial one
Ref = namedtuple('Ref', 'lm norm mean std n')
FAULTS = ('fft32', 'window_reversed', 'reflect_lo', 'reflect_hi', 'run_lo', 'run_hi', 'twiddle')
TWIDDLE_BIN, TWIDDLE_REL = 64, 1e-7


def n_frames(S):
    return 1 + S // HOP


def frames_pad(S, pad_to):
    n = n_frames(S)
    return n + (pad_to - n % pad_to) % pad_to if pad_to > 0 else n


def valid_frames(length, S):
    return min(-(-int(length) // HOP), n_frames(S))


# ---------------------------------------------------------------- the windowed float32 frames (shared by ref64 / emu32)
def frames_f32(audio_row, preemph, window, fault=None):
    """[T, 512] float32: pre-emphasis in two rounded float32 steps, the whole row reflect-padded by 256, frame t =
    ypad[160 t : 160 t + 512] times the 320-tap window centred at offset 96 (zero outside it), products in float32."""
    x = np.asarray(audio_row, F32)
    S = x.size
    assert S > PAD, 'reflect padding needs more than 256 samples'
    y = x.copy()
    y[1:] = x[1:] - (F32(preemph) * x[:-1]).astype(F32)
    j = np.arange(PAD)                                         # (faults: the edge sample repeated, index off by one)
    lo = y[PAD - j - (fault == 'reflect_lo')]
    hi = y[S - 2 - j + (fault == 'reflect_hi')]
    ypad = np.concatenate([lo, y, hi])
    w = np.zeros(NFFT, F32)
    w[WOFF:WOFF + WIN] = np.asarray(window, F32)[::-1] if fault == 'window_reversed' else np.asarray(window, F32)
    T = n_frames(S)
    idx = HOP * np.arange(T)[:, None] + np.arange(NFFT)[None, :]
    return (ypad[idx] * w[None, :]).astype(F32)


def _stats64(lm, n):
    """mean / unbiased std over the first n frames in float64; a row that is constant there has std exactly 0"""
    M = lm.shape[0]
    if n == 0:
        return np.full(M, np.nan), np.full(M, np.nan)
    v = lm[:, :n]
    mean = v.mean(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.sqrt(((v - mean[:, None]) ** 2).sum(1) / F64(n - 1))          # n == 1: 0 / 0 = NaN, as torch.std
    const = (v == v[:, :1]).all(1)
    mean[const] = v[const, 0]
    if n > 1:
        std[const] = 0.0
    return mean, std


def ref64(audio_row, length, preemph, window, fb):
    """-> Ref(raw log-mel [n_mels, T], normalised features [n_mels, T], mean, std, n), float64."""
    fr = frames_f32(audio_row, preemph, window).astype(F64)
    X = np.fft.rfft(fr, axis=1)
    P = X.real ** 2 + X.imag ** 2                              # [T, 257]
    lm = np.log(np.asarray(fb, F64) @ P.T + GUARD)             # [n_mels, T]
    n = valid_frames(length, len(audio_row))
    mean, std = _stats64(lm, n)
    norm = np.zeros_like(lm)
    if n:
        norm[:, :n] = (lm[:, :n] - mean[:, None]) / (std[:, None] + CONSTANT)
    return Ref(lm, norm, mean, std, n)


# ---------------------------------------------------------------- float32 restatement of the kernel, with fault switches
def _fft32(fr):
    """512-point FFT of real float32 frames [T, 512] in complex64 throughout (radix-2, float32 twiddles): what round 1 ran"""
    n = fr.shape[1]
    rev = np.array([int(format(i, '09b')[::-1], 2) for i in range(n)])
    z = fr[:, rev].astype(np.complex64)
    half = 1
    while half < n:
        tw = np.exp(-1j * np.pi * np.arange(half) / half).astype(np.complex64)
        z = z.reshape(fr.shape[0], -1, 2, half)
        a, b = z[:, :, 0, :], z[:, :, 1, :] * tw
        z = np.stack([a + b, a - b], axis=2).astype(np.complex64)
        half *= 2
    return z.reshape(fr.shape[0], n)[:, :NBIN]


def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the one float64 rounding of the sum in front of the
    float32 one matters only on an exact tie of the latter"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def mel_runs(fb):
    """[n_mels, 2] int32: the run [lo, hi) of non-zero weights of every filter; (0, 0) for an all-zero one"""
    r = np.zeros((fb.shape[0], 2), np.int32)
    for m, row in enumerate(np.asarray(fb)):
        nz = np.flatnonzero(row != 0)
        if nz.size:
            r[m] = nz[0], nz[-1] + 1
    return r


def emu32(audio_row, length, preemph, window, fb, fault=None, fault_filter=None):
    """ref64's pipeline with the kernel's rounding: float64 spectrum rounded once to float32, sqrt(f32(re re) + f32(im im))
    squared, the mel dot as a float32 fma chain in ascending k, float32 log, mean / std sums in float64 rounded to float32,
    float32 subtract and divide.  fault: one of FAULTS (fault_filter: the filter whose run 'run_lo' / 'run_hi' shorten,
    default the middle one).  -> Ref in float32."""
    assert fault is None or fault in FAULTS, fault
    fr = frames_f32(audio_row, preemph, window, fault)
    if fault == 'fft32':
        X = _fft32(fr)
    else:
        X = np.fft.rfft(fr.astype(F64), axis=1)
        if fault == 'twiddle':                                 # X[k] = E[k] + w_k O[k] with w_k off by TWIDDLE_REL
            k = TWIDDLE_BIN
            odd = fr[:, 1::2].astype(F64) @ np.exp(-2j * np.pi * k * np.arange(NFFT // 2) / (NFFT // 2))
            X[:, k] += TWIDDLE_REL * np.exp(-2j * np.pi * k / NFFT) * odd
    re, im = X.real.astype(F32), X.imag.astype(F32)
    mag = np.sqrt((re * re).astype(F32) + (im * im).astype(F32)).astype(F32)
    P = (mag * mag).astype(F32)                                # [T, 257]
    fb = np.array(fb, F32)
    if fault in ('run_lo', 'run_hi'):
        m = fb.shape[0] // 2 if fault_filter is None else fault_filter
        lo, hi = mel_runs(fb)[m]
        fb[m, lo if fault == 'run_lo' else hi - 1] = 0
    acc = np.zeros((fb.shape[0], P.shape[0]), F32)
    for k in range(NBIN):
        acc = _fma32(fb[:, k:k + 1], P[None, :, k], acc)
    lm = np.log((acc + F32(GUARD)).astype(F64)).astype(F32)    # correctly rounded float32 log
    n = valid_frames(length, len(audio_row))
    norm = np.zeros_like(lm)
    M = lm.shape[0]
    if n == 0:
        return Ref(lm, norm, np.full(M, np.nan, F32), np.full(M, np.nan, F32), 0)
    v = lm[:, :n].astype(F64)
    mean = (v.sum(1) / F64(n)).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        var = ((v - mean.astype(F64)[:, None]) ** 2).sum(1) / F64(n - 1)
        sd = (np.sqrt(var).astype(F32) + F32(CONSTANT)).astype(F32)
        norm[:, :n] = ((lm[:, :n] - mean[:, None]).astype(F32) / sd[:, None]).astype(F32)
    return Ref(lm, norm, mean, (sd - F32(CONSTANT)).astype(F32), n)


# ---------------------------------------------------------------- the metric
def err_raw(lm, ref, upto=None):
    """max |lm - lm_ref| over the frames < upto (default: all computed frames)"""
    T = ref.lm.shape[1] if upto is None else upto
    return float(np.abs(np.asarray(lm, F64)[:, :T] - ref.lm[:, :T]).max()) if T else 0.0


def err_norm(y, ref):
    """max |y - y_ref| (std_ref + 1e-5) over the valid frames (n >= 2: below that the reference is empty or NaN)"""
    assert ref.n >= 2
    d = np.abs(np.asarray(y, F64)[:, :ref.n] - ref.norm[:, :ref.n]) * (ref.std[:, None] + CONSTANT)
    return float(d.max())


def check_row(y, flen, ref, T_pad, bound=BOUND):
    """Every assertion on one normalised output row y [n_mels, T_pad] with feature length flen; -> its metric (0.0 where
    fewer than two frames are valid: nothing to measure, the values are asserted outright)."""
    y = np.asarray(y)
    assert y.shape == (ref.lm.shape[0], T_pad), (y.shape, T_pad)
    n = ref.n
    assert int(flen) == n, (flen, n)
    assert np.all(y[:, n:] == 0), 'frames at or behind the length and the padding must be exactly zero'
    if n == 0:
        return 0.0
    if n == 1:                                                  # unbiased std of one value: NaN (torch.std and k_norm alike)
        assert np.all(np.isnan(y[:, 0])), 'one valid frame: frame 0 is NaN in the reference'
        return 0.0
    assert np.all(np.isfinite(y[:, :n]))
    silent = ref.std == 0
    assert np.all(y[silent] == 0), 'digital silence (std_ref == 0) must come out as exactly 0.0'
    e = err_norm(y, ref)
    assert e <= bound, f'{e:.3e} > {bound:.1e} (log-mel units)'
    return e


# ---------------------------------------------------------------- signals, windows, banks
def _rng(seed):
    return np.random.default_rng(seed)


def noise(S, seed, scale=1.0):
    return (scale * _rng(seed).standard_normal(S)).astype(F32)


def chirp(S):
    t = np.arange(S, dtype=F64)
    return (0.3 * np.sin(2 * np.pi * 5e-5 * t * t)).astype(F32)


def tone(S, cycles_per_sample):
    return (0.5 * np.sin(2 * np.pi * cycles_per_sample * np.arange(S, dtype=F64))).astype(F32)


SIGNAL_NAMES = ('noise0.1', 'tone_bin64', 'tone_offbin', 'noise1e-4', 'noise2e4_pcm', 'noise_then_zeros', 'impulse1777',
                'dc0.25', 'chirp', 'zeros')


def signals(S=S0):
    """[10, S] float32, one row per signal of SIGNAL_NAMES"""
    gap = noise(S, 14, 0.1)
    gap[2000:] = 0
    imp = np.zeros(S, F32)
    imp[1777] = 1
    return np.stack([noise(S, 11, 0.1), tone(S, 64 / NFFT), tone(S, 0.1234), noise(S, 12, 1e-4), noise(S, 13, 2e4), gap, imp,
                     np.full(S, 0.25, F32), chirp(S), np.zeros(S, F32)])


def noise_and_tone(S=S0):
    return np.stack([noise(S, 21, 0.1), tone(S, 0.1234)])


def noise_and_chirp(S=S0, seed=22):
    return np.stack([noise(S, seed, 0.1), chirp(S)])


def window(name):
    n = np.arange(WIN, dtype=F64)
    if name == 'hann':                                          # torch.hann_window(320, periodic=False), from the fixture
        return np.load(os.path.join(GOLDEN, 'frontend.npz'))['window'].astype(F32)
    if name == 'hamming':
        return (0.54 - 0.46 * np.cos(2 * np.pi * n / (WIN - 1))).astype(F32)
    if name == 'random':                                        # positive, not symmetric: the only kind that can tell a
        return _rng(31).uniform(0.05, 1.0, WIN).astype(F32)     # reversed or shifted window index from a correct one
    raise KeyError(name)


# name -> (packed table length or None where the issue leaves it open, path, number of m0 passes of k_mel)
BANKS = {
    'slaney40_7600':    (532, 'lds', 1),
    'slaney64_8000':    (580, 'lds', 1),
    'slaney64_300_3400': (304, 'lds', 1),
    'slaney65_8000':    (584, 'lds', 2),
    'slaney80_8000':    (616, 'lds', 2),
    'slaney128_8000':   (740, 'lds', 2),
    'slaney129_8000':   (None, 'global', 3),                    # more than MEL_MAXM filters
    'hand1_fits_exactly': (768, 'lds', 1),
    'hand2_one_run_over': (772, 'global', 1),
    'hand3_edges':      (None, 'lds', 1),
    'dense_random64':   (None, 'global', 1),
}


def bank(name):
    """[n_mels, 257] float32"""
    if name.startswith('slaney'):
        p = name[len('slaney'):].split('_')
        n_mels, fmin, fmax = int(p[0]), (float(p[1]) if len(p) == 3 else 0.0), float(p[-1])
        return melbank.mel_filterbank(16000, NFFT, n_mels, fmin, fmax).astype(F32)
    r = _rng(41)
    if name in ('hand1_fits_exactly', 'hand2_one_run_over'):   # three rows on bins 0..255: 3 x 256 = MEL_FBMAX exactly
        fb = np.zeros((3, NBIN), F32)
        fb[:, :256] = r.uniform(0.001, 0.02, (3, 256))
        if name == 'hand2_one_run_over':                        # ... and four more weights: 772, one run past the table
            row = np.zeros((1, NBIN), F32)
            row[0, 100:104] = 0.01, 0.02, 0.02, 0.01
            fb = np.concatenate([fb, row])
        return fb
    if name == 'hand3_edges':
        fb = np.zeros((5, NBIN), F32)                           # row 0: all zero
        fb[1, 0] = 0.5                                          # one bin at 0
        fb[2, 256] = 0.5                                        # one bin at 256
        fb[3] = r.uniform(0.001, 0.02, NBIN)                    # all 257 bins
        fb[4, 252:257] = 0.01, 0.02, 0.03, 0.02, 0.01           # a 5-bin run that ends at bin 256
        return fb
    if name == 'dense_random64':
        return r.uniform(0.001, 0.02, (64, NBIN)).astype(F32)
    raise KeyError(name)


# ---------------------------------------------------------------- the plan workspace (layout: k_melrange in qasr_frontend.hip)
Plan = namedtuple('Plan', 'hdr ranges offs table fits total')


def pack_plan(fb):
    """What qasr_frontend_plan leaves in front of the twiddles: int hdr[4] = {magic, n_mels, table length or 769, 0};
    int ranges[n_mels][2]; int offs[n_mels]; float table[768] (runs back to back, each padded with zero weights to a
    multiple of 4; all zero where it does not fit)."""
    fb = np.asarray(fb, F32)
    M = fb.shape[0]
    ranges = mel_runs(fb)
    padded = (ranges[:, 1] - ranges[:, 0] + 3) & ~3
    offs = (np.cumsum(padded) - padded).astype(np.int32)
    total = int(padded.sum())
    fits = M <= MEL_MAXM and total <= MEL_FBMAX
    table = np.zeros(MEL_FBMAX, F32)
    if fits:
        for m, (lo, hi) in enumerate(ranges):
            table[offs[m]:offs[m] + hi - lo] = fb[m, lo:hi]
    hdr = np.array([MEL_MAGIC, M, total if fits else MEL_FBMAX + 1, 0], np.int32)
    return Plan(hdr, ranges, offs, table, fits, total)


def split_plan(ws, n_mels):
    """The bytes of a plan workspace (uint8 array) -> (hdr, ranges, offs, table, twiddle [512, 2] float64)"""
    ws = np.ascontiguousarray(ws, np.uint8)
    o_r = 16
    o_o = o_r + 8 * n_mels
    o_t = (o_o + 4 * n_mels + 15) // 16 * 16
    o_w = o_t + 4 * MEL_FBMAX
    assert ws.size >= o_w + 16 * NFFT
    return (ws[:o_r].view(np.int32), ws[o_r:o_o].view(np.int32).reshape(n_mels, 2), ws[o_o:o_o + 4 * n_mels].view(np.int32),
            ws[o_t:o_w].view(F32), ws[o_w:o_w + 16 * NFFT].view(F64).reshape(NFFT, 2))


def twiddles_exact():
    """(cos, sin)(-2 pi k / 512), k < 512, as float64 [512, 2] rounded from a higher precision: mpmath where it is installed,
    otherwise np.longdouble on the first octant and exact symmetry for the rest"""
    try:
        import mpmath
        mpmath.mp.prec = 200
        oct_ = [(mpmath.cos(2 * mpmath.pi * j / NFFT), mpmath.sin(2 * mpmath.pi * j / NFFT)) for j in range(NFFT // 8 + 1)]
        oct_ = [(float(c), float(s)) for c, s in oct_]
    except ImportError:
        assert np.finfo(np.longdouble).eps < 2e-19, 'no extended precision on this machine'
        j =np.arange(NFFT // 8 + 1, dtype=np.longdouble)
        pi = np.longdouble('3.14159265358979323846264338327950288')
        ang = 2 * pi * j / NFFT
        oct_ = [(float(c), float(s)) for c, s in zip(np.cos(ang), np.sin(ang))]
    out = np.zeros((NFFT, 2), F64)
    for k in range(NFFT):
        q, r = divmod(k, NFFT // 4)                             # angle = q * 90 degrees + r
        c, s = oct_[r] if r <= NFFT // 8 else oct_[NFFT // 4 - r][::-1]
        c, s = [(c, s), (-s, c), (-c, -s), (s, -c)][q]
        out[k] = c, -s
    return out + 0.0                                            # (-0.0 -> 0.0)


# ---------------------------------------------------------------- the case lists
Case = namedtuple('Case', 'name audio lens fb_name win_name preemph')
LENGTH_S = (257, 319, 320, 321, 2559, 2560, 4005)
PAD_TOS = (0, 5, 16)
LONG_S = (163679, 164003)                                       # T_pad 1024: k_norm's last register-path size; 1040: its loop
RAW_ROWS, RAW_LENS = (0, 2, 6, 8), (S0, 2500, 1700, 400)       # (f): noise, off-bin tone, impulse, chirp


def cases_signals():
    a = signals()
    return [Case(f'a_signals_len{L}', a, [L] * len(a), 'slaney64_8000', 'hann', 0.97) for L in (S0, 2500)]


def cases_banks():
    a = noise_and_tone()
    return [Case(f'b_bank_{b}', a, [S0, S0], b, 'hann', 0.97) for b in BANKS]


def cases_window():
    a = noise_and_chirp()
    return [Case('c_hamming', a, [S0, S0], 'slaney64_8000', 'hamming', 0.97),
            Case('c_random_window', a, [S0, S0], 'slaney64_8000', 'random', 0.97),
            Case('c_preemph0', a, [S0, S0], 'slaney64_8000', 'hann', 0.0),
            Case('c_preemph1', a, [S0, S0], 'slaney64_8000', 'hann', 1.0)]


def row_lengths(S):
    return sorted({min(L, S) for L in (0, 1, 160, 161, 320, S - 1, S)})


def case_lengths(S):
    """One row per length, each row its own noise over all S samples: what lies behind a length is non-zero and differs from
    row to row - the reflect padding and the frames across the length read it, in the reference and in the kernel."""
    lens = row_lengths(S)
    return Case(f'd_lengths_S{S}', np.stack([noise(S, 100 + S + i, 0.1) for i in range(len(lens))]), lens, 'slaney64_8000',
                'hann', 0.97)


def case_long(S):
    return Case(f'e_long_S{S}', noise_and_chirp(S, seed=23), [S, S - 20000], 'slaney64_8000', 'hann', 0.97)


def case_raw():
    a = signals()[list(RAW_ROWS)]
    return Case('f_raw', a, list(RAW_LENS), 'slaney64_8000', 'hann', 0.97)


def all_cases():
    return (cases_signals() + cases_banks() + cases_window() + [case_lengths(S) for S in LENGTH_S]
            + [case_long(S) for S in LONG_S] + [case_raw()])


_refs = {}


def case_refs(case):
    """ref64 of every row of a case, computed once per process"""
    if case.name not in _refs:
        fb, w = bank(case.fb_name), window(case.win_name)
        _refs[case.name] = [ref64(case.audio[b], case.lens[b], case.preemph, w, fb) for b in range(len(case.lens))]
    return _refs[case.name]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
