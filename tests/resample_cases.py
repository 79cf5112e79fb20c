"""Seeded PCM for the resampler tests, and a plain statement of the int16 arithmetic to hold qasr.resample against.  NumPy only.

brute_int16 is written plainly: one Python loop per output and per tap over Python integers, math.ceil-free integer
arithmetic, no vectorisation, no padding buffer.  It shares nothing with qasr/resample.py but the table and the rules."""
import numpy as np

TILE = 256                  # outputs per work-group of k_resample (RS_TILE in csrc/qasr_resample.hip)
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)
QUALITIES = ('best', 'fast')
AMP = 20000                 # tone amplitude of the issue's tone checks


def pcm(B, S, ch=1, seed=0):
    """int16 [B][S * ch]: a few sines plus noise per channel, near full scale now and then (clipped, not wrapped)"""
    rng = np.random.default_rng(seed)
    t = np.arange(S)[None, :, None]
    f = rng.uniform(0.001, 0.45, (B, 1, ch))
    x = 12000 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, (B, 1, ch))) + 9000 * rng.standard_normal((B, S, ch))
    x[:, ::97] *= 3
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(B, S * ch)


def to_float(x):
    return (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def fill_behind(x, lens, ch=1):
    """a copy of x with +32767 / -32768 alternating behind every row's length: what the kernel must never read"""
    y = x.copy()
    full = np.array([32767, -32768], dtype=np.int64)
    for b, n in enumerate(lens):
        k = np.arange(y.shape[1] - n * ch)
        y[b, n * ch:] = full[k % 2].astype(y.dtype) if y.dtype == np.int16 else full[k % 2].astype(np.float32) / 32768
    return y


def tone(sr, freq, n, amp=AMP):
    return np.rint(amp * np.sin(2 * np.pi * freq * np.arange(n) / sr)).astype(np.int16)


def mid_rms(y):
    """RMS over the middle half"""
    y = np.asarray(y, dtype=np.float64)
    q = y.size // 4
    return float(np.sqrt(np.mean(y[q:y.size - q] ** 2)))


def frames_for(plan, n_out):
    """the smallest frame count whose output length is at least n_out (exactly n_out whenever L <= M: every length occurs)"""
    n = (n_out * plan.M) // plan.L
    while plan.out_len(n) < n_out:
        n += 1
    while n > 0 and plan.out_len(n - 1) >= n_out:
        n -= 1
    assert plan.out_len(n) >= n_out and (plan.L > plan.M or plan.out_len(n) == n_out), (plan.sr_in, n_out)
    return n


def brute_int16(row, n, plan, ch=1):
    """float32 outputs of one int16 utterance, one Python integer sum per output"""
    L, M, W = plan.L, plan.M, plan.W
    table = plan.table.tolist()
    row = [int(v) for v in row[:n * ch]]
    n_out = 0
    while n_out * M < n * L:                    # ceil(n L / M) without a division
        n_out += 1
    out = np.zeros(n_out, dtype=np.float32)
    for i in range(n_out):
        p = i * M
        q, phi = divmod(p, L)
        acc = 0
        for d in range(-W, W):
            k = q - d
            if 0 <= k < n:
                acc += table[phi][d + W] * sum(row[k * ch:(k + 1) * ch])
        out[i] = np.float32(np.float64(acc) / np.float64(ch * 2 ** 45))
    return out
