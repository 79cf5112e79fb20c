"""Seeded inputs for the banded-alignment tests (qasr.align.align_band_host, k_align_band).  NumPy only.

Synthetic posteriors of a scratch transcription: a label sequence, a frame plan (frames per label, blank gaps, a leading
blank), and per frame C logits of unit Gaussian noise with the true class's raised by `a`; log-softmax in float64, stored as
float32.  At a >= 3 the true class holds most of the mass and the pruned lattice finds the full lattice's path; every case
that claims so is checked against align_host on the CPU by test_align_band_cpu.py (none skipped).  All seeds below are the first
ones tried: none had to be replaced."""
import numpy as np

C = 29
BLANK = C - 1


def synth(seed, L, a=4.0, per_label=(1, 1), gap=(0, 0), lead=0, tail=0, alphabet=C - 1, repeat_p=0.0):
    """(logp float32 [T, C], y int list [L]): label i holds per_label[0] .. per_label[1] frames and is followed by
    gap[0] .. gap[1] blank frames (at least one before an adjacent repeat); `lead` / `tail` blank frames around.  repeat_p:
    the probability that a label repeats its predecessor; otherwise it differs from it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, frames = [], [BLANK] * lead
    for i in range(L):
        if i and rng.random() < repeat_p:
            c = y[-1]
        else:
            c = int(rng.integers(0, alphabet))
            if i and c == y[-1]:
                c = (c + 1) % alphabet
        if i and c == y[-1] and frames[-1] != BLANK:
            frames.append(BLANK)
        y.append(c)
        frames += [c] * int(rng.integers(per_label[0], per_label[1] + 1))
        frames += [BLANK] * int(rng.integers(gap[0], gap[1] + 1))
    frames += [BLANK] * tail
    T = len(frames)
    z = rng.standard_normal((T, C))
    z[np.arange(T), frames] += a
    z -= z.max(axis=1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    return lp.astype(np.float32), y


# name -> (synth arguments, lens or None): BW = 256, the band moves, and the result must equal the full lattice's
MOVING = {
    'dense_L400': (dict(seed=11, L=400, a=4.0, tail=3), None),                                  # one frame per label, T = 403
    'repeats_L600': (dict(seed=12, L=600, a=4.0, per_label=(1, 2), gap=(0, 3), alphabet=6, repeat_p=0.3, tail=1), None),
    'lead300_L400': (dict(seed=13, L=400, a=3.0, per_label=(1, 3), gap=(0, 4), lead=300, tail=5), None),
    'short_lens_L400': (dict(seed=14, L=400, a=3.5, per_label=(1, 3), gap=(0, 10), tail=150), -37),   # lens = T - 37
}

_made = {}


def moving_case(name):
    """(logp [1, T, C], lens [1] or None, targets [1, L], target_lens [1]) of MOVING[name], built once"""
    if name not in _made:
        kw, cut = MOVING[name]
        lp, y = synth(**kw)
        lens = None if cut is None else np.array([lp.shape[0] + cut], dtype=np.int32)
        _made[name] = (lp[None], lens, np.array([y], dtype=np.int32), np.array([len(y)], dtype=np.int32))
    return _made[name]


# (name, band_states, synth arguments) of the device tests: the smallest shapes at which each instantiation's band moves
DEVICE = (
    ('bw256_S1201', 256, dict(seed=21, L=600, a=4.0, per_label=(1, 4), gap=(0, 3), lead=20, tail=2)),       # T about 2000
    ('bw1024_S2401', 1024, dict(seed=22, L=1200, a=4.0, per_label=(1, 2), gap=(0, 1), alphabet=8, repeat_p=0.2, tail=3)),
    ('bw4352_L2300', 4352, dict(seed=23, L=2300, a=4.0, per_label=(1, 2), gap=(0, 1), lead=40, tail=1)),    # T about 5000
)


def device_case(name):
    """(band_states, logp [1, T, C], targets [1, L], target_lens [1]) of a DEVICE entry, built once"""
    key = 'dev:' + name
    if key not in _made:
        _, bw, kw = next(d for d in DEVICE if d[0] == name)
        lp, y = synth(**kw)
        _made[key] = (bw, lp[None], np.array([y], dtype=np.int32), np.array([len(y)], dtype=np.int32))
    return _made[key]


def viterbi_f64(logp, y, blank):
    """an independent float64 Viterbi over the full lattice: the best path's score (-inf: none)"""
    lp = np.asarray(logp, dtype=np.float64)
    L = len(y)
    lab = np.full(2 * L + 1, blank)
    lab[1::2] = y
    may_skip = np.zeros(2 * L + 1, dtype=bool)
    may_skip[3::2] = np.asarray(y[1:]) != np.asarray(y[:-1])
    v = np.full(2 * L + 1, -np.inf)
    v[:2] = lp[0, lab[:2]]
    for t in range(1, lp.shape[0]):
        one = np.concatenate([[-np.inf], v[:-1]])
        two = np.where(may_skip, np.concatenate([[-np.inf, -np.inf], v[:-2]]), -np.inf)
        v = np.maximum(np.maximum(v, one), two) + lp[t, lab]
    return float(max(v[-1], v[-2])) if L else float(v[0])
