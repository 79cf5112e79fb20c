"""Seeded inputs shared by the wildcard ("star") tests on the CPU and on the GPU: the augmented-matrix oracle of
qasr.align.STAR_RULES, the list of wildcard positions, and planted recordings whose transcript skips a stretch of audio.
NumPy only."""
import numpy as np

import align_cases
import beam_cases
from qasr import align

ALIGN_FIELDS = ('start', 'nframes', 'score', 'path_score', 'total', 'ok')
BAND_FIELDS = ('start', 'nframes', 'score', 'path_score', 'ok', 'frame_logp', 'band_base')


def augmented(lp, star):
    """the matrix of STAR_RULES' statement: star as class C of C + 1"""
    return np.concatenate([lp, star[..., None]], axis=2)


def same_bytes(got, want, fields, what=''):
    """every named output equal on every byte (None equal to None)"""
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        if g is None or w is None:
            assert g is None and w is None, (what, f)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, f, np.argwhere(g.view(np.int32 if g.itemsize == 4 else np.int64) !=
                                                                 w.view(np.int32 if w.itemsize == 4 else np.int64))[:4].tolist())


def star_brute(lp, lens, penalty):
    """STAR_RULES' plane stated plainly: per row the maximum through `_order_key` (integers only, no float64 anywhere), then one
    np.float32 subtraction; 0 behind the length"""
    B, T, C = lp.shape
    out = np.zeros((B, T), dtype=np.float32)
    pen = np.float32(penalty)
    for u in range(B):
        lim = T if lens is None else min(max(int(lens[u]), 0), T)
        for t in range(lim):
            row = np.ascontiguousarray(lp[u, t])
            keys = [int(k) for k in align._order_key(row)]
            out[u, t] = np.float32(row[keys.index(max(keys))] - pen)
    return out


def logp(rng, B, T, C, blank):
    return np.stack([beam_cases.peaky_logp(rng, T, C, blank, blend=(u % 2 == 1)) for u in range(B)])


def labels_without_blank(rng, n, C, blank, repeats=0.2):
    """n random labels of [0, C) without the blank, some adjacent ones repeated"""
    pool = np.array([c for c in range(C) if c != blank] or [0])
    y = pool[rng.integers(0, len(pool), size=n)]
    for i in range(1, n):
        if rng.random() < repeats:
            y[i] = y[i - 1]
    return [int(c) for c in y]


# the positions a wildcard takes in a target of n real labels y, as lists of label ids (W = the wildcard's id)
POSITIONS = ('first', 'last', 'only', 'two_with_a_label_between', 'two_adjacent', 'next_to_a_repeat')


def with_wildcards(y, W, position):
    y = list(y)
    n = len(y)
    if position == 'first':
        return [W] + y
    if position == 'last':
        return y + [W]
    if position == 'only':
        return [W]
    if position == 'two_with_a_label_between':
        k = n // 2
        return y[:k] + [W] + y[k:k + 1] + [W] + y[k + 1:]
    if position == 'two_adjacent':
        k = n // 2
        return y[:k] + [W, W] + y[k:]
    if position == 'next_to_a_repeat':
        k = max(n // 2, 1)
        return y[:k] + y[k - 1:k] + [W] + y[k:k + 1] + y[k:]         # ... a a W b b ...
    raise ValueError(position)


def position_targets(rng, n, C, blank, pitch=None):
    """one target per entry of POSITIONS over n random real labels, padded; W = C"""
    rows = [with_wildcards(labels_without_blank(rng, n, C, blank), C, pos) for pos in POSITIONS]
    return align_cases.pad_targets(rows, blank, pitch)


# ---- planted recordings: 3 frames per label, the true class at -0.05 nat and every other near -8; a stretch of frames that
# carries the transcript's own classes (as real speech would) and that the transcript does not cover.
# (name, labels, stretch in frames, twin, seed): the seed is one at which the alignment WITHOUT a wildcard gets a start wrong
# (a stretch at the end usually costs no start - the last label and the blank swallow it - so that case needed a search)
FRAMES_PER_LABEL = 3
PLANTED = (('start', 40, 30, 'full', 0), ('middle', 40, 30, 'full', 0), ('end', 40, 30, 'full', 3),
           ('band300', 200, 300, 'band', 0), ('band900', 200, 900, 'band', 0))


def planted(name, C=29):
    """(lp [1, T, C], y, y with the wildcard C at the stretch, the planted start of every label of y, (s0, s1) the stretch's
    frames, k the number of labels in front of the stretch).  Labels never repeat their neighbour, and the stretch's first /
    last symbol differs from the label in front of / behind it - so where the stretch begins and ends is defined."""
    where, n, stretch, _, seed = next(p for p in PLANTED if p[0] == name)
    blank = C - 1
    rng = np.random.Generator(np.random.PCG64([seed, n, stretch, len(where)]))
    y = [int(rng.integers(0, blank))]
    while len(y) < n:
        c = int(rng.integers(0, blank))
        if c != y[-1]:
            y.append(c)
    k = {'start': 0, 'middle': n // 2, 'end': n}.get(where, n // 2)
    n_sym = stretch // FRAMES_PER_LABEL
    left, right = (y[k - 1] if k else None), (y[k] if k < n else None)
    sym = []
    while len(sym) < n_sym:
        c = y[int(rng.integers(0, n))]
        bad = (sym and c == sym[-1]) or (not sym and c == left) or (len(sym) == n_sym - 1 and c == right)
        if not bad:
            sym.append(c)
    classes = [c for c in y[:k] for _ in range(FRAMES_PER_LABEL)] + [c for c in sym for _ in range(FRAMES_PER_LABEL)] + \
              [c for c in y[k:] for _ in range(FRAMES_PER_LABEL)]
    T = len(classes)
    lp = (-8.0 + 0.1 * rng.standard_normal((T, C))).astype(np.float32)
    lp[np.arange(T), classes] = -0.05
    s0 = FRAMES_PER_LABEL * k
    s1 = s0 + FRAMES_PER_LABEL * n_sym
    starts = [FRAMES_PER_LABEL * i + (0 if i < k else s1 - s0) for i in range(n)]
    return lp[None], y, y[:k] + [C] + y[k:], starts, (s0, s1), k


def moving_band_case(L=200, T=1200, C=29, seed=51, band_states=256):
    """one recording whose transcript (L labels with two wildcards, spread over T frames) makes the band move"""
    blank = C - 1
    rng = np.random.Generator(np.random.PCG64(seed))
    y = labels_without_blank(rng, L - 2, C, blank, repeats=0.1)
    y = y[:L // 3] + [C] + y[L // 3:2 * L // 3] + [C] + y[2 * L // 3:]
    seq = [c for c in y for _ in range(1)]
    cuts = np.sort(rng.choice(np.arange(1, T), size=len(seq) - 1, replace=False))
    owner = np.searchsorted(cuts, np.arange(T), side='right')       # which label of y each frame belongs to
    lp = (-6.0 + 0.5 * rng.standard_normal((T, C))).astype(np.float32)
    real = np.array([c if c != C else int(rng.integers(0, blank)) for c in seq])
    lp[np.arange(T), real[owner]] = -0.1
    for i in range(1, T):                                           # a blank frame between two runs of one class
        if owner[i] != owner[i - 1] and real[owner[i]] == real[owner[i - 1]]:
            lp[i, :] = -6.0
            lp[i, blank] = -0.1
    tg, tl = align_cases.pad_targets([y], blank)
    return lp[None], tg, tl, blank, band_states
