"""Seeded inputs shared by the keyword-spotting tests on the CPU and on the GPU, a brute-force oracle of qasr.spot.SPOT_RULES'
lattice in plain integer Python (every start frame tried on its own), a plain restatement of the hit rule, and planted
recordings whose arg-max path spells a keyword over a known stretch.  NumPy only."""
import numpy as np

import beam_cases
import star_cases
from qasr import align, beam, spot

NEG = beam.NEG
HIT_FIELDS = ('hit_start', 'hit_end', 'hit_score', 'n_hits', 'ok')
ALL_FIELDS = HIT_FIELDS + ('trace_score', 'trace_start')


def logp(rng, B, T, C, blank):
    return np.stack([beam_cases.peaky_logp(rng, T, C, blank, blend=(u % 2 == 1)) for u in range(B)])


def keywords(rng, lengths, C, blank, pitch=None, repeats=0.2):
    """one keyword of every given length (labels without the blank, some adjacent ones repeated), padded with the blank"""
    rows = [star_cases.labels_without_blank(rng, n, C, blank, repeats) for n in lengths]
    return pad(rows, blank, pitch)


def pad(rows, blank, pitch=None):
    ML = max(1, max(len(r) for r in rows)) if pitch is None else pitch
    tg = np.full((len(rows), ML), blank, dtype=np.int32)
    for i, r in enumerate(rows):
        tg[i, :min(len(r), ML)] = r[:ML]
    return tg, np.array([len(r) for r in rows], dtype=np.int32)


def emissions(lp, star_row, y, blank):
    """e(t, s) of SPOT_RULES as Python integers: [T][2L] (column 0 unused)"""
    T = lp.shape[0]
    L = len(y)
    lab = [blank if s % 2 == 0 else int(y[(s - 1) // 2]) for s in range(2 * L)]
    qs = [int(q) for q in beam.quantize(star_row)]
    q = beam.quantize(lp)
    return [[min(int(q[t, lab[s]]) - qs[t], 0) for s in range(2 * L)] for t in range(T)]


def brute(lp, star_row, lim, y, blank):
    """best[s0][t] (s0 <= t < lim): the best score of y's lattice over the frames s0 .. t with frame s0 in state 1 and frame t in
    state F = 2L - 1, NEG when there is no such path; every s0 is run on its own, nothing is shared between starts.
    Dmax[t] = the maximum over s0."""
    L = len(y)
    S, F = 2 * L, 2 * L - 1
    e = emissions(lp, star_row, y, blank)
    skip = [s % 2 == 1 and s >= 3 and int(y[(s - 1) // 2]) != int(y[(s - 3) // 2]) for s in range(S)]
    best = [[NEG] * lim for _ in range(lim)]
    for s0 in range(lim):
        V = [NEG] * S
        V[1] = e[s0][1]
        best[s0][s0] = V[F]
        for t in range(s0 + 1, lim):
            W = [NEG] * S
            for s in range(1, S):
                m = max(V[s], V[s - 1] if s >= 2 else NEG, V[s - 2] if skip[s] else NEG)       # (state 0 does not exist here)
                W[s] = NEG if m == NEG else m + e[t][s]
            V = W
            best[s0][t] = V[F]
    dmax = [max(best[s0][t] for s0 in range(t + 1)) for t in range(lim)]
    return best, dmax


def hits_restated(d, st, thr, max_span):
    """the hit rule of SPOT_RULES, restated frame by frame over a trace in Python integers: the emitted (start, end, D)"""
    out = []
    have, o_start, o_end, o_d = False, 0, 0, 0
    for t in range(len(d)):
        D, s = int(d[t]), int(st[t])
        if D == NEG:
            continue
        n = t - s + 1
        if n > max_span or D < thr * n:
            continue
        if have and s <= o_end:
            if D * (o_end - o_start + 1) > o_d * n:
                o_start, o_end, o_d = s, t, D
            continue
        if have:
            out.append((o_start, o_end, o_d))
        have, o_start, o_end, o_d = True, s, t, D
    if have:
        out.append((o_start, o_end, o_d))
    return out


def planted(y, stretches, T, C, blank, seed=0, frames_per_label=3, last_frames=1):
    """lp [1, T, C] whose arg-max is the blank everywhere except that from each frame of `stretches` on it spells y,
    frames_per_label frames per label (last_frames for the last one) with one blank frame between adjacent equal labels;
    posteriors are peaked (the arg-max at -0.05 nat, every other class near -8).  Returns (lp, [(first, last)] of every planted
    occurrence).  The arg-max path scores exactly 0, so all of its sub-spans that still spell y tie at mean 0: the Viterbi row
    keeps the earliest start (stay wins a tie) and the hit rule the earliest end (a later equal mean is dropped) - with
    last_frames = 1 that hit is the whole planted stretch."""
    rng = np.random.Generator(np.random.PCG64([seed, T, C, len(y)]))
    lp = (-8.0 + 0.1 * rng.standard_normal((T, C))).astype(np.float32)
    top = np.full(T, blank)
    spans = []
    for f0 in stretches:
        t = f0
        for i, c in enumerate(y):
            if i and y[i - 1] == c:
                top[t] = blank
                t += 1
            n = last_frames if i == len(y) - 1 else frames_per_label
            top[t:t + n] = c
            t += n
        spans.append((f0, t - 1))
        assert t <= T
    lp[np.arange(T), top] = -0.05
    return lp[None], spans


def same_bytes(got, want, fields=ALL_FIELDS, what=''):
    star_cases.same_bytes(got, want, fields, what)


def host(lp, lens, tg, tl, blank, threshold, max_span, max_hits, want_trace=True, star=None):
    """star_host + spot_host as the façade composes them"""
    st = align.star_host(lp, lens, 0.0) if star is None else star
    return spot.spot_host(lp, lens, st, tg, tl, blank, spot.check_threshold(threshold, 'host'), max_span, max_hits, want_trace)
