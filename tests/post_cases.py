"""Shared by the posterior tests on the CPU and on the GPU: an independent float64 forward-backward over the CTC lattice, a
brute-force enumeration of every alignment of small cases, and helpers that run the twins.  NumPy only.

The oracle is written plainly: per-state Python loops, numpy.logaddexp, no table, no fixed point.  It shares nothing with
qasr/align.py but the rules of the lattice."""
import math

import numpy as np

import align_cases
from qasr import align

NEGF = -math.inf
POST_FIELDS = ('frame_post', 'label_post', 'total', 'ok')


def lattice(y, blank):
    """(labels of the 2L + 1 states, the states each state may step to)"""
    S = 2 * len(y) + 1
    lab = [blank if s % 2 == 0 else int(y[(s - 1) // 2]) for s in range(S)]
    succ = []
    for s in range(S):
        nxt = [s]
        if s + 1 < S:
            nxt.append(s + 1)
        if s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s]:
            nxt.append(s + 2)
        succ.append(nxt)
    return lab, succ


def oracle_post(logp, y, blank):
    """float64 log-posteriors gamma [T, S] of every state at every frame given that y was emitted, and the total
    log-likelihood; None when no alignment exists"""
    lp = np.asarray(logp, dtype=np.float64)
    T = lp.shape[0]
    lab, succ = lattice(y, blank)
    S = len(lab)
    al = np.full((T, S), NEGF)
    be = np.full((T, S), NEGF)
    for s in range(min(2, S)):
        al[0, s] = lp[0, lab[s]]
    for t in range(1, T):
        for s in range(S):
            for r in succ[s]:                                       # s -> r
                al[t, r] = np.logaddexp(al[t, r], al[t - 1, s] + lp[t, lab[r]])
    for s in range(max(S - 2, 0), S):
        be[T - 1, s] = lp[T - 1, lab[s]]
    for t in range(T - 2, -1, -1):
        for s in range(S):
            tot = NEGF
            for r in succ[s]:
                tot = np.logaddexp(tot, be[t + 1, r])
            be[t, s] = tot + lp[t, lab[s]]
    total = float(np.logaddexp.reduce(al[T - 1, max(S - 2, 0):]))
    if total == NEGF:
        return None
    with np.errstate(invalid='ignore'):
        gamma = al + be - lp[:, lab] - total
    gamma[np.isnan(gamma)] = NEGF
    return gamma, total


def brute_post(logp, y, blank):
    """the same posteriors by enumerating every alignment: P(state s at frame t | y) as sums of path probabilities"""
    lp = np.asarray(logp, dtype=np.float64)
    T = lp.shape[0]
    lab, succ = lattice(y, blank)
    S = len(lab)
    mass = np.zeros((T, S))
    whole = 0.0
    n_paths = 0

    def walk(path, logprob):
        nonlocal whole, n_paths
        if len(path) == T:
            if path[-1] >= S - 2:
                pr = math.exp(logprob)
                whole += pr
                n_paths += 1
                for t, s in enumerate(path):
                    mass[t, s] += pr
            return
        for r in succ[path[-1]]:
            walk(path + [r], logprob + lp[len(path), lab[r]])
    for s in range(min(2, S)):
        walk([s], lp[0, lab[s]])
    return (mass / whole if whole > 0 else None), n_paths


def path_states(start, nframes, L, T):
    """the state of every frame of the alignment start / nframes [L] describe (POST_RULES' path)"""
    idx = align_cases.path_frames(start, nframes, L, T)
    blanks = np.array([int((np.asarray(start[:L]) <= t).sum()) for t in range(T)], dtype=np.int64)
    return np.where(idx >= 0, 2 * idx + 1, 2 * blanks)


def bound(lim):
    """|frame_post / 2^16 - oracle| in nats where the clamp is inactive: see test_frame_post_against_the_float64_oracle"""
    return 131.0 * lim / align.ONE


def align_and_post(lp, lens, tg, tl, blank, K=1, star=None):
    """(align_host's result, post_host's result on its path)"""
    res = align.align_host(lp, lens, tg, tl, blank, problems_per_utt=K, star=star)
    return res, align.post_host(lp, lens, tg, tl, blank, res.start, res.nframes, res.ok, problems_per_utt=K, star=star)


def same_bytes(got, want, what=''):
    for f in POST_FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        g = g.cpu().numpy() if hasattr(g, 'cpu') else np.asarray(g)
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, f, np.argwhere(g != w)[:4].tolist())


def invalid_paths(res, tg, tl, p, lim):
    """copies of (start, nframes, ok) of `res` with row p made invalid in each of the ways POST_RULES names; row p must hold a
    target of >= 3 labels whose labels 1 and 2 are equal, aligned with ok = 1"""
    L = int(tl[p])
    assert L >= 3 and tg[p, 1] == tg[p, 2] and res.ok[p] == 1
    out = {}

    def variant(name):
        st, nf, ok = res.start.copy(), res.nframes.copy(), res.ok.copy()
        out[name] = (st, nf, ok)
        return st, nf, ok
    st, nf, ok = variant('overlapping runs')
    st[p, 1] = st[p, 0] + nf[p, 0] - 1
    st, nf, ok = variant('an empty run')
    nf[p, 0] = 0
    st, nf, ok = variant('a run past lim')
    nf[p, L - 1] = lim - st[p, L - 1] + 1
    st, nf, ok = variant('equal neighbours without a blank')
    nf[p, 1] = st[p, 2] - st[p, 1]
    st, nf, ok = variant('ok_in = 0')
    ok[p] = 0
    st, nf, ok = variant('garbage')
    st[p, :L] = np.array([2 ** 31 - 1, -2 ** 31, 7][:L] + [2 ** 31 - 1] * (L - 3), dtype=np.int64).astype(np.int32)
    nf[p, :L] = 2 ** 31 - 1
    return out
