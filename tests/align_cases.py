"""Seeded inputs for the forced-alignment tests and their fixture generator (tests/golden/gen_golden_align.py), and an
independent float64 CTC alignment / forward oracle to hold qasr.align against.  NumPy only.

The oracle is written plainly: per-state Python loops, numpy.logaddexp, no table, no fixed point.  It shares nothing with
qasr/align.py but the rules of the lattice."""
import math

import numpy as np

import beam_cases

NEGF = -math.inf


def oracle_align(logp, y, blank):
    """float64 Viterbi and forward over logp [T, C] for the target y: (best path score, total log-likelihood), or None when
    no alignment exists"""
    lp = np.asarray(logp, dtype=np.float64)
    T, L = lp.shape[0], len(y)
    S = 2 * L + 1
    lab = [blank if s % 2 == 0 else int(y[(s - 1) // 2]) for s in range(S)]
    V, A = [NEGF] * S, [NEGF] * S
    for s in range(min(2, S)):
        V[s] = A[s] = float(lp[0, lab[s]])
    for t in range(1, T):
        V2, A2 = [NEGF] * S, [NEGF] * S
        for s in range(S):
            preds = [s]
            if s >= 1:
                preds.append(s - 1)
            if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2]:
                preds.append(s - 2)
            best = max(V[r] for r in preds)
            tot = NEGF
            for r in preds:
                tot = float(np.logaddexp(tot, A[r]))
            x = float(lp[t, lab[s]])
            V2[s] = best + x if best != NEGF else NEGF
            A2[s] = tot + x if tot != NEGF else NEGF
        V, A = V2, A2
    if L == 0:
        best, tot = V[0], A[0]
    else:
        best, tot = max(V[S - 1], V[S - 2]), float(np.logaddexp(A[S - 1], A[S - 2]))
    return None if best == NEGF else (best, tot)


def path_frames(start, nframes, L, T):
    """the label index of every frame (-1: blank) of the alignment that start / nframes [L] describe"""
    idx = np.full(T, -1, dtype=np.int64)
    for i in range(L):
        idx[int(start[i]):int(start[i]) + int(nframes[i])] = i
    return idx


def path_is_valid(start, nframes, y, T):
    """start / nframes describe a CTC alignment of y over T frames: runs in order, none empty, a blank between repeats"""
    end = -1
    for i in range(len(y)):
        s, n = int(start[i]), int(nframes[i])
        if n < 1 or s <= end or (i and y[i] == y[i - 1] and s <= end + 1):
            return False
        end = s + n - 1
    return end < T


def edited_targets(rng, g, C, blank):
    """the targets one utterance is aligned with: its greedy string, that string with one label substituted and one
    deleted, and a hand-made one with adjacent repeats"""
    g = list(g)
    out = [g]
    if len(g) >= 3:
        e = list(g)
        i = int(rng.integers(0, len(e)))
        e[i] = int((e[i] + 1 + rng.integers(0, C - 2)) % (C - 1))         # another non-blank label (blank = C - 1)
        del e[int(rng.integers(0, len(e)))]
        out.append(e)
        r = list(g[:len(g) // 2])
        out.append(r[:2] + r[1:2] + r[1:2] + r[2:] + r[-1:])             # x a a a ... z z
    return out


# (classes, T, utterances, seed): the shapes the rules were prototyped on; odd utterances are blended
ORACLE_SHAPES = ((29, 63, 8, 301), (29, 250, 6, 302), (5207, 120, 4, 303))

_cases = None


def oracle_cases():
    """[(logp [T, C] float32, blank, target, oracle (best, total) or None)] over ORACLE_SHAPES, computed once"""
    global _cases
    if _cases is None:
        _cases = []
        for C, T, n, seed in ORACLE_SHAPES:
            rng = np.random.Generator(np.random.PCG64(seed))
            for u in range(n):
                lp = beam_cases.peaky_logp(rng, T, C, C - 1, blend=(u % 2 == 1))
                for y in edited_targets(rng, beam_cases.greedy(lp, C - 1), C, C - 1):
                    _cases.append((lp, C - 1, y, oracle_align(lp, y, C - 1)))
    return _cases


def pad_targets(rows, blank, pitch=None):
    """targets int32 [P, pitch] (tail: blank) and target_lens int32 [P] of a list of label lists"""
    pitch = max(1, max(len(r) for r in rows)) if pitch is None else pitch
    tg = np.full((len(rows), pitch), blank, dtype=np.int32)
    for i, r in enumerate(rows):
        tg[i, :len(r)] = r
    return tg, np.array([len(r) for r in rows], dtype=np.int32)


# (name, classes, T, utterances, problems per utterance, seed) of tests/golden/align.npz
FIXTURE_LISTS = (
    ('en_t63_k1', 29, 63, 4, 1, 401),
    ('en_t250_k3', 29, 250, 3, 3, 402),
    ('c64_t120_k2', 64, 120, 3, 2, 403),
)


def fixture_inputs(spec):
    """log-probabilities [B, T, C], lengths [B], targets [B * K, pitch] and target lengths of one fixture list: greedy and
    edited targets against full, short and clamped lengths"""
    _, C, T, B, K, seed = spec
    rng = np.random.Generator(np.random.PCG64(seed))
    lp = np.stack([beam_cases.peaky_logp(rng, T, C, C - 1, blend=(u % 2 == 1)) for u in range(B)])
    lens = np.array([T] + [int(rng.integers(T // 2, T)) for _ in range(B - 1)], dtype=np.int32)
    lens[-1] = T + 3
    rows = []
    for u in range(B):
        lim = min(int(lens[u]), T)
        opts = edited_targets(rng, beam_cases.greedy(lp[u, :lim], C - 1), C, C - 1)
        rows += [opts[k % len(opts)] for k in range(K)]
    tg, tl = pad_targets(rows, C - 1)
    return lp, lens, tg, tl
