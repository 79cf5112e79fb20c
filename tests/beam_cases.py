"""Seeded log-probabilities for the beam-search tests and their fixture generator (tests/golden/gen_golden_beam.py), and
an independent float64 CTC prefix beam search to hold qasr.beam against.  NumPy only.

The oracle is written plainly: dicts keyed by prefix tuples, numpy.logaddexp, no table, no fixed point, no hashes.  It
shares nothing with qasr/beam.py but the rules of the search."""
import math

import numpy as np

import ctc_cases

GAP = 0.002                 # float64 top-1 / top-2 gap below which "the best strings are equal" may be waived
MAX_WAIVED = 0.10           # ... for at most this share of a case list


def oracle_topn(row, n):
    """the n classes of largest log-probability, ties: lower class first"""
    return np.lexsort((np.arange(len(row)), -row.astype(np.float64)))[:n]


def oracle_beam(logp, W, N, blank):
    """float64 prefix beam search over logp [T, C]; returns the final beam, best first, as [(prefix tuple, score)]"""
    NEGF = -math.inf
    lae = lambda a, b: float(np.logaddexp(a, b))       # noqa: E731
    T, C = logp.shape
    beam = [((), 0.0, NEGF)]                            # (prefix, pb, pnb)
    for t in range(T):
        cands = [(int(c), float(logp[t, c])) for c in oracle_topn(logp[t], min(N, C))]
        acc = {}                                        # prefix -> [pb', pnb', tie key]
        for i, (pre, pb, pnb) in enumerate(beam):
            acc[pre] = [NEGF, NEGF, (i, -1)]
        for i, (pre, pb, pnb) in enumerate(beam):
            sc = lae(pb, pnb)
            last = pre[-1] if pre else -1
            for n, (c, lp) in enumerate(cands):
                if c == blank:
                    acc[pre][0] = lae(acc[pre][0], lp + sc)
                    continue
                if c == last:
                    if pnb != NEGF:
                        acc[pre][1] = lae(acc[pre][1], lp + pnb)
                    if pb == NEGF:
                        continue
                    v = lp + pb
                else:
                    v = lp + sc
                ext = pre + (c,)
                if ext not in acc:
                    acc[ext] = [NEGF, NEGF, (i, n)]
                acc[ext][1] = lae(acc[ext][1], v)
        ents = [(lae(a[0], a[1]), a[2], pre, a[0], a[1]) for pre, a in acc.items()]
        ents = [e for e in ents if e[0] != NEGF]
        ents.sort(key=lambda e: (-e[0], e[1]))
        beam = [(e[2], e[3], e[4]) for e in ents[:W]]
    return [(pre, lae(pb, pnb)) for pre, pb, pnb in beam]


def greedy(logp, blank):
    out, prev = [], blank
    for p in logp.argmax(1):
        if (p != prev or prev == blank) and p != blank:
            out.append(int(p))
        prev = p
    return tuple(out)


def peaky_logp(rng, T, C, blank, sharp=1.5, blend=False):
    """float32 log-probabilities [T, C] that look like a CTC model's: the classes of ctc_cases.realistic_row peak over
    Gaussian logits, with a competing class on every frame.  blend: half of the frames are mixed with their predecessor
    (0.55 p[t] + 0.45 p[t-1], renormalised), which smears label boundaries and makes the beam disagree with the arg-max."""
    row = ctc_cases.realistic_row(rng, T, blank)
    z = rng.normal(0, 1.0, size=(T, C)).astype(np.float32)
    peak = rng.gamma(2.0, sharp, size=T).astype(np.float32)
    z[np.arange(T), row] += peak + np.float32(math.log(C))
    comp = rng.integers(0, C, size=T)
    z[np.arange(T), comp] += (peak * rng.random(T).astype(np.float32)) + np.float32(math.log(C)) * (rng.random(T) < 0.3)
    z = z - z.max(1, keepdims=True)
    p = np.exp(z.astype(np.float64))
    p /= p.sum(1, keepdims=True)
    if blend:
        mix = rng.random(T) < 0.5
        mix[0] = False
        q = p.copy()
        q[mix] = 0.55 * p[mix] + 0.45 * p[np.flatnonzero(mix) - 1]
        p = q / q.sum(1, keepdims=True)
    return np.log(p).astype(np.float32)


# (name, classes, T, W, N, utterances, seed, blend, sharp): the committed case lists of the twin-against-oracle test.  The
# W = 128 and T = 1000 lists are short: the plain-Python oracle costs about T W N dictionary steps per utterance.  The
# float64 top-1 / top-2 gap of an utterance is the smallest over all of its ambiguous positions, so it shrinks with T: the
# T = 1000 lists are drawn with sharper peaks (2.5) so that no utterance of these short lists falls under GAP.
CASE_LISTS = (
    ('en_t250_w16_n20', 29, 250, 16, 20, 12, 101, False, 1.5),
    ('en_t63_w1_n20', 29, 63, 1, 20, 8, 102, False, 1.5),
    ('en_t63_w16_n40', 29, 63, 16, 40, 12, 103, False, 1.5),
    ('en_t250_w128_n20', 29, 250, 128, 20, 2, 104, False, 1.5),
    ('en_t1000_w16_n20', 29, 1000, 16, 20, 2, 105, False, 2.5),
    ('zh_t63_w16_n40', 5207, 63, 16, 40, 6, 106, False, 1.5),
    ('zh_t250_w16_n20_blend', 5207, 250, 16, 20, 6, 107, True, 1.5),
    ('zh_t63_w128_n40', 5207, 63, 128, 40, 2, 108, False, 1.5),
    ('zh_t1000_w1_n20', 5207, 1000, 1, 20, 2, 109, False, 2.5),
)


def case_list(name):
    """[(logp [T, C] float32, blank, W, N)] of one committed list: the inputs alone (checked_case_list adds the oracle)"""
    spec = next(s for s in CASE_LISTS if s[0] == name)
    _, C, T, W, N, n, seed, blend, sharp = spec
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(peaky_logp(rng, T, C, C - 1, sharp=sharp, blend=blend), C - 1, W, N) for _ in range(n)]


_checked = {}


def checked_case_list(name):
    """[(logp, blank, W, N, oracle's final beam, float64 top-1 / top-2 gap)] of one committed list.  Asserts the cap on
    waivers here, in the generator: at most MAX_WAIVED of a list may have a gap below GAP.  A list that trips this is
    sharpened (its `sharp`); the cap and the gap stay."""
    if name not in _checked:
        out = []
        for lp, blank, W, N in case_list(name):
            o = oracle_beam(lp, W, N, blank)
            out.append((lp, blank, W, N, o, o[0][1] - o[1][1] if len(o) > 1 else math.inf))
        waived = sum(c[5] < GAP for c in out)
        assert waived <= MAX_WAIVED * len(out), f'{name}: {waived} of {len(out)} cases have a float64 gap below {GAP}'
        _checked[name] = out
    return _checked[name]


def tie_rows(seed, T, C):
    """float32 log-prob-like rows with repeated values, exact zeros and both signs of zero: the tie rule of the top-N"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = -rng.gamma(0.5, 2.0, size=(T, C)).astype(np.float32)
    x = np.where(rng.random((T, C)) < 0.3, np.float32(-0.25), x)
    x[rng.random((T, C)) < 0.05] = 0.0
    x[rng.random((T, C)) < 0.02] = -0.0
    x = np.where(rng.random((T, C)) < 0.2, np.round(x), x)
    if T > 2:
        x[1] = np.float32(-1.5)                                  # a whole frame of one value
        x[2] = -np.arange(C, dtype=np.float32)                   # strictly descending
    return np.ascontiguousarray(x, dtype=np.float32)


def token_logp(tokens, n_classes, seed):
    """a token row as log-probabilities whose arg-max is that row: [T, C] float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = len(tokens)
    z = rng.normal(0, 1.0, size=(T, n_classes))
    z[np.arange(T), tokens] = z.max(1) + rng.gamma(2.0, 1.0, size=T) + 0.5
    z -= np.log(np.exp(z).sum(1, keepdims=True))
    return z.astype(np.float32)


# (name, classes, T, W, N, utterances, seed, blend) of tests/golden/beam.npz
FIXTURE_LISTS = (
    ('en_t63_w16_n20', 29, 63, 16, 20, 3, 201, False),
    ('en_t250_w8_n40', 29, 250, 8, 40, 2, 202, True),
    ('zh_t63_w16_n20', 5207, 63, 16, 20, 2, 203, True),
    ('zh_t120_w4_n40', 5207, 120, 4, 40, 2, 204, False),
)


def fixture_inputs(spec):
    """log-probabilities [B, T, C] and lengths [B] of one fixture list (the first utterance runs to T)"""
    _, C, T, W, N, n, seed, blend = spec
    rng = np.random.Generator(np.random.PCG64(seed))
    lp = np.stack([peaky_logp(rng, T, C, C - 1, blend=blend) for _ in range(n)])
    lens = np.array([T] + [int(rng.integers(T // 2, T)) for _ in range(n - 1)], dtype=np.int32)
    return lp, lens


def dense(top_id, top_lp, n_classes):
    """[B, T, C] float32 log-probabilities that hold top_lp at top_id and -1e30 elsewhere: what a fixture keeps of a wide
    distribution (the search reads nothing but each frame's N best classes)"""
    B, T, _ = top_id.shape
    lp = np.full((B, T, n_classes), -1e30, dtype=np.float32)
    np.put_along_axis(lp, top_id.astype(np.int64), top_lp.astype(np.float32), axis=2)
    return lp
