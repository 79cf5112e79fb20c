"""Generators and oracles for the phrase-boosting tests (qasr/boost.py, k_beam_boost).  NumPy only.

The oracles here share no code with qasr/boost.py: phrases are plain tuples, the boost of a string is a brute-force sum
over its substrings (`Brute.final`), and the float64 search is beam_cases.oracle_beam's rules plus the boost term, computed as
boost(p + c) - boost(p) from the brute-force function.  There is no trie, no fail link, no state, no table."""
import math

import numpy as np

import beam_cases
from beam_cases import GAP, MAX_WAIVED
from beam_lm_cases import EN_VOCAB, ZH_VOCAB

ONE = 1 << 16
EN_SPACE = EN_VOCAB.index(' ')


class Brute:
    """phrases: [(label tuple, weight in nats)].  whole: compile as space + labels + space with bonus 0 on the two added
    spaces (leading / trailing spaces of the phrase are stripped first).  Everything is integers of 2^-16 nat."""

    def __init__(self, phrases, whole, space=-1):
        self.whole, self.space = bool(whole), int(space)
        comp = {}
        for ids, w in phrases:
            ids = [int(c) for c in ids]
            wq = int(np.rint(float(w) * ONE))
            if whole:
                while ids and ids[0] == space:
                    ids = ids[1:]
                while ids and ids[-1] == space:
                    ids = ids[:-1]
                key, bonus = (space,) + tuple(ids) + (space,), (0,) + (wq,) * len(ids) + (0,)
            else:
                key, bonus = tuple(ids), (wq,) * len(ids)
            assert len(ids) > 0
            old = comp.get(key)
            comp[key] = bonus if old is None else tuple(max(a, b) for a, b in zip(old, bonus))
        self.comp = comp
        self.maxlen = max(len(k) for k in comp)
        # inc of a phrase prefix u: the largest bonus at its last position over the phrases that start with u
        self.prefixes = {}
        for key in comp:
            for k in range(1, len(key) + 1):
                u = key[:k]
                self.prefixes[u] = max(q[k - 1] for p, q in comp.items() if p[:k] == u)
        # g of a compiled phrase: the incs behind its longest proper prefix that is a compiled phrase itself
        self.g = {key: self._tail(key, proper=True) for key in comp}
        self.pot_of = {u: self._tail(u, proper=False) for u in self.prefixes}
        self._memo = {}

    def _tail(self, u, proper):
        j = 0
        for k in range(1, len(u) + (0 if proper else 1)):
            if u[:k] in self.comp:
                j = k
        return sum(self.prefixes[u[:k]] for k in range(j + 1, len(u) + 1))

    def _padded(self, y, end):
        y = tuple(int(c) for c in y)
        if not self.whole:
            return y
        return (self.space,) + y + ((self.space,) if end else ())

    def _substring_sum(self, s):
        tot = 0
        for i in range(len(s)):
            for key, g in self.g.items():
                if s[i:i + len(key)] == key:
                    tot += g
        return tot

    def final(self, y):
        """the boost of a finished hypothesis: the sum of g over all occurrences of compiled phrases as substrings"""
        return self._substring_sum(self._padded(y, True))

    def running(self, y):
        """the boost of an unfinished prefix: the occurrences so far, plus the provisional bonus of the longest suffix that
        is the beginning of a phrase"""
        s = self._padded(y, False)
        pot = 0
        for k in range(min(len(s), self.maxlen), 0, -1):
            if s[len(s) - k:] in self.prefixes:
                pot = self.pot_of[s[len(s) - k:]]
                break
        return self._substring_sum(s) + pot

    def running_fast(self, y):
        """running(y), memoised over prefixes (the substring sum split by the position where an occurrence ends)"""
        y = tuple(y)
        hit = self._memo.get(y)
        if hit is None:
            s = self._padded(y, False)
            ends = sum(g for key, g in self.g.items() if len(key) <= len(s) and s[len(s) - len(key):] == key)
            banked = ends + (self._memo_banked(y[:-1]) if y else 0)
            pot = 0
            for k in range(min(len(s), self.maxlen), 0, -1):
                if s[len(s) - k:] in self.prefixes:
                    pot = self.pot_of[s[len(s) - k:]]
                    break
            hit = self._memo[y] = (banked, pot)
        return hit[0] + hit[1]

    def _memo_banked(self, y):
        self.running_fast(y)
        return self._memo[tuple(y)][0]


def oracle_beam_boost(logp, W, N, blank, brute):
    """beam_cases.oracle_beam with the boost term: float64, dicts keyed by prefix tuples; returns the final beam after
    the finalisation and the one re-ordering, best first, as [(prefix, score, boost in nats)]"""
    NEGF = -math.inf
    lae = lambda a, b: float(np.logaddexp(a, b))       # noqa: E731
    T, C = logp.shape
    beam = [((), 0.0, NEGF)]
    for t in range(T):
        cands = [(int(c), float(logp[t, c])) for c in beam_cases.oracle_topn(logp[t], min(N, C))]
        acc = {}
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
                v += (brute.running_fast(ext) - brute.running_fast(pre)) / ONE
                if ext not in acc:
                    acc[ext] = [NEGF, NEGF, (i, n)]
                acc[ext][1] = lae(acc[ext][1], v)
        ents = [(lae(a[0], a[1]), a[2], pre, a[0], a[1]) for pre, a in acc.items()]
        ents = [e for e in ents if e[0] != NEGF]
        ents.sort(key=lambda e: (-e[0], e[1]))
        beam = [(e[2], e[3], e[4]) for e in ents[:W]]
    out = []
    for rank, (pre, pb, pnb) in enumerate(beam):
        fin = brute.final(pre)
        out.append((lae(pb, pnb) + (fin - brute.running_fast(pre)) / ONE, rank, pre, fin / ONE))
    out.sort(key=lambda e: (-e[0], e[1]))
    return [(e[2], e[0], e[3]) for e in out]


# ---------------------------------------------------------------------------------------------------------- phrase sets
NESTED = ((0, 1), (0, 1, 0, 1), (1, 0, 1), (1,))          # ab, abab, bab, b over a 4-label alphabet


def random_set(rng, n_labels=4, whole=False, space=3):
    """1 .. 5 phrases of 1 .. 4 labels over a tiny alphabet, overlapping and nested on purpose, weights 0 .. 3 nats in
    steps of 1/4.  With whole words the phrases avoid a leading / trailing space (it would be stripped) but may hold one."""
    pool = [list(p) for p in NESTED]
    out = []
    for _ in range(int(rng.integers(1, 6))):
        if rng.random() < 0.4:
            ids = list(pool[int(rng.integers(0, len(pool)))])
        else:
            ids = [int(c) for c in rng.integers(0, n_labels, size=int(rng.integers(1, 5)))]
        if whole:
            while ids and ids[0] == space:
                ids = ids[1:]
            while ids and ids[-1] == space:
                ids = ids[:-1]
            if not ids:
                ids = [0]
        out.append((tuple(ids), float(rng.integers(0, 13)) / 4.0))
    return out


def differing_piece(best, other, whole, space, rng):
    """a phrase out of `other` around the first place where it differs from `best`: 2 .. 4 labels, or (whole words) the
    word of `other` that holds the place; None if there is none"""
    d = next((i for i in range(min(len(best), len(other))) if best[i] != other[i]), min(len(best), len(other)))
    if d >= len(other):
        return None
    if whole:
        if other[d] == space:
            return None
        a = d
        while a > 0 and other[a - 1] != space:
            a -= 1
        b = d
        while b + 1 < len(other) and other[b + 1] != space:
            b += 1
        return tuple(other[a:b + 1])
    a = max(0, d - int(rng.integers(0, 2)))
    return tuple(other[a:a + int(rng.integers(2, 5))]) or None


# (name, classes, T, W, N, utterances, seed, sharp): the twin-against-oracle lists
CASE_LISTS = (
    ('en_t63_w16_n40', 29, 63, 16, 40, 10, 501, 1.5),
    ('en_t63_w1_n40', 29, 63, 1, 40, 10, 502, 1.5),
    ('en_t250_w16_n20', 29, 250, 16, 20, 4, 503, 2.0),
    ('zh_t63_w16_n40', 5207, 63, 16, 40, 6, 504, 1.5),
)


def case_list(name):
    """[(logp [T, C], blank, W, N, phrases [(labels, weight)], whole, space)] of one list.  The phrases of an utterance are
    drawn partly from its competing labels (pieces of the unboosted float64 search's runners-up, for W = 1 of a wider
    search's), so that boosting can win, partly at random; weights 0.5 .. 3 nats."""
    _, C, T, W, N, n, seed, sharp = next(s for s in CASE_LISTS if s[0] == name)
    rng = np.random.Generator(np.random.PCG64(seed))
    blank = C - 1
    en = C == 29
    whole, space = en, (EN_SPACE if en else -1)
    out = []
    for _ in range(n):
        lp = beam_cases.peaky_logp(rng, T, C, blank, sharp=sharp)
        o = beam_cases.oracle_beam(lp, max(W, 8), N, blank)
        phrases = []
        for other in o[1:4]:
            piece = differing_piece(o[0][0], other[0], whole, space, rng)
            if piece:
                phrases.append((piece, float(rng.uniform(0.5, 3.0))))
        for _ in range(2):                                          # and phrases that need not occur at all
            ids = tuple(int(c) for c in rng.integers(0, blank, size=int(rng.integers(1, 5))) if not (whole and c == space))
            if ids:
                phrases.append((ids, float(rng.uniform(0.5, 3.0))))
        best = o[0][0]
        if len(best) > 4 and not whole:                             # a piece of the best string: a phrase that does occur
            a = int(rng.integers(0, len(best) - 3))
            phrases.append((tuple(best[a:a + 3]), float(rng.uniform(0.5, 3.0))))
        out.append((lp, blank, W, N, phrases, whole, space))
    return out


_checked = {}


def checked_case_list(name):
    """[(logp, blank, W, N, phrases, whole, space, the boosted oracle's final beam, its top-1 / top-2 gap, the unboosted
    oracle's best string)].  Asserts the cap on waivers here, on the oracle alone: at most MAX_WAIVED of a list may have a
    gap below GAP.  A list that trips this is sharpened; the cap and the gap stay."""
    if name not in _checked:
        out = []
        for lp, blank, W, N, phrases, whole, space in case_list(name):
            o = oracle_beam_boost(lp, W, N, blank, Brute(phrases, whole, space))
            plain = beam_cases.oracle_beam(lp, W, N, blank)[0][0]
            out.append((lp, blank, W, N, phrases, whole, space, o, o[0][1] - o[1][1] if len(o) > 1 else math.inf, plain))
        waived = sum(c[8] < GAP for c in out)
        assert waived <= MAX_WAIVED * len(out), f'{name}: {waived} of {len(out)} cases have a float64 gap below {GAP}'
        _checked[name] = out
    return _checked[name]


def vocab_for(C):
    return EN_VOCAB if C == 29 else ZH_VOCAB


def gpu_phrases(rng, lp, lens, blank, whole, space, n_random=3):
    """phrases for a GPU batch [B, T, C]: pieces of the frames' best classes (so that matches happen) and random ones"""
    out = []
    for b in range(lp.shape[0]):
        lim = int(lens[b]) if lens is not None else lp.shape[1]
        if lim < 4:
            continue
        g = [c for c in beam_cases.greedy(lp[b, :lim], blank)]
        if whole:
            words, cur = [], []
            for c in g + [space]:
                if c == space:
                    if cur:
                        words.append(tuple(cur))
                    cur = []
                else:
                    cur.append(c)
            for w in words[:3]:
                out.append((w[:64], float(rng.uniform(0.5, 3.0))))
            if len(words) > 2:
                out.append(((words[1] + (space,) + words[2])[:64], float(rng.uniform(0.5, 3.0))))
        else:
            for a in range(0, max(len(g) - 3, 1), 5):
                out.append((tuple(g[a:a + int(rng.integers(1, 5))]), float(rng.uniform(0.5, 3.0))))
    for _ in range(n_random):
        ids = tuple(int(c) for c in rng.integers(0, blank, size=int(rng.integers(1, 5))) if not (whole and c == space))
        if ids:
            out.append((ids, float(rng.uniform(0.5, 3.0))))
    return [(list(p), w) for p, w in out if len(p)]


# (name, model of beam_lm_cases or None, classes, T, W, N, utterances, seed) of tests/golden/boost.npz: the twin's recorded outputs
FIXTURE_LISTS = (
    ('en_t63_w8_n20', None, 29, 63, 8, 20, 3, 601),
    ('zh_t40_w4_n20', None, 5207, 40, 4, 20, 2, 602),
    ('en3_t63_w8_n20', 'en3', 29, 63, 8, 20, 3, 603),
)


def fixture_inputs(spec):
    """log-probabilities [B, T, C], lengths [B] and the phrases of one fixture list (alpha 1.0, beta 0.5 with a model)"""
    import beam_lm_cases
    name, model, C, T, W, N, n, seed = spec
    rng = np.random.Generator(np.random.PCG64(seed))
    if model is None:
        lp = np.stack([beam_cases.peaky_logp(rng, T, C, C - 1) for _ in range(n)])
        lens = np.array([T] + [T // 2] * (n - 1), dtype=np.int32)
        if n > 2:
            lens[-1] = 0
    else:
        lp, lens = beam_lm_cases.batch_inputs(model, T, n, seed)
    whole = C == 29
    return lp, lens, gpu_phrases(rng, lp, lens, C - 1, whole, EN_SPACE if whole else -1)
