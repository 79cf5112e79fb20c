"""Fixtures of the beam search with a language model: a seeded generator of small ARPA models (counts over a synthetic
word list or label stream, absolute discounting, written as text), seeded log-probabilities that spell sentences of such
a model, and an independent float64 oracle - a dict-of-tuples ARPA reader with the plain recursive back-off, and the
prefix beam search of beam_cases.oracle_beam extended by the rules of qasr.beam.LM_RULES with numpy.logaddexp.  NumPy only;
nothing here is shared with qasr/ngram.py or qasr/beam.py.

The committed models (tests/golden/lm_*.arpa[.gz]) are what `write_models` generates; test_beam_lm_cpu.py checks that."""
import gzip
import math
import os

import numpy as np

from beam_cases import GAP, MAX_WAIVED, oracle_topn

LN10 = math.log(10.0)
OOV_SCORE = -1000.0
EN_VOCAB = list("abcdefghijklmnopqrstuvwxyz '")            # 28 labels, blank = 28
ZH_LABELS = 5206
ZH_VOCAB = [chr(0x4e00 + i) for i in range(ZH_LABELS)]      # stand-ins for the Zh model's labels, blank = 5206
DISCOUNT = 0.6

# (name, file, mode, order, word-list size or active labels, training tokens, seed)
MODELS = (
    ('en3', 'lm_en_word3.arpa', 'word', 3, 300, 900, 11),
    ('en1', 'lm_en_word1.arpa', 'word', 1, 300, 900, 12),
    ('en5', 'lm_en_word5.arpa', 'word', 5, 120, 500, 13),
    ('zh2', 'lm_zh_char2.arpa.gz', 'char', 2, 300, 1200, 14),
)


# ------------------------------------------------------------------------------------------------------- the generator
def word_list(rng, n):
    """n distinct words of 1 .. 6 letters (the apostrophe among them)"""
    letters = EN_VOCAB[:26] + ["'"]
    out, seen = [], set()
    while len(out) < n:
        w = ''.join(letters[i] for i in rng.integers(0, 26 if rng.random() < 0.9 else 27, size=int(rng.integers(1, 7))))
        if w not in seen and w.strip("'"):
            seen.add(w)
            out.append(w)
    return out


def corpus(rng, tokens, n_train):
    """sentences (lists of tokens) of 2 .. 9 tokens: a Zipf draw, half of the time steered by the previous token, so that
    higher orders carry information"""
    n = len(tokens)
    zipf = 1.0 / np.arange(1, n + 1)
    zipf /= zipf.sum()
    follow = rng.integers(0, n, size=(n, 3))
    out, total = [], 0
    while total < n_train:
        ln = int(rng.integers(2, 10))
        s, prev = [], None
        for _ in range(ln):
            if prev is not None and rng.random() < 0.5:
                i = int(follow[prev, rng.integers(0, 3)])
            else:
                i = int(rng.choice(n, p=zipf))
            s.append(tokens[i])
            prev = i
        out.append(s)
        total += ln
    return out


def arpa_text(sentences, order):
    """An ARPA model of `sentences` by absolute discounting with back-off, normalised in float64: p(w | ctx) =
    (c - D) / c(ctx) for seen n-grams, the rest of the mass backs off.  <s> has -99 as KenLM writes it; <unk> gets the
    mass of one unseen token."""
    counts = [None] + [dict() for _ in range(order)]
    for s in sentences:
        seq = ['<s>'] + list(s) + ['</s>']
        for k in range(1, order + 1):
            for i in range(len(seq) - k + 1):
                g = tuple(seq[i:i + k])
                if k == 1 and g[0] == '<s>':
                    continue
                counts[k][g] = counts[k].get(g, 0) + 1
    uni = counts[1]
    total = sum(uni.values()) + 1.0
    prob = {('<unk>',): math.log10(1.0 / total), ('<s>',): -99.0}
    for g, c in uni.items():
        prob[g] = math.log10(c / total)
    bow = {}

    def cond(ctx, w):
        g = ctx + (w,)
        if g in prob:
            return prob[g]
        return bow.get(ctx, 0.0) + cond(ctx[1:], w)

    for k in range(2, order + 1):
        by_ctx = {}
        for g, c in counts[k].items():
            by_ctx.setdefault(g[:-1], []).append((g[-1], c))
        for ctx in sorted(by_ctx):
            seen = by_ctx[ctx]
            c_ctx = float(sum(c for _, c in seen))
            lower = sum(10.0 ** cond(ctx[1:], w) for w, _ in seen)
            for w, c in seen:
                prob[ctx + (w,)] = math.log10((c - DISCOUNT) / c_ctx)
            bow[ctx] = math.log10((DISCOUNT * len(seen) / c_ctx) / max(1.0 - lower, 1e-9))
    lines = ['\\data\\']
    grams = [None] + [sorted(g for g in prob if len(g) == k) for k in range(1, order + 1)]
    grams[1].sort(key=lambda g: (g[0] not in ('<unk>', '<s>', '</s>'), g))
    for k in range(1, order + 1):
        lines.append(f'ngram {k}={len(grams[k])}')
    for k in range(1, order + 1):
        lines += ['', f'\\{k}-grams:']
        for g in grams[k]:
            b = bow.get(g)
            lines.append(f'{prob[g]:.6f}\t{" ".join(g)}' + (f'\t{b:.6f}' if b is not None and k < order else ''))
    lines += ['', '\\end\\', '']
    return '\n'.join(lines)


def model_tokens(spec):
    """the token list (words, or active labels) and the training sentences of one committed model"""
    _, _, mode, order, n, n_train, seed = spec
    rng = np.random.Generator(np.random.PCG64(seed))
    if mode == 'word':
        tokens = word_list(rng, n)
    else:
        tokens = [ZH_VOCAB[i] for i in sorted(rng.choice(ZH_LABELS, size=n, replace=False).tolist())]
    return tokens, corpus(rng, tokens, n_train)


def model_text(name):
    spec = next(s for s in MODELS if s[0] == name)
    return arpa_text(model_tokens(spec)[1], spec[3])


def model_path(golden_dir, name):
    return os.path.join(golden_dir, next(s for s in MODELS if s[0] == name)[1])


def write_models(golden_dir):
    for spec in MODELS:
        text, path = model_text(spec[0]), os.path.join(golden_dir, spec[1])
        if path.endswith('.gz'):
            with open(path, 'wb') as f, gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0) as z:
                z.write(text.encode('utf-8'))
        else:
            with open(path, 'w', encoding='utf-8') as f:
                f.write(text)


def scaled_model_text(mode, order, n_tokens, n_train, seed):
    """a larger model of the same make (the profile's: a few hundred thousand n-grams)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if mode == 'word':
        tokens = word_list(rng, n_tokens)
    else:
        tokens = [ZH_VOCAB[i] for i in sorted(rng.choice(ZH_LABELS, size=n_tokens, replace=False).tolist())]
    return arpa_text(corpus(rng, tokens, n_train), order), tokens


# ------------------------------------------------------------------------------------------------------- the oracle
class OracleLM:
    """An ARPA file as two dicts of word tuples, with the recursive back-off: float64, log10 as written"""

    def __init__(self, path):
        self.prob, self.bow, self.order = {}, {}, 0
        op = gzip.open if path.endswith('.gz') else open
        k = 0
        with op(path, 'rt', encoding='utf-8') as f:
            for line in f:
                line = line.strip()
                if not line or line.startswith('ngram ') or line in ('\\data\\', '\\end\\'):
                    continue
                if line.startswith('\\'):
                    k = int(line[1:line.index('-')])
                    self.order = max(self.order, k)
                    continue
                parts = line.split()
                g = tuple(parts[1:1 + k])
                self.prob[g] = float(parts[0])
                if len(parts) > k + 1:
                    self.bow[g] = float(parts[k + 1])

    def known(self, w):
        return (w,) in self.prob

    def cond(self, ctx, w):
        """ln p(w | ctx), ctx a tuple of words (any length; the last order - 1 count)"""
        ctx = tuple(ctx)[max(0, len(ctx) - (self.order - 1)):] if self.order > 1 else ()
        return LN10 * self._cond(ctx, w)

    def _cond(self, ctx, w):
        g = ctx + (w,)
        if g in self.prob:
            return self.prob[g]
        return self.bow.get(ctx, 0.0) + self._cond(ctx[1:], w)


def _advance(lm, vocab, space, state, c, alpha, beta):
    """state = (history words, current word labels, lm total) of a prefix; returns (term, state of prefix + c)"""
    hist, cur, tot = state
    if space is None:                                   # character mode
        w = vocab[c] if c < len(vocab) else None
        if w is None or not lm.known(w):
            t, hist = alpha * OOV_SCORE + beta, ()
        else:
            t, hist = alpha * lm.cond(hist, w) + beta, hist + (w,)
        return t, (hist, (), tot + t)
    if c != space:
        return 0.0, (hist, cur + (c,), tot)
    if not cur:                                         # a leading or doubled space
        return 0.0, state
    t, hist = _word_term(lm, vocab, hist, cur, alpha, beta)
    return t, (hist, (), tot + t)


def _word_term(lm, vocab, hist, cur, alpha, beta):
    w = ''.join(vocab[i] for i in cur)
    if not lm.known(w):
        return alpha * OOV_SCORE + beta, ()
    return alpha * lm.cond(hist, w) + beta, hist + (w,)


def oracle_beam_lm(logp, W, N, blank, lm, vocab, alpha, beta):
    """float64 prefix beam search with the model; returns the final beam, best first, as [(prefix, score, lm total)]"""
    NEGF = -math.inf
    lae = lambda a, b: float(np.logaddexp(a, b))       # noqa: E731
    T, C = logp.shape
    space = vocab.index(' ') if ' ' in vocab else None
    start = ('<s>',) if lm.known('<s>') else ()
    beam = [((), 0.0, NEGF, (start, (), 0.0))]
    for t in range(T):
        cands = [(int(c), float(logp[t, c])) for c in oracle_topn(logp[t], min(N, C))]
        acc = {}
        for i, (pre, pb, pnb, st) in enumerate(beam):
            acc[pre] = [NEGF, NEGF, (i, -1), st]
        for i, (pre, pb, pnb, st) in enumerate(beam):
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
                term, st2 = _advance(lm, vocab, space, st, c, alpha, beta)
                if ext not in acc:
                    acc[ext] = [NEGF, NEGF, (i, n), st2]
                acc[ext][1] = lae(acc[ext][1], v + term)
        ents = [(lae(a[0], a[1]), a[2], pre, a[0], a[1], a[3]) for pre, a in acc.items()]
        ents = [e for e in ents if e[0] != NEGF]
        ents.sort(key=lambda e: (-e[0], e[1]))
        beam = [(e[2], e[3], e[4], e[5]) for e in ents[:W]]
    out = []
    for pre, pb, pnb, (hist, cur, tot) in beam:
        sc = lae(pb, pnb)
        if space is not None and cur:
            t = _word_term(lm, vocab, hist, cur, alpha, beta)[0]
            sc, tot = sc + t, tot + t
        out.append((pre, sc, tot))
    out.sort(key=lambda e: -e[1])                       # stable: ties keep the previous rank
    return out


# ------------------------------------------------------------------------------------------------------- the inputs
def sentence_labels(rng, spec, n_words, tokens=None):
    """labels of a sentence drawn like the model's training text (word mode: words joined by spaces); tokens: those of a
    scaled model instead of the committed one's"""
    tokens = model_tokens(spec)[0] if tokens is None else tokens
    sent = corpus(rng, tokens, n_words)[0][:n_words]
    if spec[2] == 'word':
        return [EN_VOCAB.index(ch) for ch in ' '.join(sent)]
    return [ZH_VOCAB.index(ch) for ch in sent]


def frame_row(rng, labels, T, blank):
    """a CTC frame row of T frames that spells `labels` (as far as T reaches): runs of 1 .. 3 frames, blanks between"""
    row, prev = [], None
    for c in labels:
        if c == prev or rng.random() < 0.5:
            row += [blank] * int(rng.integers(1, 3))
        row += [c] * int(rng.integers(1, 4))
        prev = c
    row = row[:T]
    return np.array(row + [blank] * (T - len(row)), dtype=np.int64)


def lm_logp(rng, spec, T, sharp=1.5, tokens=None):
    """float32 log-probabilities [T, C] around a sentence of the model `spec`: peaks over Gaussian logits, and on every
    frame a competing class that is a label the model knows (so that the model has something to decide)"""
    word = spec[2] == 'word'
    C = 29 if word else ZH_LABELS + 1
    blank = C - 1
    labels = []
    while len(labels) < max(T // 2, 1):
        labels += sentence_labels(rng, spec, 6, tokens) + ([EN_VOCAB.index(' ')] if word else [])
    row = frame_row(rng, labels, T, blank)
    active = np.array(sorted(set(labels)))
    z = rng.normal(0, 1.0, size=(T, C)).astype(np.float32)
    peak = rng.gamma(2.0, sharp, size=T).astype(np.float32)
    z[np.arange(T), row] += peak + np.float32(math.log(C))
    comp = active[rng.integers(0, len(active), size=T)]
    z[np.arange(T), comp] += (peak * rng.random(T).astype(np.float32)) + np.float32(math.log(C)) * (rng.random(T) < 0.1)
    z = z - z.max(1, keepdims=True)
    p = np.exp(z.astype(np.float64))
    p /= p.sum(1, keepdims=True)
    return np.log(p).astype(np.float32)


# (name, model, T, W, N, alpha, beta, utterances, seed, sharp): the committed lists of the twin-against-oracle test
CASE_LISTS = (
    ('en_t63_w1', 'en3', 63, 1, 20, 0.5, 0.0, 6, 301, 1.5),
    ('en_t63_w16', 'en3', 63, 16, 20, 2.0, 1.5, 6, 302, 1.5),
    ('en_t250_w16', 'en3', 250, 16, 20, 0.5, 1.5, 4, 303, 1.5),
    ('en_t63_w128', 'en3', 63, 128, 20, 2.0, 0.0, 2, 304, 1.5),
    ('en_t250_w128', 'en3', 250, 128, 20, 0.5, 0.0, 1, 305, 2.0),
    ('zh_t63_w1', 'zh2', 63, 1, 20, 2.0, 1.5, 4, 306, 1.5),
    ('zh_t63_w16', 'zh2', 63, 16, 20, 0.5, 0.0, 4, 307, 1.5),
    ('zh_t250_w16', 'zh2', 250, 16, 20, 2.0, 0.0, 2, 308, 1.5),
    ('zh_t63_w128', 'zh2', 63, 128, 20, 0.5, 1.5, 2, 309, 1.5),
    ('zh_t250_w128', 'zh2', 250, 128, 20, 2.0, 1.5, 1, 310, 2.0),
)


def case_list(name):
    """[logp [T, C] float32] of one committed list"""
    _, model, T, W, N, alpha, beta, n, seed, sharp = next(s for s in CASE_LISTS if s[0] == name)
    spec = next(s for s in MODELS if s[0] == model)
    rng = np.random.Generator(np.random.PCG64(seed))
    return [lm_logp(rng, spec, T, sharp) for _ in range(n)]


_checked = {}


def checked_case_list(name, golden_dir):
    """[(logp, the oracle's final beam, float64 top-1 / top-2 gap)] of one committed list; asserts the cap on waivers here,
    in the generator: a list that trips it is drawn sharper, the cap and the gap stay"""
    if name not in _checked:
        _, model, T, W, N, alpha, beta, n, seed, sharp = next(s for s in CASE_LISTS if s[0] == name)
        lm = OracleLM(model_path(golden_dir, model))
        vocab = EN_VOCAB if model.startswith('en') else ZH_VOCAB
        out = []
        for lp in case_list(name):
            o = oracle_beam_lm(lp, W, N, lp.shape[1] - 1, lm, vocab, alpha, beta)
            out.append((lp, o, o[0][1] - o[1][1] if len(o) > 1 else math.inf))
        waived = sum(c[2] < GAP for c in out)
        assert waived <= MAX_WAIVED * len(out), f'{name}: {waived} of {len(out)} cases have a float64 gap below {GAP}'
        _checked[name] = out
    return _checked[name]


# (name, model, T, W, N, alpha, beta, utterances, seed) of tests/golden/beam_lm.npz: the twin's recorded outputs
FIXTURE_LISTS = (
    ('en3_t63_w16_n20', 'en3', 63, 16, 20, 1.0, 0.5, 3, 401),
    ('en5_t120_w8_n40', 'en5', 120, 8, 40, 0.7, -0.5, 2, 402),
    ('en1_t63_w4_n20', 'en1', 63, 4, 20, 2.0, 0.0, 2, 403),
    ('zh2_t63_w16_n20', 'zh2', 63, 16, 20, 1.5, 1.0, 2, 404),
)


def vocab_of(model):
    return EN_VOCAB if model.startswith('en') else ZH_VOCAB


def batch_inputs(model, T, n, seed, sharp=1.5):
    """log-probabilities [n, T, C] around sentences of `model` and lengths [n]: T, then shorter ones, the last 0 if n > 2"""
    spec = next(s for s in MODELS if s[0] == model)
    rng = np.random.Generator(np.random.PCG64(seed))
    lp = np.stack([lm_logp(rng, spec, T, sharp) for _ in range(n)])
    lens = np.array([T] + [T // 2] * (n - 1), dtype=np.int32)
    if n > 2:
        lens[-1] = 0
    return lp, lens
