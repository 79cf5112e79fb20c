"""Back-off n-gram language models for the CTC beam search (qasr/beam.py, k_beam_lm of csrc/qasr_beam.hip): a reader of
ARPA text files, the fixed-point model and its packed form.  NumPy only: no kenlm, no ctc_decoders.

Mode, as ctc_decoders' Scorer takes it from the vocabulary: labels that contain ' ' make the model word-based (its tokens
are words, scored when a space ends a non-empty word); otherwise it is character-based (every label is a token; the Zh model).

Arithmetic.  A log10 probability or back-off x becomes q = rint(x * ln 10 * 2^16) in float64, clamped to +-2^30; entries
of -99 or below (and -inf) take the floor -2^30.  raw(ctx, w) is a sum of at most `order` such integers (`NgramLM.raw`),
clamped to +-(2^31 - 1) so that the kernel keeps one frame's values as int32.  An out-of-vocabulary word scores OOV_Q =
-1000 * 2^16 (ctc_decoders' OOV_SCORE, whatever <unk> has) and empties the context.

Structure.  One context node per n-gram of order below the model's (closed under "drop the first word" and "drop the
last word"; added ones have back-off 0), sorted by order: node 0 is the empty context, `level[k] .. level[k + 1]` are the
nodes of k words, suffix(node) is the node without its first word, one level down.  Every n-gram is a transition
(context node, word id) -> (prob_q, next) with next = the node of the longest suffix of context + word that is a node.
Word ids are the positions of the 1-grams in the file.

pack() -> one little-endian blob, everything int32 unless said:
  header[32]: MAGIC, VERSION, order, mode (0 character, 1 word), n_nodes, start (the node of <s>, or 0), trans_cap,
              trans_probe (the longest probe chain of a stored key), n_labels, word_cap, word_probe, n_words,
              total bytes, level[0 .. 7] at [13 .. 20] (level[k] for k > order - 1 equals n_nodes), rest 0
  trans[trans_cap][4]: node, word, prob_q, next; an empty slot has node -1.  Slot of a key: `trans_slot`, then linear
              probing; a look-up ends at an empty slot or after trans_probe probes.
  words[word_cap][4]: hash low, hash high, word id, 0; an empty slot has id -1.  Word mode: the 64-bit hash of a word is
              beam._hmix folded over its label ids from 0; slot = hash & (word_cap - 1), linear probing, word_probe bound.
              Words that the vocabulary cannot spell are left out; two words of one hash are refused.
  nodes[n_nodes][2]: backoff_q, suffix
  label_to_word[n_labels]: the word id of a label in character mode, -1: none (all -1 in word mode)
(the two tables of 16-byte slots come first, so that a slot is one aligned vector load)
Capacities are powers of two, at most half full (`min_capacity`: the smallest power of two above the count, for tests of
long probe chains); a probe bound above MAX_PROBE doubles the table.  qasr_lm_check (include/qasr.h) validates a blob.

Out of scope: KenLM binary files (export ARPA), orders above 6, </s> scoring, the dictionary FST of ctc_decoders."""
import gzip
import math
import os

import numpy as np

from .beam import FRAC, ONE, Q_CEIL, Q_FLOOR, _HMUL, _M64, _hmix

MAGIC = 0x314D4C51                  # 'QLM1'
VERSION = 1
MAX_ORDER = 6
MAX_PROBE = 1024
HEADER_INTS = 32
OOV_Q = -1000 * ONE
RAW_LIM = (1 << 31) - 1
MAX_ALPHA = 16.0
MAX_BETA = 16.0
_LN10 = math.log(10.0)


class BinaryModelError(ModuleNotFoundError):
    """a KenLM binary file: reading one needs kenlm / ctc_decoders, which this project does not use"""


def quantize_log10(x):
    """log10 value -> fixed point (see the module docstring)"""
    x = float(x)
    if not x > -99.0:                    # -99, anything below, -inf and NaN: the floor
        return Q_FLOOR
    return int(min(max(np.rint(np.float64(x) * _LN10 * ONE), Q_FLOOR), Q_CEIL))


def fixed_weights(alpha, beta):
    """(alpha_q, beta_q) = rint(. * 2^16); refuses alpha outside 0 .. 16 and |beta| > 16"""
    alpha, beta = float(alpha), float(beta)
    if not 0.0 <= alpha <= MAX_ALPHA:
        raise ValueError(f'alpha must be 0 .. {MAX_ALPHA:g}, got {alpha}')
    if not abs(beta) <= MAX_BETA:
        raise ValueError(f'beta must be -{MAX_BETA:g} .. {MAX_BETA:g}, got {beta}')
    return int(np.rint(alpha * ONE)), int(np.rint(beta * ONE))


def term(raw, alpha_q, beta_q):
    """the language-model term of one scored token"""
    return ((int(raw) * int(alpha_q) + (1 << (FRAC - 1))) >> FRAC) + int(beta_q)


def word_hash(ids):
    h = np.zeros(1, np.uint64)
    for c in ids:
        h = _hmix(h, np.array([c], np.int64))
    return int(h[0])


def trans_slot(node, word, cap):
    x = ((((int(node) & 0xffffffff) << 32) | (int(word) & 0xffffffff)) * _HMUL) & _M64
    return (x ^ (x >> 32)) & (cap - 1)


def _pow2_above(n):
    c = 1
    while c <= n:
        c <<= 1
    return c


class NgramLM:
    """One model for one vocabulary.  words: the 1-grams in file order; order; word_mode; space (label id, -1 in character
    mode); start (context node of <s>, else 0); raw(ctx, w) / lookup_word(hash) are the host statement of the kernel's walk."""

    def __init__(self, order, words, grams, vocabulary, source='', min_capacity=False):
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f'n-gram models of order 1 .. {MAX_ORDER} are supported, got {order}')
        self.order, self.words, self.source = order, list(words), source
        self.min_capacity = bool(min_capacity)               # what pack() does when it is not told
        self.vocabulary = list(vocabulary)
        self.word_mode = ' ' in self.vocabulary
        self.space = self.vocabulary.index(' ') if self.word_mode else -1
        self.n_labels = len(self.vocabulary)
        self._build(grams)
        self._blobs = {}

    # ------------------------------------------------------------------------------------------------ reading
    @classmethod
    def from_arpa(cls, path, vocabulary, min_capacity=False):
        """A text ARPA file (gzip-compressed too), orders 1 .. 6.  A KenLM binary file is refused: export ARPA."""
        path = os.fspath(path)
        why = ('is a KenLM binary file; reading one needs kenlm / ctc_decoders, which this build does not use: export '
               'the model as ARPA text (the file lmplz writes) and pass that')
        if path.endswith(('.binary', '.bin', '.klm', '.trie', '.probing')):
            raise BinaryModelError(f'{path} {why}')
        with open(path, 'rb') as f:
            head = f.read(64)
        if head.startswith(b'mmap lm http://kheafield.com/code'):
            raise BinaryModelError(f'{path} {why}')
        opener = gzip.open if head[:2] == b'\x1f\x8b' else open
        counts, grams, k = {}, [None] + [dict() for _ in range(MAX_ORDER)], 0
        words, wid = [], {}
        seen_data = False
        with opener(path, 'rt', encoding='utf-8', errors='strict') as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip('\r\n')
                if not line.strip():
                    continue
                if line.startswith('\\'):
                    tag = line.strip()
                    if tag == '\\data\\':
                        seen_data = True
                    elif tag == '\\end\\':
                        break
                    elif tag.endswith('-grams:') and tag[1:-7].isdigit():
                        k = int(tag[1:-7])
                        if not 1 <= k <= MAX_ORDER:
                            raise ValueError(f'{path}: order {k}: orders 1 .. {MAX_ORDER} are supported')
                    else:
                        raise ValueError(f'{path}:{no}: unknown section {tag!r}')
                    continue
                if not seen_data:
                    raise ValueError(f'{path}:{no}: not an ARPA file (no \\data\\ section)')
                if k == 0:
                    if line.startswith('ngram '):
                        a, b = line[6:].split('=')
                        counts[int(a)] = int(b)
                    continue
                f_ = line.split()                                 # log10 p, k words, an optional back-off
                toks = f_[1:1 + k]
                if not k + 1 <= len(f_) <= k + 2:
                    raise ValueError(f'{path}:{no}: expected a {k}-gram')
                if k == 1:
                    if toks[0] in wid:
                        raise ValueError(f'{path}:{no}: the 1-gram {toks[0]!r} is listed twice')
                    wid[toks[0]] = len(words)
                    words.append(toks[0])
                try:
                    key = tuple(wid[t] for t in toks)
                except KeyError:
                    raise ValueError(f'{path}:{no}: a word of this {k}-gram has no 1-gram') from None
                grams[k][key] = (float(f_[0]), float(f_[k + 1]) if len(f_) > k + 1 else 0.0)
        order = max([k for k in range(1, MAX_ORDER + 1) if grams[k]] + [0])
        if max(counts, default=0) > MAX_ORDER:
            raise ValueError(f'{path}: order {max(counts)}: orders 1 .. {MAX_ORDER} are supported')
        if order == 0:
            raise ValueError(f'{path}: no n-grams')
        return cls(order, words, grams[:order + 1], vocabulary, source=path, min_capacity=min_capacity)

    # ------------------------------------------------------------------------------------------------ the fixed-point model
    def _build(self, grams):
        order = self.order
        wid = {w: i for i, w in enumerate(self.words)}
        ctx = {(): 0.0}
        for k in range(1, order):
            for g, (_, bo) in grams[k].items():
                ctx[g] = bo
        todo = [g[:-1] for k in range(1, order + 1) for g in grams[k]] + list(ctx)
        while todo:                                              # closure: contexts of every n-gram, suffixes and prefixes of every node
            g = todo.pop()
            if g not in ctx:
                ctx[g] = 0.0
            for h in (g[1:], g[:-1]):
                if g and h not in ctx:
                    ctx[h] = 0.0
                    todo.append(h)
        keys = sorted(ctx, key=lambda g: (len(g), g))
        node = {g: i for i, g in enumerate(keys)}
        self.node_of = node
        self.level = [0] * 8
        for k in range(8):
            self.level[k] = sum(len(g) < k for g in keys)
        self.backoff = np.array([quantize_log10(ctx[g]) if g else 0 for g in keys], np.int32)
        self.suffix = np.array([node[g[1:]] if g else 0 for g in keys], np.int32)
        trans = {}
        for k in range(1, order + 1):
            for g, (lp, _) in grams[k].items():
                nx = g if k < order else g[1:]
                while nx not in node:
                    nx = nx[1:]
                trans[(node[g[:-1]], g[-1])] = (quantize_log10(lp), node[nx])
        self.trans = trans
        bos = wid.get('<s>')
        self.start = node.get((bos,), 0) if bos is not None and order > 1 else 0
        self.label_to_word = np.full(self.n_labels, -1, np.int32)
        self.word_of_hash = {}
        if self.word_mode:
            lab = {c: i for i, c in enumerate(self.vocabulary)}
            for w, i in wid.items():
                if not w or ' ' in w or any(ch not in lab for ch in w):
                    continue
                h = word_hash([lab[ch] for ch in w])
                if h in self.word_of_hash:
                    raise ValueError(f'the words {self.words[self.word_of_hash[h]]!r} and {w!r} have one 64-bit label hash')
                self.word_of_hash[h] = i
        else:
            for i, c in enumerate(self.vocabulary):
                self.label_to_word[i] = wid.get(c, -1)
            n_tok = sum(w not in ('<s>', '</s>', '<unk>') for w in self.words)
            if 2 * int((self.label_to_word >= 0).sum()) < n_tok:
                raise ValueError('fewer than half of this model\'s 1-grams are labels of the vocabulary: a word model needs a '
                                 'vocabulary with a space (word mode), a character model one whose labels are its 1-grams')
        self._memo = {}

    def raw(self, ctx, w):
        """(raw, next context) of word id w (-1: out of vocabulary) after context node ctx"""
        r = self._memo.get((ctx, w))
        if r is None:
            if w < 0:
                r = (OOV_Q, 0)
            else:
                acc, nd, nxt = 0, int(ctx), 0
                for _ in range(self.order):
                    hit = self.trans.get((nd, w))
                    if hit is not None:
                        acc, nxt = acc + hit[0], hit[1]
                        break
                    acc, nd = acc + int(self.backoff[nd]), int(self.suffix[nd])
                r = (min(max(acc, -RAW_LIM), RAW_LIM), nxt)
            self._memo[(ctx, w)] = r
        return r

    def lookup_word(self, h):
        return self.word_of_hash.get(int(h), -1)

    def context_of(self, word_ids):
        """the node a history of word ids leaves (the longest suffix that is a node)"""
        g = tuple(word_ids)[-(self.order - 1):] if self.order > 1 else ()
        while g not in self.node_of:
            g = g[1:]
        return self.node_of[g]

    # ------------------------------------------------------------------------------------------------ packing
    def pack(self, min_capacity=None) -> bytes:
        key = self.min_capacity if min_capacity is None else bool(min_capacity)
        if key not in self._blobs:
            self._blobs[key] = self._pack(key)
        return self._blobs[key]

    def _pack(self, tight):
        n_nodes = len(self.backoff)
        cap = _pow2_above(len(self.trans)) if tight else _pow2_above(2 * len(self.trans))
        while True:
            tab = np.zeros((cap, 4), np.int32)
            tab[:, 0] = -1
            probe = 1
            for (nd, w), (pq, nx) in self.trans.items():
                s, n = trans_slot(nd, w, cap), 1
                while tab[s, 0] != -1:
                    s, n = (s + 1) & (cap - 1), n + 1
                tab[s] = (nd, w, pq, nx)
                probe = max(probe, n)
            if probe <= MAX_PROBE:
                break
            cap *= 2
        wcap = (_pow2_above(len(self.word_of_hash)) if tight else _pow2_above(2 * len(self.word_of_hash))) if self.word_mode else 1
        while True:
            wt = np.zeros((wcap, 4), np.int32)
            wt[:, 2] = -1
            wprobe = 1
            for h, i in self.word_of_hash.items():
                s, n = h & (wcap - 1), 1
                while wt[s, 2] != -1:
                    s, n = (s + 1) & (wcap - 1), n + 1
                wt[s] = np.array([h & 0xffffffff, h >> 32, i, 0], np.uint32).view(np.int32)
                wprobe = max(wprobe, n)
            if wprobe <= MAX_PROBE:
                break
            wcap *= 2
        hdr = np.zeros(HEADER_INTS, np.int32)
        nodes = np.stack([self.backoff, self.suffix], axis=1).astype(np.int32)
        l2w = self.label_to_word.astype(np.int32)
        total = 4 * (HEADER_INTS + nodes.size + tab.size + l2w.size + wt.size)
        hdr[:13] = (MAGIC, VERSION, self.order, int(self.word_mode), n_nodes, self.start, cap, probe, self.n_labels, wcap, wprobe,
                    len(self.words), total)
        hdr[13:21] = self.level
        return b''.join(a.astype('<i4').tobytes() for a in (hdr, tab, wt, nodes, l2w))
