"""Phrase boosting ("hot words") for the CTC beam search (qasr/beam.py, k_beam_boost of csrc/qasr_beam_boost.hip): the
rules (BOOST_RULES), the phrase automaton, its packed form.  NumPy only.

pack() -> one little-endian blob, everything int32:
  header[32]: MAGIC, VERSION, total bytes, n_nodes, n_labels, start state, whole_words (0 / 1), table capacity (a power
              of two), probe bound (the longest probe chain of a stored key), rest 0
  table[capacity][4]: node, label, next, 0; an empty slot has node -1.  It holds only the transitions with node != root
              and delta(node, label) != delta(root, label).  Slot of a key: qasr.ngram.trans_slot, then linear probing; a
              look-up ends at a hit, at an empty slot or after `probe bound` probes, and a miss is root_next[label].
  nodes[n_nodes][2]: pot_q, bank_q (node 0 is the root)
  root_next[n_labels]: delta(root, label), the dense root row
(the table of 16-byte slots comes first, so that a slot is one aligned vector load, as in the packed n-gram model)
Capacities are at most half full (`min_capacity`: the smallest power of two above the count, for tests of long probe
chains); a probe bound above MAX_PROBE doubles the table.  qasr_boost_check (include/qasr.h) validates a blob."""
import numpy as np

from .beam import ONE
from .ngram import MAX_PROBE, _pow2_above, trans_slot

BOOST_RULES = """Phrase boosting (`boost`: qasr.boost.PhraseSet; `_search_one_boost` of qasr/beam.py, k_beam_boost on the device).

Input.  A list of phrases, each with a weight in nats PER LABEL, 0 <= weight <= 16, weight_q = rint(weight * 2^16).  A
phrase is text mapped through the vocabulary, or a list of label ids.  Refused (ValueError) before anything runs: an empty
list or an empty phrase, a character outside the vocabulary, a label >= n_labels (the blank is n_labels) or negative, more
than 64 labels in one phrase.  Duplicates merge (the max rule below).

Whole words (default: on when the vocabulary has a space, else off).  On: leading and trailing spaces of a phrase are
stripped and it is compiled as space + labels + space; the two added spaces carry bonus 0, every label of the phrase
itself (inner spaces too) carries weight_q.  Off: the phrase is compiled as it is.

Trie of the compiled phrases.  inc[n]: the maximum bonus over the phrases passing through node n; cum[n] = cum[parent] +
inc[n]; end[n]: a compiled phrase ends at n; lastend[n]: the nearest end node among n and its ancestors, else the root;
pot[n] = cum[n] - cum[lastend[n]] (the provisional bonus of an unfinished match; 0 at an end node); g[n] = cum[n] -
cum[nearest PROPER end ancestor, else root] at an end node, else 0; fail[n]: the longest proper suffix of n's string that
is a node; bank[n] = g[n] + bank[fail[n]] (every phrase that ends here, nested suffixes included); delta(n, c): the child
by c, else delta(fail[n], c), else (at the root) the root.  A set with a pot or bank above 2^30 is refused (weights are
not negative, so neither is a pot or a bank).

Search.  An entry keeps its automaton state and a running boost_tot.  The first entry starts in delta(root, space) with
whole words on, else in the root.  Extending parent p (state s) by a label c != blank moves to s' = delta(s, c) (a label
>= n_labels: the root) with the term pot[s'] - pot[s] + bank[s'].  The term joins the language-model term exactly where
LM_RULES puts that one: added to the score of a new prefix, kept as part of the entry's `own` for the E contribution, and
summed into boost_tot (lm_tot stays the model's share alone).  Blank steps and the A path add nothing.

After the last frame, for every entry: with whole words on one step by a virtual space (the term is added, the state
moves); then pot[state] is subtracted (an unfinished match earns nothing); both go to the score and to boost_tot.  With
a word-mode model the model's unfinished-word term is added in the same pass.  Then ONE re-ordering by score, ties by
previous rank.

Consequences.  For every reported hypothesis y, exactly: boost_tot = the sum of g over all occurrences of compiled
phrases as substrings of space + y + space (whole words on) or of y (off).  With every weight 0 the result equals the
search without boosting on every byte and boost_tot is 0."""

MAGIC = 0x31534251                  # 'QBS1'
VERSION = 1
HEADER_INTS = 32
MAX_PHRASE = 64
MAX_WEIGHT = 16.0
LIM = 1 << 30


def weight_q(w):
    w = float(w)
    if not 0.0 <= w <= MAX_WEIGHT:
        raise ValueError(f'boost: a weight must be 0 .. {MAX_WEIGHT:g} nats per label, got {w}')
    return int(np.rint(w * ONE))


class PhraseSet:
    """The compiled phrases of one vocabulary.  phrases: a list of text | label list | (text | label list, weight);
    `weight` is the default of entries without one.  vocabulary: the labels (needed for text; gives n_labels and the
    space); without one pass n_labels and, for whole words, space.  pot / bank / delta(state, label) / start are the host
    statement of the kernel's automaton."""

    def __init__(self, phrases, vocabulary=None, weight=1.0, whole_words=None, n_labels=None, space=None,
                 min_capacity=False):
        if isinstance(phrases, (str, bytes)):
            raise ValueError('boost: phrases must be a list, not one string')
        phrases = list(phrases)
        if not phrases:
            raise ValueError('boost: the list of phrases is empty')
        vocab = None if vocabulary is None else list(vocabulary)
        if vocab is None and n_labels is None:
            raise ValueError('boost: give the vocabulary, or n_labels')
        self.n_labels = len(vocab) if vocab is not None else int(n_labels)
        if self.n_labels < 1:
            raise ValueError(f'boost: n_labels {self.n_labels}')
        if vocab is not None:
            self.space = vocab.index(' ') if ' ' in vocab else -1
        else:
            self.space = -1 if space is None else int(space)
            if not -1 <= self.space < self.n_labels:
                raise ValueError(f'boost: space {self.space} is no label')
        self.whole_words = self.space >= 0 if whole_words is None else bool(whole_words)
        if self.whole_words and self.space < 0:
            raise ValueError('boost: whole_words needs a vocabulary with a space')
        self.min_capacity = bool(min_capacity)
        lab = None if vocab is None else {c: i for i, c in enumerate(vocab)}
        default_q = weight_q(weight)
        compiled = {}                                        # labels (compiled) -> bonus per position, merged by max
        for k, ph in enumerate(phrases):
            wq = default_q
            if isinstance(ph, tuple) and len(ph) == 2 and not isinstance(ph[1], str) and np.ndim(ph[1]) == 0 \
                    and (isinstance(ph[0], str) or np.ndim(ph[0]) == 1):
                ph, wq = ph[0], weight_q(ph[1])
            if isinstance(ph, str):
                if lab is None:
                    raise ValueError(f'boost: phrase {k} is text, which needs the vocabulary')
                bad = [ch for ch in ph if ch not in lab]
                if bad:
                    raise ValueError(f'boost: phrase {k} ({ph!r}) holds {bad[0]!r}, which is not in the vocabulary')
                ids = [lab[ch] for ch in ph]
            else:
                ids = [int(c) for c in ph]
            if any(not 0 <= c < self.n_labels for c in ids):
                raise ValueError(f'boost: phrase {k} holds a label outside 0 .. {self.n_labels - 1} (the blank is no label)')
            if self.whole_words:
                while ids and ids[0] == self.space:
                    ids = ids[1:]
                while ids and ids[-1] == self.space:
                    ids = ids[:-1]
            if not ids:
                raise ValueError(f'boost: phrase {k} is empty')
            if len(ids) > MAX_PHRASE:
                raise ValueError(f'boost: phrase {k} has {len(ids)} labels, at most {MAX_PHRASE}')
            bonus = [wq] * len(ids)
            if self.whole_words:
                ids, bonus = [self.space] + ids + [self.space], [0] + bonus + [0]
            key = tuple(ids)
            old = compiled.get(key)
            compiled[key] = tuple(bonus) if old is None else tuple(max(a, b) for a, b in zip(old, bonus))
        self.compiled = compiled
        self._build()
        self._blobs = {}

    # ------------------------------------------------------------------------------------------------ the automaton
    def _build(self):
        children, parent, label, inc, end = [{}], [0], [-1], [0], [False]
        for ids, bonus in self.compiled.items():
            n = 0
            for c, bq in zip(ids, bonus):
                m = children[n].get(c)
                if m is None:
                    m = len(children)
                    children[n][c] = m
                    children.append({}), parent.append(n), label.append(c), inc.append(0), end.append(False)
                inc[m] = max(inc[m], bq)
                n = m
            end[n] = True
        nn = len(children)
        cum, lastend, pot, g = [0] * nn, [0] * nn, [0] * nn, [0] * nn
        fail, bank = [0] * nn, [0] * nn
        order = [0]
        for n in order:                                      # breadth first: parents and shorter strings come first
            order.extend(children[n].values())
        diff = [None] * nn                                   # per node: label -> next where it differs from the root's row
        diff[0] = {}
        root = children[0]
        for n in order[1:]:
            p, c = parent[n], label[n]
            cum[n] = cum[p] + inc[n]
            pe = lastend[p]                                  # nearest end among the proper ancestors (or the root)
            lastend[n] = n if end[n] else pe
            pot[n] = cum[n] - cum[lastend[n]]
            g[n] = cum[n] - cum[pe] if end[n] else 0
            if p == 0:
                fail[n] = 0
            else:
                f = fail[p]
                while f and c not in children[f]:
                    f = fail[f]
                fail[n] = children[f].get(c, 0)
            bank[n] = g[n] + bank[fail[n]]
            d = dict(diff[fail[n]])
            d.update(children[n])
            diff[n] = {k: v for k, v in d.items() if v != root.get(k, 0)}
        if max(pot) > LIM or max(bank) > LIM:
            raise ValueError(f'boost: the phrases nest too deeply: a pot or bank above 2^30 ({max(pot)}, {max(bank)})')
        self.n_nodes = nn
        self.children, self.fail_link, self.g = children, fail, g
        self.pot, self.bank = np.array(pot, np.int64), np.array(bank, np.int64)
        self.root_next = np.zeros(self.n_labels, np.int32)
        for c, m in root.items():
            self.root_next[c] = m
        self.diff = diff
        self.start = int(self.root_next[self.space]) if self.whole_words else 0

    def delta(self, s, c):
        """the state after label c in state s (a label outside the vocabulary: the root)"""
        c = int(c)
        if not 0 <= c < self.n_labels:
            return 0
        hit = self.diff[int(s)].get(c)
        return int(self.root_next[c]) if hit is None else hit

    def term(self, s, c):
        """(term, next state) of extending an entry in state s by label c"""
        t = self.delta(s, c)
        return int(self.pot[t] - self.pot[s] + self.bank[t]), t

    def finish(self, s):
        """the correction after the last frame for an entry in state s"""
        tot = 0
        if self.whole_words:
            tm, s = self.term(s, self.space)
            tot += tm
        return tot - int(self.pot[s])

    def score(self, labels):
        """boost_tot of a finished label sequence (what the search reports for it)"""
        s, tot = self.start, 0
        for c in labels:
            tm, s = self.term(s, c)
            tot += tm
        return tot + self.finish(s)

    # ------------------------------------------------------------------------------------------------ packing
    def pack(self, min_capacity=None) -> bytes:
        key = self.min_capacity if min_capacity is None else bool(min_capacity)
        if key not in self._blobs:
            self._blobs[key] = self._pack(key)
        return self._blobs[key]

    def _pack(self, tight):
        trans = [(n, c, t) for n in range(1, self.n_nodes) for c, t in self.diff[n].items()]
        cap = _pow2_above(len(trans)) if tight else _pow2_above(2 * len(trans))
        while True:
            tab = np.zeros((cap, 4), np.int32)
            tab[:, 0] = -1
            probe = 1
            for n, c, t in trans:
                s, k = trans_slot(n, c, cap), 1
                while tab[s, 0] != -1:
                    s, k = (s + 1) & (cap - 1), k + 1
                tab[s] = (n, c, t, 0)
                probe = max(probe, k)
            if probe <= MAX_PROBE:
                break
            cap *= 2
        nodes = np.stack([self.pot, self.bank], axis=1).astype(np.int32)
        hdr = np.zeros(HEADER_INTS, np.int32)
        total = 4 * (HEADER_INTS + tab.size + nodes.size + self.n_labels)
        hdr[:9] = (MAGIC, VERSION, total, self.n_nodes, self.n_labels, self.start, int(self.whole_words), cap, probe)
        return b''.join(a.astype('<i4').tobytes() for a in (hdr, tab, nodes, self.root_next))


class PackedView:
    """A packed set read back (the kernel's view of it): delta by one bounded probe sequence, pot, bank."""

    def __init__(self, blob):
        a = np.frombuffer(bytes(blob), '<i4')
        h = a[:HEADER_INTS]
        if int(h[0]) != MAGIC or int(h[1]) != VERSION or int(h[2]) != len(blob):
            raise ValueError('boost: not a packed phrase set')
        self.n_nodes, self.n_labels, self.start = int(h[3]), int(h[4]), int(h[5])
        self.whole_words, self.cap, self.probe = bool(h[6]), int(h[7]), int(h[8])
        o = HEADER_INTS
        self.table = a[o:o + 4 * self.cap].reshape(self.cap, 4)
        o += 4 * self.cap
        nodes = a[o:o + 2 * self.n_nodes].reshape(self.n_nodes, 2)
        self.pot, self.bank = nodes[:, 0].astype(np.int64), nodes[:, 1].astype(np.int64)
        o += 2 * self.n_nodes
        self.root_next = a[o:o + self.n_labels]

    def delta(self, s, c):
        if not 0 <= c < self.n_labels:
            return 0
        if s != 0:
            k = trans_slot(s, c, self.cap)
            for _ in range(self.probe):
                e = self.table[k]
                if e[0] == s and e[1] == c:
                    return int(e[2])
                if e[0] < 0:
                    break
                k = (k + 1) & (self.cap - 1)
        return int(self.root_next[c])


def as_phrase_set(boost, vocabulary, weight=1.0):
    """decode(boost=) / BeamSearchDecoderWithLM(boost=): a PhraseSet as it is (its vocabulary size is checked), a list
    of phrases compiled for `vocabulary` with the default weight"""
    vocab = list(vocabulary)
    if isinstance(boost, PhraseSet):
        if boost.n_labels != len(vocab):
            raise ValueError(f'boost: the phrase set was compiled for {boost.n_labels} labels, the vocabulary has {len(vocab)}')
        return boost
    return PhraseSet(boost, vocab, weight=weight)


def read_phrase_file(path):
    """one phrase per line with an optional <tab>weight; '#' lines and blank lines are skipped.  Returns a list of text
    or (text, weight)."""
    out = []
    with open(path, encoding='utf-8') as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip() or line.lstrip().startswith('#'):
                continue
            if '\t' in line:
                text, w = line.rsplit('\t', 1)
                try:
                    out.append((text, float(w)))
                except ValueError:
                    raise ValueError(f'{path}:{no}: the weight {w!r} is no number') from None
            else:
                out.append(line)
    return out
