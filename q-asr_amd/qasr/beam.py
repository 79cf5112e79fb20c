"""CTC prefix beam search in fixed point, without and with an n-gram language model (LM_RULES below): the host statement of k_topn / k_beam / k_beam_lm
(csrc/qasr_beam.hip, include/qasr.h), of k_beam_boost (phrase boosting: qasr/boost.py, csrc/qasr_beam_boost.hip) and the step from the final beam to strings.  NumPy only: no GPU, no native library.

`topn_host` and `beam_search_host` are the CPU fallback of BeamSearchDecoderWithLM / EncDecCTCModel.decode(beam_width=)
and the yardstick the GPU tests compare the kernels with, bit for bit.

Arithmetic.  A float32 log-probability x becomes the integer q = rint(x * 2^16) (`quantize`: the float32 product is exact;
it is clamped to [-2^30, 2^30] before rounding, NaN takes the floor, rounding is to nearest-even).  Scores are sums of such
integers in int64: with T <= MAX_T = 65536 frames |score| < 2^30 * 2^16 + 3 * 2^16 * 45426 < 2^47, far from the sentinel
NEG = -2^62 that stands for log 0; nothing is ever added to NEG.  lae(a, b) (log-add-exp): NEG is the neutral element;
otherwise m = max(a, b), d = m - min(a, b), the result is m if d >= 16 * 2^16, else m + TAB[d >> 6] with
TAB[i] = rint(log1p(exp(-(64 i) / 2^16)) * 2^16) (`lae_table`: 16384 entries of 16 bits, built once in float64; the kernel
gets it as an argument and never calls exp or log).  lae is commutative; it is not associative, and no accumulator of the
search receives more than two contributions, so the order of accumulation cannot change a bit.

Search.  Per utterance the beam is an ordered list of at most W entries (prefix, pb, pnb), score = lae(pb, pnb), starting as
[((), 0, NEG)].  For every frame t < min(lens[b], T) with candidates (c_n, q_n), n < N, best first (`topn_host`; slots with
c_n < 0 are empty), the next beam is chosen among
  * every entry p (slot i) itself: pb' = q_blank + score(p) (NEG if blank is no candidate); pnb' = lae(A, E) with
    A = q_last + pnb(p) if last(p) is a candidate and pnb(p) != NEG, and E = the extension of p's parent by last(p) (below) if
    the parent - the entry whose prefix is p without its last label - is in the beam; score' = lae(pb', pnb');
  * every new prefix p + c_n, c_n != blank, that is not itself an entry of the beam: pb' = NEG, pnb' = q_n + pb(p) if
    c_n == last(p) (none if pb(p) == NEG), else q_n + score(p).
Candidates whose score is NEG are dropped; the best W of the rest by score descending form the next beam, ties by the index
i * (N + 1) + (0 for the entry itself, n + 1 for its extension by candidate n) ascending: a total order that does not depend
on thread order.  "Is p + c in the beam" compares a 64-bit hash of the prefix (`_hmix`, h(()) = 0) together with its length;
the first matching slot counts, and the same rule finds an entry's parent.  The result is the final beam in order."""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

FRAC = 16
ONE = 1 << FRAC
SH = 6                                  # table step: 2^SH fixed-point units
DMAX = 16 * ONE                         # differences from here on add nothing
TAB_ENTRIES = DMAX >> SH                # 16384
NEG = -(1 << 62)                        # log 0
Q_FLOOR = -(1 << 30)                    # clamp of one frame's q
Q_CEIL = 1 << 30
EMPTY_Q = -(1 << 31)                    # cand_q of an empty candidate slot (cand_id -1)
MAX_W = 128
MAX_N = 64
MAX_T = 65536
_HMUL = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1

_tab = None


def lae_table() -> np.ndarray:
    """TAB as uint16 [16384] (values <= 45426)"""
    global _tab
    if _tab is None:
        i = np.arange(TAB_ENTRIES, dtype=np.float64)
        t = np.rint(np.log1p(np.exp(-(i * (1 << SH)) / ONE)) * ONE)
        assert t.max() <= 65535 and t.min() >= 0
        _tab = t.astype(np.uint16)
    return _tab


def quantize(x) -> np.ndarray:
    """float32 log-probabilities -> int32 fixed point (see the module docstring)"""
    with np.errstate(over='ignore', invalid='ignore'):
        y = np.asarray(x, dtype=np.float32) * np.float32(ONE)
        y = np.where(y >= np.float32(Q_FLOOR), y, np.float32(Q_FLOOR))          # NaN and -inf take the floor
        y = np.minimum(y, np.float32(Q_CEIL))
        return np.rint(y).astype(np.int32)


def _order_key(x):
    """float32 -> int32 that orders like the float on every bit pattern (-0 < +0), as qasr.ctc and k_ctc use it"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def lae(a, b, tab=None):
    """element-wise log-add-exp of int64 fixed-point arrays (or scalars)"""
    tab = lae_table() if tab is None else tab
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    m, n = np.maximum(a, b), np.minimum(a, b)
    d = m - n
    near = (n != NEG) & (d < DMAX)
    return np.where(near, m + tab[np.where(near, d >> SH, 0)].astype(np.int64), m)


def topn_host(log_probs, n, lens=None):
    """log_probs float32 [B, T, C]; n = cutoff_top_n (1 .. 64).  Returns cand_id int32 [B, T, n] and cand_q int32 [B, T, n]:
    per frame the min(n, C) classes of largest log-probability, best first (order of the float bit patterns, ties: lower
    class id first) with their fixed-point values; the remaining slots, and every frame t >= min(lens[b], T), hold
    -1 / EMPTY_Q."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'topn_host: log_probs must be [B, T, C] with B, T, C >= 1, got {lp.shape}')
    if not 1 <= int(n) <= MAX_N:
        raise ValueError(f'topn_host: cutoff_top_n must be 1 .. {MAX_N}, got {n}')
    B, T, C = lp.shape
    n = int(n)
    ne = min(n, C)
    cid = np.full((B, T, n), -1, dtype=np.int32)
    cq = np.full((B, T, n), EMPTY_Q, dtype=np.int32)
    for b in range(B):
        lim = T if lens is None else int(min(max(int(lens[b]), 0), T))
        if not lim:
            continue
        key = _order_key(lp[b, :lim]).astype(np.int64)
        if ne < C:                                                  # cut the sort down: everything >= the ne-th largest key
            kth = -np.partition(-key, ne - 1, axis=1)[:, ne - 1]
        for t in range(lim):
            row = key[t]
            pool = np.flatnonzero(row >= kth[t]) if ne < C else np.arange(C)
            order = pool[np.argsort(-row[pool], kind='stable')[:ne]]           # pool ascends: ties keep the lower id first
            cid[b, t, :ne] = order
            cq[b, t, :ne] = quantize(lp[b, t, order])
    return cid, cq


@dataclass
class BeamResult:
    """Outputs of one search (arrays: NumPy on the host, torch tensors from the device binding), hypotheses best first.
    labels [B, n_best, T] int32 (tail and unused rows: blank), n_labels [B, n_best] int32, score [B, n_best] int64 fixed
    point (unused rows: NEG; score / 2^16 is the log-probability), n_hyps [B] int32."""
    labels: object
    n_labels: object
    score: object
    n_hyps: object
    blank: int = -1
    lm_score: object = None             # with a language model: int64 [B, n_best], the model's share of score (unused rows: 0)
    boost_score: object = None          # with a phrase set: int64 [B, n_best], the boosting's share of score (unused rows: 0)


def _hmix(h, c):
    """hash of prefix + (c) from the hash of prefix: uint64 arrays"""
    with np.errstate(over='ignore'):
        x = (h ^ (c.astype(np.uint64) + np.uint64(1))) * np.uint64(_HMUL)
    return x ^ (x >> np.uint64(32))


def _search_one(cid, cq, lim, blank, W, tab):
    """one utterance: cid / cq [T, N]; returns the final beam as a list of (labels, score)"""
    N = cid.shape[1]
    i64 = np.int64
    pb, pnb, sc = np.array([0], i64), np.array([NEG], i64), np.array([0], i64)
    hsh, phs = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    ln, last, node = np.zeros(1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int64)
    nodes_parent, nodes_label = [], []                      # node id = t * W + slot in the kernel; here: a growing list + map
    node_of = {}
    for t in range(lim):
        nb = len(sc)
        if nb == 0:
            break
        c, q = cid[t].astype(np.int64), cq[t].astype(i64)
        valid = c >= 0
        isb = valid & (c == blank)
        # the entries themselves
        match = (last[:, None] == c[None, :]) & valid[None, :]
        has, nl = match.any(1), match.argmax(1)
        pm = (phs[:, None] == hsh[None, :]) & (ln[:, None] == ln[None, :] + 1)
        hasp, ps = pm.any(1), pm.argmax(1)
        q_l = q[nl]
        pb_n = sc + q[isb.argmax()] if isb.any() else np.full(nb, NEG, i64)
        own = has & (pnb != NEG)
        a = np.where(own, q_l + np.where(own, pnb, 0), NEG)
        pbase = np.where(last[ps] == last, pb[ps], sc[ps])
        ext = has & hasp & (pbase != NEG)
        e = np.where(ext, q_l + np.where(ext, pbase, 0), NEG)
        pnb_n = lae(a, e, tab)
        sc_n = lae(pb_n, pnb_n, tab)
        child = np.zeros((nb, N), dtype=bool)
        sel = has & hasp
        child[ps[sel], nl[sel]] = True
        # new prefixes
        base = np.where(c[None, :] == last[:, None], pb[:, None], sc[:, None])
        ok = (valid & ~isb)[None, :] & ~child & (base != NEG)
        v = np.where(ok, np.where(ok, base, 0) + q[None, :], NEG)
        allc = np.concatenate([sc_n[:, None], v], axis=1).ravel()
        n_live = int((allc != NEG).sum())
        order = np.argsort(-allc, kind='stable')[:min(W, n_live)]
        src, k = order // (N + 1), order % (N + 1)
        kept = k == 0
        cn = c[np.maximum(k - 1, 0)]
        n_pb = np.where(kept, pb_n[src], NEG)
        n_pnb = np.where(kept, pnb_n[src], allc[order])
        n_sc = allc[order]
        n_hsh = np.where(kept, hsh[src], _hmix(hsh[src], cn))
        n_phs = np.where(kept, phs[src], hsh[src])
        n_ln = np.where(kept, ln[src], ln[src] + 1).astype(np.int32)
        n_last = np.where(kept, last[src], cn).astype(np.int32)
        n_node = np.where(kept, node[src], t * W + np.arange(len(order)))
        for s in np.flatnonzero(~kept):
            node_of[int(n_node[s])] = len(nodes_parent)
            nodes_parent.append(int(node[src[s]]))
            nodes_label.append(int(cn[s]))
        pb, pnb, sc, hsh, phs, ln, last, node = n_pb, n_pnb, n_sc, n_hsh, n_phs, n_ln, n_last, n_node
    out = []
    for h in range(len(sc)):
        labs, nd = [], int(node[h])
        for _ in range(int(ln[h])):
            if nd < 0:
                break
            j = node_of[nd]
            labs.append(nodes_label[j])
            nd = nodes_parent[j]
        out.append((labs[::-1], int(sc[h])))
    return out


LM_RULES = """The search with a language model (`lm`: qasr.ngram.NgramLM; `_search_one_lm` here, k_beam_lm on the device).

raw(ctx, w): acc = 0, node = ctx; at most `order` times: a transition (node, w) adds its prob_q, makes its `next` the new
context and stops; a miss adds backoff_q[node] and moves to suffix[node].  A walk that never hits ends in the empty context.
The sum is clamped to +-(2^31 - 1).  An out-of-vocabulary word (word mode: its label hash is not in the word table;
character mode: a label without a 1-gram) has raw = -1000 * 2^16 and the empty context.
term = ((raw * alpha_q + 2^15) >> 16) + beta_q (int64 product, arithmetic shift), alpha_q = rint(alpha * 2^16),
beta_q = rint(beta * 2^16), 0 <= alpha <= 16, |beta| <= 16.

An entry keeps, next to its other state, its context node (the first: <s>, or the empty context without one), the hash
of its current word (_hmix over the labels since the last space, 0 when empty), the term of its own creation `own` and
the running sum lm_tot.  Extending a parent p by a label c != blank has the term
  character mode: term(raw(ctx(p), word of c)); the context moves on;
  word mode: c == space after a non-empty current word (last(p) exists and is no space): term(raw(ctx(p), word of the
    hash)), the context moves on and the word starts empty; a leading or doubled space: 0, the context stays; any other
    label: 0, and the word hash advances.
The term is added to the score of a new prefix p + c (own = term, lm_tot = lm_tot(p) + term) and, when p + c is an
entry already, to the E contribution of the module docstring as that entry's `own` (the term depends on the prefix
alone).  Blank steps and the A path add nothing.  After the last frame, in word mode, every entry whose current word is
not empty receives that word's term once (score and lm_tot), and the beam is re-ordered by score, ties by previous rank.
</s> is never scored.  Candidate order, the tie rule, hashes and the trie are those of the search without a model."""


def _search_one_lm(cid, cq, lim, blank, W, tab, lm, alpha_q, beta_q):
    """one utterance under LM_RULES; returns the final beam as a list of (labels, score, lm_tot)"""
    N = cid.shape[1]
    i64 = np.int64
    word_mode, space, nlab, l2w = lm.word_mode, lm.space, lm.n_labels, lm.label_to_word
    half = 1 << (FRAC - 1)
    pb, pnb, sc = np.array([0], i64), np.array([NEG], i64), np.array([0], i64)
    hsh, phs = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    ln, last, node = np.zeros(1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int64)
    ctx, wh = np.array([lm.start], np.int32), np.zeros(1, np.uint64)
    own, lmt = np.zeros(1, i64), np.zeros(1, i64)
    nodes_parent, nodes_label = [], []
    node_of = {}
    for t in range(lim):
        nb = len(sc)
        if nb == 0:
            break
        c, q = cid[t].astype(np.int64), cq[t].astype(i64)
        valid = c >= 0
        isb = valid & (c == blank)
        match = (last[:, None] == c[None, :]) & valid[None, :]
        has, nl = match.any(1), match.argmax(1)
        pm = (phs[:, None] == hsh[None, :]) & (ln[:, None] == ln[None, :] + 1)
        hasp, ps = pm.any(1), pm.argmax(1)
        q_l = q[nl]
        pb_n = sc + q[isb.argmax()] if isb.any() else np.full(nb, NEG, i64)
        ownp = has & (pnb != NEG)
        a = np.where(ownp, q_l + np.where(ownp, pnb, 0), NEG)
        pbase = np.where(last[ps] == last, pb[ps], sc[ps])
        ext = has & hasp & (pbase != NEG)
        e = np.where(ext, q_l + np.where(ext, pbase, 0) + own, NEG)
        pnb_n = lae(a, e, tab)
        sc_n = lae(pb_n, pnb_n, tab)
        child = np.zeros((nb, N), dtype=bool)
        sel = has & hasp
        child[ps[sel], nl[sel]] = True
        base = np.where(c[None, :] == last[:, None], pb[:, None], sc[:, None])
        ok = (valid & ~isb)[None, :] & ~child & (base != NEG)
        # the terms of this frame, evaluated once
        scored, raws = np.zeros((nb, N), dtype=bool), np.zeros((nb, N), i64)
        if word_mode:
            inword = (last >= 0) & (last != space)
            for n in np.flatnonzero(valid & (c == space)):
                for i in np.flatnonzero(ok[:, n] & inword):
                    raws[i, n], scored[i, n] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[0], True
        else:
            wids = np.where(valid & (c < nlab), l2w[np.clip(c, 0, nlab - 1)], -1)
            for i, n in zip(*np.nonzero(ok)):
                raws[i, n] = lm.raw(int(ctx[i]), int(wids[n]))[0]
            scored = ok
        tm = np.where(scored, ((raws * alpha_q + half) >> FRAC) + beta_q, 0)
        v = np.where(ok, np.where(ok, base, 0) + q[None, :] + tm, NEG)
        allc = np.concatenate([sc_n[:, None], v], axis=1).ravel()
        n_live = int((allc != NEG).sum())
        order = np.argsort(-allc, kind='stable')[:min(W, n_live)]
        src, k = order // (N + 1), order % (N + 1)
        kept = k == 0
        kn = np.maximum(k - 1, 0)
        cn = c[kn]
        n_pb = np.where(kept, pb_n[src], NEG)
        n_pnb = np.where(kept, pnb_n[src], allc[order])
        n_sc = allc[order]
        n_hsh = np.where(kept, hsh[src], _hmix(hsh[src], cn))
        n_phs = np.where(kept, phs[src], hsh[src])
        n_ln = np.where(kept, ln[src], ln[src] + 1).astype(np.int32)
        n_last = np.where(kept, last[src], cn).astype(np.int32)
        n_node = np.where(kept, node[src], t * W + np.arange(len(order)))
        n_own = np.where(kept, own[src], tm[src, kn])
        n_lmt = np.where(kept, lmt[src], lmt[src] + tm[src, kn])
        n_ctx, n_wh = ctx[src].copy(), wh[src].copy()
        for s in np.flatnonzero(~kept):
            i, n = int(src[s]), int(kn[s])
            if word_mode and cn[s] != space:
                n_wh[s] = _hmix(wh[i:i + 1], cn[s:s + 1])[0]
            else:
                n_wh[s] = 0
                if not word_mode:
                    n_ctx[s] = lm.raw(int(ctx[i]), int(wids[n]))[1]
                elif scored[i, n]:
                    n_ctx[s] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[1]
            node_of[int(n_node[s])] = len(nodes_parent)
            nodes_parent.append(int(node[i]))
            nodes_label.append(int(cn[s]))
        pb, pnb, sc, hsh, phs, ln, last, node = n_pb, n_pnb, n_sc, n_hsh, n_phs, n_ln, n_last, n_node
        ctx, wh, own, lmt = n_ctx, n_wh, n_own, n_lmt
    if word_mode and len(sc):                                   # the unfinished word of every entry, then the order
        sc, lmt = sc.copy(), lmt.copy()
        for i in np.flatnonzero((last >= 0) & (last != space)):
            tv = ((lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[0] * alpha_q + half) >> FRAC) + beta_q
            sc[i] += tv
            lmt[i] += tv
        rank = np.argsort(-sc, kind='stable')
    else:
        rank = np.arange(len(sc))
    out = []
    for h in rank:
        labs, nd = [], int(node[h])
        for _ in range(int(ln[h])):
            if nd < 0:
                break
            j = node_of[nd]
            labs.append(nodes_label[j])
            nd = nodes_parent[j]
        out.append((labs[::-1], int(sc[h]), int(lmt[h])))
    return out


def _search_one_boost(cid, cq, lim, blank, W, tab, lm, alpha_q, beta_q, bs):
    """one utterance under BOOST_RULES of qasr/boost.py (bs: a PhraseSet), with LM_RULES when lm is not None; returns the
    final beam as a list of (labels, score, lm_tot, boost_tot)"""
    N = cid.shape[1]
    i64 = np.int64
    has_lm = lm is not None
    word_mode = has_lm and lm.word_mode
    if has_lm:
        space, nlab, l2w = lm.space, lm.n_labels, lm.label_to_word
    half = 1 << (FRAC - 1)
    pb, pnb, sc = np.array([0], i64), np.array([NEG], i64), np.array([0], i64)
    hsh, phs = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    ln, last, node = np.zeros(1, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int64)
    ctx, wh = np.array([lm.start if has_lm else 0], np.int32), np.zeros(1, np.uint64)
    own, lmt = np.zeros(1, i64), np.zeros(1, i64)
    bst, btot = np.array([bs.start], np.int64), np.zeros(1, i64)
    nodes_parent, nodes_label = [], []
    node_of = {}
    for t in range(lim):
        nb = len(sc)
        if nb == 0:
            break
        c, q = cid[t].astype(np.int64), cq[t].astype(i64)
        valid = c >= 0
        isb = valid & (c == blank)
        match = (last[:, None] == c[None, :]) & valid[None, :]
        has, nl = match.any(1), match.argmax(1)
        pm = (phs[:, None] == hsh[None, :]) & (ln[:, None] == ln[None, :] + 1)
        hasp, ps = pm.any(1), pm.argmax(1)
        q_l = q[nl]
        pb_n = sc + q[isb.argmax()] if isb.any() else np.full(nb, NEG, i64)
        ownp = has & (pnb != NEG)
        a = np.where(ownp, q_l + np.where(ownp, pnb, 0), NEG)
        pbase = np.where(last[ps] == last, pb[ps], sc[ps])
        ext = has & hasp & (pbase != NEG)
        e = np.where(ext, q_l + np.where(ext, pbase, 0) + own, NEG)
        pnb_n = lae(a, e, tab)
        sc_n = lae(pb_n, pnb_n, tab)
        child = np.zeros((nb, N), dtype=bool)
        sel = has & hasp
        child[ps[sel], nl[sel]] = True
        base = np.where(c[None, :] == last[:, None], pb[:, None], sc[:, None])
        ok = (valid & ~isb)[None, :] & ~child & (base != NEG)
        # the terms of this frame, evaluated once: the model's, then the boost's
        scored, raws = np.zeros((nb, N), dtype=bool), np.zeros((nb, N), i64)
        if word_mode:
            inword = (last >= 0) & (last != space)
            for n in np.flatnonzero(valid & (c == space)):
                for i in np.flatnonzero(ok[:, n] & inword):
                    raws[i, n], scored[i, n] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[0], True
        elif has_lm:
            wids = np.where(valid & (c < nlab), l2w[np.clip(c, 0, nlab - 1)], -1)
            for i, n in zip(*np.nonzero(ok)):
                raws[i, n] = lm.raw(int(ctx[i]), int(wids[n]))[0]
            scored = ok
        tm = np.where(scored, ((raws * alpha_q + half) >> FRAC) + beta_q, 0)
        btm, bnx = np.zeros((nb, N), i64), np.zeros((nb, N), i64)
        for i, n in zip(*np.nonzero(ok)):
            btm[i, n], bnx[i, n] = bs.term(int(bst[i]), int(c[n]))
        v = np.where(ok, np.where(ok, base, 0) + q[None, :] + tm + btm, NEG)
        allc = np.concatenate([sc_n[:, None], v], axis=1).ravel()
        n_live = int((allc != NEG).sum())
        order = np.argsort(-allc, kind='stable')[:min(W, n_live)]
        src, k = order // (N + 1), order % (N + 1)
        kept = k == 0
        kn = np.maximum(k - 1, 0)
        cn = c[kn]
        n_pb = np.where(kept, pb_n[src], NEG)
        n_pnb = np.where(kept, pnb_n[src], allc[order])
        n_sc = allc[order]
        n_hsh = np.where(kept, hsh[src], _hmix(hsh[src], cn))
        n_phs = np.where(kept, phs[src], hsh[src])
        n_ln = np.where(kept, ln[src], ln[src] + 1).astype(np.int32)
        n_last = np.where(kept, last[src], cn).astype(np.int32)
        n_node = np.where(kept, node[src], t * W + np.arange(len(order)))
        n_own = np.where(kept, own[src], tm[src, kn] + btm[src, kn])
        n_lmt = np.where(kept, lmt[src], lmt[src] + tm[src, kn])
        n_btot = np.where(kept, btot[src], btot[src] + btm[src, kn])
        n_bst = np.where(kept, bst[src], bnx[src, kn])
        n_ctx, n_wh = ctx[src].copy(), wh[src].copy()
        for s in np.flatnonzero(~kept):
            i, n = int(src[s]), int(kn[s])
            if has_lm:
                if word_mode and cn[s] != space:
                    n_wh[s] = _hmix(wh[i:i + 1], cn[s:s + 1])[0]
                else:
                    n_wh[s] = 0
                    if not word_mode:
                        n_ctx[s] = lm.raw(int(ctx[i]), int(wids[n]))[1]
                    elif scored[i, n]:
                        n_ctx[s] = lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[1]
            node_of[int(n_node[s])] = len(nodes_parent)
            nodes_parent.append(int(node[i]))
            nodes_label.append(int(cn[s]))
        pb, pnb, sc, hsh, phs, ln, last, node = n_pb, n_pnb, n_sc, n_hsh, n_phs, n_ln, n_last, n_node
        ctx, wh, own, lmt, bst, btot = n_ctx, n_wh, n_own, n_lmt, n_bst, n_btot
    if len(sc):                                                 # the corrections of every entry, then ONE re-ordering
        sc, lmt, btot = sc.copy(), lmt.copy(), btot.copy()
        if word_mode:
            for i in np.flatnonzero((last >= 0) & (last != space)):
                tv = ((lm.raw(int(ctx[i]), lm.lookup_word(wh[i]))[0] * alpha_q + half) >> FRAC) + beta_q
                sc[i] += tv
                lmt[i] += tv
        for i in range(len(sc)):
            fin = bs.finish(int(bst[i]))
            sc[i] += fin
            btot[i] += fin
        rank = np.argsort(-sc, kind='stable')
    else:
        rank = np.arange(len(sc))
    out = []
    for h in rank:
        labs, nd = [], int(node[h])
        for _ in range(int(ln[h])):
            if nd < 0:
                break
            j = node_of[nd]
            labs.append(nodes_label[j])
            nd = nodes_parent[j]
        out.append((labs[::-1], int(sc[h]), int(lmt[h]), int(btot[h])))
    return out


def beam_search_host(cand_id, cand_q, lens=None, blank=None, beam_width=16, n_best=None, lm=None, alpha=0.0,
                     beta=0.0, boost=None) -> BeamResult:
    """cand_id / cand_q int32 [B, T, N] as topn_host (or k_topn) writes them; lens int [B] or None (the padded row);
    blank: the blank id (required); beam_width W: 1 .. 128; n_best: 1 .. W hypotheses to report (None: W).  lm: a
    qasr.ngram.NgramLM (None: the search without a model, alpha and beta unused) with its weights 0 <= alpha <= 16,
    |beta| <= 16: the rules of LM_RULES; the result then carries lm_score.  boost: a qasr.boost.PhraseSet (None: no
    boosting, the searches above as they are), with or without a model: BOOST_RULES of qasr/boost.py; the result then
    carries boost_score."""
    if blank is None:
        raise ValueError('beam_search_host: blank is required (the decoder\'s last class)')
    cid, cq = np.asarray(cand_id), np.asarray(cand_q)
    if cid.ndim != 3 or cid.shape != cq.shape or min(cid.shape) < 1:
        raise ValueError(f'beam_search_host: candidates must be two [B, T, N] arrays, got {cid.shape} / {cq.shape}')
    B, T, N = cid.shape
    W = int(beam_width)
    nbest = W if n_best is None else int(n_best)
    if not 1 <= W <= MAX_W:
        raise ValueError(f'beam_search_host: beam_width must be 1 .. {MAX_W}, got {W}')
    if not 1 <= N <= MAX_N:
        raise ValueError(f'beam_search_host: at most {MAX_N} candidates per frame, got {N}')
    if not 1 <= nbest <= W:
        raise ValueError(f'beam_search_host: n_best must be 1 .. beam_width, got {nbest}')
    if T > MAX_T:
        raise ValueError(f'beam_search_host: at most {MAX_T} frames, got {T}')
    if lm is not None:
        from .ngram import fixed_weights
        alpha_q, beta_q = fixed_weights(alpha, beta)
        if lm.n_labels != int(blank):
            raise ValueError(f'beam_search_host: the model was loaded for {lm.n_labels} labels, blank is {blank}')
    else:
        alpha_q = beta_q = 0
    if boost is not None and boost.n_labels != int(blank):
        raise ValueError(f'beam_search_host: the phrase set was compiled for {boost.n_labels} labels, blank is {blank}')
    tab = lae_table()
    labels = np.full((B, nbest, T), blank, dtype=np.int32)
    n_labels = np.zeros((B, nbest), dtype=np.int32)
    score = np.full((B, nbest), NEG, dtype=np.int64)
    n_hyps = np.zeros(B, dtype=np.int32)
    lm_score = None if lm is None else np.zeros((B, nbest), dtype=np.int64)
    boost_score = None if boost is None else np.zeros((B, nbest), dtype=np.int64)
    for b in range(B):
        lim = T if lens is None else int(min(max(int(lens[b]), 0), T))
        if boost is not None:
            beam = _search_one_boost(cid[b].astype(np.int32), cq[b].astype(np.int32), lim, int(blank), W, tab, lm, alpha_q,
                                     beta_q, boost)[:nbest]
        elif lm is None:
            beam = _search_one(cid[b].astype(np.int32), cq[b].astype(np.int32), lim, int(blank), W, tab)[:nbest]
        else:
            beam = _search_one_lm(cid[b].astype(np.int32), cq[b].astype(np.int32), lim, int(blank), W, tab, lm, alpha_q,
                                  beta_q)[:nbest]
        n_hyps[b] = len(beam)
        for h, ent in enumerate(beam):
            labs, s = ent[0], ent[1]
            labels[b, h, :len(labs)] = labs
            n_labels[b, h] = len(labs)
            score[b, h] = s
            if lm is not None:
                lm_score[b, h] = ent[2]
            if boost is not None:
                boost_score[b, h] = ent[3]
    return BeamResult(labels, n_labels, score, n_hyps, int(blank), lm_score, boost_score)


def search_host(log_probs, lens=None, blank=None, beam_width=16, n_best=None, cutoff_top_n=40, lm=None, alpha=0.0,
                beta=0.0, boost=None) -> BeamResult:
    """topn_host + beam_search_host on float32 log-probabilities [B, T, C] (blank None: the last class)"""
    lp = np.asarray(log_probs, dtype=np.float32)
    blank = lp.shape[-1] - 1 if blank is None else blank
    cid, cq = topn_host(lp, cutoff_top_n, lens)
    return beam_search_host(cid, cq, lens, blank, beam_width, n_best, lm, alpha, beta, boost)


def _np(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def to_hypotheses(result: BeamResult, vocabulary: Sequence[str]) -> List[list]:
    """Per utterance the list of its hypotheses, best first, as qasr.ctc.Hypothesis: text, labels and utt_score = the beam
    score (log-probability of the prefix, summed over its alignments inside the beam).  start_s / end_s / score / words stay
    empty here: a prefix stands for many alignments, so no label has one time or one frame score (qasr.align gives the times of
    its best alignment: decode(beam_width=, timestamps=True))."""
    from .ctc import Hypothesis
    labels, n_labels, score, n_hyps = _np(result.labels), _np(result.n_labels), _np(result.score), _np(result.n_hyps)
    lm_score = None if result.lm_score is None else _np(result.lm_score)
    boost_score = None if result.boost_score is None else _np(result.boost_score)
    vocab = list(vocabulary)
    out = []
    for b in range(labels.shape[0]):
        hyps = []
        for h in range(int(n_hyps[b])):
            ids = labels[b, h, :int(n_labels[b, h])].tolist()
            hyp = Hypothesis(''.join(vocab[i] for i in ids), ids, [], [], None, float(score[b, h]) / ONE, [])
            if lm_score is not None:
                hyp.lm_score = float(lm_score[b, h]) / ONE
            if boost_score is not None:
                hyp.boost_score = float(boost_score[b, h]) / ONE
            hyps.append(hyp)
        out.append(hyps)
    return out
