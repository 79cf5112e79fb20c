"""Keyword spotting over CTC log-probabilities in fixed point: the host statement of k_spot (csrc/qasr_spot.hip, include/qasr.h)
and the step from its outputs to keyword hits with times and scores.  NumPy only: no GPU, no native library.

`spot_host` is the CPU path of EncDecCTCModel.spot / spot_long and the yardstick the GPU tests compare k_spot with, byte for
byte.  quantize, NEG and the float order `_order_key` are those of qasr.beam and are not restated; the lattice step (states,
predecessors, skip condition, tie order) is RULES of qasr.align; the filler score is the plane of qasr.align.star_host with
penalty 0."""
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .align import BAND_MAX_FRAMES
from .beam import NEG, ONE, _order_key, quantize  # noqa: F401  (_order_key: star_host's maximum, the order the plane is taken in)

MAX_LABELS = 127                        # QASR_SPOT_MAX_LABELS
MAX_SPAN = 65536                        # QASR_SPOT_MAX_SPAN
MIN_THRESHOLD = -16.0                   # nats per frame; QASR_SPOT_MIN_THRESHOLD_Q / 2^16

SPOT_RULES = """Where each of K keywords occurs in each of B utterances, and how well it matches: the keyword's CTC lattice with a free start
and a free end, scored by the likelihood ratio against the frame's best class.
Problems: keywords k < K are shared by all utterances (targets int32 [K, ML], target_lens int32 [K]); problem p = u * K + k.
Frames run t < lim = min(max(lens[u], 0), T) (lens None: T), T <= BAND_MAX_FRAMES = 2^22.  There is no workspace, so nothing ties
this to MAX_T.
States are RULES's (qasr.align): s = 1 .. 2L - 1, lab(s) = y[(s - 1) / 2] for odd s and blank for even s.  State 0 is not a blank
state here: it is the constant fresh start, value 0 with start frame = the frame being entered.  A leading blank can never beat
it, so it is not computed.
Emission: e(t, s) = min(quantize(logp[u][t][lab(s)]) - quantize(star[u][t]), 0) in int64, <= 0: the likelihood ratio against the
frame's best class.  star is the float32 plane [B, star_pitch] of star_host(log_probs, lens, 0.0); any plane is taken as given.
One Viterbi row of pairs (D int64, start int32).  Frame 0: state 1 = (e(0, 1), 0); every other state is dead (NEG, -1).  Frames
t >= 1: the predecessors of s are stay (s), s - 1 and s - 2 (s - 2 only if s is odd, s >= 3 and y[(s - 1) / 2] != y[(s - 3) / 2]);
for s = 1 the s - 1 predecessor is the fresh start (0, t).  The tie order is RULES's: stay first, then s - 1, then s - 2, each
replacing only on strict >.  The winner's start travels with its score; D' = winner + e(t, s); a state whose predecessors are
all dead stays dead.  Nothing is added to NEG.  (Frame 0 is the same step taken from a row of dead states.)
Candidate at frame t: the final state is F = 2L - 1 only (a trailing blank adds <= 0).  With n = t - start + 1, a live F is a
candidate when n <= max_span and D >= threshold_q * n.  threshold_q is int32 fixed point (nats per frame * 2^16) in
-16 * 2^16 .. 0 and max_span is in 1 .. 65536, so every product here and below fits in int64.
Hits: one greedy pass in time order with one open hit per problem.  A candidate that overlaps the open hit (start_t <= open.end)
replaces it iff its mean is strictly higher, D_t * n_open > D_open * n_t; otherwise the candidate is dropped.  A candidate that
does not overlap closes the open hit, which is emitted, and opens a new one.  The end of the row closes the last hit.
n_hits[p] counts every emitted hit; the first max_hits of them are stored, in time order, as hit_start, hit_end (inclusive
frames) and hit_score (D, int64); rows behind them are 0.
Validity: ok[p] = 0, with no hits (and a trace row of 0), for L < 1, L > ML, L > MAX_LABELS = 127, a label outside [0, C) or a
label equal to blank.  lim == 0 gives ok = 1 and no hits.
Optional trace: trace_score int64 and trace_start int32 [P, trace_pitch] hold (D, start) of F at every t < lim - a dead F is
NEG / -1 - and 0 for lim <= t < T."""


@dataclass
class SpotResult:
    """Outputs of SPOT_RULES (arrays: NumPy on the host, torch tensors from the device binding), P = B * K rows, problem
    p = u * K + k: hit_start / hit_end int32 [P, max_hits] (inclusive frames), hit_score int64 [P, max_hits] (D: / 2^16 / frames =
    nats per frame), n_hits int32 [P] (every emitted hit, stored or not), ok int32 [P]; trace_score int64 / trace_start int32
    [P, T] or None."""
    hit_start: object
    hit_end: object
    hit_score: object
    n_hits: object
    ok: object
    trace_score: object = None
    trace_start: object = None
    n_keywords: int = 1


def check_threshold(threshold, who) -> int:
    """threshold (nats per frame) as int32 fixed point; refused by name unless finite and in MIN_THRESHOLD .. 0"""
    try:
        x = float(threshold)
    except (TypeError, ValueError):
        x = float('nan')
    if not MIN_THRESHOLD <= x <= 0.0:                               # (NaN and the infinities fail the comparison too)
        raise ValueError(f'{who}: threshold must be a finite number of nats per frame in {MIN_THRESHOLD:g} .. 0, got {threshold!r}')
    return int(np.rint(x * ONE))


def check_max_span(max_span, who) -> int:
    n = int(max_span)
    if not 1 <= n <= MAX_SPAN:
        raise ValueError(f'{who}: max_span must be 1 .. {MAX_SPAN} frames, got {max_span!r}')
    return n


def _greedy_hits(d, st, thr, max_span):
    """the hit rule of SPOT_RULES over one problem's trace (d int64 [lim], st int32 [lim]): the emitted (start, end, D), in order"""
    t = np.arange(len(d), dtype=np.int64)
    n = t - st.astype(np.int64) + 1
    cand = np.flatnonzero((d != NEG) & (n <= max_span) & (d >= np.int64(thr) * n))
    hits, cur = [], None
    for i in cand:
        c = (int(st[i]), int(i), int(d[i]))
        if cur is not None and c[0] <= cur[1]:
            if c[2] * (cur[1] - cur[0] + 1) > cur[2] * (c[1] - c[0] + 1):
                cur = c
        else:
            if cur is not None:
                hits.append(cur)
            cur = c
    if cur is not None:
        hits.append(cur)
    return hits


def _spot_utt(lp, st_row, lim, ys, blank):
    """the Viterbi rows of SPOT_RULES for one utterance and its valid keywords ys (lists of labels) over lp float32 [T, C] and
    the plane row st_row [T]: (D int64 [n, lim], start int32 [n, lim]) of every keyword's final state"""
    n = len(ys)
    i64 = np.int64
    S = 2 * max(len(y) for y in ys)                                 # states 0 .. S - 1; a keyword's own are 1 .. 2L - 1
    lab = np.full((n, S), blank, dtype=np.int64)
    skip = np.zeros((n, S), dtype=bool)
    fin = np.empty(n, dtype=np.int64)
    for j, y in enumerate(ys):
        L = len(y)
        ya = np.asarray(y, dtype=np.int64)
        lab[j, 1:2 * L:2] = ya
        if L > 1:
            skip[j, 3:2 * L:2] = ya[1:] != ya[:-1]
        fin[j] = 2 * L - 1
    rows = np.arange(n)
    qs = quantize(st_row[:lim]).astype(i64)
    D = np.full((n, S), NEG, i64)                                   # (states above a keyword's F run too; nothing reads them)
    B = np.full((n, S), -1, np.int32)
    out_d = np.empty((n, lim), i64)
    out_s = np.empty((n, lim), np.int32)
    neg1, neg2 = np.full((n, 1), NEG, i64), np.full((n, 2), NEG, i64)
    m1, m2 = np.full((n, 1), -1, np.int32), np.full((n, 2), -1, np.int32)
    for t in range(lim):
        e = np.minimum(quantize(lp[t][lab]).astype(i64) - qs[t], 0)
        a1, s1 = np.concatenate([neg1, D[:, :-1]], axis=1), np.concatenate([m1, B[:, :-1]], axis=1)
        a1[:, 1], s1[:, 1] = 0, t                                   # the fresh start
        a2 = np.where(skip, np.concatenate([neg2, D[:, :-2]], axis=1), NEG)
        s2 = np.concatenate([m2, B[:, :-2]], axis=1)
        best, bs = D, B
        m = a1 > best
        best, bs = np.where(m, a1, best), np.where(m, s1, bs)
        m = a2 > best
        best, bs = np.where(m, a2, best), np.where(m, s2, bs)
        live = best != NEG
        live[:, 0] = False                                          # state 0 is not computed
        D = np.where(live, np.where(live, best, 0) + e, NEG)
        B = np.where(live, bs, -1).astype(np.int32)
        out_d[:, t], out_s[:, t] = D[rows, fin], B[rows, fin]
    return out_d, out_s


def spot_host(log_probs, lens, star, targets, target_lens, blank, threshold_q, max_span, max_hits, want_trace=False) -> SpotResult:
    """SPOT_RULES on the host: the NumPy twin of k_spot.  log_probs float32 [B, T, C]; lens int [B] or None; star float32 [B, T]
    (star_host(log_probs, lens, 0.0)); targets int32 [K, ML] and target_lens int32 [K]; blank: the blank id; threshold_q: int,
    nats per frame * 2^16, -16 * 2^16 .. 0; max_span: frames, 1 .. 65536; max_hits >= 1: the row pitch of the hit outputs."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'spot_host: log_probs must be [B, T, C] with B, T, C >= 1, got {lp.shape}')
    B, T, C = lp.shape
    if T > BAND_MAX_FRAMES:
        raise ValueError(f'spot_host: at most {BAND_MAX_FRAMES} frames, got {T}')
    if star is None:
        raise ValueError('spot_host: star is required (star_host(log_probs, lens, 0.0))')
    st = np.asarray(star, dtype=np.float32)
    if st.shape != (B, T):
        raise ValueError(f'spot_host: star must be a float32 plane [{B}, {T}], got {st.shape}')
    tg = np.asarray(targets)
    tl = np.asarray(target_lens)
    if tg.ndim != 2 or tg.shape[0] < 1 or tl.shape != (tg.shape[0],):
        raise ValueError(f'spot_host: targets must be [K, max_labels] with K >= 1 and one length each, got {tg.shape} / {tl.shape}')
    K, ML = tg.shape
    if not 1 <= ML <= MAX_LABELS:
        raise ValueError(f'spot_host: max_labels (the row pitch of targets) must be 1 .. {MAX_LABELS}, got {ML}')
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f'spot_host: blank {blank} is outside [0, {C})')
    thr = int(threshold_q)
    if not -16 * ONE <= thr <= 0:
        raise ValueError(f'spot_host: threshold_q must be {-16 * ONE} .. 0, got {threshold_q!r}')
    max_span = check_max_span(max_span, 'spot_host')
    MH = int(max_hits)
    if MH < 1:
        raise ValueError(f'spot_host: max_hits must be at least 1, got {max_hits!r}')
    tg = tg.astype(np.int32)
    P = B * K
    hit_start = np.zeros((P, MH), dtype=np.int32)
    hit_end = np.zeros((P, MH), dtype=np.int32)
    hit_score = np.zeros((P, MH), dtype=np.int64)
    n_hits = np.zeros(P, dtype=np.int32)
    ok = np.zeros(P, dtype=np.int32)
    trace_score = np.zeros((P, T), dtype=np.int64) if want_trace else None
    trace_start = np.zeros((P, T), dtype=np.int32) if want_trace else None
    good = []
    for k in range(K):
        L = int(tl[k])
        if L < 1 or L > ML or L > MAX_LABELS:
            continue
        y = tg[k, :L]
        if y.min() < 0 or y.max() >= C or (y == blank).any():
            continue
        good.append(k)
    for u in range(B):
        lim = T if lens is None else int(min(max(int(lens[u]), 0), T))
        for k in good:
            ok[u * K + k] = 1
        if lim == 0 or not good:
            continue
        d, s = _spot_utt(lp[u], st[u], lim, [tg[k, :int(tl[k])] for k in good], blank)
        for j, k in enumerate(good):
            p = u * K + k
            if want_trace:
                trace_score[p, :lim], trace_start[p, :lim] = d[j], s[j]
            hits = _greedy_hits(d[j], s[j], thr, max_span)
            n_hits[p] = len(hits)
            for i, (a, b, sc) in enumerate(hits[:MH]):
                hit_start[p, i], hit_end[p, i], hit_score[p, i] = a, b, sc
    return SpotResult(hit_start, hit_end, hit_score, n_hits, ok, trace_score, trace_start, K)


def _np(x):
    if x is None:
        return None
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def to_hits(result: SpotResult, keywords: Sequence, seconds_per_frame: float) -> List[list]:
    """One list of qasr.ctc.KeywordHit per utterance, sorted by start (ties: by keyword index): keyword = keywords[k] (the
    string, or the label ids, as given), index = k, start_s = the first frame's start and end_s = the last frame's end in
    seconds, frames = n, score = D / 2^16 / n in nats per frame, <= 0 (0: the keyword is the greedy path over its span).  Only
    the stored hits (the first max_hits of a problem) are listed."""
    from .ctc import KeywordHit
    hs, he, sc, nh = _np(result.hit_start), _np(result.hit_end), _np(result.hit_score), _np(result.n_hits)
    K = int(result.n_keywords)
    if len(keywords) != K or hs.shape[0] % K:
        raise ValueError(f'to_hits: {len(keywords)} keywords for a result of {K} per utterance and {hs.shape[0]} rows')
    spf = float(seconds_per_frame)
    out = []
    for u in range(hs.shape[0] // K):
        hits = []
        for k in range(K):
            p = u * K + k
            for i in range(min(int(nh[p]), hs.shape[1])):
                a, b = int(hs[p, i]), int(he[p, i])
                n = b - a + 1
                hits.append(KeywordHit(keywords[k], k, a * spf, (b + 1) * spf, float(sc[p, i]) / ONE / n, n))
        hits.sort(key=lambda h: (h.start_s, h.index))
        out.append(hits)
    return out
