"""CTC forced alignment and transcript scoring in fixed point: the host statement of k_align (csrc/qasr_align.hip,
include/qasr.h) and the step from its outputs to strings, label times and word times.  NumPy only: no GPU, no native library.

`align_host` is the CPU path of EncDecCTCModel.align / decode(beam_width=, timestamps=True) and the yardstick the GPU tests
compare k_align with, byte for byte.  The arithmetic (quantize, lae, its table, NEG) is that of qasr.beam and is not restated.

RULES.  A problem p is a pair (utterance u = p // K, target y[0 .. L)), K = problems per utterance.  Frames run t < lim,
lim = min(max(lens[u], 0), T) (lens None: T).  States run s = 0 .. 2L; lab(s) = blank for even s and y[(s - 1) / 2] for odd s;
q(t, s) = quantize(logp[u][t][lab(s)]).  Two int64 rows V (Viterbi) and A (forward) are NEG except V[0] = A[0] = q(0, 0) and,
if L > 0, V[1] = A[1] = q(0, 1).  For t >= 1 the predecessors of s are s, s - 1 (s >= 1) and s - 2 (only if s is odd, s >= 3
and y[(s - 1) / 2] != y[(s - 3) / 2]); a missing predecessor is NEG.
  Viterbi: best = the maximum of the three; ties keep the smaller step (stay, then s - 1, then s - 2, each replacing only on
    strict >).  V'[s] = NEG if best == NEG, else best + q(t, s); the backpointer is the step 0, 1 or 2.
  Forward: x = lae(lae(A[s], A[s - 1]), A[s - 2]) in exactly this order (lae is not associative); A'[s] = NEG if x == NEG, else
    x + q(t, s).  Nothing is ever added to NEG.
End: the final state is 2L if V[2L] > V[2L - 1], else 2L - 1 (L == 0: state 0); path_score = V[final];
total = lae(A[2L], A[2L - 1]) (L == 0: A[0]).  The backpointers are walked from t = lim - 1 down.  For label i, start[i] is the
first frame whose state is 2i + 1 and nframes[i] the number of such frames (one run: the path is monotone); score[i] is the
maximum of the float32 logp[u][t][y[i]] over those frames in the `_order_key` order (exact; k_ctc's rule).
Not alignable (ok[p] = 0; start, nframes and score rows zero; path_score = total = NEG): V[final] == NEG (fewer frames than
labels plus adjacent repeats); lim == 0 with L > 0; L < 0, L above the row pitch or above MAX_LABELS; a label outside [0, C)
or equal to blank.  lim == 0 with L == 0 is ok = 1 with both scores 0.

Long recordings (a whole transcript against a whole recording, past MAX_LABELS and MAX_T) are aligned inside a band of lattice
states that follows the path: BAND_RULES, `align_band_host` (the host statement of k_align_band, csrc/qasr_align_band.hip) and
`segment_scores` at the end of this module; they are the CPU path of EncDecCTCModel.align_long.

Audio the transcript does not cover is given a wildcard label whose emission is a per-frame plane: STAR_RULES, `star_host` (the
host statement of k_star, csrc/qasr_star.hip) and the `star=` argument of both twins.

How sure an alignment is - the posterior of the path's own state at every frame, by a backward pass over the same lattice:
POST_RULES, `post_host` (the host statement of k_post, csrc/qasr_post.hip) and `post_to_hypotheses`; for long recordings the
same inside the band of the banded alignment: POST_BAND_RULES and `post_band_host` (the host statement of k_post_band,
csrc/qasr_post_band.hip), the CPU path of EncDecCTCModel.align_long(posteriors=True)."""
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .beam import MAX_T, NEG, ONE, Q_FLOOR, _order_key, lae, lae_table, quantize

MAX_LABELS = 2048                       # QASR_ALIGN_MAX_LABELS
STAR_MAX_PENALTY = 16.0                 # nats per frame; qasr_ctc_star refuses more

STAR_RULES = """The wildcard ("star") is one more label, id C (one past the last class), whose emission does not come from the matrix but
from a float32 plane star [B, T]: wherever RULES or BAND_RULES read logp[u][t][c], c == C reads star[u][t] - the quantised
emission q, the per-label score and frame_logp alike.  Nothing else changes: the wildcard differs from every real label, so it
may skip the blank below it; two adjacent wildcards are a repeat and need the blank between them; a wildcard takes at least
one frame.  Without a plane, id C is a label outside [0, C) and the problem is not alignable (ok = 0).
Hence, for any inputs, every output (start, nframes, score, path_score, total, ok, frame_logp, band_base) equals on every byte
the output of the same function, called without a plane, on np.concatenate([log_probs, star[..., None]], axis=2) with C + 1
classes.  total with a wildcard in the target follows the same rule; it is a score, not a likelihood.
The plane of star_host: star[u][t] = max over c < C of logp[u][t][c] (the float32 maximum in the `_order_key` order, k_ctc's
and k_align's) minus float32(penalty), one IEEE float32 subtraction, for t < lim; 0 for t >= lim.  penalty is finite, in
0 .. STAR_MAX_PENALTY nats.  A row of all -inf gives -inf, which quantize takes to its floor."""


@dataclass
class AlignResult:
    """Outputs of one alignment, row pitch max_labels (arrays: NumPy on the host, torch tensors from the device binding).
    labels [P, max_labels] int32 and n_labels [P] int32 are the targets as given; start / nframes [P, max_labels] int32 and
    score [P, max_labels] float32 (tails 0) have the meaning of qasr.ctc.CtcResult's; path_score / total [P] int64 fixed
    point (/ 2^16 = nats: the best alignment's and the CTC log-likelihood; total None when not requested); ok [P] int32."""
    labels: object
    n_labels: object
    start: object = None
    nframes: object = None
    score: object = None
    path_score: object = None
    total: object = None
    ok: object = None
    blank: int = -1
    problems_per_utt: int = 1


def star_host(log_probs, lens, penalty) -> np.ndarray:
    """The wildcard's emission plane of STAR_RULES: log_probs float32 [B, T, C]; lens int [B] or None; penalty: nats per frame,
    finite, 0 .. STAR_MAX_PENALTY.  Returns float32 [B, T]."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'star_host: log_probs must be [B, T, C] with B, T, C >= 1, got {lp.shape}')
    pen = check_star_penalty(penalty, 'star_host')
    B, T, _ = lp.shape
    best = _order_key(lp).max(axis=2)
    out = (best ^ ((best >> 31) & np.int32(0x7fffffff))).view(np.float32) - pen      # float32 - float32: one subtraction
    if lens is not None:
        lim = np.clip(np.asarray(lens, dtype=np.int64).reshape(B), 0, T)
        out[np.arange(T)[None, :] >= lim[:, None]] = 0
    return out


def check_star_penalty(penalty, who) -> np.float32:
    """penalty as float32; refused by name unless finite and in 0 .. STAR_MAX_PENALTY"""
    try:
        pen = float(penalty)
    except (TypeError, ValueError):
        pen = float('nan')
    if not 0.0 <= pen <= STAR_MAX_PENALTY:                          # (NaN and the infinities fail the comparison too)
        raise ValueError(f'{who}: penalty must be a finite number of nats in 0 .. {STAR_MAX_PENALTY:g}, got {penalty!r}')
    return np.float32(pen)


def _star_plane(star, B, T, who):
    if star is None:
        return None
    st = np.asarray(star, dtype=np.float32)
    if st.shape != (B, T):
        raise ValueError(f'{who}: star must be a float32 plane [{B}, {T}], got {st.shape}')
    return st


def _emit(lp, st, t, c):
    """lp[t, c] (index arrays that broadcast), the wildcard id lp.shape[1] reading the plane row st[t] (STAR_RULES)"""
    if st is None:
        return lp[t, c]
    wild = c == lp.shape[1]
    return np.where(wild, st[t], lp[t, np.where(wild, 0, c)])


def _label_runs(states, lp, y, st=None):
    """per label of y its first frame, frame count and best frame log-probability along the path `states` [lim]"""
    L = len(y)
    start = np.zeros(L, dtype=np.int32)
    nframes = np.zeros(L, dtype=np.int32)
    score = np.zeros(L, dtype=np.float32)
    fr = np.flatnonzero(states & 1)                                 # the label frames, in time (= label) order
    if L:
        idx = states[fr] >> 1
        first_of = np.flatnonzero(np.concatenate([[True], idx[1:] != idx[:-1]]))
        start[idx[first_of]] = fr[first_of]
        nframes[idx[first_of]] = np.diff(np.concatenate([first_of, [len(fr)]]))
        best = np.maximum.reduceat(_order_key(_emit(lp, st, fr, np.asarray(y, dtype=np.int64)[idx])), first_of)
        score[idx[first_of]] = (best ^ ((best >> 31) & np.int32(0x7fffffff))).view(np.float32)
    return start, nframes, score


def _align_one(lp, lim, y, blank, tab, want_total, st=None):
    """one problem with a valid target y (L >= 0) over lp float32 [T, C] (st: the wildcard's plane row [T] or None); returns
    (ok, start, nframes, score, path, total)"""
    L = len(y)
    i64 = np.int64
    if lim == 0:
        return (1, None, None, None, 0, 0) if L == 0 else (0, None, None, None, NEG, NEG)
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = y[1:] != y[:-1]
    q = quantize(_emit(lp, st, np.arange(lim)[:, None], lab[None, :]))             # int32 [lim, S]
    negs = np.full(2, NEG, i64)

    def first():
        r = np.full(S, NEG, i64)
        r[:min(2, S)] = q[0, :min(2, S)]
        return r

    V = first()
    bp = np.zeros((lim, S), dtype=np.uint8)
    for t in range(1, lim):
        ext = np.concatenate([negs, V])
        a1, a2 = ext[1:S + 1], np.where(skip, ext[:S], NEG)
        best, step = V, np.zeros(S, dtype=np.uint8)
        m = a1 > best
        best, step = np.where(m, a1, best), np.where(m, 1, step)
        m = a2 > best
        best, step = np.where(m, a2, best), np.where(m, 2, step)
        live = best != NEG
        V = np.where(live, np.where(live, best, 0) + q[t].astype(i64), NEG)
        bp[t] = step
    fin = 0 if L == 0 else (2 * L if V[2 * L] > V[2 * L - 1] else 2 * L - 1)
    path_score = int(V[fin])
    if path_score == NEG:
        return 0, None, None, None, NEG, NEG
    total = NEG
    if want_total:
        A = first()
        for t in range(1, lim):
            ext = np.concatenate([negs, A])
            x = lae(lae(A, ext[1:S + 1], tab), np.where(skip, ext[:S], NEG), tab)
            live = x != NEG
            A = np.where(live, np.where(live, x, 0) + q[t].astype(i64), NEG)
        total = int(A[0]) if L == 0 else int(lae(A[2 * L], A[2 * L - 1], tab))
    states = np.empty(lim, dtype=np.int64)
    s = fin
    for t in range(lim - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    start, nframes, score = _label_runs(states, lp, y, st)
    return 1, start, nframes, score, path_score, total


def align_host(log_probs, lens, targets, target_lens, blank, problems_per_utt=1, want_total=True, star=None) -> AlignResult:
    """log_probs float32 [B, T, C]; lens int [B] or None; targets int32 [P, max_labels] and target_lens int32 [P] with
    P = B * problems_per_utt (problem p belongs to utterance p // problems_per_utt); blank: the blank id.  The RULES of the
    module docstring; want_total=False skips the forward pass (total None).  star: a float32 plane [B, T] that makes id C the
    wildcard label (STAR_RULES); None: id C is a label outside [0, C)."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'align_host: log_probs must be [B, T, C] with B, T, C >= 1, got {lp.shape}')
    B, T, C = lp.shape
    K = int(problems_per_utt)
    tg = np.asarray(targets)
    tl = np.asarray(target_lens)
    if K < 1 or tg.ndim != 2 or tg.shape[0] != B * K or tl.shape != (B * K,):
        raise ValueError(f'align_host: targets must be [B * problems_per_utt, max_labels] with one length each, got '
                         f'{tg.shape} / {tl.shape} for B {B}, problems_per_utt {K}')
    P, ML = tg.shape
    if not 1 <= ML <= MAX_LABELS:
        raise ValueError(f'align_host: max_labels (the row pitch of targets) must be 1 .. {MAX_LABELS}, got {ML}')
    if T > MAX_T:
        raise ValueError(f'align_host: at most {MAX_T} frames, got {T}')
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f'align_host: blank {blank} is outside [0, {C})')
    tg = tg.astype(np.int32)
    star = _star_plane(star, B, T, 'align_host')
    n_ids = C + (star is not None)
    tab = lae_table()
    start = np.zeros((P, ML), dtype=np.int32)
    nframes = np.zeros((P, ML), dtype=np.int32)
    score = np.zeros((P, ML), dtype=np.float32)
    path_score = np.full(P, NEG, dtype=np.int64)
    total = np.full(P, NEG, dtype=np.int64)
    ok = np.zeros(P, dtype=np.int32)
    for p in range(P):
        u = p // K
        lim = T if lens is None else int(min(max(int(lens[u]), 0), T))
        L = int(tl[p])
        if L < 0 or L > ML:
            continue
        y = tg[p, :L]
        if L and (y.min() < 0 or y.max() >= n_ids or (y == blank).any()):
            continue
        ok[p], st, nf, sc, ps, tot = _align_one(lp[u], lim, y, blank, tab, want_total, None if star is None else star[u])
        if ok[p]:
            path_score[p], total[p] = ps, tot
            if st is not None:
                start[p, :L], nframes[p, :L], score[p, :L] = st, nf, sc
    return AlignResult(tg, tl.astype(np.int32), start, nframes, score, path_score, total if want_total else None, ok, blank, K)


def _np(x):
    if x is None:
        return None
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _words_with_star(h, vocab, wild):
    """the word groups of qasr.ctc.to_hypotheses with the wildcard a word of its own, whether or not the vocabulary has ' '"""
    chars = [vocab[c] for c in h.labels]
    words, group = [], []

    def close():
        if group:
            words.append((''.join(chars[k] for k in group), h.start_s[group[0]], h.end_s[group[-1]], min(h.score[k] for k in group)))
            group.clear()
    for k, c in enumerate(h.labels):
        if c == wild:
            close()
            group.append(k)
            close()
        elif chars[k] == ' ':
            close()
        else:
            group.append(k)
    close()
    return words


def to_hypotheses(result: AlignResult, vocabulary: Sequence[str], seconds_per_frame: float, star_token=None) -> List:
    """One qasr.ctc.Hypothesis per problem, through qasr.ctc.to_hypotheses (the code greedy decoding uses, so label and word
    times mean the same): text and labels are the target's, start_s / end_s / score / words come from the best alignment,
    utt_score = path_score / 2^16 and ctc_score = total / 2^16 (None when total was not requested).  A problem that is not
    alignable (ok == 0) has empty time lists, score None and utt_score = ctc_score = -inf.
    star_token: the string of the wildcard label len(vocabulary) + 1 (STAR_RULES); it stands in text at its positions and is a
    word of its own, and a transcript that holds it has ctc_score None."""
    from . import ctc as qctc
    labels, n_labels, ok = _np(result.labels), _np(result.n_labels), _np(result.ok)
    path, total = _np(result.path_score), _np(result.total)
    n = np.clip(n_labels, 0, labels.shape[1]).astype(np.int32)
    view = qctc.CtcResult(labels, np.where(ok != 0, n, 0).astype(np.int32), _np(result.start), _np(result.nframes),
                          _np(result.score), None, result.blank)
    vocab = list(vocabulary)
    wild = len(vocab) + 1 if star_token is not None else None        # (blank = len(vocab) sits between: it never occurs in a target)
    if wild is not None:
        vocab += ['', star_token]
    hyps = qctc.to_hypotheses(view, vocab, seconds_per_frame)
    for p, h in enumerate(hyps):
        if ok[p]:
            h.utt_score = float(path[p]) / ONE
            h.ctc_score = None if total is None else float(total[p]) / ONE
            if wild is not None and wild in h.labels:
                h.ctc_score = None                                      # total is a score there, not a likelihood (STAR_RULES)
                h.words = _words_with_star(h, vocab, wild)
        else:
            ids = [int(i) for i in labels[p, :n[p]]]
            text = ''.join(vocab[i] if 0 <= i < len(vocab) else '' for i in ids)
            hyps[p] = qctc.Hypothesis(text, ids, [], [], None, float('-inf'), [], None, float('-inf'))
    return hyps


# ---- banded alignment of one long recording against its whole transcript (k_align_band, csrc/qasr_align_band.hip)
BAND_MAX_LABELS = 1 << 20               # QASR_BAND_MAX_LABELS
BAND_MAX_FRAMES = 1 << 22               # QASR_BAND_MAX_FRAMES
BAND_STATES = (256, 1024, 4352)         # k_align's 256 threads x NS = 1, 4, 17
BAND_BLOCK = 32                         # frames between two looks at where the band should be
SEGMENT_WINDOW = 30                     # frames of one mean in segment_scores

BAND_RULES = """Everything of RULES (the module docstring) holds - states, predecessors, tie order, q = rint(logp * 2^16), int64 sums, NEG,
end states, per-label start / nframes / score - with these changes.
One problem per recording: K = 1, problem p aligns targets[p] against log_probs[p]; L <= BAND_MAX_LABELS, T <= BAND_MAX_FRAMES.
Viterbi only: no forward pass, no total, no table.
The band: BW in BAND_STATES; S = 2L + 1, top = max(0, S - BW); the band is the states [base, min(base + BW, S)), base = 0 at
t = 0.  At every frame t >= 1 with t % 32 == 0, before that frame's update: m = the lowest in-band state whose V (after frame
t - 1) is the band's maximum; if that maximum is NEG the base stays, otherwise base <- max(base, min(m - BW / 2, top)).  States
below the new base are dropped; states that enter are NEG.  The base never decreases.
A predecessor below base is NEG; states outside the band are NEG and have no backpointer; the final state (2L or 2L - 1 as in
RULES, an out-of-band one counting as NEG) must be in the last frame's band.
ok = 0 for the reasons of RULES (L above BAND_MAX_LABELS in place of MAX_LABELS), or when V[final] == NEG because the band lost
the path; start, nframes, score and frame_logp rows are then zero and path_score = NEG.
When S <= BW the base never moves and start, nframes, score, path_score and ok equal align_host(want_total=False) on every byte.
frame_logp float32 [P, T]: the float32 log-probability of the path's state's label at each frame < lim, 0 behind and 0 when
ok = 0.  band_base int32 [P, ceil(T / 32)]: the base in force during each 32-frame block that has a frame < lim, 0 behind; it is
kept when the path was lost (that is where to look), and is 0 for a problem whose lattice never ran (a bad target, lim == 0)."""


@dataclass
class BandResult(AlignResult):
    """AlignResult (total None, problems_per_utt 1) plus frame_logp float32 [P, T] and band_base int32 [P, ceil(T / 32)]
    (None when not requested) of BAND_RULES; band_states is the width used."""
    frame_logp: object = None
    band_base: object = None
    band_states: int = 0


def pick_band_states(n_labels, band_states=None) -> int:
    """band_states as given (refused by name unless one of BAND_STATES); None: the smallest width that holds all
    2 * n_labels + 1 states, else the widest"""
    if band_states is None:
        S = 2 * int(n_labels) + 1
        return next((b for b in BAND_STATES if S <= b), BAND_STATES[-1])
    if int(band_states) not in BAND_STATES:
        raise ValueError(f'band_states must be one of {BAND_STATES}, got {band_states}')
    return int(band_states)


def _align_band_one(lp, lim, y, blank, BW, st=None):
    """one problem with a valid target y over lp float32 [T, C] (st: the wildcard's plane row [T] or None): (ok, start, nframes,
    score, path, frame_logp [lim], bases)"""
    L = len(y)
    i64 = np.int64
    nb_blocks = (lim + BAND_BLOCK - 1) // BAND_BLOCK
    bases = np.zeros(nb_blocks, dtype=np.int32)
    if lim == 0:
        return (1, None, None, None, 0, None, bases) if L == 0 else (0, None, None, None, NEG, None, bases)
    S = 2 * L + 1
    top = max(0, S - BW)
    n = min(BW, S)                                                  # states in the band (constant: base <= top)
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = y[1:] != y[:-1]
    negs = np.full(2, NEG, i64)
    base = 0
    V = np.full(n, NEG, i64)                                        # V[i]: state base + i
    V[:min(2, S)] = quantize(_emit(lp, st, 0, lab[:min(2, S)]))
    bp = np.zeros((lim, n), dtype=np.uint8)                         # bp[t, i]: state bases[t // 32] + i
    for t in range(1, lim):
        if t % BAND_BLOCK == 0:
            if V.max() != NEG:
                m = base + int(np.argmax(V))                        # the first maximum: the lowest state
                new = max(base, min(m - BW // 2, top))
                if new > base:
                    V = np.concatenate([V[new - base:], np.full(new - base, NEG, i64)])
                    base = new
            bases[t // BAND_BLOCK] = base
        sl = slice(base, base + n)
        q = quantize(_emit(lp, st, t, lab[sl])).astype(i64)
        ext = np.concatenate([negs, V])                             # what lies below base is NEG
        a1, a2 = ext[1:n + 1], np.where(skip[sl], ext[:n], NEG)
        best, step = V, np.zeros(n, dtype=np.uint8)
        m1 = a1 > best
        best, step = np.where(m1, a1, best), np.where(m1, 1, step)
        m2 = a2 > best
        best, step = np.where(m2, a2, best), np.where(m2, 2, step)
        live = best != NEG
        V = np.where(live, np.where(live, best, 0) + q, NEG)
        bp[t] = step

    def at(s):
        return int(V[s - base]) if base <= s < base + n else NEG
    fin = 0 if L == 0 else (2 * L if at(2 * L) > at(2 * L - 1) else 2 * L - 1)
    path_score = at(fin)
    if path_score == NEG:
        return 0, None, None, None, NEG, None, bases
    states = np.empty(lim, dtype=np.int64)
    s = fin
    for t in range(lim - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s - int(bases[t // BAND_BLOCK])])
    start, nframes, score = _label_runs(states, lp, y, st)
    return 1, start, nframes, score, path_score, _emit(lp, st, np.arange(lim), lab[states]), bases


def align_band_host(log_probs, lens, targets, target_lens, blank, band_states=None, want_band_base=True, star=None) -> BandResult:
    """BAND_RULES on the host.  log_probs float32 [P, T, C]; lens int [P] or None; targets int32 [P, max_labels] and
    target_lens int32 [P]; blank: the blank id; band_states: one of BAND_STATES (None: pick_band_states of the row pitch);
    star: a float32 plane [P, T] that makes id C the wildcard label (STAR_RULES)."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'align_band_host: log_probs must be [P, T, C] with P, T, C >= 1, got {lp.shape}')
    P, T, C = lp.shape
    tg = np.asarray(targets)
    tl = np.asarray(target_lens)
    if tg.ndim != 2 or tg.shape[0] != P or tl.shape != (P,):
        raise ValueError(f'align_band_host: targets must be [P, max_labels] with one length each, got {tg.shape} / {tl.shape} '
                         f'for P {P}')
    ML = tg.shape[1]
    if not 1 <= ML <= BAND_MAX_LABELS:
        raise ValueError(f'align_band_host: max_labels (the row pitch of targets) must be 1 .. {BAND_MAX_LABELS}, got {ML}')
    if T > BAND_MAX_FRAMES:
        raise ValueError(f'align_band_host: at most {BAND_MAX_FRAMES} frames, got {T}')
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f'align_band_host: blank {blank} is outside [0, {C})')
    BW = pick_band_states(ML, band_states)
    tg = tg.astype(np.int32)
    star = _star_plane(star, P, T, 'align_band_host')
    n_ids = C + (star is not None)
    start = np.zeros((P, ML), dtype=np.int32)
    nframes = np.zeros((P, ML), dtype=np.int32)
    score = np.zeros((P, ML), dtype=np.float32)
    path_score = np.full(P, NEG, dtype=np.int64)
    ok = np.zeros(P, dtype=np.int32)
    frame_logp = np.zeros((P, T), dtype=np.float32)
    band_base = np.zeros((P, (T + BAND_BLOCK - 1) // BAND_BLOCK), dtype=np.int32)
    for p in range(P):
        lim = T if lens is None else int(min(max(int(lens[p]), 0), T))
        L = int(tl[p])
        if L < 0 or L > ML:
            continue
        y = tg[p, :L]
        if L and (y.min() < 0 or y.max() >= n_ids or (y == blank).any()):
            continue
        ok[p], st, nf, sc, ps, fl, bases = _align_band_one(lp[p], lim, y, blank, BW, None if star is None else star[p])
        band_base[p, :len(bases)] = bases
        if ok[p]:
            path_score[p] = ps
            if st is not None:
                start[p, :L], nframes[p, :L], score[p, :L] = st, nf, sc
                frame_logp[p, :lim] = fl
    return BandResult(tg, tl.astype(np.int32), start, nframes, score, path_score, None, ok, blank, 1, frame_logp,
                      band_base if want_band_base else None, BW)


def segment_scores(frame_logp, f0, f1) -> np.ndarray:
    """Min-mean confidence of segments (Kuerzinger et al., CTC-segmentation): for the frames [f0[i], f1[i]) of frame_logp [T],
    in float64, the mean over all of them when there are at most SEGMENT_WINDOW, else the minimum over t of the mean of
    frame_logp[t : t + SEGMENT_WINDOW] (whole windows inside the segment only).  An empty segment scores -inf."""
    x = np.asarray(frame_logp, dtype=np.float64).reshape(-1)
    f0 = np.atleast_1d(np.asarray(f0, dtype=np.int64))
    f1 = np.atleast_1d(np.asarray(f1, dtype=np.int64))
    out = np.full(len(f0), -np.inf, dtype=np.float64)
    for i, (a, b) in enumerate(zip(f0, f1)):
        a, b = max(int(a), 0), min(int(b), len(x))
        if b - a <= 0:
            continue
        if b - a <= SEGMENT_WINDOW:
            out[i] = x[a:b].mean()
        else:
            out[i] = np.lib.stride_tricks.sliding_window_view(x[a:b], SEGMENT_WINDOW).mean(axis=1).min()
    return out


# ---- posteriors along an alignment: forward-backward over the lattice of RULES (k_post, csrc/qasr_post.hip)
POST_RULES = """How much of the transcript's probability mass agrees with the alignment: the log-posterior of the path's own state at every
frame.  The inputs are align_host's plus the alignment's start, nframes [P, max_labels] and ok [P].
Lattice: states, lab(s), q(t, s), lim, the predecessors and the forward row A are exactly those of RULES; A(t, s) is the forward
row after frame t.
Backward row: Bk(lim - 1, s) = q(lim - 1, s) for s in {2L, 2L - 1} (L == 0: s = 0), NEG elsewhere.  For t < lim - 1 the successors
of s are s, s + 1 (if s + 1 <= 2L) and s + 2 (only if s is odd, s + 2 <= 2L - 1 and y[(s + 1) / 2] != y[(s - 1) / 2]); a missing
successor is NEG.  x = lae(lae(Bk[s], Bk[s + 1]), Bk[s + 2]) in exactly this order; Bk'[s] = NEG if x == NEG, else x + q(t, s).
Nothing is ever added to NEG.
The path comes from start / nframes, not from backpointers: frame t is in state 2i + 1 when start[i] <= t < start[i] + nframes[i],
otherwise in the blank state 2j, j = the number of labels with start[i] <= t.
Validity: start / nframes must describe a CTC alignment of the target over lim frames - runs in order, none empty, a blank frame
between adjacent equal labels, the last run ends by lim.  ok_post[p] = 0 when they do not, when ok[p] == 0, and for a target
align_host refuses (L < 0, L above the row pitch or MAX_LABELS, a label outside [0, C) or equal to blank, lim == 0 with L > 0);
all outputs of such a problem are zero and total = NEG.  start / nframes are only ever compared with frame numbers, never used as
an index.  A valid path has a finite score (q is clamped), so A and Bk along it are never NEG.
Outputs: total int64 [P] = lae(A[2L], A[2L - 1]) at lim - 1 (L == 0: A[0]), align_host's total on every byte.
g(t) = A(t, s_t) + Bk(t, s_t) - q(t, s_t) - total in int64.  frame_post int32 [P, T] = g(t) clamped to [Q_FLOOR, 0] for t < lim
(lae is not exact: g can come out a little above 0), 0 behind lim.  label_post int32 [P, max_labels] = the minimum of frame_post
over the label's run, its least certain frame; tails 0.  ok int32 [P].  lim == 0 with L == 0: ok = 1, total = 0.
Star: id C reads the plane wherever logp[u][t][c] is read (STAR_RULES); every output equals on every byte the call without a
plane on the matrix with the plane appended as class C of C + 1.  total with a wildcard is a score, not a likelihood."""


@dataclass
class PostResult:
    """Outputs of POST_RULES (arrays: NumPy on the host, torch tensors from the device binding): frame_post int32 [P, T] and
    label_post int32 [P, max_labels] fixed-point log-posteriors (/ 2^16 = nats, <= 0), total int64 [P] (None when not
    requested from the device), ok int32 [P]."""
    frame_post: object = None
    label_post: object = None
    total: object = None
    ok: object = None


def _path_ok(start, nframes, y, lim):
    """start / nframes [L] describe a CTC alignment of y over lim frames (the validity of POST_RULES), in Python integers"""
    end = -1
    for i in range(len(y)):
        s, n = int(start[i]), int(nframes[i])
        if n < 1 or s <= end or (i and y[i] == y[i - 1] and s <= end + 1):
            return False
        end = s + n - 1
    return end < lim


def _post_one(lp, lim, y, blank, tab, start, nframes, st=None):
    """one problem with a valid target y and a valid path over lp float32 [T, C]: (total, frame_post int32 [lim], label_post
    int32 [L])"""
    L = len(y)
    i64 = np.int64
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = y[1:] != y[:-1]
    skipb = np.zeros(S, dtype=bool)                                 # s may step to s + 2: s + 2 may come from s
    skipb[:S - 2] = skip[2:]
    q = quantize(_emit(lp, st, np.arange(lim)[:, None], lab[None, :]))             # int32 [lim, S]
    negs = np.full(2, NEG, i64)
    t = np.arange(lim)
    start, nframes = np.asarray(start, dtype=i64), np.asarray(nframes, dtype=i64)
    j = np.searchsorted(start, t, side='right')                     # labels with start <= t (start ascends: the path is valid)
    in_run = (j > 0) & (t < (start + nframes)[np.maximum(j, 1) - 1]) if L else np.zeros(lim, dtype=bool)
    states = np.where(in_run, 2 * j - 1, 2 * j)
    A = np.full(S, NEG, i64)
    A[:min(2, S)] = q[0, :min(2, S)]
    fa = np.empty(lim, dtype=i64)
    fa[0] = A[states[0]]
    for f in range(1, lim):
        ext = np.concatenate([negs, A])
        x = lae(lae(A, ext[1:S + 1], tab), np.where(skip, ext[:S], NEG), tab)
        live = x != NEG
        A = np.where(live, np.where(live, x, 0) + q[f].astype(i64), NEG)
        fa[f] = A[states[f]]
    total = int(A[0]) if L == 0 else int(lae(A[2 * L], A[2 * L - 1], tab))
    Bk = np.full(S, NEG, i64)
    Bk[max(S - 2, 0):] = q[lim - 1, max(S - 2, 0):]
    fb = np.empty(lim, dtype=i64)
    fb[lim - 1] = Bk[states[lim - 1]]
    for f in range(lim - 2, -1, -1):
        ext = np.concatenate([Bk, negs])
        x = lae(lae(Bk, ext[1:S + 1], tab), np.where(skipb, ext[2:S + 2], NEG), tab)
        live = x != NEG
        Bk = np.where(live, np.where(live, x, 0) + q[f].astype(i64), NEG)
        fb[f] = Bk[states[f]]
    g = fa + fb - q[t, states].astype(i64) - i64(total)
    frame_post = np.clip(g, Q_FLOOR, 0).astype(np.int32)
    label_post = np.zeros(L, dtype=np.int32)
    for i in range(L):
        label_post[i] = frame_post[int(start[i]):int(start[i] + nframes[i])].min()
    return total, frame_post, label_post


def post_host(log_probs, lens, targets, target_lens, blank, start, nframes, ok, problems_per_utt=1, star=None) -> PostResult:
    """POST_RULES on the host: the NumPy twin of k_post and the CPU path of align(posteriors=True).  log_probs, lens, targets,
    target_lens, blank, problems_per_utt and star as in align_host; start, nframes int32 [P, max_labels] and ok int32 [P] (None:
    all 1) are the alignment's own."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'post_host: log_probs must be [B, T, C] with B, T, C >= 1, got {lp.shape}')
    B, T, C = lp.shape
    K = int(problems_per_utt)
    tg = np.asarray(targets)
    tl = np.asarray(target_lens)
    if K < 1 or tg.ndim != 2 or tg.shape[0] != B * K or tl.shape != (B * K,):
        raise ValueError(f'post_host: targets must be [B * problems_per_utt, max_labels] with one length each, got '
                         f'{tg.shape} / {tl.shape} for B {B}, problems_per_utt {K}')
    P, ML = tg.shape
    if not 1 <= ML <= MAX_LABELS:
        raise ValueError(f'post_host: max_labels (the row pitch of targets) must be 1 .. {MAX_LABELS}, got {ML}')
    if T > MAX_T:
        raise ValueError(f'post_host: at most {MAX_T} frames, got {T}')
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f'post_host: blank {blank} is outside [0, {C})')
    a_start, a_nframes = np.asarray(start), np.asarray(nframes)
    a_ok = np.ones(P, dtype=np.int32) if ok is None else np.asarray(ok)
    if a_start.shape != (P, ML) or a_nframes.shape != (P, ML) or a_ok.shape != (P,):
        raise ValueError(f'post_host: start / nframes must be [{P}, {ML}] and ok [{P}], got {a_start.shape} / {a_nframes.shape} / '
                         f'{a_ok.shape}')
    tg = tg.astype(np.int32)
    star = _star_plane(star, B, T, 'post_host')
    n_ids = C + (star is not None)
    tab = lae_table()
    frame_post = np.zeros((P, T), dtype=np.int32)
    label_post = np.zeros((P, ML), dtype=np.int32)
    total = np.full(P, NEG, dtype=np.int64)
    ok_post = np.zeros(P, dtype=np.int32)
    for p in range(P):
        u = p // K
        lim = T if lens is None else int(min(max(int(lens[u]), 0), T))
        L = int(tl[p])
        if a_ok[p] == 0 or L < 0 or L > ML:
            continue
        y = tg[p, :L]
        if L and (y.min() < 0 or y.max() >= n_ids or (y == blank).any()):
            continue
        if not _path_ok(a_start[p, :L], a_nframes[p, :L], y, lim):  # (lim == 0 with L > 0 fails here)
            continue
        ok_post[p] = 1
        if lim == 0:
            total[p] = 0
            continue
        total[p], frame_post[p, :lim], label_post[p, :L] = _post_one(lp[u], lim, y, blank, tab, a_start[p, :L], a_nframes[p, :L],
                                                                     None if star is None else star[u])
    return PostResult(frame_post, label_post, total, ok_post)


def _word_groups(labels, vocab, wild):
    """the label indices of every word of to_hypotheses: the labels between ' ' labels, the wildcard a word of its own"""
    groups, group = [], []
    for k, c in enumerate(labels):
        if wild is not None and c == wild:
            groups += [group, [k]]
            group = []
        elif vocab[c] == ' ':
            groups.append(group)
            group = []
        else:
            group.append(k)
    return [g for g in groups + [group] if g]


def post_to_hypotheses(result: AlignResult, post: PostResult, vocabulary: Sequence[str], seconds_per_frame: float, lens=None,
                       star_token=None) -> List:
    """`to_hypotheses` plus the posteriors of `post` (POST_RULES) in the optional fields of qasr.ctc.Hypothesis: post, per label
    the mean over its run of exp(frame_post / 2^16), in 0 .. 1; post_min, per label exp(label_post / 2^16), its least certain
    frame; word_post, one value per entry of words: the mean over the frames of the word's labels; frame_post, a float32 array
    of the lim log-posteriors (nats) of the path's states.  lens: the frame counts [B] the alignment ran with (None: all T).  A
    problem whose posteriors are not ok (or that is not alignable) gets empty lists."""
    hyps = to_hypotheses(result, vocabulary, seconds_per_frame, star_token)
    fp_all, ok, a_ok = _np(post.frame_post), _np(post.ok), _np(result.ok)
    start, nframes = _np(result.start), _np(result.nframes)
    T = fp_all.shape[1]
    K = int(result.problems_per_utt)
    ln = None if lens is None else _np(lens)
    vocab = list(vocabulary)
    wild = len(vocab) + 1 if star_token is not None else None
    if wild is not None:
        vocab += ['', star_token]
    for p, h in enumerate(hyps):
        if not (ok[p] and a_ok[p]):
            h.post, h.post_min, h.word_post, h.frame_post = [], [], [], np.zeros(0, dtype=np.float32)
            continue
        lim = T if ln is None else int(min(max(int(ln[p // K]), 0), T))
        pr = np.exp(fp_all[p, :lim].astype(np.float64) / ONE)
        runs = [pr[int(start[p, i]):int(start[p, i]) + int(nframes[p, i])] for i in range(len(h.labels))]
        h.post = [float(r.mean()) for r in runs]
        h.post_min = [float(r.min()) for r in runs]
        h.word_post = [float(np.concatenate([runs[k] for k in g]).mean()) for g in _word_groups(h.labels, vocab, wild)]
        assert len(h.word_post) == len(h.words), (len(h.word_post), len(h.words))
        h.frame_post = (fp_all[p, :lim].astype(np.float64) / ONE).astype(np.float32)
    return hyps


# ---- posteriors along a banded alignment: forward-backward inside the band k_align_band chose (k_post_band, csrc/qasr_post_band.hip)
POST_BAND_RULES = """POST_RULES for a recording that only fits k_align_band: the forward and the backward pass run over the part of the lattice that
the band of BAND_RULES kept, so every quantity is one of the restricted lattice - total is the log-likelihood of the
alignments that stay inside the band, a lower bound (up to lae's error) on the full lattice's.  The inputs are align_band_host's
plus its start, nframes [P, max_labels], ok [P] and band_base [P, ceil(T / 32)], and the width BW in BAND_STATES it ran with.
Shapes are BAND_RULES's: K = 1, L <= BAND_MAX_LABELS, T <= BAND_MAX_FRAMES.  States, lab(s), q(t, s), lim, S = 2L + 1,
top = max(0, S - BW), the predecessors and successors, lae and its order are those of RULES and POST_RULES.
Cells: base(t) = band_base[p][t // 32]; (t, s) exists iff base(t) <= s < min(base(t) + BW, S).
Edges: (t - 1, s') -> (t, s) is an edge of RULES whose two cells exist and with s' >= base(t) - k_align_band's "a predecessor
below the new base is NEG", so the Viterbi path of k_align_band runs over existing edges only.
Forward row: A(0, s) = q(0, s) for s < 2 (s < S), NEG elsewhere; A(t, s) = x + q(t, s), x = lae(lae(A[s], A[s - 1]), A[s - 2]) over
the existing edges into (t, s), a missing one counting as NEG; NEG if x == NEG: k_align_band's step with lae in place of max.
Backward row: Bk(lim - 1, s) = q(lim - 1, s) for s in {2L, 2L - 1} (L == 0: s = 0) that exist at lim - 1, NEG elsewhere;
Bk(t, s) = x + q(t, s), x = lae(lae(Bk[s], Bk[s + 1]), Bk[s + 2]) over the existing edges out of (t, s).  A state whose successors
all lie outside is NEG at that frame; in particular a cell of a block's last frame that lies below the next block's base is a
dead end.  Nothing is ever added to NEG.
total = lae(A[2L], A[2L - 1]) at lim - 1 (L == 0: A[0]); an end state outside the last band counts as NEG.
The path is read from start / nframes as in POST_RULES; g(t) = A(t, s_t) + Bk(t, s_t) - q(t, s_t) - total, frame_post = g clamped
to [Q_FLOOR, 0] for t < lim and 0 behind, label_post = the minimum of frame_post over the label's run, tails 0.
Validity.  ok = 0, every output row zero and total = NEG: POST_RULES's reasons (BAND_MAX_LABELS in place of MAX_LABELS); a
band_base row that is no trajectory of k_align_band - over the blocks that have a frame < lim it must start at 0, never
decrease, move by less than BW / 2 per block and stay in [0, top]; a path that leaves its frame's band (no cell (t, s_t)); a
path over a missing edge (s_t < base(t + 1) for t + 1 < lim); total == NEG.  Everything is decided by comparisons: start,
nframes and band_base are never used as an index before they are checked (a checked start or end is a frame number < lim and
may then select a block of band_base).  lim == 0 with L == 0: ok = 1, total = 0.
When S <= BW the base is 0 throughout and every output equals post_host's on every byte.
Star: id C reads the plane wherever logp[p][t][c] is read (STAR_RULES); every output equals on every byte the call without a
plane on the matrix with the plane appended as class C of C + 1."""


def _band_base_ok(bases, nblk, top, BW):
    """the first nblk entries of a band_base row are a trajectory k_align_band can produce (POST_BAND_RULES), in Python integers"""
    prev = 0
    for j in range(nblk):
        b = int(bases[j])
        if b < 0 or b > top or (b != 0 if j == 0 else (b < prev or b - prev >= BW // 2)):
            return False
        prev = b
    return True


def _post_band_one(lp, lim, y, blank, tab, BW, start, nframes, bases, st=None):
    """one problem with a valid target y, a valid path and a valid band_base row `bases` over lp float32 [T, C]: (total,
    frame_post int32 [lim], label_post int32 [L]), or None when the path is not inside the band or total == NEG"""
    L = len(y)
    i64 = np.int64
    S = 2 * L + 1
    n = min(BW, S)                                                  # states in the band (constant: base <= top)
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = y
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = y[1:] != y[:-1]
    skipb = np.zeros(S, dtype=bool)                                 # s may step to s + 2
    skipb[:S - 2] = skip[2:]
    t = np.arange(lim)
    start, nframes = np.asarray(start, dtype=i64), np.asarray(nframes, dtype=i64)
    j = np.searchsorted(start, t, side='right')
    in_run = (j > 0) & (t < (start + nframes)[np.maximum(j, 1) - 1]) if L else np.zeros(lim, dtype=bool)
    states = np.where(in_run, 2 * j - 1, 2 * j)
    bt = np.asarray(bases, dtype=i64)[t // BAND_BLOCK]              # base(t)
    if ((states < bt) | (states >= bt + BW)).any() or (states[:-1] < bt[1:]).any():
        return None                                                 # no such cell, or no such edge
    negs = np.full(2, NEG, i64)

    def q_at(f, b):
        return quantize(_emit(lp, st, f, lab[b:b + n])).astype(i64)

    def add(x, q):
        live = x != NEG
        return np.where(live, np.where(live, x, 0) + q, NEG)
    b = 0
    A = np.full(n, NEG, i64)                                        # A[i]: state b + i
    A[:min(2, S)] = q_at(0, 0)[:min(2, S)]
    fa = np.empty(lim, dtype=i64)
    fa[0] = A[states[0]]
    for f in range(1, lim):
        nb = int(bt[f])
        if nb > b:                                                  # (nb - b < BW / 2 <= n)
            A = np.concatenate([A[nb - b:], np.full(nb - b, NEG, i64)])
            b = nb
        ext = np.concatenate([negs, A])                             # what lies below base is NEG
        A = add(lae(lae(A, ext[1:n + 1], tab), np.where(skip[b:b + n], ext[:n], NEG), tab), q_at(f, b))
        fa[f] = A[states[f] - b]

    def at(s):
        return int(A[s - b]) if b <= s < b + n else NEG
    total = at(0) if L == 0 else int(lae(at(2 * L), at(2 * L - 1), tab))
    if total == NEG:
        return None
    Bk = np.full(n, NEG, i64)                                       # Bk[i]: state b + i
    q = q_at(lim - 1, b)
    for s in range(max(S - 2, 0), S):
        if b <= s < b + n:
            Bk[s - b] = q[s - b]
    fb = np.empty(lim, dtype=i64)
    fb[lim - 1] = Bk[states[lim - 1] - b]
    for f in range(lim - 2, -1, -1):
        ext = np.concatenate([Bk, negs])                            # what lies above the band is NEG
        x = lae(lae(Bk, ext[1:n + 1], tab), np.where(skipb[b:b + n], ext[2:n + 2], NEG), tab)       # x[i]: state base(f + 1) + i
        nb = int(bt[f])
        if nb < b:                                                  # the states below base(f + 1) are dead ends at f
            x = np.concatenate([np.full(b - nb, NEG, i64), x[:n - (b - nb)]])
            b = nb
        Bk = add(x, q_at(f, b))
        fb[f] = Bk[states[f] - b]
    g = fa + fb - quantize(_emit(lp, st, t, lab[states])).astype(i64) - i64(total)
    frame_post = np.clip(g, Q_FLOOR, 0).astype(np.int32)
    label_post = np.zeros(L, dtype=np.int32)
    for i in range(L):
        label_post[i] = frame_post[int(start[i]):int(start[i] + nframes[i])].min()
    return total, frame_post, label_post


def post_band_host(log_probs, lens, targets, target_lens, blank, start, nframes, ok, band_base, band_states, star=None) -> PostResult:
    """POST_BAND_RULES on the host: the NumPy twin of k_post_band and the CPU path of align_long(posteriors=True).  log_probs,
    lens, targets, target_lens, blank and star as in align_band_host; start, nframes int32 [P, max_labels], ok int32 [P] (None:
    all 1) and band_base int32 [P, ceil(T / 32)] are that alignment's own (want_band_base=True), band_states the width it used."""
    lp = np.asarray(log_probs, dtype=np.float32)
    if lp.ndim != 3 or min(lp.shape) < 1:
        raise ValueError(f'post_band_host: log_probs must be [P, T, C] with P, T, C >= 1, got {lp.shape}')
    P, T, C = lp.shape
    tg = np.asarray(targets)
    tl = np.asarray(target_lens)
    if tg.ndim != 2 or tg.shape[0] != P or tl.shape != (P,):
        raise ValueError(f'post_band_host: targets must be [P, max_labels] with one length each, got {tg.shape} / {tl.shape} '
                         f'for P {P}')
    ML = tg.shape[1]
    if not 1 <= ML <= BAND_MAX_LABELS:
        raise ValueError(f'post_band_host: max_labels (the row pitch of targets) must be 1 .. {BAND_MAX_LABELS}, got {ML}')
    if T > BAND_MAX_FRAMES:
        raise ValueError(f'post_band_host: at most {BAND_MAX_FRAMES} frames, got {T}')
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f'post_band_host: blank {blank} is outside [0, {C})')
    if band_states is None or int(band_states) not in BAND_STATES:
        raise ValueError(f'post_band_host: band_states must be one of {BAND_STATES}, got {band_states}')
    BW = int(band_states)
    NB = (T + BAND_BLOCK - 1) // BAND_BLOCK
    a_start, a_nframes = np.asarray(start), np.asarray(nframes)
    a_ok = np.ones(P, dtype=np.int32) if ok is None else np.asarray(ok)
    if band_base is None:
        raise ValueError('post_band_host: band_base is required (align_band_host(want_band_base=True))')
    a_base = np.asarray(band_base)
    if a_start.shape != (P, ML) or a_nframes.shape != (P, ML) or a_ok.shape != (P,) or a_base.shape != (P, NB):
        raise ValueError(f'post_band_host: start / nframes must be [{P}, {ML}], ok [{P}] and band_base [{P}, {NB}], got '
                         f'{a_start.shape} / {a_nframes.shape} / {a_ok.shape} / {a_base.shape}')
    tg = tg.astype(np.int32)
    star = _star_plane(star, P, T, 'post_band_host')
    n_ids = C + (star is not None)
    tab = lae_table()
    frame_post = np.zeros((P, T), dtype=np.int32)
    label_post = np.zeros((P, ML), dtype=np.int32)
    total = np.full(P, NEG, dtype=np.int64)
    ok_post = np.zeros(P, dtype=np.int32)
    for p in range(P):
        lim = T if lens is None else int(min(max(int(lens[p]), 0), T))
        L = int(tl[p])
        if a_ok[p] == 0 or L < 0 or L > ML:
            continue
        y = tg[p, :L]
        if L and (y.min() < 0 or y.max() >= n_ids or (y == blank).any()):
            continue
        if not _path_ok(a_start[p, :L], a_nframes[p, :L], y, lim):  # (lim == 0 with L > 0 fails here)
            continue
        if not _band_base_ok(a_base[p], (lim + BAND_BLOCK - 1) // BAND_BLOCK, max(0, 2 * L + 1 - BW), BW):
            continue
        if lim == 0:
            ok_post[p], total[p] = 1, 0
            continue
        got = _post_band_one(lp[p], lim, y, blank, tab, BW, a_start[p, :L], a_nframes[p, :L], a_base[p],
                             None if star is None else star[p])
        if got is not None:
            ok_post[p] = 1
            total[p], frame_post[p, :lim], label_post[p, :L] = got
    return PostResult(frame_post, label_post, total, ok_post)
